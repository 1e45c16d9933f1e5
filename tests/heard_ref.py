"""Who heard each transmission, restated (TEST INFRASTRUCTURE; the definition is in include/gnuais_hip.h under
gnuais_batch_drain_frames_heard).

  records   what unique_ref.UniqueRef.push gives for the same state: frames, times, copies, unchanged
  first     first[0] = 0, first[i + 1] - first[i] = copies[i]
  members   cluster i's members are members[first[i] : first[i + 1]], by (t, channel); a member is (channel, the copy's
            own flags, t, the copy's signal record -- zeros where none is given)
  t = -1    a cluster of one member with t = -1
  primary   one of the members: the one with the record's channel and t
  late      copies that chain onto a tail entry are counted in `late` and listed nowhere

HeardRef is unique_ref.UniqueRef, imported unchanged, with push_heard beside push: one more loop over the same dict and
sorted().  The two may alternate on one object; the carried state is UniqueRef's."""
import numpy as np

import unique_ref as ur
from gnuais_amd.lib import HEARER_DTYPE, SIGNAL_DTYPE


class HeardRef(ur.UniqueRef):
    def push_heard(self, frames: np.ndarray, times: np.ndarray, rows: int, signal=None):
        """one drain: -> (frames, int64 times, int32 copies, int32 first, members)"""
        W = self.W
        times = np.asarray(times, dtype=np.int64)
        if signal is None:
            signal = np.zeros(len(frames), dtype=SIGNAL_DTYPE)
        # the lists from the state BEFORE the push: the same walk as UniqueRef.push, keeping the members
        lists = {}              # frame index of a cluster's primary -> the frame indices of its members, in member order
        by = {}
        for i, (f, t) in enumerate(zip(frames, times)):
            if t < 0:
                lists[i] = [i]
            else:
                by.setdefault(ur.key_of(f), []).append((int(t), int(f["channel"]), i))
        for k, mem in by.items():
            last, from_tail, cur = self.tail.get(k), k in self.tail, []

            def close():
                if cur and not from_tail:
                    p = min(cur, key=lambda m: (int(frames[m[2]]["flags"]) & ur.REPAIRED, m[0], m[1]))
                    lists[p[2]] = [m[2] for m in cur]

            for m in sorted(mem):
                if last is not None and m[0] - last > W:
                    close()
                    cur, from_tail = [], False
                cur.append(m)
                last = m[0]
            close()
        f_out, t_out, copies = self.push(frames, times, rows)
        # the records of push() name their primaries: (channel, t, stamp) is unique per frame
        where = {(int(f["channel"]), int(t), ur.stamp(f), int(f["flags"])): i for i, (f, t) in enumerate(zip(frames, times))}
        first = np.zeros(len(f_out) + 1, dtype=np.int32)
        members = []
        for q, (f, t) in enumerate(zip(f_out, t_out)):
            mine = lists[where[(int(f["channel"]), int(t), ur.stamp(f), int(f["flags"]))]]
            assert len(mine) == int(copies[q])
            for i in mine:
                members.append((int(frames[i]["channel"]), int(frames[i]["flags"]), -1 if times[i] < 0 else int(times[i]),
                                tuple(signal[i].tolist())))
            first[q + 1] = len(members)
        return f_out, t_out, copies, first, np.array(members, dtype=HEARER_DTYPE).reshape(-1)


def check_invariants(frames, times, copies, first, members):
    """what holds for every heard drain, whoever made it"""
    assert first.dtype == np.int32 and members.dtype == HEARER_DTYPE and copies.dtype == np.int32
    assert len(first) == len(frames) + 1 and first[0] == 0 and first[-1] == len(members)
    assert np.array_equal(np.diff(first), copies)
    for i, (f, t) in enumerate(zip(frames, times)):
        m = members[first[i]:first[i + 1]]
        order = list(zip(m["t"].tolist(), m["channel"].tolist()))
        assert order == sorted(order) and len(set(order)) == len(order), order
        assert (int(-1 if t < 0 else t), int(f["channel"])) in order
        if t < 0:
            assert len(m) == 1 and m["t"][0] == -1
        p = m[order.index((int(-1 if t < 0 else t), int(f["channel"])))]
        assert int(p["flags"]) == int(f["flags"])
