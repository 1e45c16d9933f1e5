"""One record per transmission, restated (TEST INFRASTRUCTURE; the definition is in include/gnuais_hip.h under
gnuais_batch_unique).

  key      nbits and the 53 payload bytes (channel, end_bit, flags are not part of it)
  members  the frames of a key with t >= 0, by (t, channel); member i joins the cluster of member i - 1 iff
           t_i - t_{i-1} <= W
  primary  the first member by (flags bit 6, t, channel); its record and time are delivered with copies = the size
  t = -1   a cluster by itself; these come first, in the plain drain's order (channel, 37-bit stamp); the rest by
           (t, channel) of the primary
  drains   with n = rows at the drain, a cluster whose last member has t_last + W >= n stays open as (key, t_last); in the
           next drain it is a virtual first member: frames that chain onto it are late (counted, not delivered) and move
           t_last on; entries with t_last + W < n are dropped

UniqueRef is that with a dict, sorted() and one loop.  receivers() builds the test input both test files share: groups
of receivers that hear the same transmissions with independent noise and their own delay."""
import numpy as np

from gnuais_amd import synth

REPAIRED = 0x40


def stamp(f) -> int:
    return int(f["end_bit"]) | (((int(f["flags"]) >> 1) & 31) << 32)


def key_of(f):
    return int(f["nbits"]), f["payload"].tobytes()


class UniqueRef:
    def __init__(self, window: int):
        assert window > 0
        self.W = int(window)
        self.reset()

    def reset(self):
        self.tail = {}          # key -> t_last
        self.late = 0

    def push(self, frames: np.ndarray, times: np.ndarray, rows: int):
        """one drain: -> (frames, int64 times, int32 copies)"""
        W = self.W
        out = []                # (order, index of the primary, copies)
        by = {}
        for i, (f, t) in enumerate(zip(frames, times)):
            if t < 0:
                out.append(((0, int(f["channel"]), stamp(f)), i, 1))
            else:
                by.setdefault(key_of(f), []).append((int(t), int(f["channel"]), i))
        tail = {}

        def close(k, members, from_tail, t_last):
            if from_tail:
                self.late += len(members)
            else:
                t, ch, i = min(members, key=lambda m: (int(frames[m[2]]["flags"]) & REPAIRED, m[0], m[1]))
                out.append(((1, t, ch), i, len(members)))
            if t_last + W >= rows:
                tail[k] = t_last

        for k in set(by) | set(self.tail):
            from_tail, last, cur = k in self.tail, self.tail.get(k), []
            for m in sorted(by.get(k, [])):
                if last is not None and m[0] - last > W:
                    close(k, cur, from_tail, last)
                    cur, from_tail = [], False
                cur.append(m)
                last = m[0]
            close(k, cur, from_tail, last)
        self.tail = tail
        out.sort()
        idx = np.array([i for _, i, _ in out], dtype=np.int64)
        return (frames[idx].copy(), np.asarray(times, dtype=np.int64)[idx].copy(),
                np.array([c for _, _, c in out], dtype=np.int32))


# the ragged calls of the receivers input (the frame times' segment rule depends on the cuts)
RAGGED = [1, 777, 2047, 2048, 2049, 3000, 1500]
TOTAL = 10 * 1280
DELAYS6 = [0, 19, 38, 57, 76, 95]
DELAYS7 = [0, 16, 32, 48, 64, 80, 95]


def ragged_cuts(total: int = TOTAL):
    calls = RAGGED + [total - sum(RAGGED)]
    assert calls[-1] > 0
    return np.cumsum([0] + calls)


def receivers(groups: int, delays, total: int = TOTAL, seed: int = 12, sigma: float = 1000.0, n_slots: int = 8):
    """int16 [total][groups * len(delays)]: receiver g * len(delays) + d hears group g's transmissions (slots 0 ..
    n_slots - 1, one payload stream per group) with noise of its own, delays[d] rows late.  The last slots stay empty, so
    that the rotation brings only silence to the front."""
    cols = []
    for g in range(groups):
        prng = np.random.default_rng([seed, g, 0x554e])
        pay = [synth.random_position_report(prng) for _ in range(n_slots)]
        for d, delay in enumerate(delays):
            x, placed = synth.make_stream(total, seed=seed, channel=g * len(delays) + d, sigma=sigma,
                                          payloads=lambda rng, slot, pay=pay: pay[slot] if slot < len(pay) else None)
            assert len(placed) == n_slots
            cols.append(np.roll(x, delay))
    return np.stack(cols, axis=1)
