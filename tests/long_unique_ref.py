"""Each long transmission once, restated (TEST INFRASTRUCTURE; the definition is in include/gnuais_hip.h under
gnuais_batch_long_unique).

The restatement is unique_ref.UniqueRef -- and heard_ref.HeardRef for the member lists -- imported unchanged, with the long
key and with t taken from the record: key_of() and stamp() of unique_ref read a record's nbits, payload, end_bit and flags
by name, so on a LONG_FRAME_DTYPE record they are the long key (nbits and the 132 payload bytes) and the long stamp.  A
member's signal record is all zero: heard_ref gives zeros where no signal is passed.

Also here, shared by the CPU and the GPU test file: random long record sets, the seven-receiver input of the issue, and
SampleRef, the oracle's slices through long_ref.LongDeframer with the definition's receive time."""
import numpy as np

import heard_ref as hr
import long_ref as lr
import unique_ref as ur
from gnuais_amd import synth
from gnuais_amd.lib import LONG_FRAME_DTYPE

REPAIRED = ur.REPAIRED


class LongUniqueRef:
    def __init__(self, window: int):
        self.r = hr.HeardRef(window)

    def reset(self):
        self.r.reset()

    @property
    def late(self):
        return self.r.late

    @property
    def tail(self):
        return self.r.tail

    def push(self, frames: np.ndarray, rows: int):
        """one drain: -> (records, int32 copies)"""
        f, _, c = self.r.push(frames, frames["t"], rows)
        return f, c

    def push_heard(self, frames: np.ndarray, rows: int):
        """one drain: -> (records, int32 copies, int32 first, members)"""
        f, _, c, first, members = self.r.push_heard(frames, frames["t"], rows)
        return f, c, first, members


# ---- random record sets --------------------------------------------------------------------------------------------------
def key_pool(rng):
    """1..24 keys; among them families that differ only in nbits, only in the last used payload byte, and only in the
    record's word 37 (payload bytes 128..131, behind every used byte: the key is all 132 bytes)"""
    pool, want = [], int(rng.integers(1, 25))
    while len(pool) < want:
        nbytes = int(rng.choice([54, 60, 100, 126]))
        p = np.zeros(132, dtype=np.uint8)
        p[:nbytes] = rng.integers(0, 256, nbytes, dtype=np.uint8)
        pool.append((8 * nbytes, p))
        kind = int(rng.integers(0, 5))
        if kind == 0:                                       # the same bytes, another nbits
            pool.append((8 * nbytes + 8, p))
        elif kind == 1:                                     # only the last used byte differs
            q = p.copy()
            q[nbytes - 1] ^= 1 << int(rng.integers(0, 8))
            pool.append((8 * nbytes, q))
        elif kind == 2:                                     # only word 37 differs
            q = p.copy()
            q[128 + int(rng.integers(0, 4))] ^= 1 << int(rng.integers(0, 8))
            pool.append((8 * nbytes, q))
    return pool


def random_set(rng, W):
    """LONG_FRAME_DTYPE records: transmissions whose copies lie on different channels -- equal t among them, gaps of exactly
    W and W + 1 -- both values of flags bit 6, some t = -1, any reserved byte; shuffled"""
    pool = key_pool(rng)
    n_ch = int(rng.integers(1, 40))
    rec, seen = [], set()
    for _ in range(int(rng.integers(1, 30))):
        k = int(rng.integers(0, len(pool)))
        t = int(rng.integers(0, 6000))
        for _ in range(int(rng.integers(1, 9))):
            t += int(rng.choice([0, 0, int(rng.integers(1, W + 1)), W, W + 1]))
            ch = int(rng.integers(0, n_ch))
            untimed = rng.random() < 0.08
            if not untimed and (ch, t) in seen:             # one channel never closes two frames on one row
                continue
            seen.add((ch, t))
            rec.append((k, ch, -1 if untimed else t, int(rng.integers(0, 2))))
    order = rng.permutation(len(rec))
    fr = np.zeros(len(rec), dtype=LONG_FRAME_DTYPE)
    for j, i in enumerate(order):
        k, ch, t, rep = rec[i]
        fr[j]["channel"], fr[j]["end_bit"], fr[j]["t"] = ch, 1000 + 7 * int(i), t       # the stamp: unique, unrelated to t
        fr[j]["payload"], fr[j]["nbits"] = pool[k][1], pool[k][0]
        fr[j]["flags"] = 1 | (REPAIRED if rep else 0) | (int(rng.integers(0, 32)) << 1)
        fr[j]["reserved"] = int(rng.integers(0, 256))
    return fr


def cut_into_drains(rng, fr):
    """[(records, rows)]: 1..5 drains at random rows; drain d holds the records with rows[d-1] <= t < rows[d], the untimed
    ones anywhere"""
    tm = fr["t"]
    top = int(tm.max()) + 1 if len(tm) and tm.max() >= 0 else 1
    n = int(rng.integers(1, 6))
    rows = sorted(int(r) for r in rng.integers(0, top + 1, n - 1)) + [top + int(rng.integers(0, 3000))]
    which = np.searchsorted(np.array(rows), tm, side="right")
    which[tm < 0] = rng.integers(0, n, int(np.count_nonzero(tm < 0)))
    return [(fr[which == d], rows[d]) for d in range(n)]


def random_cases(seed, n_sets=150):
    """[(W, [(records, rows)])]: n_sets random sets cut into drains, W from {1, 64, 700}, and the empty push"""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n_sets):
        W = int(rng.choice([1, 64, 700]))
        cases.append((W, cut_into_drains(rng, random_set(rng, W))))
    cases.append((9, [(np.zeros(0, dtype=LONG_FRAME_DTYPE), 0)]))
    return cases


def write_cases(path, cases):
    """int32 W, int32 drains, then per drain int32 n, int64 rows, n records"""
    with open(path, "wb") as f:
        for W, drains in cases:
            f.write(np.array([W, len(drains)], dtype=np.int32).tobytes())
            for fr, rows in drains:
                f.write(np.int32(len(fr)).tobytes() + np.int64(rows).tobytes() + fr.tobytes())


# ---- the seven receivers of one region -----------------------------------------------------------------------------------
TOTAL7 = 6 * 8 * 1280
COUNTS7 = [5, 5, 4, 5, 5, 5, 5]         # long frames per receiver (receiver 2 loses the 432-bit one)


def seven_receivers(sigma: float = 500.0):
    """int16 [TOTAL7][7]: the seed-9 stream of long bursts with receiver c's own noise, unique_ref.DELAYS7[c] rows late"""
    cols = [np.roll(synth.make_stream(TOTAL7, seed=9, channel=c, sigma=sigma, payloads=lr.long_payloads())[0], d)
            for c, d in enumerate(ur.DELAYS7)]
    return np.stack(cols, axis=1)


def ragged_cuts7():
    return ur.ragged_cuts(TOTAL7)


class SampleRef:
    """the restatement behind the samples: the oracle's slices segment by segment into one LongDeframer per channel, and
    the definition's t from where each closing bit lies"""

    def __init__(self, n_ch):
        from oracle_lib import Oracle
        self.o = Oracle(n_ch)
        self.n = 0
        self.ds = [lr.LongDeframer() for _ in range(n_ch)]
        self.segs = [[] for _ in range(n_ch)]               # per channel: (bits fed before, first row, rows, bits)
        self.given = [0] * n_ch

    def run(self, x):
        import frame_time_ref as ftr
        for s0 in range(0, x.shape[0], ftr.SEG):
            seg = np.ascontiguousarray(x[s0:s0 + ftr.SEG])
            for c, bits in enumerate(self.o.run(seg, want_bits=True)["bits"]):
                self.segs[c].append((self.ds[c].fed, self.n + s0, seg.shape[0], len(bits)))
                self.ds[c].feed(bits)
        self.n += x.shape[0]

    def t(self, c, f):
        import frame_time_ref as ftr
        for fed, row0, l_s, cnt in self.segs[c]:
            if fed <= f["index"] < fed + cnt:
                return ftr.interp(row0, 0, f["index"] - fed, l_s, cnt)
        raise AssertionError((c, f["index"]))

    def drain(self):
        """the long frames closed since the last drain, as the plain long drain delivers them"""
        out = []
        for c, d in enumerate(self.ds):
            mine = d.long_frames()
            for f in mine[self.given[c]:]:
                out.append((c, f["end_bit"], lr.record(c, f, self.t(c, f))))
            self.given[c] = len(mine)
        out.sort(key=lambda r: (r[0], r[1]))
        return np.array([r[2] for r in out], dtype=LONG_FRAME_DTYPE)


# ---- further inputs of the GPU tests -------------------------------------------------------------------------------------
GROUP_BYTES = (54, 100, 126)            # one burst every six slots
TOTAL_G = len(GROUP_BYTES) * 6 * 1280


def group_payloads(group: int, sizes=GROUP_BYTES, every: int = 6):
    """make_stream's `payloads`: slot every*k carries a payload of sizes[k] bytes of the group's own (long_payloads() gives
    every group the same bytes)"""
    def pick(rng, slot):
        if slot % every or slot // every >= len(sizes):
            return None
        n = sizes[slot // every]
        return bytes(np.random.default_rng([77, group, n]).integers(0, 256, n, dtype=np.uint8))
    return pick


def group_receivers(groups: int, delays=ur.DELAYS7, sigma: float = 500.0):
    """int16 [TOTAL_G][groups * len(delays)]: receiver g * len(delays) + d hears group g's three long bursts with noise of
    its own, delays[d] rows late"""
    cols = []
    for g in range(groups):
        for d, delay in enumerate(delays):
            x = synth.make_stream(TOTAL_G, seed=9, channel=g * len(delays) + d, sigma=sigma, payloads=group_payloads(g))[0]
            cols.append(np.roll(x, delay))
    return np.stack(cols, axis=1)


def slots_stream(total, slot_payloads, seed=21, channel=0, sigma=300.0):
    """a channel with the given {slot: payload}"""
    return synth.make_stream(total, seed=seed, channel=channel, sigma=sigma, payloads=lambda rng, slot: slot_payloads.get(slot))[0]


def short_long_payload(seed: int = 1, nbytes: int = 54):
    return bytes(np.random.default_rng([31, seed]).integers(0, 256, nbytes, dtype=np.uint8))
