"""Restatement of the long-frame repair (include/gnuais_hip.h, gnuais_batch_long_repair) for the tests: D' bit by bit
(long_ref.LongDeframer) with the raw bits of every frame kept, and brute force over every trial p.

RawLongDeframer feeds long_ref.LongDeframer one bit at a time and keeps what the definition calls r: the bits seen in
ST_DATA -- stuffed zeros included, the sixth 1 of the closing flag not -- since the last entry to ST_DATA.

brute_force_many() runs ST_DATA of that machine over r' and one more 1 for EVERY p, bit by bit, as
repair_ref.brute_force_many does for the chain's repair, with the two numbers of the definition as parameters: the
give-up test `bufferpos >= limit` and the smallest n' a trial may have.  limit = 1031, n' > 426 is the long repair;
limit = 449, n' > 0 is the chain's.  numpy only carries the trials side by side; nothing here works on words, masks of
stuffed bits or CRC tables: those are the code under test."""
import numpy as np

import long_ref as lr
from repair_ref import FRAME_REPAIRED, ST_DATA, crc_holds, payload_of

LIMIT = lr.LONG_LIMIT           # 1031
MIN_BITS = lr.SHORT_BITS        # n' > 426
MAX_RAW = 1280                  # gnuais_long_repair_candidate takes no more raw bits
REC_RAW = 1236                  # 1030 stored bits and at most 206 stuffed zeros


class RawLongDeframer(lr.LongDeframer):
    """closed[i]["raw"]: the raw bits of that frame (uint8)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.raw = []

    def feed(self, bits, states=None):
        for x in bits:
            x = int(x)
            before, stuffed, n_closed = self.state, self.bitstuff, len(self.closed)
            super().feed([x], states)
            if before == ST_DATA:
                if not (stuffed and x == 1):            # every bit of ST_DATA but the sixth 1
                    self.raw.append(x)
            elif self.state == ST_DATA:                 # protodec.c:1076-1082: a frame starts
                self.raw = []
            if len(self.closed) > n_closed:
                self.closed[-1]["raw"] = np.array(self.raw, dtype=np.uint8)

    def candidates(self):
        """the frames D' counts in `failed`"""
        return [f for f in self.closed if f["n"] > lr.SHORT_BITS and not f["good"]]


def brute_force_many(raws, limit=LIMIT, min_bits=MIN_BITS):
    """every trial p of each of several candidates of ONE length (raws [records][rawlen]), bit by bit: per record the
    list [(p, n', payload bytes)] of the trials that pass, ascending p"""
    raws = np.atleast_2d(np.asarray(raws, dtype=np.uint8)) & 1
    M, L = raws.shape
    T = L - 1
    if T <= 0:
        return [[] for _ in range(M)]
    R = np.concatenate([np.repeat(raws, T, axis=0), np.ones((M * T, 1), dtype=np.uint8)], axis=1)
    rows = np.arange(M * T)
    trial = rows % T
    R[rows, trial] ^= 1
    R[rows, trial + 1] ^= 1
    ant = np.zeros(M * T, dtype=np.int64)
    bs = np.zeros(M * T, dtype=bool)
    last = np.zeros(M * T, dtype=np.uint8)
    pos = np.zeros(M * T, dtype=np.int64)
    stop_at = np.full(M * T, -1, dtype=np.int64)
    gone = np.zeros(M * T, dtype=bool)                  # bufferpos reached the limit: protodec_reset()
    buf = np.zeros((M * T, limit + 1), dtype=np.uint8)
    for i in range(L + 1):
        x = R[:, i]
        act = (stop_at < 0) & ~gone
        stuffed = act & bs                              # protodec.c:996-1006
        stop_at[stuffed & (x == 1)] = i
        bs[stuffed] = False
        norm = act & ~stuffed                           # protodec.c:1008-1026
        run = norm & (x == last) & (x == 1)
        ant[run] += 1
        ant[norm & ~run] = 0
        five = run & (ant == 4)
        bs[five] = True
        ant[five] = 0
        idx = np.nonzero(norm)[0]
        buf[idx, pos[idx]] = x[idx]
        pos[idx] += 1
        gone |= norm & (pos >= limit)
        last = x.copy()                                 # protodec.c:1004 / 1119
    n = pos - 22
    formed = np.nonzero((stop_at == L) & ~gone & (n > min_bits) & (n % 8 == 0))[0]
    # protodec_calculate_crc(n') on each well-formed trial's buffer: protodec_sdlc_crc's bit loop, the trials side by side
    nbits = (n[formed] // 8 + 2) * 8
    B = buf[formed].astype(np.int64)
    crc = np.full(formed.size, 0xFFFF, dtype=np.int64)
    for k in range(int(nbits.max()) if formed.size else 0):
        nxt = np.where((crc ^ B[:, k]) & 1, (crc >> 1) ^ 0x8408, crc >> 1)
        crc = np.where(k < nbits, nxt, crc)
    out = [[] for _ in range(M)]
    for r in formed[(~crc & 0xFFFF) == 0x0F47]:
        assert crc_holds(buf[r], int(n[r]))
        out[r // T].append((int(r % T), int(n[r]), payload_of(buf[r], int(n[r]))))
    return out


def brute_force(raw, **k):
    return brute_force_many([raw], **k)[0]


def repair(raw, **k):
    """(number of passing trials, p, n', payload) -- the last three of the one trial when the number is 1, else None"""
    passing = brute_force(raw, **k)
    if len(passing) == 1:
        return (1,) + passing[0]
    return (len(passing), None, None, None)


def repairs(raws, group=8, **k):
    """repair() of many records, those of one length side by side"""
    raws = [np.asarray(r, dtype=np.uint8) for r in raws]
    out = [None] * len(raws)
    by_len = {}
    for i, r in enumerate(raws):
        by_len.setdefault(r.size, []).append(i)
    for idx in by_len.values():
        for j in range(0, len(idx), group):
            part = idx[j:j + group]
            for i, passing in zip(part, brute_force_many([raws[q] for q in part], **k)):
                out[i] = (1,) + passing[0] if len(passing) == 1 else (len(passing), None, None, None)
    return out


def candidate_raw(payload):
    """the raw bits D' records for a frame with this payload (any length): body + FCS with stuffing, then 0 and five 1s"""
    from gnuais_amd import synth
    return np.concatenate([synth.hdlc_frame_bits(bytes(payload))[32:-8], np.array([0, 1, 1, 1, 1, 1], dtype=np.uint8)])


def flipped(raw, p):
    out = np.array(raw, dtype=np.uint8)
    out[p] ^= 1
    out[p + 1] ^= 1
    return out


def decode_streams(bit_streams, seen=None, times=None):
    """RawLongDeframer over each channel's bits, then records_of(): (records, counters, the deframers)"""
    ds = []
    for c, bits in enumerate(bit_streams):
        d = RawLongDeframer(seen=0 if seen is None else int(seen[c]))
        d.feed(bits)
        ds.append(d)
    return records_of(ds, times) + (ds,)


def records_of(ds, times=None):
    """what these channels' RawLongDeframers closed, with the repair of what they count in `failed`: (records, counters
    [n][3]: delivered, failed, repaired).  The records are the good long frames and the repaired ones in (channel, 37-bit
    stamp) order.  times: optional callable(channel, frame) -> t"""
    cands = [(c, f) for c, d in enumerate(ds) for f in d.candidates()]
    got = repairs([f["raw"] for _, f in cands])
    out = []
    repaired = np.zeros(len(ds), dtype=np.int32)
    for c, d in enumerate(ds):
        for f in d.long_frames():
            out.append((c, f["end_bit"] & ((1 << 37) - 1), lr.record(c, f, -1 if times is None else times(c, f))))
    for (c, f), (k, p, n1, payload) in zip(cands, got):
        if k == 1:
            r = lr.record(c, dict(end_bit=f["end_bit"], n=n1, payload=payload), -1 if times is None else times(c, f))
            r["flags"] |= FRAME_REPAIRED
            out.append((c, f["end_bit"] & ((1 << 37) - 1), r))
            repaired[c] += 1
    out.sort(key=lambda r: (r[0], r[1]))
    counters = np.array([d.long_counters() + (int(repaired[c]),) for c, d in enumerate(ds)], dtype=np.int32).reshape(-1, 3)
    return np.array([r[2] for r in out], dtype=lr.LONG_FRAME_DTYPE), counters


def damaged_channel_bits(rng, c):
    """a channel's stream like long_ref.channel_bits: bursts of 53 .. 127 bytes, noise between them; a burst carries a
    symbol error, a single flipped bit, two symbol errors, or nothing"""
    sizes = [53, 54, 60, 100, 126, 127, 80]
    rng.shuffle(sizes)
    parts = []
    for k, nb in enumerate(sizes[: 3 + c % 4]):
        b = lr.burst(rng.integers(0, 256, nb, dtype=np.uint8)).copy()
        kind = (c + k) % 4
        lo, hi = 40, b.size - 12
        if kind == 0:
            p = int(rng.integers(lo, hi))
            b[p:p + 2] ^= 1
        elif kind == 1:
            b[int(rng.integers(lo, hi))] ^= 1
        elif kind == 2:
            p = int(rng.integers(lo, hi - 40))
            b[p:p + 2] ^= 1
            b[p + 30:p + 32] ^= 1
        parts += [rng.integers(0, 2, int(rng.integers(0, 40)), dtype=np.uint8), b]
    return np.concatenate(parts + [rng.integers(0, 2, 30, dtype=np.uint8)])
