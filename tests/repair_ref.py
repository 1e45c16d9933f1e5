"""Restatement of the single-symbol repair (include/gnuais_hip.h, gnuais_batch_repair) for the tests: a bit-by-bit
deframer that keeps the raw bits of every frame, and brute force over every trial p.

Deframer is protodec_decode() (src/protodec.c:988-1122) statement by statement, with one addition: the bits seen in
ST_DATA -- stuffed zeros included, the sixth 1 of the closing flag not -- are kept with the frame.  Its counters are
checked against the oracle's wherever it is used.

brute_force() runs ST_DATA of the same transcription over r' and one more 1 for EVERY p, bit by bit; numpy only carries
many trials side by side (one row per trial, one step of the machine per column).  Nothing here works on words, masks
of stuffed bits or CRC tables: those are the code under test."""
import numpy as np

ST_SKURR, ST_PREAMBLE, ST_STARTSIGN, ST_DATA, ST_STOPSIGN = 1, 2, 3, 4, 5
FRAME_REPAIRED = 0x40


def crc_holds(buffer, n):
    """protodec_calculate_crc(n) on d->buffer (protodec.c:120-167 with protodec_sdlc_crc, 106-118)"""
    buflen = n // 8 + 2
    crc = 0xFFFF
    for j in range(buflen):
        for i in range(8):
            k = i + 8 * j
            bit = int(buffer[k]) if k < len(buffer) else 0
            crc = (crc >> 1) ^ 0x8408 if (crc ^ bit) & 1 else crc >> 1
    return (~crc & 0xFFFF) == 0x0F47


def payload_of(buffer, n):
    """the n/8 payload bytes of a frame record: byte j = buffer[8j .. 8j+7], least significant first"""
    return bytes(sum(int(buffer[8 * j + i]) << i for i in range(8)) for j in range(n // 8))


class Deframer:
    """One channel's decoder.  closed: a dict per frame that reached ST_STOPSIGN's good branch (stop bit 0, length > 0):
    raw (uint8 bits), n, good, payload, end_bit (bits fed before the bit that closed it, all 37 and more)"""

    def __init__(self):
        self.received = self.lost = self.lost2 = 0
        self.seen = 0
        self.closed = []
        self.buffer = [0] * 450
        self.raw = []
        self.protodec_reset()

    def protodec_reset(self):
        self.state = ST_SKURR
        self.nstartsign = self.antallpreamble = self.antallenner = 0
        self.last = self.bitstuff = self.bufferpos = 0

    def feed(self, bits):
        for x in bits:
            x = int(x)
            s = self.state
            if s == ST_DATA:
                if self.bitstuff:
                    if x == 1:
                        self.state = ST_STOPSIGN
                        self.bitstuff = 0
                    else:
                        self.raw.append(0)
                        self.last = x
                        self.bitstuff = 0
                else:
                    if x == self.last and x == 1:
                        self.antallenner += 1
                        if self.antallenner == 4:
                            self.bitstuff = 1
                            self.antallenner = 0
                    else:
                        self.antallenner = 0
                    self.raw.append(x)
                    self.buffer[self.bufferpos] = x
                    self.bufferpos += 1
                    if self.bufferpos >= 449:
                        self.protodec_reset()
            elif s == ST_SKURR:
                if x != self.last:
                    self.antallpreamble += 1
                else:
                    self.antallpreamble = 0
                self.last = x
                if self.antallpreamble > 14 and x == 0:
                    self.state = ST_PREAMBLE
                    self.antallpreamble = 0
            elif s == ST_PREAMBLE:
                if x != self.last and self.nstartsign == 0:
                    self.antallpreamble += 1
                elif x == 1:
                    if self.nstartsign == 0:
                        self.nstartsign = 3
                        self.last = x
                    elif self.nstartsign == 5:
                        self.nstartsign += 1
                        self.antallpreamble = 0
                        self.state = ST_STARTSIGN
                    else:
                        self.nstartsign += 1
                elif self.nstartsign == 0:
                    self.nstartsign = 1
                else:
                    self.protodec_reset()
            elif s == ST_STARTSIGN:
                if self.nstartsign >= 7:
                    if x == 0:
                        self.state = ST_DATA
                        self.nstartsign = 0
                        self.antallenner = 0
                        self.buffer = [0] * 450
                        self.bufferpos = 0
                        self.raw = []
                    else:
                        self.protodec_reset()
                elif x == 0:
                    self.protodec_reset()
                self.nstartsign += 1
            elif s == ST_STOPSIGN:
                n = self.bufferpos - 6 - 16
                if x == 0 and n > 0:
                    good = crc_holds(self.buffer, n)
                    if good:
                        self.received += 1
                    else:
                        self.lost += 1
                    self.closed.append(dict(raw=np.array(self.raw, dtype=np.uint8), n=n, good=good,
                                            payload=payload_of(self.buffer, n), end_bit=self.seen))
                else:
                    self.lost2 += 1
                self.protodec_reset()
            self.last = x
            self.seen += 1


def brute_force_many(raws):
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
    gone = np.zeros(M * T, dtype=bool)                  # bufferpos reached 449: protodec_reset()
    buf = np.zeros((M * T, 450), dtype=np.uint8)
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
        gone |= norm & (pos >= 449)
        last = x.copy()                                 # protodec.c:1004 / 1119
    n = pos - 22
    formed = np.nonzero((stop_at == L) & ~gone & (n > 0) & (n % 8 == 0))[0]
    # protodec_calculate_crc(n') on each well-formed trial's buffer: protodec_sdlc_crc's bit loop (protodec.c:110-115),
    # the trials side by side
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


def brute_force(raw):
    """every trial p of one candidate: [(p, n', payload bytes)] of the trials that pass, ascending p"""
    return brute_force_many([raw])[0]


def repair(raw):
    """(number of passing trials, p, n', payload) -- the last three of the one trial when the number is 1, else None"""
    passing = brute_force(raw)
    if len(passing) == 1:
        return (1,) + passing[0]
    return (len(passing), None, None, None)


def record(channel, end_bit, n, payload, repaired=False):
    """the 64-byte frame record as a tuple of FRAME_DTYPE's fields"""
    pl = np.zeros(53, dtype=np.uint8)
    pl[: n // 8] = np.frombuffer(payload, dtype=np.uint8)[: n // 8]
    flags = 1 | (((end_bit >> 32) & 31) << 1) | (FRAME_REPAIRED if repaired else 0)
    return (channel, end_bit & 0xFFFFFFFF, pl, flags, n)


def decode_streams(bit_streams):
    """Deframer over each channel's bits.  Returns (frames, repairs, counters): frames = the good frames and the repaired
    ones as records in drain order (channel, end_bit); repairs [n_channels]; counters [n_channels][3]"""
    ds = []
    for bits in bit_streams:
        d = Deframer()
        d.feed(bits)
        ds.append(d)
    return records_of(ds)


def records_of(ds):
    """decode_streams() of channels whose Deframers have been fed already (in parts, a protodec_reset() between them)"""
    recs, failed, counters = [], [], []
    for c, d in enumerate(ds):
        for f in d.closed:
            if f["good"]:
                recs.append((c, f["end_bit"], record(c, f["end_bit"], f["n"], f["payload"])))
            else:
                failed.append((c, f))
        counters.append((d.received, d.lost, d.lost2))
    repaired = np.zeros(len(ds), dtype=np.int32)
    by_len = {}
    for c, f in failed:                                 # candidates of one length side by side (brute_force_many)
        by_len.setdefault(f["raw"].size, []).append((c, f))
    for group in by_len.values():
        for k in range(0, len(group), 32):
            part = group[k:k + 32]
            for (c, f), passing in zip(part, brute_force_many([f["raw"] for _, f in part])):
                if len(passing) == 1:
                    _, n1, pl = passing[0]
                    repaired[c] += 1
                    recs.append((c, f["end_bit"], record(c, f["end_bit"], n1, pl, repaired=True)))
    recs.sort(key=lambda r: (r[0], r[1]))
    return [r[2] for r in recs], repaired, np.array(counters, dtype=np.int32)


def candidate_raw(payload):
    """the raw bits the deframer records for a frame with this payload: body + FCS with stuffing, then 0 and five 1s"""
    from gnuais_amd import synth
    return np.concatenate([synth.hdlc_frame_bits(payload)[32:-8], np.array([0, 1, 1, 1, 1, 1], dtype=np.uint8)])
