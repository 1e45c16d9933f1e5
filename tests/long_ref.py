"""Restatement of the long-frame decoder D' (include/gnuais_hip.h, gnuais_batch_long_frames) for the tests.

LongDeframer is protodec_decode() / protodec_reset() / protodec_calculate_crc() (src/protodec.c:988-1122, 87-100, 106-167)
statement by statement, as repair_ref.Deframer is, with the two numbers D' changes as parameters: the give-up test
`bufferpos >= limit` and the size of the two buffers.  limit = 449, buffer = 450 is the reference's machine; limit = 1031,
buffer = 1200 is D'.  It works bit by bit: no word tricks, no tables.  What D' adds on top -- deliver only n > 426 with a
good CRC, count the long frames delivered and those that failed -- is read off `closed` (long_frames(), long_counters())."""
import numpy as np

from repair_ref import ST_DATA, ST_PREAMBLE, ST_SKURR, ST_STARTSIGN, ST_STOPSIGN, crc_holds, payload_of

LONG_MAX_BITS = 1008
LONG_LIMIT = LONG_MAX_BITS + 22 + 1
LONG_BUFFER = 1200
SHORT_BITS = 426            # a frame of at most this many bits belongs to the chain's decoder

LONG_FRAME_DTYPE = np.dtype([("channel", "<u4"), ("end_bit", "<u4"), ("t", "<i8"), ("nbits", "<u2"), ("flags", "u1"),
                             ("reserved", "u1"), ("payload", "u1", (132,))])
assert LONG_FRAME_DTYPE.itemsize == 152


class LongDeframer:
    """One channel's decoder.  closed: a dict per frame that reached ST_STOPSIGN's good branch (stop bit 0, length > 0):
    n, good, payload, end_bit (bits fed before the bit that closed it: every bit of the count), index (how many bits this
    object had been fed before that bit, whatever `seen` started at)"""

    def __init__(self, limit=LONG_LIMIT, buffer=LONG_BUFFER, seen=0):
        self.limit, self.buflen = limit, buffer
        self.received = self.lost = self.lost2 = 0
        self.seen = seen
        self.fed = 0
        self.closed = []
        self.buffer = [0] * buffer
        self.protodec_reset()

    def protodec_reset(self):
        self.state = ST_SKURR
        self.nstartsign = self.antallpreamble = self.antallenner = 0
        self.last = self.bitstuff = self.bufferpos = 0

    def fields(self):
        """the live fields as gnuais_fsm_state reports them (antallpreamble saturated at 15)"""
        return (self.state, self.nstartsign, min(self.antallpreamble, 15), self.antallenner, self.bitstuff, self.last,
                self.bufferpos)

    def feed(self, bits, states=None):
        """states: a list that receives fields() BEFORE every bit"""
        for x in bits:
            x = int(x)
            if states is not None:
                states.append(self.fields())
            s = self.state
            if s == ST_DATA:
                if self.bitstuff:
                    if x == 1:
                        self.state = ST_STOPSIGN
                        self.bitstuff = 0
                    else:
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
                    self.buffer[self.bufferpos] = x
                    self.bufferpos += 1
                    if self.bufferpos >= self.limit:
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
                        self.buffer = [0] * self.buflen
                        self.bufferpos = 0
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
                    self.closed.append(dict(n=n, good=good, payload=payload_of(self.buffer, n), end_bit=self.seen,
                                            index=self.fed))
                else:
                    self.lost2 += 1
                self.protodec_reset()
            self.last = x
            self.seen += 1
            self.fed += 1

    # ---- what D' makes of it ------------------------------------------------------------------------------------------
    def long_frames(self):
        return [f for f in self.closed if f["n"] > SHORT_BITS and f["good"]]

    def long_counters(self):
        """(long frames delivered, long frames that failed the CRC)"""
        return (sum(1 for f in self.closed if f["n"] > SHORT_BITS and f["good"]),
                sum(1 for f in self.closed if f["n"] > SHORT_BITS and not f["good"]))


class SampleRef:
    """the restatement behind the samples: the oracle's slices segment by segment into one LongDeframer per channel, and
    the definition's t from where each closing bit lies"""

    def __init__(self, n_ch, rows=0, bits=None):
        from oracle_lib import Oracle
        self.o = Oracle(n_ch)
        self.n = rows
        self.ds = [LongDeframer(seen=0 if bits is None else int(bits[c])) for c in range(n_ch)]
        self.segs = [[] for _ in range(n_ch)]               # per channel: (bits fed before, first row, rows, bits)

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


def record(channel, f, t=-1):
    """the 152-byte record of a closed frame as a LONG_FRAME_DTYPE scalar"""
    r = np.zeros((), dtype=LONG_FRAME_DTYPE)
    r["channel"] = channel
    r["end_bit"] = f["end_bit"] & 0xFFFFFFFF
    r["t"] = t
    r["nbits"] = f["n"]
    r["flags"] = 1 | (((f["end_bit"] >> 32) & 31) << 1)
    r["payload"][: f["n"] // 8] = np.frombuffer(f["payload"], dtype=np.uint8)[: f["n"] // 8]
    return r


def records(deframers, times=None):
    """the drain of these channels' decoders: their long frames in (channel, 37-bit stamp) order.  times: optional
    callable(channel, frame) -> t"""
    out = []
    for c, d in enumerate(deframers):
        for f in d.long_frames():
            out.append((c, f["end_bit"] & ((1 << 37) - 1), record(c, f, -1 if times is None else times(c, f))))
    out.sort(key=lambda r: (r[0], r[1]))
    return np.array([r[2] for r in out], dtype=LONG_FRAME_DTYPE)


def burst(payload, training_bits=24):
    """the on-air bits of one burst with this payload (any length): gnuais_amd.synth.hdlc_frame_bits"""
    from gnuais_amd import synth
    return synth.hdlc_frame_bits(bytes(payload), training_bits=training_bits)


LONG_BYTES = (54, 60, 80, 100, 126, 127, 53, 21)    # payload sizes of the seed-9 stream, one burst every six slots


def long_payloads(sizes=LONG_BYTES, every=6):
    """make_stream's `payloads`: slot every*k carries a random payload of sizes[k] bytes.  The bytes come from a
    generator of their own, seeded by the length: whether the modem carries a burst depends on its content (the 80-byte
    burst drawn from the stream's own generator at seed 9 is lost in front of the deframer at either sigma), and these
    tests are about the deframer"""
    def pick(rng, slot):
        if slot % every or slot // every >= len(sizes):
            return None
        n = sizes[slot // every]
        return bytes(np.random.default_rng([9, n]).integers(0, 256, n, dtype=np.uint8))
    return pick


def channel_bits(rng, c):
    """a channel's stream: bursts of 53 .. 127 bytes in an order of its own, noise between them, now and then a long
    frame with a flipped bit (fails the CRC) and a run the machine gives up on"""
    sizes = [53, 54, 55, 60, 100, 126, 127]
    rng.shuffle(sizes)
    parts = []
    for k, nb in enumerate(sizes[: 3 + c % 4]):
        b = burst(rng.integers(0, 256, nb, dtype=np.uint8))
        if (c + k) % 5 == 0:
            b = b.copy()
            b[40 + int(rng.integers(0, 300))] ^= 1
        parts += [rng.integers(0, 2, int(rng.integers(0, 40)), dtype=np.uint8), b]
    return np.concatenate(parts + [rng.integers(0, 2, 30, dtype=np.uint8)])


# ---- the sentences of a long frame ----------------------------------------------------------------------------------------
def henten(rbuffer, pos, count):
    """protodec_henten(): `count` bits from `pos`, most significant first"""
    v = 0
    for i in range(pos, pos + count):
        v = (v << 1) | rbuffer[i]
    return v


def ref_sentences(payload, nbits, seq):
    """protodec_getdata()'s head and protodec_generate_nmea() (src/protodec.c:896-926, 780-893) on one frame, statement by
    statement: (the bytes serial_write() gets, the sequence digit afterwards).  d->rbuffer: the nbits/8 whole bytes, most
    significant bit first, zeros behind (protodec_calculate_crc clears it and fills in whole bytes)."""
    rbuffer = [0] * 1300
    for j in range(nbits // 8):
        for i in range(8):
            rbuffer[8 * j + i] = (payload[j] >> (7 - i)) & 1
    typ = henten(rbuffer, 0, 6)
    if typ < 1 or typ > 24:
        return b"", seq
    bufferlen, fillbits = nbits, 0
    if bufferlen % 6 > 0:
        fillbits = 6 - bufferlen % 6
        for k in range(bufferlen, bufferlen + fillbits):
            rbuffer[k] = 0
        bufferlen += fillbits
    out = b""
    senlen = 61
    if bufferlen <= senlen * 6:
        sentences = 1
    else:
        sentences = bufferlen // (senlen * 6)
        if bufferlen % (senlen * 6) != 0:
            sentences += 1
    sentencenum, pos = 0, 0
    while True:
        nmea = [0] * 100
        k = 13
        while k < senlen + 13 and bufferlen > pos:
            letter = henten(rbuffer, pos, 6)
            letter = letter + 48 if letter < 40 else letter + 56
            nmea[k] = letter
            pos += 6
            k += 1
        nmea[k:k + 6] = [44, 48, 42, 48, 48, 0]
        sentencenum += 1
        nmea[0:10] = [65, 73, 86, 68, 77, 44, 48 + sentences, 44, 48 + sentencenum, 44]
        if sentences > 1:
            nmea[10:13] = [seq + 48, 44, 44]
            if sentencenum == sentences:
                nmea[k + 1] = 48 + fillbits
        else:
            nmea[10:13] = [44, 65, 44]
        chk = nmea[0]
        m = 1
        while nmea[m] != 42:
            chk ^= nmea[m]
            m += 1
        nchk = "%X" % chk
        if len(nchk) == 1:
            nmea[k + 4] = ord(nchk[0])
        else:
            nmea[k + 3], nmea[k + 4] = ord(nchk[0]), ord(nchk[1])
        out += b"!" + bytes(nmea[:nmea.index(0)]) + b"\r\n"
        if sentencenum >= sentences:
            break
    seq += 1
    if seq > 9:
        seq = 0
    return out, seq
