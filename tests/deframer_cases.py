"""The deframer's boundary cases (TEST INFRASTRUCTURE, plain numpy: shared by tests/test_deframer_cases_cpu.py, the pins
of tests/ref_pins.py and tests/test_deframer_boundaries_gpu.py).

STREAMS: short single-channel bit streams (at most about 610 bits), each built around one thing protodec_decode()
(src/protodec.c:988-1122) does -- the 15th alternation, the flag's 1s, the stuffed 0, the sixth 1, the bit after the
closing flag, the 449-bit limit.  The split plans below cut every stream at EVERY position, so each of those events
falls on each side of a boundary between two decode_bits calls (single_splits), around a piece shorter than 8 bits
(double_splits), and on each side of a pack boundary inside one call (padded).  What the plans reach is measured on the
CPU restatement in tests/test_deframer_cases_cpu.py."""
import numpy as np

from gnuais_amd import synth

SEED = 6          # one whose `dense` blocks hold no six 1s in a row (COUNTERS below; with seed 5 one does)
FLAG = np.array([0, 1, 1, 1, 1, 1, 1, 0], dtype=np.uint8)


def _alt(n):
    return (np.arange(n) & 1).astype(np.uint8)          # 0101...


def _cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts]).astype(np.uint8)


def _no_five_ones(data):
    """the bits with a 0 wherever a fifth 1 in a row would stand: nothing in them is stuffed or closes a frame"""
    data = np.array(data, dtype=np.uint8)
    for i in range(4, data.size):
        if data[i - 4:i].all():
            data[i] = 0
    return data


def _build():
    rng = np.random.default_rng(SEED)

    def body(n):
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))

    s = {}
    s["good21_twice"] = _cat(synth.hdlc_frame_bits(body(21)), np.zeros(6), synth.hdlc_frame_bits(body(21)))
    s["ff_stuffed"] = synth.hdlc_frame_bits(b"\xff" * 11)            # a stuffed 0 after every five 1s
    s["max53"] = synth.hdlc_frame_bits(body(53))                     # the longest frame that fits
    s["ff53"] = synth.hdlc_frame_bits(b"\xff" * 53)                  # ... and the longest raw record
    s["over55"] = _cat(synth.hdlc_frame_bits(body(55)), synth.hdlc_frame_bits(body(5)))    # bufferpos reaches 449
    s["ff55"] = synth.hdlc_frame_bits(b"\xff" * 55)                  # ... with stuffed 0s among the bits counted
    s["unstuffed_ones"] = synth.hdlc_frame_bits(b"\xff" * 4, stuff=False)                  # six 1s arrive early
    for n in range(13, 19):                                          # both sides of antallpreamble > 14
        data = _no_five_ones(rng.integers(0, 2, 30))
        s["train%d" % n] = _cat(_alt(n), FLAG, data, FLAG)
    # 0 and seven 1s: given up in ST_STARTSIGN; a flag that ends after its fifth 1: given up while its 1s are counted
    s["seven_ones"] = _cat(_alt(16), [0], np.ones(7), _alt(16), FLAG[:6], synth.hdlc_frame_bits(body(3)))
    # a 1 where the closing flag's last 0 belongs: lostframes2; a frame of one byte, then 1, 0, 0
    good = synth.hdlc_frame_bits(body(21))
    s["stop_then_one"] = _cat(good[:-1], [1], synth.hdlc_frame_bits(body(1)), [1, 0, 0])
    # both sides of bufferpos - 22 > 0 (protodec.c:1097)
    s["short_frames"] = _cat(*[_cat(_alt(16), FLAG, np.zeros(n), FLAG) for n in (0, 1, 15, 16, 17, 23, 24)])
    s["dense"] = _cat(*[_cat(_alt(16), FLAG, (rng.random(30) < 0.4), FLAG) for _ in range(6)])
    bad = synth.hdlc_frame_bits(body(21))
    bad[24 + 8 + 40] ^= 1                                            # one data bit
    s["crc_bad"] = bad
    s["flags_back_to_back"] = _cat(_alt(24), np.tile(FLAG, 5))
    return s


STREAMS = _build()
NAMES = tuple(STREAMS)

# (receivedframes, lostframes, lostframes2) of each stream decoded alone
COUNTERS = {
    "good21_twice": [2, 0, 0], "ff_stuffed": [1, 0, 0], "max53": [1, 0, 0], "ff53": [1, 0, 0], "over55": [1, 0, 0],
    "unstuffed_ones": [0, 0, 1], "train13": [0, 0, 0], "train14": [0, 0, 0], "train15": [0, 0, 0], "train16": [0, 1, 0],
    "train17": [0, 1, 0], "train18": [0, 1, 0], "seven_ones": [1, 0, 0], "stop_then_one": [1, 0, 1],
    "short_frames": [2, 1, 4], "dense": [0, 6, 0], "crc_bad": [0, 1, 0], "flags_back_to_back": [0, 0, 1], "ff55": [0, 0, 0],
}


# ---------------------------------------------------------------- split plans

def single_splits():
    """(name, i) for every stream and every i in 0 .. len: s[:i] in one call, s[i:] in the next"""
    for name in NAMES:
        for i in range(STREAMS[name].size + 1):
            yield name, i


def double_splits():
    """(name, i, g) for every i and g = 1 .. 8: s[:i], s[i:i+g], s[i+g:] -- the middle piece is a pack shorter than 8 bits"""
    for name in NAMES:
        for i in range(STREAMS[name].size + 1):
            for g in range(1, 9):
                yield name, i, g


def padded(pack_bits):
    """(name, p) for p = 0 .. pack_bits-1: zeros(p) + s in ONE call, a pack boundary inside the launch at every position"""
    for name in NAMES:
        for p in range(pack_bits):
            yield name, p


def single_pieces():
    """per channel (one per split): the list of pieces its calls feed, call by call"""
    return [[STREAMS[n][:i], STREAMS[n][i:]] for n, i in single_splits()]


def double_pieces():
    return [[STREAMS[n][:i], STREAMS[n][i:i + g], STREAMS[n][i + g:]] for n, i, g in double_splits()]


def padded_pieces(pack_bits):
    return [[_cat(np.zeros(p), STREAMS[n])] for n, p in padded(pack_bits)]


# ---------------------------------------------------------------- pack sizes

def pack_words(pllinc):
    """words of a segment's bit pack, as gnuais_batch_create() derives them from the clock increment"""
    p = pllinc if pllinc else 0x10000 // 5
    return ((2048 * (p + p // 16) >> 16) + 33) // 32 + 1


# clock increment -> bits per pack (info("pack_bits")): the smallest and the largest pack create() accepts, the first
# increment of the second smallest, the default
PACK_BITS = {1: 64, 934: 96, 0: 480, 14426: 512}
PLLINC_OF_PACK = {v: k for k, v in PACK_BITS.items()}
