"""What the REAL reference (oracle/_ref/libgnuais_ref.so) answers on the seeded inputs of the pin tests
(test_oracle_vs_ref.py, test_pll_cpu.py, test_deframer_cases_cpu.py and the *_vs_reference / *_against_reference tests of test_nmea.py,
test_range.py, test_vessels.py).  Where oracle/_ref is built the answers come from it, live; elsewhere from the copy that
tests/golden/make_golden.py stored in tests/golden/ref_pins.npz by calling these same functions.  The inputs are
made here as well, so the stored answers and the tests' inputs cannot drift apart."""
import os

import numpy as np

import cases
import deframer_cases
import message_cases
import pll_ref
from gnuais_amd import params, synth
from oracle_lib import have_reference, reference

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pins.npz")
MESSAGE_SWEEP = os.path.join(os.path.dirname(GOLDEN), "message_sweep.npz")      # a fixture of its own: it is large
FSM = ("state", "nstartsign", "antallpreamble", "antallenner", "bitstuff", "last", "bufferpos")
PINS = {}


def _bytes(b):
    return np.frombuffer(b, dtype=np.uint8).copy()


# ---------------------------------------------------------------- inputs

def signal_streams(seed):
    n = 20 * 1280
    return np.stack([synth.make_stream(n, seed=seed, channel=c, sigma=s)[0]
                     for c, s in enumerate((1000.0, 3000.0, 6000.0, 12000.0))], axis=1)


def noise_and_full_scale():
    rng = np.random.default_rng(4)
    x = np.stack([rng.normal(0, 3000, 60000), rng.integers(-32768, 32768, 60000),
                  rng.normal(0, 30, 60000)], axis=1)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def filter_input():
    rng = np.random.default_rng(6)
    return rng.integers(-32768, 32768, 9000).astype(np.int16)


FILTER_TAPS = (("48k", params.taps_48k), ("192k", params.taps_192k))
FILTER_CHUNKS = (1, 5, 1020, 4096)


def stream_192k():
    x, _ = synth.make_stream(8 * 5120, seed=8, channel=0, sps=20, sigma=2000.0, occupancy=0.7)
    return x[:, None]


def deframer_bitstreams():
    rng = np.random.default_rng(12)
    out = []
    for trial in range(6):
        parts = []
        for i in range(80):
            parts.append((rng.random(int(rng.integers(0, 120))) < rng.random()).astype(np.uint8))
            if rng.random() < 0.7:
                n = int(rng.choice([0, 1, 11, 21, 21, 40, 53, 54]))
                bits = synth.hdlc_frame_bits(bytes(rng.integers(0, 256, n, dtype=np.uint8)),
                                             training_bits=int(rng.integers(0, 40)))
                if rng.random() < 0.2:
                    bits[int(rng.integers(0, bits.size))] ^= 1
                parts.append(bits)
        out.append(np.concatenate(parts).astype(np.uint8))
    return out


def range_locations(seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(4):
        out.append((float(rng.uniform(-89.9, 89.9)), float(rng.uniform(-179.9, 179.9))))
    return out


PLL_PIN_COLUMNS = ("fast", "slow", "coin")


def pll_columns(pllinc):
    """[12000][3]: the two drift columns and the coin of pll_ref.columns(), for the pass-through table pll_ref.TAPS"""
    x = pll_ref.columns(12000, pllinc)
    return np.ascontiguousarray(x[:, [pll_ref.COLUMN_NAMES.index(n) for n in PLL_PIN_COLUMNS]])


# ---------------------------------------------------------------- the reference's answers

def _chain(x, taps=None, pllinc=0, chunk=1020, bits_of=0):
    ref = reference()
    n_ch = x.shape[1]
    ref.add_receivers(n_ch, taps=taps, pllinc=pllinc)
    ref.run_stream(x, chunk, capture_bits_of=bits_of)
    return {"taps": ref.taps(0), "bits": ref.bits(), "frames": _bytes(ref.frames().tobytes()),
            "counters": ref.counters(), "pll": np.array([ref.pll(c) for c in range(n_ch)], dtype=np.int64),
            "fsm": np.array([[ref.fsm(c)[k] for k in FSM] for c in range(n_ch)], dtype=np.int64)}


def _pll(pllinc):
    x = pll_columns(pllinc)
    out = {}
    for j in range(x.shape[1]):                 # one receiver at a time: the reference records one channel's bits
        r = _chain(x[:, j:j + 1], taps=pll_ref.TAPS, pllinc=pllinc)
        for k in ("bits", "frames", "counters", "pll", "fsm"):
            out["%s_%d" % (k, j)] = r[k]
    return out


def _taps():
    ref = reference()
    ref.add_receivers(1)
    return {"taps": ref.taps(0)}


def _filter_floats():
    x = filter_input()
    out = {}
    for name, taps in FILTER_TAPS:
        for chunk in FILTER_CHUNKS:
            f, _ = reference().filter_stream(taps(), x, 1, x.size, chunk)
            out["%s_%d" % (name, chunk)] = f
    return out


def _deframer():
    out = {}
    for i, bits in enumerate(deframer_bitstreams()):
        ref = reference()
        ref.add_receivers(1)
        ref.decode_bits(0, bits)
        out["frames_%d" % i] = _bytes(ref.frames().tobytes())
        out["counters_%d" % i] = ref.counters()
        out["fsm_%d" % i] = np.array([ref.fsm(0)[k] for k in FSM], dtype=np.int64)
    return out


def _deframer_boundaries():
    """the streams of tests/deframer_cases.py, each decoded whole by a fresh receiver"""
    out = {}
    for name in deframer_cases.NAMES:
        ref = reference()
        ref.add_receivers(1)
        ref.decode_bits(0, deframer_cases.STREAMS[name])
        out["frames_" + name] = _bytes(ref.frames().tobytes())
        out["counters_" + name] = ref.counters()
        out["fsm_" + name] = np.array([ref.fsm(0)[k] for k in FSM], dtype=np.int64)
    return out


def _stdout_text(seed):
    fr, n_ch = cases.nmea_frames(seed=seed, n_channels=4, n_random=1500)
    nm, seq, tx = reference().nmea_of_frames(fr, n_ch, stdout=True)
    return {"nmea": _bytes(nm), "seq": seq, "text": _bytes(tx)}


def _nmea(seed):
    fr, n_ch = cases.nmea_frames(seed=seed, n_channels=7, n_random=900)
    nm, seq = reference().nmea_of_frames(fr, n_ch)
    return {"nmea": _bytes(nm), "seq": seq}


def _range(seed):
    fr, n_ch = cases.range_frames(seed=100 + seed, n_random=300, own_channel=True)
    return {"range_%d" % i: reference().range_of_frames(fr, n_ch, lat, lon)
            for i, (lat, lon) in enumerate(range_locations(seed))}


def _vessels(seed, n_mmsi):
    fr, n_ch = cases.vessel_frames(seed=200 + seed, n=900, n_mmsi=n_mmsi)
    return {"table": _bytes(reference().cache_of_frames(fr, n_ch, pieces=[300, 301]).tobytes())}


def _message_sweep():
    """what the reference sends and prints for the frames of tests/message_cases.py, group after group"""
    nm, seq, tx = reference().nmea_of_frames(message_cases.everything(), message_cases.N_CH, stdout=True)
    return {"nmea": _bytes(nm), "seq": seq, "text": _bytes(tx)}


PINS["taps"] = _taps
for _s in (1, 2, 3):
    PINS["signal_streams_%d" % _s] = (lambda s: lambda: _chain(signal_streams(s), bits_of=s % 4))(_s)
PINS["noise_and_full_scale"] = lambda: _chain(noise_and_full_scale(), chunk=4096, bits_of=1)
PINS["filter_floats"] = _filter_floats
PINS["192k"] = lambda: _chain(stream_192k(), taps=params.taps_192k(), pllinc=params.PLLINC_192K, chunk=4096)
PINS["deframer"] = _deframer
PINS["deframer_boundaries"] = _deframer_boundaries
for _s in pll_ref.PLLINCS:
    PINS["pll_%d" % _s] = (lambda s: lambda: _pll(s))(_s)
for _s in (71, 72):
    PINS["stdout_text_%d" % _s] = (lambda s: lambda: _stdout_text(s))(_s)
for _s in (61, 62, 63):
    PINS["nmea_%d" % _s] = (lambda s: lambda: _nmea(s))(_s)
for _s in (5, 6):
    PINS["range_%d" % _s] = (lambda s: lambda: _range(s))(_s)
for _s, _n in ((7, 40), (8, 900)):
    PINS["vessels_%d_%d" % (_s, _n)] = (lambda s, n: lambda: _vessels(s, n))(_s, _n)


def want(key):
    """The reference's answer for one pin: live where oracle/_ref is built, else the stored copy."""
    if have_reference():
        return PINS[key]()
    with np.load(GOLDEN) as z:
        got = {k.split("/", 1)[1]: z[k] for k in z.files if k.split("/", 1)[0] == key}
    assert got, "no stored answer for %r in %s (re-run tests/golden/make_golden.py)" % (key, GOLDEN)
    return got


def want_message_sweep():
    """want()'s rule for the sweep of tests/message_cases.py, whose answer is stored in MESSAGE_SWEEP"""
    if have_reference():
        return _message_sweep()
    with np.load(MESSAGE_SWEEP) as z:
        return {k: z[k] for k in z.files}


def store():
    """tests/golden/make_golden.py: every pin's answer from the live reference into GOLDEN."""
    np.savez_compressed(GOLDEN, **{"%s/%s" % (k, n): v for k, fn in PINS.items() for n, v in fn().items()})


def store_message_sweep():
    np.savez_compressed(MESSAGE_SWEEP, **_message_sweep())
