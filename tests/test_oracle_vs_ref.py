"""Pins the CPU restatement (oracle/ais_oracle.c) against the REAL reference
objects (oracle/_ref/libgnuais_ref.so) on randomised, seeded inputs.  The reference's
answers come from oracle/_ref where it is built and otherwise from the copy stored in
tests/golden/ref_pins.npz (tests/ref_pins.py)."""
import numpy as np
import pytest

from gnuais_amd import params
from oracle_lib import Oracle
import ref_pins


def compare(key, x, pllinc=0, bits_of=0):
    want = ref_pins.want(key)
    n_ch = x.shape[1]
    o = Oracle(n_ch, taps=want["taps"], pllinc=pllinc)
    r = o.run(x, want_bits=True, want_filtered=True)
    assert np.array_equal(want["bits"], r["bits"][bits_of])
    assert want["frames"].tobytes() == o.frames().tobytes()
    assert np.array_equal(want["counters"], o.counters())
    for c in range(n_ch):
        assert tuple(want["pll"][c]) == o.pll(c)
        h = o.hdlc(c)
        assert all(h[k] == want["fsm"][c][i] for i, k in enumerate(ref_pins.FSM))
    return o, r


def test_taps_identical():
    assert np.array_equal(ref_pins.want("taps")["taps"].view(np.uint32), params.taps_48k().view(np.uint32))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_signal_streams(seed):
    o, r = compare("signal_streams_%d" % seed, ref_pins.signal_streams(seed), bits_of=seed % 4)
    assert o.counters()[:, 0].sum() > 10


def test_pure_noise_and_full_scale():
    compare("noise_and_full_scale", ref_pins.noise_and_full_scale(), bits_of=1)


def test_filter_floats_bit_equal_any_chunking():
    x = ref_pins.filter_input()
    want = ref_pins.want("filter_floats")
    for name, taps in ref_pins.FILTER_TAPS:
        for chunk in ref_pins.FILTER_CHUNKS:
            f = want["%s_%d" % (name, chunk)]
            o = Oracle(1, taps=taps())
            r = o.run(x[:, None], want_filtered=True)
            assert np.array_equal(f.view(np.uint32), r["filtered"][:, 0].view(np.uint32))


def test_192k_parameters():
    compare("192k", ref_pins.stream_192k(), pllinc=params.PLLINC_192K)


def test_deframer_random_bitstreams():
    want = ref_pins.want("deframer")
    for trial, bits in enumerate(ref_pins.deframer_bitstreams()):
        o = Oracle(1)
        o.decode_bits(0, bits)
        assert want["frames_%d" % trial].tobytes() == o.frames().tobytes()
        assert np.array_equal(want["counters_%d" % trial], o.counters())
        h = o.hdlc(0)
        assert all(h[k] == want["fsm_%d" % trial][i] for i, k in enumerate(ref_pins.FSM))
