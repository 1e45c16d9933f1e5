"""The long frames' signal records and cover on the CPU (gnuais_batch_long_frame_signal): the figures of the base input
LS9 on the restatement tests/long_signal_ref.py -- so the GPU tests, which compare against it, cannot pass on empty
inputs -- the host object's entry with records, gnuais_long_uniq_push_heard_signal, against heard_ref; and the build's
own declarations."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import heard_ref as hr
import long_signal_ref as lsr
import long_unique_ref as lur
import occupancy_ref as orf
from gnuais_amd.lib import HEARER_DTYPE, LONG_FRAME_DTYPE, SIGNAL_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuais_amd", "csrc")


@pytest.fixture(scope="module")
def LongUniq():
    so = os.path.join(ROOT, "gnuais_amd", "libgnuais_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-s", "-j8", "-C", CSRC])
    from gnuais_amd.receiver import LongUniq
    return LongUniq


def test_ls9_ten_long_records_all_measured_four_short_frames():
    r = lsr.ls9_restated()
    rec, sig = r["long"], r["long_sig"]
    print("long nbits", rec["nbits"].tolist(), "t", rec["t"].tolist(), "blocks", sig["blocks"].tolist(), "short", len(r["short"]))
    assert int((sig["blocks"] > 0).sum()) >= 8
    assert rec["nbits"].tolist() == [432, 480, 640, 800, 1008] * 2 and rec["channel"].tolist() == [0] * 5 + [1] * 5
    assert sig["blocks"].tolist() == [35, 39, 51, 63, 79] * 2 and np.all(sig["power"] > 0)
    assert len(r["short"]) == 4 and np.all(r["short_sig"]["blocks"] > 0)
    # 10 log10((A^2 + 2 sigma^2) / 2^31): the level the bursts were made at
    want_db = 10 * np.log10((1e8 + 2 * 800.0 ** 2) / 2 ** 31)
    assert np.all(np.abs(10 * np.log10(sig["power"] / 2.0 ** 31) - want_db) < 0.3)


def test_ls9_lag_epochs_and_cover_with_and_without_the_long_frames():
    """LAG 5562 rows against 2762; 13 final epochs at E = 64; the four short frames alone cover 78 of their 840 busy blocks,
    with the ten long frames' cover spans 588"""
    assert lsr.lag() == 5562 and lsr.lag(max_bits=448) == orf.lag(0x10000 // 5) == 2762
    r = lsr.ls9_restated()
    with_long = lsr.ls9_epochs(True)
    assert len(with_long) == (lsr.LS9_ROWS - lsr.lag()) // 4096 == 13
    # the same epochs with the short frames' cover only
    occ = lsr.LongOccupancyRef(2, 64, 16)
    for a, e in lsr.ragged(lsr.LS9_ROWS):
        occ.run_iq(a, lsr.ls9()[a:e])
    occ.add_frames(r["short"], r["short_t"])
    short_only = occ.epochs()
    busy = sum(int(e[1]["busy"].sum()) for e in with_long)
    cov_long = sum(int(e[1]["covered"].sum()) for e in with_long)
    cov_short = sum(int(e[1]["covered"].sum()) for e in short_only)
    print("busy", busy, "covered without", cov_short, "with", cov_long)
    assert [e[0] for e in short_only] == [e[0] for e in with_long] and busy == sum(int(e[1]["busy"].sum()) for e in short_only)
    assert (busy, cov_short, cov_long) == (840, 78, 588) and cov_long >= 4 * cov_short
    # the feature off: occupancy_ref's own LAG, one epoch more
    assert len(lsr.ls9_epochs(False)) == (lsr.LS9_ROWS - 2762) // 4096 == 14


def test_ls9_the_first_burst_is_measured_but_covers_nothing():
    r = lsr.ls9_restated()
    first = r["long"][0]
    assert first["t"] == 2535 and r["long_sig"][0]["blocks"] == 35
    q = int(first["t"]) - 18
    lo = q - (432 + 24) * 65536 // (0x10000 // 5) - orf.pre_rows(0x10000 // 5)
    assert lo == -83 and orf.cover_span(int(first["t"]), 432, 0x10000 // 5) == (0, 0)
    assert orf.cover_span(int(r["long"][1]["t"]), 480, 0x10000 // 5)[1] > 0


def test_long_occupancy_ref_with_448_bits_is_occupancy_ref():
    r = lsr.ls9_restated()
    a, b = lsr.LongOccupancyRef(2, 64, 16, max_bits=448), orf.OccupancyRef(2, 64, 16)
    for o in (a, b):
        o.run_iq(0, lsr.ls9())
        o.add_frames(r["short"], r["short_t"])
    ea, eb = a.epochs(), b.epochs()
    assert len(ea) == len(eb) == 14
    for x, y in zip(ea, eb):
        assert x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and np.array_equal(x[2], y[2])


def test_push_heard_signal_equals_the_restatement_and_null_equals_push_heard(LongUniq):
    """60 random sets cut into random drains, every record with a random signal record: lists, records, copies and late
    are heard_ref's byte for byte; with signal = NULL the new entry is gnuais_long_uniq_push_heard byte for byte"""
    from gnuais_amd import lib as L
    handle = L.load()
    rng = np.random.default_rng(77)
    n_members = 0
    for s, (W, drains) in enumerate(lur.random_cases(3031, n_sets=60)):
        u, v, null = LongUniq(W), LongUniq(W), LongUniq(W)
        r = hr.HeardRef(W)
        for f, rows in drains:
            sig = np.zeros(len(f), dtype=SIGNAL_DTYPE)
            sig["power"] = rng.integers(0, 2 ** 32, len(f), dtype=np.uint64)
            sig["ferr"] = rng.integers(-32768, 32768, len(f))
            sig["blocks"] = rng.integers(0, 400, len(f))
            got = u.push_heard(f, rows, signal=sig)
            wf, _, wc, wfirst, wmem = r.push_heard(f, f["t"], rows, sig)
            assert got[0].tobytes() == wf.tobytes() and np.array_equal(got[1], wc) and np.array_equal(got[2], wfirst), s
            assert got[3].dtype == HEARER_DTYPE and got[3].tobytes() == wmem.tobytes(), s
            assert u.late() == r.late
            n_members += len(wmem)
            # NULL through the new entry against the old entry
            old = v.push_heard(f, rows)
            fr = np.ascontiguousarray(f, dtype=LONG_FRAME_DTYPE)
            n = len(fr)
            out, oc = np.zeros(max(n, 1), dtype=LONG_FRAME_DTYPE), np.zeros(max(n, 1), dtype=np.int32)
            first, mem = np.zeros(n + 1, dtype=np.int32), np.zeros(max(n, 1), dtype=HEARER_DTYPE)
            k, nm = C.c_int(), C.c_int()
            assert handle.gnuais_long_uniq_push_heard_signal(null._h, fr.ctypes.data, None, n, int(rows), out.ctypes.data,
                                                             oc.ctypes.data, n, C.byref(k), first.ctypes.data,
                                                             mem.ctypes.data, C.byref(nm)) == L.OK
            assert out[:k.value].tobytes() == old[0].tobytes() and np.array_equal(oc[:k.value], old[1])
            assert np.array_equal(first[:k.value + 1], old[2]) and mem[:nm.value].tobytes() == old[3].tobytes()
            assert null.late() == v.late()
        for q in (u, v, null):
            q.close()
    assert n_members > 500


def test_push_heard_signal_refuses_what_push_heard_refuses(LongUniq):
    from gnuais_amd import lib as L
    handle = L.load()
    u = LongUniq(5)
    fr = np.zeros(1, dtype=LONG_FRAME_DTYPE)
    k = C.c_int()
    assert handle.gnuais_long_uniq_push_heard_signal(u._h, fr.ctypes.data, None, 1, 10, fr.ctypes.data, None, 1, C.byref(k),
                                                     None, None, None) == L.E_ARG
    u.close()


def test_symbols_declared_exported_bound_and_the_kernel_is_in_the_builds_resource_check():
    from gnuais_amd import lib as L
    from gnuais_amd.receiver import ReceiverBatch
    from gnuais_amd.shard import ReceiverNode
    header = open(os.path.join(ROOT, "include", "gnuais_hip.h")).read()
    for name in ("gnuais_batch_long_frame_signal", "gnuais_batch_drain_long_frames_signal", "gnuais_long_uniq_push_heard_signal",
                 "gnuais_node_long_frame_signal", "gnuais_node_drain_long_frames_signal"):
        assert name + "(" in header and name in L.SYMBOLS, name
    assert "no signal record" not in header
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(BUILD)/long_signal.o" in mk.split("all:")[0] and "long_signal.s long_signal_kernel" in mk
    assert "launch_long_signal" in open(os.path.join(CSRC, "kernels.h")).read()
    for m in ("long_frame_signal", "drain_long_frames_signal"):
        assert callable(getattr(ReceiverBatch, m)) and callable(getattr(ReceiverNode, m)), m
