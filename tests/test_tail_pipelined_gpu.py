"""Every stage queued behind the CRC stage, with calls in flight: the repair, the frames' times, their signal records, the
occupancy tail, D' and the long repair together on one batch, fed through run_iq(..., sync=False) on one caller stream
with nothing that synchronises until the last call is queued.  Every result is compared byte for byte with the
restatements (tests/tail_cases.py puts them together; tests/test_tail_cases_cpu.py shows that they are not empty), and a
twin batch with every feature off gets the same calls: its chain state must be the same.

All of the stages combine on one drain-type batch, the two duplicate merges with their heard lists included; the library
refused no combination.  A heard drain takes the frames the plain drain would take, so a case delivers one way or the
other (`heard`).

Calls in flight.  On 70 channels the device finishes a call before the host has queued the next.  So a chain of
BLOCKER_MATMULS products of 4096 x 4096 floats is queued on the caller's stream in front of the first call, and an event
behind it; once min(nbuf - 1, calls) calls are queued the event must not have fired: those calls were queued while the
device had begun none of them.  Measured on the MI355X: the queuing loop takes the host 0.11 to 0.31 ms for one or two
calls (nbuf = 2, 3) and 0.49 to 0.55 ms for seven (nbuf = 8); the blocker runs for 10.9 ms, twenty times the longest.
A second blocker stands in front of the last call, so that the first read-out, which has to wait by itself, has something
to wait for; which read-out comes first turns with the case.  (That the second blocker is still running when the last
call is queued is not asserted: with nbuf = 2 or 3 the host waits inside that call for the tail of an earlier one, and on
the MI355X that wait outlasted the blocker in the four cases with K3 on the deframer's stream.)

K3 on a stream of its own (GNUAIS_K3_SAME=0, read when the batch is created) is the topology in which the next deframer
launch waits for e_done[4] of the call before; nbuf = 2 on the plan of 48 equal calls takes each hand-off set 24 times."""
import time

import numpy as np
import pytest

import iq_ref
import tail_cases as tc
from test_iq_gpu import dev

pytestmark = pytest.mark.gpu
DEFAULT_NBUF = 3
BLOCKER_N, BLOCKER_MATMULS = 4096, 12
READ_OUTS = ["frames", "repaired", "long", "long_counters", "long_repaired", "long_fsm", "occupancy", "occupancy_lost",
             "counters", "fsm", "pll"]
_STATE = {}


def blocker():
    """a plain finite kernel sequence on the current stream: -> the event recorded behind it"""
    import torch
    if "a" not in _STATE:
        _STATE["a"] = torch.eye(BLOCKER_N, device="cuda") * 0.5
        _STATE["x"] = torch.ones(BLOCKER_N, BLOCKER_N, device="cuda")
    y = _STATE["x"]
    for _ in range(BLOCKER_MATMULS):
        y = y @ _STATE["a"]
    ev = torch.cuda.Event()
    ev.record()
    return ev


@pytest.fixture(scope="module")
def xd():
    """the input on the device, and everything loaded that a first use loads: the library's kernels, the matmul's"""
    import torch
    x = dev(np.array(tc.iq_input()))                     # (a copy: the shared input is read-only)
    b = make_batch({}, heard=True)
    b.run_iq(x[:2048])
    blocker()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = blocker()
    ev.synchronize()
    print(f"blocker: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    return x


def make_batch(opts, features=True, heard=False):
    from gnuais_amd import ReceiverBatch
    b = ReceiverBatch(tc.N_CH, max_len=tc.MAX_LEN)
    for k, v in opts.items():                               # nbuf first: the signal ring and the occupancy rings are sized by it
        b.set_option(k, v)
    if features:
        b.repair(True)
        b.frame_times(True)
        b.frame_signal(True)
        b.occupancy(tc.E, tc.MARGIN)
        b.long_frames(True)
        b.long_repair(True)
        if heard:
            b.unique(tc.UNIQUE_W)
            b.long_unique(tc.UNIQUE_W)
    return b


def queue(b, xd, calls, depth, last_blocker=True):
    """the calls, unsynchronised, behind a blocker; `depth` calls must be queued before the device begins the first"""
    t0 = time.perf_counter()
    for i, (lo, hi) in enumerate(calls):
        if i == 0:
            ev = blocker()
            t0 = time.perf_counter()
        if last_blocker and i == len(calls) - 1 and i > 0:
            blocker()                                       # the read-out that follows has something to wait for
        b.run_iq(xd[lo:hi], sync=False)
        if i + 1 == min(depth, len(calls)):
            host_ms = (time.perf_counter() - t0) * 1e3
            assert not ev.query(), f"the device began before {depth} calls were queued ({host_ms:.2f} ms)"
            print(f"queued {depth} calls in {host_ms:.2f} ms")


def read_all(b, first, heard):
    """every read-out once, READ_OUTS[first] first"""
    take = {
        "frames": b.drain_frames_heard if heard else b.drain_frames_signal,
        "repaired": b.repaired,
        "long": b.drain_long_frames_heard if heard else b.drain_long_frames,
        "long_counters": b.long_counters,
        "long_repaired": b.long_repaired,
        "long_fsm": b.long_fsm_state,
        "occupancy": b.drain_occupancy,
        "occupancy_lost": b.occupancy_lost,
        "counters": b.counters,
        "fsm": b.fsm_state,
        "pll": b.pll_state,
    }
    order = READ_OUTS[first % len(READ_OUTS):] + READ_OUTS[:first % len(READ_OUTS)]
    return {name: take[name]() for name in order}


def counters3(cnt):
    return np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]], axis=1)


def same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g.dtype.itemsize == w.dtype.itemsize and g.tobytes() == w.tobytes(), (len(g), len(w))


def check(b, off, e, first, heard, rows):
    got = read_all(b, first, heard)
    if heard:
        want_short, want_long = tc.heard(e, rows)
        same(got["frames"], want_short)
        same(got["long"], want_long)
    else:
        same(got["frames"], (e.frames, e.times, e.signal))
        assert got["long"].tobytes() == e.long_records.tobytes(), (len(got["long"]), len(e.long_records))
    assert np.array_equal(got["repaired"], e.repaired)
    d, f = got["long_counters"]
    assert np.array_equal(np.stack([d, f, got["long_repaired"]], axis=1), e.long_counters3)
    assert [tuple(int(v) for v in r) for r in got["long_fsm"]] == e.long_fsm
    occ_first, occ_rec = got["occupancy"]
    assert occ_first.tolist() == e.occ_first and got["occupancy_lost"] == 0
    for k, want in enumerate(e.occ_records):
        assert occ_rec[k].tobytes() == want.tobytes(), (k, np.argwhere(occ_rec[k] != want)[:5])
    assert np.array_equal(counters3(got["counters"]), e.counters)
    assert int(b.info("rows")) == rows and b.pending_frames() == 0 and b.pending_long_frames() == 0
    # the chain did not notice: the twin with every feature off
    assert got["counters"].tobytes() == off.counters().tobytes()
    assert got["fsm"].tobytes() == off.fsm_state().tobytes() and got["pll"].tobytes() == off.pll_state().tobytes()
    plain = e.frames[(e.frames["flags"] & 0x40) == 0]
    assert off.drain_frames().tobytes() == plain.tobytes()


def options(nbuf, pipeline, variant, lpw, pll):
    opts = {} if nbuf is None else {"nbuf": nbuf}
    opts.update(pipeline=pipeline, hdlc_variant=variant, hdlc_lpw=lpw, pll_variant=pll)
    return opts


def k3(monkeypatch, same_stream):
    if same_stream is None:
        monkeypatch.delenv("GNUAIS_K3_SAME", raising=False)
    else:
        monkeypatch.setenv("GNUAIS_K3_SAME", same_stream)


# plan, nbuf, pipeline, GNUAIS_K3_SAME, hdlc_variant, hdlc_lpw, pll_variant, heard
CASES = [
    ("ragged", 2, 1, "0", 0, 8, 7, False),
    ("equal", 2, 1, "0", 1, 64, 8, False),
    ("ragged", None, 1, None, 1, 64, 8, False),
    ("equal", 8, 1, None, 0, 8, 7, False),
    ("ragged", 8, 1, "0", 0, 64, 7, True),
    ("equal", None, 1, "0", 1, 8, 8, False),
    ("ragged", 2, 0, None, 0, 8, 8, False),
    ("equal", 2, 1, None, 1, 8, 7, True),
]


@pytest.mark.parametrize("plan,nbuf,pipeline,k3_same,variant,lpw,pll,heard", CASES)
def test_all_stages_together_calls_in_flight(xd, monkeypatch, plan, nbuf, pipeline, k3_same, variant, lpw, pll, heard):
    k3(monkeypatch, k3_same)
    opts = options(nbuf, pipeline, variant, lpw, pll)
    b, off = make_batch(opts, heard=heard), make_batch(opts, features=False)
    e = tc.build(plan)
    queue(b, xd, e.calls, (nbuf or DEFAULT_NBUF) - 1)
    queue(off, xd, e.calls, (nbuf or DEFAULT_NBUF) - 1, last_blocker=False)
    check(b, off, e, CASES.index((plan, nbuf, pipeline, k3_same, variant, lpw, pll, heard)), heard, tc.TOTAL)


@pytest.mark.parametrize("how", ["reset", "protodec_reset"])
def test_a_reset_between_two_piled_up_halves(xd, monkeypatch, how):
    """half the calls queued, then reset() (or protodec_reset()) at once, with no sync by the test, then the rest: the
    restatements reset at the same point.  After reset() nothing from before it appears: the expectation is a fresh batch
    given the second half.  The call has to wait for everything queued by itself: the event behind the first half has
    fired when it returns."""
    import torch
    k3(monkeypatch, "0" if how == "reset" else None)
    nbuf = 2 if how == "reset" else DEFAULT_NBUF
    opts = options(nbuf, 1, 0, 8, 8)
    b, off = make_batch(opts), make_batch(opts, features=False)
    half = len(tc.plan("ragged")) // 2
    whole = tc.build("ragged")
    e = tc.build("ragged", first_call=half) if how == "reset" else tc.build("ragged", protodec_at=half)
    for q in (b, off):
        queue(q, xd, whole.calls[:half], nbuf - 1, last_blocker=q is b)
        done = torch.cuda.Event()
        done.record()
        getattr(q, how)()
        assert done.query()
        queue(q, xd, whole.calls[half:], nbuf - 1, last_blocker=q is b)
    rows = tc.TOTAL - whole.calls[half][0] if how == "reset" else tc.TOTAL
    check(b, off, e, 8 if how == "reset" else 9, False, rows)


def test_the_long_repair_switched_off_and_on_between_two_piled_up_halves(xd, monkeypatch):
    """long_repair(False), long_repair(True) between the halves of the plan of equal calls: D' is not reset, the candidate
    counters and the call parity start over, and every result is that of the uninterrupted run"""
    import torch
    k3(monkeypatch, "0")
    opts = options(2, 1, 1, 64, 7)
    b, off = make_batch(opts), make_batch(opts, features=False)
    e = tc.build("equal")
    half = len(e.calls) // 2 + 1                            # an odd number of calls: the parity is 1 when the switch turns
    queue(b, xd, e.calls[:half], 1)
    done = torch.cuda.Event()
    done.record()
    b.long_repair(False)
    assert done.query() and b.info("long_repair") == 0
    b.long_repair(True)
    queue(b, xd, e.calls[half:], 1)
    queue(off, xd, e.calls, 1, last_blocker=False)
    check(b, off, e, 10, False, tc.TOTAL)


def test_autotune_rebinds_the_streams_then_the_whole_plan(xd, monkeypatch):
    """autotune() on the audio of the input's first call, every stage on: it tries the stages on other streams, keeps an
    assignment and resets.  The plan behind it gives what a fresh batch gives."""
    k3(monkeypatch, None)
    opts = options(None, 1, 0, 8, 8)
    b, off = make_batch(opts, heard=False), make_batch(opts, features=False)
    e = tc.build("ragged")
    lo, hi = e.calls[0]
    audio = dev(iq_ref.discriminate(tc.iq_input()[lo:hi], None)[0])
    for q in (b, off):
        q.autotune(audio)
        assert int(q.info("rows")) == 0
    queue(b, xd, e.calls, DEFAULT_NBUF - 1)
    queue(off, xd, e.calls, DEFAULT_NBUF - 1, last_blocker=False)
    check(b, off, e, 0, False, tc.TOTAL)
