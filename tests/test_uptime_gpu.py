"""Every clock carry of a long-running receiver on the device: the chain's row count across 2^31 and 2^32, the deframer's
bit count across 2^32 (both deframer forms, K3, the repair stage) and the frames' 37-bit stamp across 2^32 and 2^37 in
every place that reads it.  gnuais_batch_set_clock() starts the clocks at the origins of tests/uptime_ref.py; every
expected value comes from the CPU restatements at the same origin (tests/uptime_ref.py, frame_time_ref, frame_signal_ref,
occupancy_ref, unique_ref / heard_ref, repair_ref, the host formatter and the host fold) and never from a second device
run.  Every comparison is an exact equality; every test asserts from the oracle alone that each channel decodes at least
two frames and has one that closes after its carry."""
import functools

import numpy as np
import pytest

import frame_signal_ref as fsr
import frame_time_ref as ftr
import heard_ref as hr
import iq_ref
import occupancy_ref as orf
import repair_ref as rr
import unique_ref as ur
import uptime_ref as up
from chain_parity import FSM_KEYS, oracle_fsm_rows
from gnuais_amd import synth
from oracle_lib import FRAME_DTYPE, Oracle

pytestmark = pytest.mark.gpu
COUNTER_KEYS = ("receivedframes", "lostframes", "lostframes2")
CALL = up.CALL


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def new_batch(n_ch, rows, bits, max_len=CALL, **options):
    from gnuais_amd import ReceiverBatch
    b = ReceiverBatch(n_ch, max_len=max_len)
    for k, v in options.items():
        b.set_option(k, v)
    b.set_clock(rows, bits)
    assert b.info("rows") == rows
    return b


def counters3(b):
    cnt = b.counters()
    return np.stack([cnt[k] for k in COUNTER_KEYS], axis=1)


def fsm_rows(b):
    f = b.fsm_state()
    return np.stack([f[k] for k in FSM_KEYS], axis=1)


def check_floor(frames0, bits, n_ch, carry=up.CARRY32):
    total, after = up.floors(frames0, bits, n_ch, carry)
    assert total.min() >= 2 and after.min() >= 1, (total.min(), after.min())
    assert (total - after).max() >= 1                     # and somewhere a frame closes before it


def as_sets(frames, times=None):
    """records (with their times) as a sorted list: what holds across the 2^37 wrap inside one drained span"""
    t = np.zeros(len(frames), dtype=np.int64) if times is None else times
    return sorted((f.tobytes(), int(x)) for f, x in zip(frames, t))


# ---- a. the carry at every bit of a frame, through decode_bits --------------------------------------------------

N_SWEEP = 320


@functools.lru_cache(maxsize=None)
def sweep_stream():
    """idle, a frame, idle, a short frame with stuffed bits (the frame of the mid-call sweep), idle, another one (the
    frame the seam cuts open), idle, a last frame, idle; -> (bits, start of each frame's training bits, their lengths)"""
    rng = np.random.default_rng(17)
    bodies = [bytes(rng.integers(0, 256, 21, dtype=np.uint8)),
              b"\xf8\xff\x1f" + bytes(rng.integers(0, 256, 8, dtype=np.uint8)),
              bytes(rng.integers(0, 256, 5, dtype=np.uint8)) + b"\xff\x7f\xfe" + bytes(rng.integers(0, 256, 3, dtype=np.uint8)),
              bytes(rng.integers(0, 256, 21, dtype=np.uint8))]
    parts, starts, lens = [np.zeros(50, dtype=np.uint8)], [], []
    pos = 50
    for body in bodies:
        f = synth.hdlc_frame_bits(body)
        starts.append(pos)
        lens.append(len(f))
        parts += [f, np.zeros(90, dtype=np.uint8)]
        pos += len(f) + 90
    return np.concatenate(parts).astype(np.uint8), starts, lens


def sweep_plan(kind):
    """(cuts of the calls, p0): "mid": the second frame alone in call 2 of three, the sweep over it and the idle bits
    around it; "seam": two calls, the cut 72 bits into the third frame (training bits, flag, 40 data bits), the sweep
    over that frame"""
    s, starts, lens = sweep_stream()
    if kind == "mid":
        assert lens[1] <= 170
        p0 = starts[1] - 75
        assert p0 > starts[0] + lens[0] + 1 and p0 + N_SWEEP > starts[1] + lens[1] + 50
        return [0, starts[1] - 45, starts[1] + lens[1] + 45, len(s)], p0
    cut = starts[2] + 72
    p0 = cut - 160
    assert lens[2] <= 225 and p0 < starts[2] - 40 and p0 + N_SWEEP > starts[2] + lens[2] + 1
    return [0, cut, len(s)], p0


@functools.lru_cache(maxsize=None)
def sweep_expected(kind, drains):
    """the oracle at origin zero, call by call: [(state machines, counters, cells of the frames in progress, the frames
    of a drain behind this call in the oracle's order, or None)]"""
    s, _, _ = sweep_stream()
    cuts, _ = sweep_plan(kind)
    o = Oracle(N_SWEEP)
    out = []
    for k, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
        for c in range(N_SWEEP):
            o.decode_bits(c, s[a:e])
        rows = np.array(oracle_fsm_rows(o, N_SWEEP), dtype=np.int64)
        inside = np.flatnonzero((rows[:, 0] == 4) | (rows[:, 0] == 5))[::7]
        cells = {int(c): o.frame_cells(int(c)) for c in inside}
        fr = None
        if k in drains:
            fr = o.frames()
            o.clear_frames()
        out.append((rows, o.counters().copy(), cells, fr))
    return out


def run_sweep(kind, carry, variant, drains, wrap_inside_a_drain=False):
    s, _, _ = sweep_stream()
    cuts, p0 = sweep_plan(kind)
    bits = up.sweep(N_SWEEP, p0, carry)
    steps = sweep_expected(kind, drains)
    all0 = np.concatenate([st[3] for st in steps if st[3] is not None])
    check_floor(all0, bits, N_SWEEP, carry)
    b = new_batch(N_SWEEP, 0, bits, max_len=48000, hdlc_variant=variant)
    b.frame_times(True)
    open_seen = 0
    for k, ((a, e), (rows, counters, cells, fr0)) in enumerate(zip(zip(cuts[:-1], cuts[1:]), steps)):
        b.decode_bits([s[a:e]] * N_SWEEP)
        assert np.array_equal(fsm_rows(b), rows), (k, np.flatnonzero((fsm_rows(b) != rows).any(axis=1))[:8])
        assert np.array_equal(counters3(b), counters), (k, np.flatnonzero((counters3(b) != counters).any(axis=1))[:8])
        for c, want in cells.items():
            got = b.frame_bits(c)
            assert got is not None and np.array_equal(got, want), ("frame cells", k, c)
        open_seen += len(cells)
        if kind == "seam" and k == 0:
            fed = [v + e for v in bits]
            assert fed[160] == carry and fed[161] == carry - 1 and len(cells) >= 40
        if fr0 is None:
            continue
        want = up.shift_frames(fr0, bits)
        if k + 1 < len(steps):
            got, t = b.drain_frames(), None
        else:
            got, t = b.drain_frames_timed()
            assert t.dtype == np.int64 and np.all(t == -1) and len(t) == len(want)
        if wrap_inside_a_drain:
            assert as_sets(got) == as_sets(want)
        else:
            assert len(got) == len(want), (k, len(got), len(want))
            bad = np.flatnonzero(got != want)
            assert got.tobytes() == want.tobytes(), (k, [(int(got[i]["channel"]), int(got[i]["end_bit"]), int(got[i]["flags"]),
                                                          int(want[i]["end_bit"]), int(want[i]["flags"])) for i in bad[:4]])
    assert kind != "seam" or open_seen >= 40
    b.close()


@pytest.mark.parametrize("variant", [1, 0])
def test_a_the_2_32_carry_at_every_bit_of_a_frame_inside_a_call(variant):
    """320 channels, one bit stream, channel c with 2^32 - p0 - c bits behind it: the carry of the bit count lands on 320
    consecutive bits -- idle, training bits, both flags, data with stuffed bits, the closing bit, idle.  The drain behind
    the last call holds, per channel, frames stamped on both sides of the carry, in the oracle's order."""
    run_sweep("mid", up.CARRY32, variant, drains=(0, 2))


@pytest.mark.parametrize("variant", [1, 0])
def test_a_the_2_32_carry_at_every_bit_of_a_frame_the_seam_of_two_calls_cuts_open(variant):
    """the same over a frame that is open between two calls: the count goes through ctl with the frame in progress; on
    channel 160 it is exactly 2^32 after call 1, on channel 161 2^32 - 1"""
    run_sweep("seam", up.CARRY32, variant, drains=(1,))


@pytest.mark.parametrize("variant", [1, 0])
def test_a_the_2_37_wrap_at_every_bit_of_a_frame(variant):
    """the stamp's own wrap: channel c has 2^37 - p0 - c bits behind it.  A drain behind every call: the swept frame is
    alone in its drain, so the frames of every drain close on one side of the wrap and the order is the oracle's."""
    run_sweep("mid", up.CARRY37, variant, drains=(0, 1, 2))


@pytest.mark.parametrize("variant", [1, 0])
def test_a_one_drained_span_across_the_2_37_wrap_keeps_its_records(variant):
    """what include/gnuais_hip.h promises for a span whose frames close on both sides of the wrap: the set of records
    (and their times, -1 here; with samples in test b) -- not the order inside that drain"""
    run_sweep("mid", up.CARRY37, variant, drains=(0, 2), wrap_inside_a_drain=True)


# ---- b. the same through samples, with times -----------------------------------------------------------------

N_B = 70
CALLS_B = [CALL, CALL, CALL, 1, 2047, 2049, CALL - 4097]


@functools.lru_cache(maxsize=None)
def samples_b():
    x = np.stack([synth.make_stream(5 * CALL, seed=23, channel=c, occupancy=0.9)[0] for c in range(N_B)], axis=1)
    ref = ftr.FrameTimeRef(N_B)
    ref.run(x[:4 * CALL])
    f0, _ = ref.drain()
    mine = np.sort(ftr.stamp(f0[f0["channel"] == 0]))
    p0 = int(mine[mine >= 1700][0]) - 100       # in front of a frame channel 0 closes in call 2 (a call feeds 1536 bits)
    return x, f0, p0


def bits_b(kind):
    _, f0, p0 = samples_b()
    if kind == "zero":
        return [0] * N_B
    return up.sweep(N_B, p0, up.CARRY37 if kind == "wrap37" else up.CARRY32, 5)


def check_timed(b, ref, as_set=False):
    fr, t = b.drain_frames_timed()
    wf, wt = ref.drain()
    assert t.dtype == np.int64
    if as_set:
        assert as_sets(fr, t) == as_sets(wf, wt)
    else:
        assert fr.tobytes() == wf.tobytes(), (len(fr), len(wf))
        assert np.array_equal(t, wt), np.argwhere(t != wt)[:5]
    return wf, wt


@pytest.mark.parametrize("variant", [7, 8])
@pytest.mark.parametrize("bits", ["zero", "carry32"])
@pytest.mark.parametrize("R", up.origins())
def test_b_frames_and_times_through_samples(R, bits, variant):
    """70 channels (one full wave and a ragged one), three calls of 7680 rows and a ragged fourth, a drain behind every
    call: records and times == FrameTimeRef at the origin; then protodec_reset() and one more call"""
    x, f0, _ = samples_b()
    B = bits_b(bits)
    if bits != "zero":
        check_floor(f0, B, N_B)
    b = new_batch(N_B, R, B, pll_variant=variant)
    b.frame_times(True)
    ref = ftr.FrameTimeRef(N_B, rows=R, bits=B)
    xd = dev(x)
    pos, n = 0, 0
    for ln in CALLS_B:
        b.run(xd[pos:pos + ln])
        ref.run(x[pos:pos + ln])
        pos += ln
        assert b.info("rows") == R + pos
        wf, wt = check_timed(b, ref)
        n += len(wf)
        assert len(wt) == 0 or (wt.min() >= R + pos - ln - 0 and wt.max() < R + pos)
    assert n >= 2 * N_B and pos == 4 * CALL
    b.protodec_reset()
    ref.protodec_reset()
    b.run(xd[pos:pos + CALL])
    ref.run(x[pos:pos + CALL])
    assert len(check_timed(b, ref)[0]) >= N_B
    b.close()


def test_b_one_drained_span_across_the_2_37_wrap_keeps_its_records_and_times():
    """the calls of test b queued and drained once, the stamps wrapping inside the span: the set of (record, time)"""
    x, f0, _ = samples_b()
    B, R = bits_b("wrap37"), up.ROWS[1]
    check_floor(f0, B, N_B, up.CARRY37)
    b = new_batch(N_B, R, B)
    b.frame_times(True)
    ref = ftr.FrameTimeRef(N_B, rows=R, bits=B)
    xd = dev(x)
    pos = 0
    for ln in CALLS_B:
        b.run(xd[pos:pos + ln], sync=False)
        ref.run(x[pos:pos + ln])
        pos += ln
    wf, wt = check_timed(b, ref, as_set=True)
    assert len(wf) >= 2 * N_B and wt.min() >= R
    b.close()


# ---- c. I/Q input with signal records and channel load --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def samples_c():
    from test_frame_signal_gpu import iq_input
    x = iq_input(N_B, 3 * CALL)
    a, _ = iq_ref.discriminate(x, None)
    ref = ftr.FrameTimeRef(N_B)
    ref.run(a)
    return x, ref.drain()[0]


@pytest.mark.parametrize("R", [up.ROWS[0], up.ROWS[2]])
def test_c_signal_records_and_channel_load_of_iq_input(R):
    """two I/Q calls, an audio-type call of 2000 rows (so the next run of I/Q calls is latched at a large row that is no
    multiple of 64), a third I/Q call; frame_times, frame_signal and occupancy(64, 16) switched on behind set_clock.  Every
    drain == FrameSignalRef, the block sums read across the carry == BlockSums, the epochs and their blocks ==
    OccupancyRef fed the restatement's own frames and times."""
    from test_frame_signal_gpu import Front
    x, f0 = samples_c()
    E, margin = 64, 16                  # the smallest epoch the library takes
    B = up.sweep(N_B, 2000, up.CARRY32, 5)
    check_floor(f0, B, N_B)
    b = new_batch(N_B, R, B)
    b.frame_times(True)
    b.frame_signal(True)
    b.occupancy(E, margin)
    ref, front = fsr.FrameSignalRef(N_B, rows=R, bits=B), Front(N_B, 0)
    ref.switch_on()
    occ = orf.OccupancyRef(N_B, E, margin)
    occ.reset(R)
    n, seen, n_sig, n_ep = R, 0, 0, 0
    rng = np.random.default_rng(3)
    quiet = rng.integers(-200, 200, (2000, N_B)).astype(np.int16)
    for step, seg in enumerate((x[:CALL], x[CALL:2 * CALL], None, x[2 * CALL:])):
        if seg is None:
            b.run(dev(quiet))
            ref.run_audio(quiet)
            occ.run_audio(n, len(quiet))
            n += len(quiet)
        else:
            b.run_iq(dev(seg))
            occ.run_iq(n, seg)
            ref.run_iq(seg, front.audio(seg))
            n += len(seg)
        assert b.info("rows") == n
        fr, t, sig = b.drain_frames_signal()
        wf, wt, ws = ref.drain()
        assert fr.tobytes() == wf.tobytes() and np.array_equal(t, wt), (step, len(fr), len(wf))
        assert sig.tobytes() == ws.tobytes(), (step, np.argwhere(sig != ws)[:5])
        n_sig += int((ws["blocks"] > 0).sum())
        occ.add_frames(wf, wt)
        if seg is not None:
            j1 = n // 64
            j0 = max(ref.sums.v0 // 64, j1 - 150)            # from the run's first block on, rows before v0 zero
            got = b.signal_blocks(j0, j1 - j0)
            assert np.array_equal(got, ref.sums.blocks(j0, j1 - j0)), (step, j0, np.argwhere(got != ref.sums.blocks(j0, j1 - j0))[:4])
            if step == 1:
                assert j0 * 64 < R + CALL <= j1 * 64          # read across the seam of calls 1 and 2
        first, rec = b.drain_occupancy()
        want = occ.epochs()[seen:]
        assert first.tolist() == [w[0] for w in want], (step, first[:4], [w[0] for w in want][:4])
        b0 = -(-occ.runs[-1]["v0"] // 64)
        for k, (f_0, wrec, words) in enumerate(want):
            assert rec[k].tobytes() == wrec.tobytes(), (step, f_0, np.argwhere(rec[k] != wrec)[:5])
            if f_0 >= b0:
                got = b.occupancy_blocks(f_0, E)
                assert np.array_equal(got, words), (step, f_0)
        seen += len(want)
        n_ep += len(want)
    assert n_sig >= 2 * N_B and n_ep == 4 and b.occupancy_lost() == 0
    assert ref.sums.v0 == R + 2 * CALL + 2000 and ref.sums.v0 % 64
    b.close()


# ---- d. one transmission heard by several receivers -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def samples_d():
    x = ur.receivers(1, ur.DELAYS6)
    ref = ftr.FrameTimeRef(6)
    ref.run(x)
    f0, _ = ref.drain()
    # the copies of the fourth transmission: stamped 2^32 - 1 on the even receivers, 2^32 on the odd ones
    bits = [up.CARRY32 - int(ftr.stamp(f0[f0["channel"] == c])[3]) - (1 - c % 2) for c in range(6)]
    return x, f0, bits


@pytest.mark.parametrize("per_call", [True, False])
@pytest.mark.parametrize("heard", [False, True])
def test_d_one_transmission_heard_by_six_receivers(heard, per_call):
    """rows origin 2^32 - 3840: the member-order word is 32 bits wide in the first drains and 33 in the later ones; the
    receivers' bit origins put the copies of one transmission on both sides of 2^32"""
    x, f0, bits = samples_d()
    check_floor(f0, bits, 6)
    R, W = up.ROWS[1], 128
    b = new_batch(6, R, bits, max_len=ur.TOTAL)
    b.frame_times(True)
    b.unique(W)
    ft, ref = ftr.FrameTimeRef(6, rows=R, bits=bits), hr.HeardRef(W)
    xd = dev(x)
    cuts = ur.ragged_cuts()
    records = copies = 0
    widths = set()
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.run(xd[a:e])
        ft.run(x[a:e])
        if not per_call and e != cuts[-1]:
            continue
        rows = R + int(e)
        assert b.info("rows") == rows
        widths.add(rows.bit_length())
        fr, tm = ft.drain()
        got = b.drain_frames_heard() if heard else b.drain_frames_unique()
        want = ref.push_heard(fr, tm, rows) if heard else ref.push(fr, tm, rows)
        assert got[0].tobytes() == want[0].tobytes(), (len(got[0]), len(want[0]))
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        if heard:
            assert np.array_equal(got[3], want[3]) and got[4].tobytes() == want[4].tobytes()
            hr.check_invariants(*got)
        assert b.unique_late() == ref.late
        records += len(got[0])
        copies += int(got[2].sum())
    assert widths == ({32, 33} if per_call else {33})
    assert records == 8 and copies + ref.late == 48
    b.close()


# ---- e. order and last writer across the carry ----------------------------------------------------------------

N_E = 4


def mmsi_of(frames):
    bits = np.unpackbits(frames["payload"][:, 1:5], axis=1)
    return (bits[:, :30].astype(np.int64) << np.arange(29, -1, -1)).sum(axis=1)


@functools.lru_cache(maxsize=None)
def traffic_e():
    from test_vessels import _vessel_traffic
    streams = _vessel_traffic(81, N_E, 900, 40)
    o = Oracle(N_E)
    for c, s in enumerate(streams):
        o.decode_bits(c, s)
    f0 = o.frames()
    bits = []
    for c in range(N_E):
        st = np.sort(ftr.stamp(f0[f0["channel"] == c]))
        bits.append(up.CARRY32 - int(st[len(st) // 2]))     # half of the channel's frames on either side
    check_floor(f0, bits, N_E)
    want = up.shift_frames(f0, bits)
    hi = (want["flags"] >> 1) & 31
    for c in range(N_E):                                    # frames of one vessel on both sides of 2^32 in every channel
        m = want["channel"] == c
        assert len(set(mmsi_of(want[m & (hi == 0)])) & set(mmsi_of(want[m & (hi == 1)]))) >= 10
    return streams, want, bits


def test_e_the_data_tell_a_broken_key_apart():
    """CPU-side premise of test e: sorted on the low 32 bits of the stamp alone, the same records give other sentences'
    order and another vessel table"""
    from gnuais_amd import nmea_from_frames, vessels_from_frames
    _, want, _ = traffic_e()
    broken = want[np.lexsort((want["end_bit"], want["channel"]))]
    assert nmea_from_frames(broken, np.zeros(N_E, dtype=np.uint8)) != nmea_from_frames(want, np.zeros(N_E, dtype=np.uint8))
    assert vessels_from_frames(broken).tobytes() != vessels_from_frames(want).tobytes()


def test_e_sentences_in_order_across_the_carry():
    from gnuais_amd import messages_from_frames, nmea_from_frames
    streams, want, bits = traffic_e()
    b = new_batch(N_E, 0, bits, max_len=48000)
    b.decode_bits(streams)
    seq, seq0 = np.zeros(N_E, dtype=np.uint8), np.zeros(N_E, dtype=np.uint8)
    text, ns, nf = b.drain_nmea(seq)
    wtext = nmea_from_frames(want, seq0)
    assert nf == len(want) and ns == wtext.count(b"\r\n") and text == wtext and np.array_equal(seq, seq0)
    b.close()
    b = new_batch(N_E, 0, bits, max_len=48000)
    b.decode_bits(streams)
    seq, seq0 = np.zeros(N_E, dtype=np.uint8), np.zeros(N_E, dtype=np.uint8)
    nm, tx, ns, nlines, nf = b.drain_messages(seq, b"ABCD")
    wnm, wtx = messages_from_frames(want, seq0, b"ABCD")
    assert nf == len(want) and nm == wnm and tx == wtx and np.array_equal(seq, seq0)
    assert ns == wnm.count(b"\r\n") and nlines == wtx.count(b"\n")
    b.close()


def test_e_the_later_report_wins_across_the_carry():
    from gnuais_amd import VESSEL_DTYPE, vessels_from_frames
    streams, want, bits = traffic_e()
    table = vessels_from_frames(want)
    assert len(table) >= 40 and len(np.unique(table["set"])) >= 4
    b = new_batch(N_E, 0, bits, max_len=48000)
    b.vessel_table_enable(500)
    b.decode_bits(streams)
    got = b.fold_vessels()
    for name in VESSEL_DTYPE.names:
        assert np.array_equal(got[name], table[name]), ("fold", name)
    assert got.tobytes() == table.tobytes()
    b.vessel_table_update()
    assert b.drain_frames().tobytes() == want.tobytes()
    got = b.vessel_table()
    for name in VESSEL_DTYPE.names:
        assert np.array_equal(got[name], table[name]), ("carried", name)
    assert got.tobytes() == table.tobytes()
    b.close()


def test_e_a_streaming_batch_across_the_carry():
    """run + run + stream_nmea: two launches share a ring, so the span is ordered by the sort on (channel, stamp); the
    carry of every channel's bit count lies inside the second span.  Text and the carried table against the host
    formatter and fold over the oracle's frames, shifted, span by span."""
    import cases
    from gnuais_amd import VESSEL_DTYPE, nmea_from_frames, vessels_from_frames
    n_ch, call, n_spans = 8, 2 * 1280, 4
    pool, _ = cases.vessel_frames(seed=31, n_channels=1, n=400, n_mmsi=12)
    bodies = [bytes(f["payload"][: int(f["nbits"]) // 8]) for f in pool if int(f["nbits"]) == 168]     # one slot each

    def payloads(rng, slot):
        return bodies[int(rng.integers(0, len(bodies)))]

    x = np.stack([synth.make_stream(2 * call * n_spans, seed=35, channel=c, payloads=payloads)[0] for c in range(n_ch)], axis=1)
    o = Oracle(n_ch)
    spans0 = []
    for i in range(n_spans):
        o.run(x[2 * i * call:2 * (i + 1) * call])
        spans0.append(o.frames())
        o.clear_frames()
    bits = []
    for c in range(n_ch):
        st = ftr.stamp(spans0[1][spans0[1]["channel"] == c])
        assert len(st) >= 2
        bits.append(up.CARRY32 - int(st[len(st) // 2]))
    check_floor(np.concatenate(spans0), bits, n_ch)
    b = new_batch(n_ch, up.ROWS[1], bits, max_len=call)
    b.vessel_table_enable(100)
    xd = dev(x)
    texts = []
    for i in range(n_spans):
        b.run(xd[2 * i * call:(2 * i + 1) * call], sync=False)
        b.run(xd[(2 * i + 1) * call:(2 * i + 2) * call], sync=False)
        texts.append(b.stream_nmea())
    for _ in range(b.stream_depth):
        texts.append(b.stream_nmea())
    texts = [t for t in texts if t[2] >= 0]
    assert len(texts) == n_spans
    seq, table = np.zeros(n_ch, dtype=np.uint8), np.zeros(0, dtype=VESSEL_DTYPE)
    for i, (text, ns, nf) in enumerate(texts):
        want = up.shift_frames(spans0[i], bits)
        wtext = nmea_from_frames(want, seq)
        assert nf == len(want) and text == wtext and ns == wtext.count(b"\r\n"), i
        table = vessels_from_frames(want, table)
    assert b.vessel_table().tobytes() == table.tobytes() and len(table) >= 10
    b.close()


# ---- f. repair ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 1])
def test_f_a_repaired_frame_keeps_its_candidates_stamp_across_the_carry(variant):
    """one frame with a single symbol error, then an intact one, on four channels: the repaired frame closes just after
    the carry (stamp 2^32), just before it (2^32 - 1), with the carry inside it, and far from it"""
    from test_repair_gpu import GAP, crafted_payload, flipped_frame, records
    rng = np.random.default_rng(91)
    pa, pb = crafted_payload(rng, 21), bytes(rng.integers(0, 256, 21, dtype=np.uint8))
    s = np.array(GAP + flipped_frame(pa, 30) + GAP + synth.hdlc_frame_bits(pb).tolist() + GAP, dtype=np.uint8)
    streams = [s] * 4
    want0, rep, cnt = rr.decode_streams(streams)
    want0 = records(want0)
    assert np.array_equal(rep, np.ones(4)) and np.array_equal(cnt, np.tile([1, 1, 0], (4, 1)))
    e_r = int(ftr.stamp(want0[(want0["channel"] == 0) & ((want0["flags"] & 0x40) != 0)])[0])
    bits = [up.CARRY32 - e_r, up.CARRY32 - e_r - 1, up.CARRY32 - e_r + 100, 12345]
    check_floor(want0[want0["channel"] < 3], bits[:3], 3)
    want = up.shift_frames(want0, bits)
    assert [int(v) for v in ftr.stamp(want[(want["flags"] & 0x40) != 0])] == [1 << 32, (1 << 32) - 1, (1 << 32) + 100, 12345 + e_r]
    b = new_batch(4, 0, bits, max_len=48000, hdlc_variant=variant)
    b.repair(True)
    b.decode_bits(streams)
    got = b.drain_frames()
    assert got.tobytes() == want.tobytes(), (got[["channel", "end_bit", "flags"]], want[["channel", "end_bit", "flags"]])
    assert np.array_equal(counters3(b), cnt) and np.array_equal(b.repaired(), rep)
    b.close()


# ---- g. set_clock itself --------------------------------------------------------------------------------------

def test_g_set_clock_errors_reset_and_info():
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import E_ARG, E_STATE, GnuaisError

    def refused(call, code):
        with pytest.raises(GnuaisError) as e:
            call()
        assert e.value.code == code

    n_ch = 5
    x = np.stack([synth.make_stream(CALL, seed=29, channel=c, occupancy=0.9)[0] for c in range(n_ch)], axis=1)
    fresh = ReceiverBatch(n_ch, max_len=CALL)
    fresh.frame_times(True)
    fresh.run(dev(x))
    f_fresh, t_fresh = fresh.drain_frames_timed()
    state = (fresh.fsm_state().tobytes(), fresh.counters().tobytes(), fresh.pll_state().tobytes())
    assert len(f_fresh) >= 2 * n_ch

    b = ReceiverBatch(n_ch, max_len=CALL)
    b.frame_times(True)
    refused(lambda: b.set_clock(-1), E_ARG)
    b.set_clock(up.ROWS[3], 7)                      # a scalar: every channel
    assert b.info("rows") == up.ROWS[3]
    b.set_clock(up.ROWS[1], up.sweep(n_ch, 700, up.CARRY32, 5))       # again, while nothing has run
    assert b.info("rows") == up.ROWS[1]
    b.run(dev(x))
    assert b.info("rows") == up.ROWS[1] + CALL
    refused(lambda: b.set_clock(0), E_STATE)        # a run call has been made
    fr, t = b.drain_frames_timed()
    want = up.shift_frames(f_fresh, up.sweep(n_ch, 700, up.CARRY32, 5))
    assert fr.tobytes() == want.tobytes() and np.array_equal(t, t_fresh + up.ROWS[1])
    assert len(np.unique(fr["flags"] >> 1 & 31)) == 2
    # reset brings every clock back to zero: the run of a fresh batch
    b.reset()
    assert b.info("rows") == 0
    b.run(dev(x))
    fr, t = b.drain_frames_timed()
    assert fr.tobytes() == f_fresh.tobytes() and np.array_equal(t, t_fresh)
    assert (b.fsm_state().tobytes(), b.counters().tobytes(), b.pll_state().tobytes()) == state
    b.reset()
    b.set_clock(256)                                # allowed again behind a reset; None: no bits
    b.decode_bits([np.zeros(8, dtype=np.uint8)] * n_ch)
    refused(lambda: b.set_clock(0), E_STATE)        # a decode call has been made
    assert b.info("rows") == 256
    b.close()
    # not with the AFC or a wide stage configured
    a = ReceiverBatch(n_ch, max_len=CALL)
    a.afc(1024)
    refused(lambda: a.set_clock(256), E_STATE)
    a.close()
    w = ReceiverBatch(4, max_len=CALL)
    w.channeliser(6, 288000, (-25000, 25000))
    refused(lambda: w.set_clock(256), E_STATE)
    w.close()
    fresh.close()
