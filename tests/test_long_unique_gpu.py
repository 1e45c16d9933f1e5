"""Each long transmission once on the device (gnuais_batch_long_unique, frame_unique.hip over LongDev).  The expected value is
always the restatement tests/long_unique_ref.py applied to what drain_long_frames() of a TWIN batch gives for the same
calls -- a path that exists and is tested by itself -- so the new drains are never compared with themselves.  Every test
also checks that the chain's frames, counters, fsm_state and pll_state equal the twin's."""
import ctypes as C

import numpy as np
import pytest

import long_ref as lr
import long_unique_ref as lur
import unique_ref as ur
from gnuais_amd import synth
from gnuais_amd.lib import E_ARG, E_STATE, HEARER_DTYPE, LONG_FRAME_DTYPE, GnuaisError
from test_iq_gpu import dev

pytestmark = pytest.mark.gpu
GAP = np.zeros(40, dtype=np.uint8)
REPAIRED = lur.REPAIRED


def chain_state(b):
    return (b.drain_frames().tobytes(), b.counters().tobytes(), b.fsm_state().tobytes(), b.pll_state().tobytes())


def pair(n_ch, W, max_len=lur.TOTAL_G, repair=False, hash_bits=64):
    """the batch under test and its twin, which only decodes long frames"""
    from gnuais_amd import ReceiverBatch
    b, t = ReceiverBatch(n_ch, max_len=max_len), ReceiverBatch(n_ch, max_len=max_len)
    for x in (b, t):
        x.long_frames(True)
        if repair:
            x.long_repair(True)
    assert b.info("long_unique") == 0
    b.long_unique(W)
    assert b.info("long_unique") == W and b.info("unique") == 0 and b.info("frame_times") == 0
    if hash_bits != 64:
        b.set_option("unique_hash_bits", hash_bits)
    return b, t


class Check:
    """drain by drain: the merged drain of `b` against the restatement over the twin's plain long drain"""

    def __init__(self, b, t, W):
        self.b, self.t, self.ref = b, t, lur.LongUniqueRef(W)
        self.twin_frames = self.copies = self.records = 0

    def drain(self, heard=False):
        got = self.b.drain_long_frames_heard() if heard else self.b.drain_long_frames_unique()
        fr = self.t.drain_long_frames()
        rows = int(self.t.info("rows"))
        assert rows == int(self.b.info("rows"))
        want = self.ref.push_heard(fr, rows) if heard else self.ref.push(fr, rows)
        assert len(got[0]) == len(want[0]), (len(got[0]), len(want[0]), len(fr))
        assert np.array_equal(got[1], want[1]) and got[1].dtype == np.int32, (got[1], want[1])
        assert got[0].tobytes() == want[0].tobytes() and got[0].dtype == LONG_FRAME_DTYPE
        if heard:
            assert np.array_equal(got[2], want[2]) and got[2].dtype == np.int32
            assert got[3].tobytes() == want[3].tobytes() and got[3].dtype == HEARER_DTYPE
            assert np.array_equal(np.diff(got[2]), got[1]) and got[2][0] == 0 and got[2][-1] == len(got[3])
            assert not got[3]["signal"]["power"].any() and not got[3]["signal"]["ferr"].any() and not got[3]["signal"]["blocks"].any()
        assert self.b.long_unique_late() == self.ref.late == int(self.b.info("long_unique_late"))
        self.twin_frames += len(fr)
        self.copies += int(got[1].sum())
        self.records += len(got[0])
        assert self.copies + self.b.long_unique_late() == self.twin_frames
        assert self.b.pending_long_frames() == 0
        return got

    def end(self):
        """the chain did not notice: its frames, counters and state are the twin's"""
        assert chain_state(self.b) == chain_state(self.t)


def run_calls(b, t, x, cuts, each=None):
    xd = dev(x)
    for a, e in zip(cuts[:-1], cuts[1:]):
        b.run(xd[a:e])
        t.run(xd[a:e])
        if each:
            each()


@pytest.fixture(scope="module")
def seven():
    return lur.seven_receivers()


@pytest.fixture(scope="module")
def seventy():
    return lur.group_receivers(10)


@pytest.mark.parametrize("per_call", [False, True])
def test_seven_receivers_drained_once_and_after_every_ragged_call(seven, per_call):
    b, t = pair(7, 128, max_len=lur.TOTAL7)
    ck = Check(b, t, 128)
    run_calls(b, t, seven, lur.ragged_cuts7(), ck.drain if per_call else None)
    got = ck.drain()
    assert ck.twin_frames == 34 and ck.records == 5
    if not per_call:
        assert np.count_nonzero(got[1] == 7) >= 4 and b.long_unique_late() == 0     # a merge that merges nothing fails here
    ck.end()


@pytest.mark.parametrize("hash_bits", [64, 1, 3])
@pytest.mark.parametrize("per_call", [False, True])
def test_seventy_receivers_and_forced_hash_collisions(seventy, per_call, hash_bits):
    """10 groups x 7 delays, each group with payloads of its own; with the hash cut to 1 and 3 bits different keys share a
    hash and the exact path -- 17 sorts by the key words -- gives the same records"""
    b, t = pair(70, 128, hash_bits=hash_bits)
    ck = Check(b, t, 128)
    run_calls(b, t, seventy, ur.ragged_cuts(lur.TOTAL_G), ck.drain if per_call else None)
    got = ck.drain()
    assert ck.twin_frames > 150 and 25 <= ck.records <= 30
    if not per_call:
        assert got[1].max() == 7 and np.count_nonzero(got[1] == 7) > 10
    ck.end()


@pytest.mark.parametrize("n_ch", [300, 600])
def test_a_cluster_wider_than_a_workgroup(n_ch):
    """n_ch channels carry one 54-byte burst, delays c % 41, noise of their own (sigma 300): one cluster.  The modem
    loses this burst at some of the delays that are 1 or 2 modulo 5 (the oracle does too: 245 of 300 and 508 of 600
    receivers decode it), so it is the 600-channel case whose cluster spans more than one workgroup of 256 lanes"""
    one = lur.slots_stream(4096, {0: lur.short_long_payload(1)}, seed=6, sigma=0.0)
    rng = np.random.default_rng(5)
    x = np.stack([np.roll(one, c % 41) for c in range(n_ch)], axis=1).astype(np.int32)
    x = np.clip(x + rng.normal(0.0, 300.0, x.shape).round().astype(np.int32), -32768, 32767).astype(np.int16)
    b, t = pair(n_ch, 128, max_len=4096)
    ck = Check(b, t, 128)
    run_calls(b, t, x, [0, 4096])
    got = ck.drain(heard=True)
    assert ck.records == 1 and got[1].tolist() == [ck.twin_frames] and ck.twin_frames > (256 if n_ch == 600 else 200)
    ck.end()


def chain_input():
    """one payload in slots 0, 6, 12, 18 on alternating channels: the copies lie 7680 rows apart (+- 2)"""
    p = lur.short_long_payload(1)
    return np.stack([lur.slots_stream(24 * 1280, {s: p for s in (0, 6, 12, 18) if (s // 6) % 2 == c}, seed=22, channel=c)
                     for c in range(2)], axis=1)


@pytest.mark.parametrize("W,one_cluster", [(7700, True), (7660, False)])
def test_a_chain_of_copies_six_slots_apart(W, one_cluster):
    x = chain_input()
    b, t = pair(2, W, max_len=x.shape[0])
    ck = Check(b, t, W)
    run_calls(b, t, x, [0, x.shape[0]])
    got = ck.drain()
    assert ck.twin_frames == 4
    assert got[1].tolist() == ([4] if one_cluster else [1] * 4)
    ck.end()


def late_input(delays):
    """slot 1 on every channel (delayed), and the same payload once more in slot 7 of channel 0"""
    p = lur.short_long_payload(1)
    cols = [np.roll(lur.slots_stream(12 * 1280, {1: p, 7: p} if c == 0 else {1: p}, seed=22, channel=c), d)
            for c, d in enumerate(delays)]
    return np.stack(cols, axis=1)


def test_late_copies_across_a_drain():
    """delays 0 and 600, W = 700, the cut between the ends of the two copies: the second drain delivers nothing and counts
    one late copy; W rows later the tail is empty and the same payload is a transmission again"""
    x = late_input([0, 600])
    b, t = pair(2, 700, max_len=x.shape[0])
    ck = Check(b, t, 700)
    xd = dev(x)
    for (a, e), (n_rec, late) in zip([(0, 4000), (4000, 6000), (6000, x.shape[0])], [(1, 0), (0, 1), (1, 1)]):
        b.run(xd[a:e])
        t.run(xd[a:e])
        got = ck.drain()
        assert len(got[0]) == n_rec and b.long_unique_late() == late, (a, e, len(got[0]), b.long_unique_late())
        assert got[1].tolist() == [1] * n_rec
    assert ck.twin_frames == 3
    ck.end()


def test_reset_protodec_reset_and_the_switch_of_long_frames():
    x = late_input([0, 600, 4000])
    xd = dev(x)
    W = 4000
    b, t = pair(3, W, max_len=x.shape[0])
    ck = Check(b, t, W)
    for (a, e), (n_rec, late) in zip([(0, 4000), (4000, 4700), (4700, 8000)], [(1, 0), (0, 1), (0, 2)]):
        b.run(xd[a:e])
        t.run(xd[a:e])
        got = ck.drain()
        assert len(got[0]) == n_rec and b.long_unique_late() == late
        if e == 4700:                   # between the second copy's end and the third one's start: keeps tail and late
            b.protodec_reset()
            t.protodec_reset()
            assert b.long_unique_late() == 1
    # reset: rows start again at 0; a kept tail entry would swallow the first copy as a late one
    b.reset()
    t.reset()
    ck = Check(b, t, W)
    assert b.long_unique_late() == 0 and b.info("long_unique") == W
    b.run(xd[:8000])
    t.run(xd[:8000])
    got = ck.drain()
    assert got[1].tolist() == [3] and b.long_unique_late() == 0
    # the tail is open (t_last about 7818, rows 8000).  A switch of long frames, on to on, clears it and keeps the window:
    # channel 0's second copy (about row 11500) chains onto nothing and is a transmission
    for r in (b, t):
        r.long_frames(True)
    assert b.info("long_unique") == W and b.long_unique_late() == 0
    ck = Check(b, t, W)
    b.run(xd[8000:])
    t.run(xd[8000:])
    got = ck.drain()
    assert got[1].tolist() == [1] and b.long_unique_late() == 0
    # switching the feature itself clears both as well; switching long frames off switches the feature off
    b.long_unique(W + 1)
    assert b.info("long_unique") == W + 1 and b.long_unique_late() == 0
    ck.end()
    b.long_frames(False)
    assert b.info("long_unique") == 0 and b.info("long_unique_late") == 0
    b.long_frames(True)
    assert b.info("long_unique") == 0
    with pytest.raises(GnuaisError) as e:
        b.drain_long_frames_unique()
    assert e.value.code == E_STATE


def square(bits, start, total, amplitude=12000):
    """an unshaped NRZI square wave of the on-air bits, 5 rows a bit, from row `start`; silence around it"""
    x = np.zeros(total, dtype=np.int16)
    lev = np.repeat(synth.nrzi_levels(np.asarray(bits, dtype=np.uint8)), 5) * amplitude
    x[start:start + lev.size] = lev.astype(np.int16)
    return x


@pytest.mark.parametrize("both_damaged", [False, True])
def test_the_intact_copy_is_the_primary_before_an_earlier_repaired_one(both_damaged):
    """one wrong symbol is two adjacent wrong bits behind the NRZI decoder; the damaged copy is heard 20 rows earlier"""
    payload = lur.short_long_payload(4)
    good = lr.burst(np.frombuffer(payload, dtype=np.uint8))
    bad = good.copy()
    bad[200:202] ^= 1
    x = np.stack([square(bad, 100, 4096), square(bad if both_damaged else good, 120, 4096)], axis=1)
    b, t = pair(2, 128, max_len=4096, repair=True)
    ck = Check(b, t, 128)
    run_calls(b, t, x, [0, 4096])
    f, c, first, mem = ck.drain(heard=True)
    assert ck.twin_frames == 2 and c.tolist() == [2] and mem["channel"].tolist() == [0, 1]
    assert bytes(f[0]["payload"][:54]) == payload and int(f[0]["nbits"]) == 432
    assert int(mem["flags"][0]) & REPAIRED and bool(int(mem["flags"][1]) & REPAIRED) == both_damaged
    if both_damaged:
        assert int(f[0]["channel"]) == 0 and int(f[0]["flags"]) & REPAIRED
    else:
        assert int(f[0]["channel"]) == 1 and not int(f[0]["flags"]) & REPAIRED
    assert b.long_repaired().tolist() == t.long_repaired().tolist() == [1, 1 if both_damaged else 0]
    ck.end()


def three_payloads(n_ch, total=4096):
    """n_ch noise-free receivers, each hears one 54-byte burst in slot 0: payload c % 3, delay c % 41"""
    base = [lur.slots_stream(total, {0: lur.short_long_payload(10 + k)}, seed=6, channel=k, sigma=0.0) for k in range(3)]
    return np.stack([np.roll(base[c % 3], c % 41) for c in range(n_ch)], axis=1)


@pytest.mark.parametrize("n_ch", [1, 63, 64, 65, 255, 256, 257])
def test_drains_of_a_chosen_number_of_records(n_ch):
    b, t = pair(n_ch, 128, max_len=4096)
    ck = Check(b, t, 128)
    got = ck.drain(heard=n_ch & 1)              # a drain of 0 records
    assert len(got[0]) == 0 and got[0].dtype == LONG_FRAME_DTYPE
    run_calls(b, t, three_payloads(n_ch), [0, 4096])
    got = ck.drain(heard=n_ch & 1)
    assert ck.twin_frames == n_ch and ck.records == min(n_ch, 3) and int(got[1].sum()) == n_ch
    ck.end()


def test_untimed_records_come_first_each_by_itself():
    n_ch = 5
    pay = [np.frombuffer(lur.short_long_payload(20 + k), dtype=np.uint8) for k in range(2)]
    streams = [np.concatenate([GAP, lr.burst(pay[c % 2]), GAP, lr.burst(pay[0]), GAP]) for c in range(n_ch)]
    b, t = pair(n_ch, 128, max_len=4096)
    ck = Check(b, t, 128)
    b.decode_bits(streams)
    t.decode_bits(streams)
    f, c = ck.drain()                           # a drain that holds only t = -1 records
    assert len(f) == 2 * n_ch and np.all(f["t"] == -1) and np.all(c == 1)
    b.decode_bits(streams)
    t.decode_bits(streams)
    run_calls(b, t, three_payloads(n_ch), [0, 4096])
    f, c, first, mem = ck.drain(heard=True)     # mixed: the untimed ones first, in the plain long drain's order
    assert np.all(f["t"][: 2 * n_ch] == -1) and np.all(f["t"][2 * n_ch:] >= 0) and len(f) == 2 * n_ch + 3
    assert np.all(c[: 2 * n_ch] == 1) and sorted(c[2 * n_ch:].tolist()) == [1, 2, 2]
    assert f["channel"][: 2 * n_ch].tolist() == sorted(f["channel"][: 2 * n_ch].tolist())
    assert np.all(mem["t"][: 2 * n_ch] == -1)
    ck.end()


def test_the_switch_and_its_states(seven):
    from gnuais_amd import ReceiverBatch

    def state_error(fn, *a):
        with pytest.raises(GnuaisError) as e:
            fn(*a)
        assert e.value.code == E_STATE, e.value

    b, t = ReceiverBatch(7, max_len=lur.TOTAL7), ReceiverBatch(7, max_len=lur.TOTAL7)
    assert b.info("long_unique") == 0 and b.info("long_unique_late") == 0       # off by default
    state_error(b.long_unique, 128)             # long frames are off
    state_error(b.drain_long_frames_unique)     # never decoded long frames
    for r in (b, t):
        r.long_frames(True)
    state_error(b.drain_long_frames_unique)     # the feature is off
    state_error(b.drain_long_frames_heard)
    with pytest.raises(GnuaisError) as e:
        b.long_unique(-1)
    assert e.value.code == E_ARG
    b.long_unique(128)
    xd = dev(seven)
    half = lur.TOTAL7 // 2
    # a plain long drain in between: its records are never seen by the stage
    b.run(xd[:half])
    t.run(xd[:half])
    plain = b.drain_long_frames()
    assert plain.tobytes() == t.drain_long_frames().tobytes() and len(plain) > 7 and b.long_unique_late() == 0
    b.run(xd[half:])
    t.run(xd[half:])
    # too little room: GNUAIS_E_ARG, nothing consumed, tail and late as they were
    n = b.pending_long_frames()
    assert n == 34 - len(plain)
    out, cps = np.zeros(n, dtype=LONG_FRAME_DTYPE), np.zeros(n, dtype=np.int32)
    got = C.c_int(-1)
    rc = b._lib.gnuais_batch_drain_long_frames_unique(b._h, out.ctypes.data, cps.ctypes.data, n - 1, C.byref(got))
    assert rc == E_ARG and got.value == 0 and b.pending_long_frames() == n and b.long_unique_late() == 0
    first, mem, nm = np.zeros(n + 1, dtype=np.int32), np.zeros(n, dtype=HEARER_DTYPE), C.c_int(-1)
    rc = b._lib.gnuais_batch_drain_long_frames_heard(b._h, out.ctypes.data, cps.ctypes.data, n - 1, C.byref(got),
                                                     first.ctypes.data, mem.ctypes.data, C.byref(nm))
    assert rc == E_ARG and got.value == 0 and nm.value == 0 and b.pending_long_frames() == n
    f, c = b.drain_long_frames_unique()
    want = lur.LongUniqueRef(128).push(t.drain_long_frames(), lur.TOTAL7)
    assert f.tobytes() == want[0].tobytes() and np.array_equal(c, want[1]) and int(c.sum()) == n
    assert chain_state(b) == chain_state(t)
    b.long_unique(0)
    assert b.info("long_unique") == 0
    state_error(b.drain_long_frames_unique)


def test_both_merges_on_are_independent(seven):
    """the seed-9 stream also carries a 424-bit and a 168-bit frame: drain_frames_unique delivers those exactly as it does
    with the long merge off, the long drain delivers the five long frames, and each merge counts its own late copies"""
    from gnuais_amd import ReceiverBatch
    b, s, t = (ReceiverBatch(7, max_len=lur.TOTAL7) for _ in range(3))
    for r in (b, s):                            # s: the short merge alone
        r.frame_times(True)
        r.unique(128)
    for r in (b, t):                            # t: long frames alone
        r.long_frames(True)
    b.long_unique(128)
    ref = lur.LongUniqueRef(128)
    xd = dev(seven)
    # the cuts split the 480-bit cluster (copies from row 10471 to 10567) and the 424-bit one (48565 to 48659)
    cuts = [0, 10520, 48600, lur.TOTAL7]
    short = long = 0
    for a, e in zip(cuts[:-1], cuts[1:]):
        for r in (b, s, t):
            r.run(xd[a:e])
        got, want = b.drain_frames_unique(), s.drain_frames_unique()
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        short += len(got[0])
        f, c = b.drain_long_frames_unique()
        wf, wc = ref.push(t.drain_long_frames(), int(e))
        assert f.tobytes() == wf.tobytes() and np.array_equal(c, wc)
        long += len(f)
        assert b.unique_late() == s.unique_late() and b.long_unique_late() == ref.late
    assert short == 2 and long == 5
    assert b.unique_late() > 0 and b.long_unique_late() > 0 and b.info("unique_late") == s.unique_late()
    assert b.counters().tobytes() == t.counters().tobytes() and b.pll_state().tobytes() == t.pll_state().tobytes()
    assert b.fsm_state().tobytes() == t.fsm_state().tobytes()


def test_iq_input_two_receivers():
    total = 3 * 6 * 1280
    x = np.stack([np.roll(synth.make_iq_stream(total, seed=3, channel=c, sigma=800.0, gated=True,
                                               payloads=lur.group_payloads(0))[0], d, axis=0)
                  for c, d in enumerate([0, 19])], axis=1)
    b, t = pair(2, 128, max_len=8192)
    ck = Check(b, t, 128)
    xd = dev(x)
    for a, e in [(0, 1020), (1020, 1021), (1021, 9213), (9213, 17000), (17000, total)]:
        b.run_iq(xd[a:e])
        t.run_iq(xd[a:e])
        if e == 9213:
            ck.drain()
    got = ck.drain(heard=True)
    assert ck.twin_frames >= 4 and ck.records <= 3 and ck.records < ck.twin_frames
    ck.end()


def test_heard_equals_the_unique_drain_of_a_twin_and_the_restatement(seventy):
    """two batches with the merge on get the same calls; one drains with the lists, one without, drain by drain"""
    b, t = pair(70, 128, hash_bits=3)
    u, _ = pair(70, 128)
    ck = Check(b, t, 128)
    xd = dev(seventy)
    cuts = ur.ragged_cuts(lur.TOTAL_G)
    members = 0
    for a, e in zip(cuts[:-1], cuts[1:]):
        for r in (b, t, u):
            r.run(xd[a:e])
        f, c, first, mem = ck.drain(heard=True)
        uf, uc = u.drain_long_frames_unique()
        assert f.tobytes() == uf.tobytes() and c.tobytes() == uc.tobytes()
        assert b.long_unique_late() == u.long_unique_late()
        for i in range(len(f)):                 # the primary is one of the members
            m = mem[first[i]:first[i + 1]]
            hit = m[(m["channel"] == f[i]["channel"]) & (m["t"] == f[i]["t"])]
            assert len(hit) == 1 and int(hit["flags"][0]) == int(f[i]["flags"])
        members += len(mem)
    assert members + b.long_unique_late() == ck.twin_frames > 150
    ck.end()


def test_a_node_merges_copies_that_lie_on_different_shards(seven):
    from gnuais_amd.shard import ReceiverNode
    nd, tw = (ReceiverNode(7, devices=[0, 0], max_len=lur.TOTAL7) for _ in range(2))
    assert len(nd.shards) == 2
    with pytest.raises(GnuaisError) as e:
        nd.long_unique(128)                     # the node does not decode long frames yet
    assert e.value.code == E_STATE
    for r in (nd, tw):
        r.long_frames(True)
    nd.long_unique(128)
    ref = lur.LongUniqueRef(128)
    cuts = lur.ragged_cuts7()
    n_rec = n_twin = copies = 0
    for k, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
        for r in (nd, tw):
            r.run_host(seven[a:e])
            r.sync()
        fr = tw.drain_long_frames()
        if k & 1:
            got, want = nd.drain_long_frames_unique(), ref.push(fr, int(e))
        else:
            got, want = nd.drain_long_frames_heard(), ref.push_heard(fr, int(e))
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and len(got) == len(want)
        assert nd.long_unique_late() == ref.late
        n_rec, n_twin, copies = n_rec + len(got[0]), n_twin + len(fr), copies + int(got[1].sum())
    assert n_twin == 34 and n_rec == 5 and copies + nd.long_unique_late() == 34
    assert nd.drain_frames().tobytes() == tw.drain_frames().tobytes() and nd.counters().tobytes() == tw.counters().tobytes()
    assert nd.pll_state().tobytes() == tw.pll_state().tobytes()
    nd.reset()
    assert nd.long_unique_late() == 0
    nd.long_frames(False)                       # switches the node's merge off as well
    with pytest.raises(GnuaisError) as e:
        nd.drain_long_frames_unique()
    assert e.value.code == E_STATE
    nd.close()
    tw.close()


def test_one_larger_shape(seventy):
    """the seventy receivers tiled to 2030 channels: every transmission is heard by up to 7 x 29 receivers, 29 of them at
    the same row"""
    xt = dev(seventy).repeat(1, 29).contiguous()
    n_ch = xt.shape[1]
    b, t = pair(n_ch, 128)
    ck = Check(b, t, 128)
    for r in (b, t):
        r.run(xt)
    got = ck.drain(heard=True)
    assert ck.twin_frames > 150 * 29 and 25 <= ck.records <= 30 and got[1].max() == 7 * 29
    ck.end()


def test_decode_file_prints_each_long_transmission_once_with_its_hearers(seven, tmp_path):
    """scripts/decode_file.py --long --unique ROWS --heard on the seven receivers, written as a capture: the 34 copies of
    the five long transmissions are printed once each, with a line of who heard them"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "capture.s16")
    seven.tofile(path)
    run = lambda *a: subprocess.run([sys.executable, os.path.join(root, "scripts", "decode_file.py"), path, "--raw", "7",
                                     "--call", "8192", *a], check=True, capture_output=True, timeout=300)
    plain, merged = run("--long"), run("--long", "--unique", "128", "--heard")
    assert b"34 long frames (more than two slots)\n" in plain.stderr
    assert (b"5 long frames (more than two slots), printed once from 34 copies, 0 more copies came after their "
            b"transmission was printed\n") in merged.stderr
    heard = [l for l in merged.stdout.split(b"\n") if l.startswith(b"  heard: ")]
    assert sorted(l.count(b",") + 1 for l in heard)[-5:] == [7, 7, 7, 7, 7] and 6 <= len(heard) <= 7
    assert merged.stdout.count(b"!AIVDM") < plain.stdout.count(b"!AIVDM")


def test_a_ring_that_overflowed_is_reported_with_what_it_held_merged():
    """as gnuais_batch_drain_long_frames reports it: GNUAIS_E_OVERFLOW, the oldest records, here merged (untimed records
    from decode_bits: each by itself, in the plain drain's order); the next drain is clean"""
    from gnuais_amd.lib import E_OVERFLOW
    N = 1                                       # one channel: which records a full ring kept does not depend on append order
    b, t = pair(N, 128, max_len=2048)
    cap = int(b.info("long_frame_cap"))
    one = np.concatenate([lr.burst(np.frombuffer(lur.short_long_payload(30), dtype=np.uint8)), np.zeros(2, np.uint8)])
    for _ in range(cap // N + 2):
        b.decode_bits([one] * N)
        t.decode_bits([one] * N)
    with pytest.raises(GnuaisError) as e:
        b.drain_long_frames_heard()
    with pytest.raises(GnuaisError) as et:
        t.drain_long_frames()
    assert e.value.code == et.value.code == E_OVERFLOW and len(et.value.frames) == cap
    want = lur.LongUniqueRef(128).push_heard(et.value.frames, int(t.info("rows")))
    assert len(e.value.frames) == 4 and all(g.tobytes() == w.tobytes() for g, w in zip(e.value.frames, want))
    assert len(e.value.frames[0]) == cap and b.pending_long_frames() == 0 and b.long_unique_late() == 0
    b.decode_bits([one] * N)
    f, c = b.drain_long_frames_unique()
    assert len(f) == N and c.tolist() == [1] * N
    assert b.counters().tobytes() == t.counters().tobytes()
