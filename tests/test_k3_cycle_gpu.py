"""The serial cycle deframer -> K3 -> discard (gnuais_capi.hip run_tail, capi_delivery.hip, hdlc_crc.hip), against the
CPU restatement: a discard that leaves no dispatch behind (it rides on the next deframer launch, or becomes the memset
it was for whoever looks at the ring first), in every order a caller can mix it with runs, drains and resets, with and
without the pipeline; and K3 at its own edges -- a partial last block, a block boundary in mid batch, 255 / 256 / 257
candidates in a block, no / one / the most stuffed bits, the shortest and the longest frames, a frame one bit off --
frame records byte for byte, in order, and the counters per channel.  Bit-exact, no tolerance anywhere."""
import functools

import numpy as np
import pytest

import deframer_cases as dc
from chain_parity import batch, dev
from gnuais_amd import synth
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

N_CH, CALL = 64, 4096
GAP = np.zeros(6, dtype=np.uint8)


def counters3(b):
    cnt = b.counters()
    return np.stack([cnt["receivedframes"], cnt["lostframes"], cnt["lostframes2"]], axis=1)


@functools.lru_cache(maxsize=None)
def calls():
    """three calls of 64 channels x 4096 samples of `synth` input, and the restatement's frames of each call alone
    (a frame that straddles two calls closes in the later one), of the first call on a fresh receiver, and its counters
    after each"""
    x = np.stack([synth.make_stream(3 * CALL, seed=23, channel=c, occupancy=0.9)[0] for c in range(N_CH)], axis=1)
    xs = [np.ascontiguousarray(x[i * CALL:(i + 1) * CALL]) for i in range(3)]
    o = Oracle(N_CH)
    frames, cnt = [], []
    for seg in xs:
        o.clear_frames()
        o.run(seg)
        frames.append(o.frames().copy())
        cnt.append(o.counters().copy())
    assert all(len(f) >= N_CH // 2 for f in frames), [len(f) for f in frames]
    return xs, frames, cnt


def new_batch(pipeline, variant=1):
    b = batch(N_CH, max_len=CALL)
    b.set_option("pipeline", pipeline)
    b.set_option("hdlc_variant", variant)
    return b


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("pipeline", [1, 0])
def test_run_discard_run_drain_is_the_second_call(pipeline, variant):
    xs, frames, cnt = calls()
    b = new_batch(pipeline, variant)
    b.run(dev(xs[0]), sync=False)
    b.discard_frames()
    b.run(dev(xs[1]), sync=False)
    got = b.drain_frames()
    assert len(got) == len(frames[1]) and got.tobytes() == frames[1].tobytes()
    assert np.array_equal(counters3(b), cnt[1])             # the counters are not the ring's: nothing of them is discarded
    assert b.pending_frames() == 0
    # ... and the ring goes on from there: a third call, nothing discarded
    b.run(dev(xs[2]))
    assert b.drain_frames().tobytes() == frames[2].tobytes()
    b.close()


@pytest.mark.parametrize("pipeline", [1, 0])
def test_run_discard_drain_is_empty(pipeline):
    xs, frames, cnt = calls()
    b = new_batch(pipeline)
    b.run(dev(xs[0]), sync=False)
    b.discard_frames()
    assert b.pending_frames() == 0 and len(b.drain_frames()) == 0
    assert np.array_equal(counters3(b), cnt[0])
    b.run(dev(xs[1]))                                       # the discard is spent: this call's frames stay
    assert b.drain_frames().tobytes() == frames[1].tobytes()
    b.close()


@pytest.mark.parametrize("pipeline", [1, 0])
def test_discard_discard_run_drain(pipeline):
    xs, frames, cnt = calls()
    b = new_batch(pipeline)
    b.discard_frames()
    b.discard_frames()
    b.run(dev(xs[0]), sync=False)
    assert b.drain_frames().tobytes() == frames[0].tobytes()
    b.run(dev(xs[1]), sync=False)
    b.discard_frames()
    b.discard_frames()                                      # two in a row are one
    b.run(dev(xs[2]), sync=False)
    assert b.drain_frames().tobytes() == frames[2].tobytes()
    assert np.array_equal(counters3(b), cnt[2])
    b.close()


@pytest.mark.parametrize("pipeline", [1, 0])
def test_discard_then_a_call_without_the_deframer(pipeline):
    """stage_mask 0x03 runs the FIR and the PLL stage only: no deframer launch for the discard to ride on, so it takes
    effect as the memset -- the drain is empty -- and does not wait for a later launch to wipe that launch's frames"""
    xs, frames, cnt = calls()
    b = new_batch(pipeline)
    b.run(dev(xs[0]), sync=False)
    b.discard_frames()
    b.set_option("stage_mask", 0x03)
    b.run(dev(xs[1]), sync=False)
    assert b.pending_frames() == 0 and len(b.drain_frames()) == 0
    assert np.array_equal(counters3(b), cnt[0])             # K3 did not run
    b.set_option("stage_mask", 0x1f)
    b.reset()                                               # (the masked call left the stages' states apart)
    b.run(dev(xs[0]))
    assert b.drain_frames().tobytes() == frames[0].tobytes()
    b.close()


@pytest.mark.parametrize("pipeline", [1, 0])
def test_discard_then_reset(pipeline):
    xs, frames, cnt = calls()
    b = new_batch(pipeline)
    b.run(dev(xs[0]), sync=False)
    b.discard_frames()
    b.reset()
    assert b.pending_frames() == 0
    b.run(dev(xs[0]), sync=False)                           # a reset receiver, and no discard left over to wipe this
    assert b.drain_frames().tobytes() == frames[0].tobytes()
    assert np.array_equal(counters3(b), cnt[0])
    b.close()


def test_discard_then_bits_and_discard_into_streaming():
    """gnuais_batch_decode_bits launches a deframer too (it carries the discard); the switch to the streamed delivery
    hands ring 0 out (a pending discard takes effect first)"""
    xs, frames, cnt = calls()
    streams = [dc.STREAMS["good21_twice"]] * N_CH
    o = Oracle(N_CH)
    for c, s in enumerate(streams):
        o.decode_bits(c, s)
    b = batch(N_CH, max_len=CALL)
    b.run(dev(xs[0]), sync=False)
    b.discard_frames()
    b.reset()
    b.decode_bits(streams)
    b.discard_frames()
    b.protodec_reset()
    b.decode_bits(streams)                                  # the second pair of frames alone, 610 bits later in time
    got = b.drain_frames()
    want = o.frames()
    assert len(got) == len(want) == 2 * N_CH
    assert got["payload"].tobytes() == want["payload"].tobytes() and np.array_equal(got["channel"], want["channel"])
    b.reset()
    b.run(dev(xs[0]), sync=False)
    b.discard_frames()
    texts = [b.stream_nmea() for _ in range(b.stream_depth + 2)]
    assert sum(t[1] for t in texts) == 0 and b"".join(t[0] for t in texts) == b""
    b.close()


# ---------------------------------------------------------------- K3 at its own edges

def framed(body):
    return np.concatenate([synth.hdlc_frame_bits(bytes(body)), GAP])


def stuffed_bits(body):
    return synth.hdlc_frame_bits(bytes(body)).size - synth.hdlc_frame_bits(bytes(body), stuff=False).size


@functools.lru_cache(maxsize=None)
def edge_pool():
    """name -> one frame's on-air bits: bodies with no, one and the most stuffed bits (the all-ones body of the longest
    frame: the longest raw record a candidate can have), the shortest and the longest lengths around what the CRC stage
    accepts, a frame one data bit off, and the deframer's own boundary streams"""
    rng = np.random.default_rng(3)
    pool = {}
    want = {0: None, 1: None}
    while any(v is None for v in want.values()):
        body = rng.integers(0, 256, 21, dtype=np.uint8).tobytes()
        k = stuffed_bits(body)
        if k in want and want[k] is None:
            want[k] = body
    pool["stuffed0"], pool["stuffed1"] = framed(want[0]), framed(want[1])
    pool["stuffed_most"] = framed(b"\xff" * 53)
    assert stuffed_bits(b"\xff" * 53) >= 84
    for n in (0, 1, 2, 3, 4, 52, 53, 54):                  # both sides of the shortest and of the longest accepted length
        pool["len%d" % n] = framed(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    for name in ("crc_bad", "good21_twice", "ff_stuffed", "max53", "ff53", "over55", "short_frames", "dense", "stop_then_one"):
        pool[name] = np.concatenate([dc.STREAMS[name], GAP])
    return pool


def edge_streams(n_ch):
    pool = edge_pool()
    names = sorted(pool)
    rng = np.random.default_rng(100 + n_ch)
    out = []
    for c in range(n_ch):
        pick = [names[(c + 7 * k) % len(names)] for k in range(3)] if c % 5 else []     # every fifth channel: nothing at all
        rng.shuffle(pick)
        out.append(np.concatenate([GAP] + [pool[n] for n in pick]).astype(np.uint8))
    return out


def compare_bits(streams, max_len=48000, variant=1, split=None):
    """decode_bits of the streams (split: in two calls at that bit) on the batch and the restatement"""
    n_ch = len(streams)
    o = Oracle(n_ch)
    for c, s in enumerate(streams):
        o.decode_bits(c, s)
    b = batch(n_ch, max_len=max_len)
    b.set_option("hdlc_variant", variant)
    if split is None:
        b.decode_bits(streams)
    else:
        b.decode_bits([s[:split] for s in streams])
        b.decode_bits([s[split:] for s in streams])
    got, want = b.drain_frames(), o.frames()
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(counters3(b), o.counters())
    b.close()
    return o


@pytest.mark.parametrize("n_ch", [31, 32, 33, 65])
def test_partial_blocks_and_a_block_boundary_in_mid_batch(n_ch):
    streams = edge_streams(n_ch)
    o = compare_bits(streams)
    cnt = o.counters()
    assert cnt[:, 0].sum() >= n_ch and cnt[:, 1].sum() >= n_ch // 2         # good frames and failed candidates in every block
    compare_bits(streams, split=300)                        # the same in two launches: frames in progress across them


def test_the_edge_frames_one_by_one():
    """every frame of the pool on a channel of its own: what is accepted and what is not is the restatement's word"""
    pool = edge_pool()
    names = sorted(pool)
    o = compare_bits([pool[n] for n in names])
    cnt = {n: o.counters()[i].tolist() for i, n in enumerate(names)}
    assert cnt["stuffed0"] == cnt["stuffed1"] == cnt["stuffed_most"] == [1, 0, 0]
    assert cnt["len1"] == cnt["len53"] == [1, 0, 0], cnt    # the shortest and the longest frame the CRC stage accepts
    assert cnt["len0"][0] == 0 and cnt["len54"][0] == 0, cnt
    assert cnt["crc_bad"] == [0, 1, 0]


DENSE_DATA = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 1, 0, 0, 1, 0], dtype=np.uint8)
DENSE = np.concatenate([(np.arange(16) & 1).astype(np.uint8), dc.FLAG, DENSE_DATA, dc.FLAG])   # 62 bits: one candidate, CRC fails


def block_streams(total, seed, each=8):
    """32 channels whose candidates number `total`, `each` on all but the last: a good 3-byte frame among dense cycles
    (one failed candidate each), the good frames in different places so that some land on each side of a pass boundary"""
    rng = np.random.default_rng(seed)
    per = [each] * 31 + [total - each * 31]
    out = []
    for c, n in enumerate(per):
        good = synth.hdlc_frame_bits(rng.integers(0, 256, 3, dtype=np.uint8).tobytes())
        at = c % n
        parts = [DENSE] * at + [good, GAP] + [DENSE] * (n - 1 - at)
        out.append(np.concatenate(parts).astype(np.uint8))
    return out


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("total", [255, 256, 257])
def test_a_block_with_255_256_257_candidates(total, variant):
    """max_len 4096: a launch takes 960 bits per channel, so every channel's candidates close in ONE K3 launch and the
    first block's candidate number 256 is the last of a pass, the first of the next, or one short of it.  A second
    block (a partial one) of two and a bit passes follows."""
    streams = block_streams(total, total) + block_streams(320, 9, each=10)[:29]
    assert max(s.size for s in streams) <= 960
    o = compare_bits(streams, max_len=4096, variant=variant)
    cnt = o.counters()
    assert cnt[:32, :2].sum() == total and cnt[:32, 0].sum() == 32 and cnt[:, 2].sum() == 0
    assert cnt[32:, :2].sum() == 290


def test_the_repair_still_finds_its_candidates():
    """the repair kernel walks the slots K3 walked (same block -> channel map, cand_first / cand_count)"""
    import repair_ref as rr
    from test_repair_gpu import crafted_channel, records
    n_ch = 33
    streams = [crafted_channel(c)[0] for c in range(n_ch)]
    want, want_rep, want_cnt = rr.decode_streams(streams)
    b = batch(n_ch)
    b.repair(True)
    b.decode_bits(streams)
    got = b.drain_frames()
    assert got.tobytes() == records(want).tobytes()
    assert np.array_equal(counters3(b), want_cnt) and np.array_equal(b.repaired(), want_rep) and want_rep.sum() == n_ch
    b.close()


def test_the_streamed_text_still_follows_the_chunk_table():
    """stream_nmea takes a one-launch ring's order from K3's chunk table (block, pass, position): a block of 257
    candidates, two passes, and a partial block behind it"""
    from gnuais_amd import nmea_from_frames
    streams = block_streams(257, 5) + block_streams(320, 6, each=10)[:29]
    n_ch = len(streams)
    o = Oracle(n_ch)
    for c, s in enumerate(streams):
        o.decode_bits(c, s)
    frames = o.frames()
    assert len(frames) == n_ch
    want = nmea_from_frames(frames, np.zeros(n_ch, dtype=np.uint8))
    b = batch(n_ch, max_len=4096)
    texts = [b.stream_nmea()]                               # switches the delivery on: K3 moves to a fresh ring
    b.decode_bits(streams)
    texts += [b.stream_nmea() for _ in range(b.stream_depth + 1)]
    assert b"".join(t[0] for t in texts) == want
    assert sum(max(t[2], 0) for t in texts) == n_ch
    b.close()
