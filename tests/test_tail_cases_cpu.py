"""The input of tests/test_tail_pipelined_gpu.py is worth running: from the restatements alone (tests/tail_cases.py), what
the stages behind the CRC stage have to deliver on it.  A GPU test that compares empty lists passes whatever the device
does, so these floors are asserted here, where no device is needed.

What the restatements give (both call plans, the bits do not depend on the plan): 745 frames received and 49 repaired by
the chain, 253 long frames received and 38 repaired on all 70 channels, 14 occupancy epochs; 192 long frames are open
across a call boundary in the ragged plan and all 291 in the plan of equal calls; the merges find 297 transmissions heard
twice among the chain's frames and 90 among the long ones.  The floors below sit well under those figures and far above the "half the channels", "at least one" and "a handful" that make the comparison mean something."""
import numpy as np
import pytest

import repair_ref as rr
import tail_cases as tc


def test_the_plans():
    ragged, equal = tc.plan("ragged"), tc.plan("equal")
    assert sum(ragged) == sum(equal) == tc.TOTAL
    assert ragged[:7] == [4096, 1, 2047, 5000, 33, 7000, 4096] and len(ragged) == 22 and max(ragged) == tc.MAX_LEN
    assert equal == [1280] * 48                             # nbuf = 2 takes each hand-off set 24 times


def test_no_channel_is_a_turned_copy_of_another():
    """a stage that reads another call's hand-off set must change a result: no two channels carry the same frames or
    the same samples"""
    e = tc.build("ragged")
    per = [e.frames[e.frames["channel"] == c] for c in range(tc.N_CH)]
    seen = set()
    for p in per:
        short = tuple(bytes(f["payload"]) for f in p if f["nbits"] == 168)
        assert len(short) >= 3 and short not in seen
        seen.add(short)
    x = tc.iq_input()
    assert len({x[:, c].tobytes() for c in range(tc.N_CH)}) == tc.N_CH


@pytest.mark.parametrize("name", ["ragged", "equal"])
def test_the_input_is_worth_running(name):
    e = tc.build(name)
    w = e.worth
    assert w["calls"] >= 12
    assert w["long_channels"] >= 60                         # long frames on at least half the channels: all 70
    assert w["long_across_calls"] >= 100                    # open across a call boundary: 192 (ragged), 291 (equal)
    assert w["long_received"] >= 200 and w["long_repaired"] >= 20       # 253 and 38
    assert w["short_received"] >= 600 and w["short_repaired"] >= 40     # 745 and 49
    assert w["epochs"] == 14 and w["epochs_before_the_last_call"] >= 10   # final in calls other than the last
    rep = (e.frames["flags"] & rr.FRAME_REPAIRED) != 0
    assert rep.sum() == e.repaired.sum() == w["short_repaired"]
    assert (e.times >= 0).all() and (e.signal["blocks"] > 0).sum() > 700    # nearly every frame is measured
    assert {int(n) for n in e.long_records["nbits"]} >= {432, 480, 640, 800, 1008}
    lrep = (e.long_records["flags"] & rr.FRAME_REPAIRED) != 0
    assert lrep.sum() == w["long_repaired"] and (e.long_records["t"] > 0).all()
    assert len(e.occ_first) == 14 and sum(int(r["covered"].sum()) for r in e.occ_records) > 1000
    short, long_ = tc.heard(e, tc.TOTAL)
    assert (short[2] == 2).sum() >= 200 and (long_[1] == 2).sum() >= 60      # duplicate clusters: 297 and 90
    assert (short[2] == 1).sum() >= 100 and (long_[1] == 1).sum() >= 60      # and transmissions heard once: 200 and 111
    # the input ends in noise: every machine hunts for a preamble, but they stand in eight different states
    assert len(set(e.long_fsm)) >= 5


def test_the_plans_differ_in_the_times_only():
    a, b = tc.build("ragged"), tc.build("equal")
    assert a.frames.tobytes() == b.frames.tobytes() and not np.array_equal(a.times, b.times)
    assert np.abs(a.times - b.times).max() <= 5             # the definition interpolates per segment: a bit or so
    assert np.array_equal(a.long_counters3, b.long_counters3) and a.long_fsm == b.long_fsm


def test_the_reset_and_protodec_reset_expectations_differ_from_the_plain_one():
    """what the switch cases of the GPU test compare with: a reset in front of call 11 is a fresh batch from that row on;
    a protodec_reset there drops the frames in progress and keeps the counters"""
    plain, fresh, pd = tc.build("ragged"), tc.build("ragged", first_call=11), tc.build("ragged", protodec_at=11)
    assert fresh.calls == plain.calls[11:] and len(fresh.calls) == 11
    assert 250 < len(fresh.frames) < len(plain.frames) - 250 and fresh.times.min() < 2 * 1280
    assert 80 < len(fresh.long_records) < len(plain.long_records) - 80
    assert 0 < len(fresh.occ_first) < 14 and fresh.occ_first[0] == 0
    lost = len(plain.frames) + len(plain.long_records) - len(pd.frames) - len(pd.long_records)
    assert 5 <= lost <= tc.N_CH                             # at most the one frame each channel was in
    assert pd.counters.sum() < plain.counters.sum() and len(pd.occ_first) == 14
