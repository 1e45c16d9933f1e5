"""What the long frames' signal records and cover (gnuais_batch_long_frame_signal, long_signal.hip) cost at the C3 shape
(16384 x 48000 at 48 kHz): device-resident I/Q tiled from 256 base streams that carry a long burst (54 .. 126 bytes) every
six slots and a position report in half of the slots in front of them, with long frames, the long repair, frame times,
frame signal and the occupancy on.

  python scripts/time_long_signal.py [--out FILE]     ms per run_iq call with the switch on against off, on that input
                                                      ("full": every channel closes five long frames a call) and on
                                                      time_iq.py's, which holds no long frame ("none": the launch alone);
                                                      four batches on the same box in alternating legs; one JSON line
  python scripts/time_long_signal.py --off-only       the off legs alone: the same configuration at a commit where the switch
                                                      does not exist
The structure is scripts/time_long_repair.py's: a leg is --groups groups of --calls pipelined calls; in front of every
group the batch is synchronised and long frames are switched on again (which empties the long ring; the long repair is
switched on again behind it); that part is not timed.  A group starts from an idle pipeline, so the figures lie above
bench.py's steady state and compare with each other.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from time_iq import SHAPES, batch_for, device_iq

LONG_BYTES = (54, 60, 80, 100, 126)


def long_base(k, total, sps):
    """k base streams [total][k][2]: gated bursts over noise, a long one every six slots"""
    from gnuais_amd import synth

    def pick(rng, slot):
        if slot % 6 == 0:
            return bytes(rng.integers(0, 256, LONG_BYTES[slot // 6 % len(LONG_BYTES)], dtype=np.uint8))
        if slot % 6 < 5:                            # the slots a burst of 126 bytes still occupies
            return None
        return synth.random_position_report(rng) if rng.random() < 0.5 else None

    return np.stack([synth.make_iq_stream(total, seed=synth.SEED, channel=c, sps=sps, sigma=800.0, gated=True, payloads=pick,
                                          rate_hz=9600 * sps)[0] for c in range(k)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3, help="calls per group (the long ring must hold them)")
    ap.add_argument("--groups", type=int, default=8, help="groups per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating legs per case")
    ap.add_argument("--epoch", type=int, default=1024, help="blocks of an occupancy epoch")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_long_signal.py measures on the GPU"
    n_ch, total, sps = SHAPES["C3"]
    base = torch.from_numpy(long_base(256, total, sps)).cuda()
    xd = base.repeat(1, n_ch // 256, 1).contiguous()

    def make(on):
        b = batch_for("C3", n_ch, total)
        b.frame_times(True)
        b.frame_signal(True)
        b.long_frames(True)
        b.long_repair(True)
        if on:
            b.long_frame_signal(True)
        b.occupancy(a.epoch, 16)
        return b

    # two inputs: every channel closes five long frames a call; no channel ever does (time_iq.py's position reports)
    inputs = {"full": xd, "none": device_iq(n_ch, total, sps)}
    cases = {f"off_{k}": (make(False), x) for k, x in inputs.items()}
    if not a.off_only:
        cases.update({f"on_{k}": (make(True), x) for k, x in inputs.items()})

    def group(batch, x):
        batch.sync()
        batch.long_frames(True)                     # empties the long ring; synchronises
        batch.long_repair(True)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            batch.run_iq(x, sync=False)
            batch.discard_frames()
        batch.sync()
        return time.perf_counter() - t0

    def leg(batch, x):
        group(batch, x)                             # warm-up
        return sum(group(batch, x) for _ in range(a.groups)) * 1e3 / (a.groups * a.calls)

    ms = {name: [] for name in cases}
    for _ in range(a.legs):
        for name, (batch, x) in cases.items():
            ms[name].append(leg(batch, x))
    res = dict(shape="C3", n_channels=n_ch, samples=total, calls_per_group=a.calls, groups_per_leg=a.groups)
    for name, (batch, _) in cases.items():
        res[name + "_ms"] = [round(v, 4) for v in ms[name]]
        res[name + "_median_ms"] = round(float(np.median(ms[name])), 4)
        d, f = batch.long_counters()
        res[name + "_long_per_call"] = int((d.sum() + batch.long_repaired().sum()) // a.calls)
    for k in inputs:
        res[f"off_{k}_spread_ms"] = round(float(max(ms[f"off_{k}"]) - min(ms[f"off_{k}"])), 4)
        if not a.off_only:
            res[f"added_{k}_ms"] = round(res[f"on_{k}_median_ms"] - res[f"off_{k}_median_ms"], 4)
    if not a.off_only:
        res["occupancy_lag_rows"] = dict(on=int(cases["on_full"][0].info("occupancy_lag")),
                                         off=int(cases["off_full"][0].info("occupancy_lag")))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
