"""What the long-frame decoder (gnuais_batch_long_frames, hdlc_long.hip) costs at the C3 shape (16384 x 48000 at 48 kHz),
device-resident audio tiled from 256 base streams as bench.py tiles it.

  python scripts/time_long_frames.py [--out FILE]     ms per run call, three cases on the same box in alternating legs:
                                                      off      the feature off, bench.py's input (no long frames)
                                                      on       the feature on, the same input: the walk alone
                                                      on_full  the feature on, every channel carrying back-to-back
                                                               126-byte bursts: every lane closes a long frame every
                                                               1100 bits or so
A leg is --groups groups of --calls pipelined calls.  In front of every group the batch is synchronised and, where the
feature is on, switched on again, which empties the long ring (it holds one call's worst case, a few calls of the full
input): that part is not timed, and every case gets the same structure, so the three figures compare with each other; a
group starts from an idle pipeline, so they lie above bench.py's steady state.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from time_iq import SHAPES, batch_for


def device_audio(n_ch, total, sps, payloads=None, k=256):
    import torch
    from gnuais_amd import synth, tile_channels
    if payloads is None:
        base, _ = synth.make_base_streams(k, total, sps=sps, occupancy=0.8)
    else:
        base = np.stack([synth.make_stream(total, channel=c, sps=sps, payloads=payloads)[0] for c in range(k)])
    return tile_channels(torch.from_numpy(base).cuda(), n_ch)


def back_to_back(rng, slot):
    """a 126-byte burst (about 1080 bits, 4.2 slots) every five slots"""
    return bytes(rng.integers(0, 256, 126, dtype=np.uint8)) if slot % 5 == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3, help="calls per group (the long ring must hold them on the full input)")
    ap.add_argument("--groups", type=int, default=8, help="groups per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating legs per case")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_long_frames.py measures on the GPU"
    n_ch, total, sps = SHAPES["C3"]
    bench_in = device_audio(n_ch, total, sps)
    full_in = device_audio(n_ch, total, sps, payloads=back_to_back)
    cases = {"off": (batch_for("C3", n_ch, total), bench_in, False), "on": (batch_for("C3", n_ch, total), bench_in, True),
             "on_full": (batch_for("C3", n_ch, total), full_in, True)}
    for batch, _, on in cases.values():
        if on:
            batch.long_frames(True)

    def group(batch, x, on):
        batch.sync()
        if on:
            batch.long_frames(True)                 # empties the long ring; synchronises
        t0 = time.perf_counter()
        for _ in range(a.calls):
            batch.run(x, sync=False)
            batch.discard_frames()
        batch.sync()
        return time.perf_counter() - t0

    def leg(name):
        batch, x, on = cases[name]
        group(batch, x, on)                         # warm-up
        return sum(group(batch, x, on) for _ in range(a.groups)) * 1e3 / (a.groups * a.calls)

    ms = {name: [] for name in cases}
    for _ in range(a.legs):
        for name in cases:
            ms[name].append(leg(name))
    res = dict(shape="C3", n_channels=n_ch, samples=total, calls_per_group=a.calls, groups_per_leg=a.groups)
    for name in cases:
        res[name + "_ms"] = [round(v, 4) for v in ms[name]]
        res[name + "_median_ms"] = round(float(np.median(ms[name])), 4)
    res["off_spread_ms"] = round(float(max(ms["off"]) - min(ms["off"])), 4)
    res["added_on_ms"] = round(res["on_median_ms"] - res["off_median_ms"], 4)
    res["added_on_full_ms"] = round(res["on_full_median_ms"] - res["off_median_ms"], 4)
    # what the last group of each case delivered (the ring is not drained above: it holds that group's frames)
    for name, (batch, _, on) in cases.items():
        if on:
            res[name + "_long_frames_per_call"] = int(batch.pending_long_frames() // a.calls)
            res[name + "_long_frame_cap"] = int(batch.info("long_frame_cap"))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
