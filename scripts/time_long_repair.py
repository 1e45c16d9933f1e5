"""What the repair of long frames (gnuais_batch_long_repair: hdlc_long.hip's form that keeps the raw bits, and
hdlc_long_repair.hip behind it) costs at the C3 shape (16384 x 48000 at 48 kHz), device-resident audio tiled from 256 base
streams as bench.py tiles it.

  python scripts/time_long_repair.py [--out FILE]     ms per run call, three cases on the same box in alternating legs:
                                                      long         long frames on, the repair off, bench.py's input: the
                                                                   baseline
                                                      repair       the repair on, the same input (no long frame fails):
                                                                   the other form of D' and the empty repair launch
                                                      repair_full  the repair on, every channel carrying back-to-back
                                                                   126-byte bursts, each with ONE wrong symbol: every
                                                                   lane lists a candidate every 1100 bits or so
The structure is scripts/time_long_frames.py's: a leg is --groups groups of --calls pipelined calls; in front of every
group the batch is synchronised and long frames are switched on again (which empties the long ring and, for the last two
cases, is followed by switching the repair on again); that part is not timed.  A group starts from an idle pipeline, so
the figures lie above bench.py's steady state and compare with each other.
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
from time_long_frames import device_audio


def damaged_base(k, total, sps):
    """k base streams like synth.make_stream's with a 126-byte burst every five slots, one symbol of each inverted: the
    NRZI level of one symbol is wrong, which is two adjacent wrong bits behind the decoder"""
    from gnuais_amd import synth
    out = np.empty((k, total), dtype=np.int16)
    slot_len = synth.SLOT_BITS * sps
    n_slots = (total + slot_len - 1) // slot_len
    for c in range(k):
        rng = np.random.default_rng([synth.SEED, c])
        level = np.zeros(n_slots * slot_len + 64 * sps, dtype=np.float64)
        for slot in range(0, n_slots, 5):
            bits = synth.hdlc_frame_bits(bytes(rng.integers(0, 256, 126, dtype=np.uint8)))
            lev = synth.nrzi_levels(bits, start_level=int(rng.integers(0, 2)))
            lev[int(rng.integers(48, bits.size - 16))] *= -1
            lev = np.repeat(lev, sps)
            start = slot * slot_len + synth.START_OFFSET_BITS * sps
            end = min(start + lev.size, level.size)
            level[start:end] = lev[: end - start]
        shaped = np.convolve(level, synth.gaussian_kernel(sps), mode="same")[:total]
        x = np.rint(12000.0 * shaped + rng.normal(0.0, 1000.0, total))
        out[c] = np.clip(x, -32768, 32767).astype(np.int16)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3, help="calls per group (the long ring must hold them on the full input)")
    ap.add_argument("--groups", type=int, default=8, help="groups per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating legs per case")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from gnuais_amd import tile_channels
    assert torch.cuda.is_available(), "time_long_repair.py measures on the GPU"
    n_ch, total, sps = SHAPES["C3"]
    bench_in = device_audio(n_ch, total, sps)
    full_in = tile_channels(torch.from_numpy(damaged_base(256, total, sps)).cuda(), n_ch)
    cases = {"long": (batch_for("C3", n_ch, total), bench_in, False), "repair": (batch_for("C3", n_ch, total), bench_in, True),
             "repair_full": (batch_for("C3", n_ch, total), full_in, True)}

    def group(batch, x, repair):
        batch.sync()
        batch.long_frames(True)                     # empties the long ring; synchronises
        if repair:
            batch.long_repair(True)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            batch.run(x, sync=False)
            batch.discard_frames()
        batch.sync()
        return time.perf_counter() - t0

    def leg(name):
        batch, x, repair = cases[name]
        group(batch, x, repair)                     # warm-up
        return sum(group(batch, x, repair) for _ in range(a.groups)) * 1e3 / (a.groups * a.calls)

    ms = {name: [] for name in cases}
    for _ in range(a.legs):
        for name in cases:
            ms[name].append(leg(name))
    res = dict(shape="C3", n_channels=n_ch, samples=total, calls_per_group=a.calls, groups_per_leg=a.groups)
    for name in cases:
        res[name + "_ms"] = [round(v, 4) for v in ms[name]]
        res[name + "_median_ms"] = round(float(np.median(ms[name])), 4)
    res["long_spread_ms"] = round(float(max(ms["long"]) - min(ms["long"])), 4)
    res["added_repair_ms"] = round(res["repair_median_ms"] - res["long_median_ms"], 4)
    res["added_repair_full_ms"] = round(res["repair_full_median_ms"] - res["long_median_ms"], 4)
    # what the last group of each case did (the ring is not drained above: it holds that group's frames)
    for name, (batch, _, repair) in cases.items():
        d, f = batch.long_counters()
        res[name + "_per_call"] = dict(delivered=int(d.sum() // a.calls), failed=int(f.sum() // a.calls),
                                       repaired=int(batch.long_repaired().sum() // a.calls))
    res["long_frame_cap"] = int(cases["repair_full"][0].info("long_frame_cap"))
    res["long_cand_cap"] = int(cases["repair_full"][0].info("long_cand_cap"))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
