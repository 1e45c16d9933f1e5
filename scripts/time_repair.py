"""What the repair of CRC-failed frames (gnuais_batch_repair, hdlc_repair.hip) costs at BASELINE shapes (C3: 16384 x 48000
at 48 kHz; C5: 16384 x 192000 at 192 kHz), device-resident audio tiled from 256 base streams as bench.py tiles it.
--sigma sets the noise of the base streams: 1000 is the bench's input (few failed candidates), 6000 the weak-signal case
(most candidates fail).

  python scripts/time_repair.py --shape C3          ms per run call with the feature on against off, two batches on the
                                                    same box, alternating legs of --calls calls; one JSON line (--out FILE)
                                                    with the failed candidates and the repairs per call
  python scripts/time_repair.py --shape C3 --kernel-only --calls 20
                                                    timed calls alone, for `rocprofv3 --kernel-trace --stats
                                                    --output-format csv -- ...`
  python scripts/time_repair.py --summarise STATS.csv
                                                    hdlc_repair_kernel's and hdlc_crc_kernel's times from such a stats file
"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from time_iq import SHAPES, batch_for


def device_audio(n_ch, total, sps, sigma, k=256):
    import torch
    from gnuais_amd import synth, tile_channels
    base, _ = synth.make_base_streams(k, total, sps=sps, occupancy=0.8, sigma=sigma)
    return tile_channels(torch.from_numpy(base).cuda(), n_ch)


def summarise(path):
    out = dict(kernels=[])
    for r in csv.DictReader(open(path)):
        name = r.get("Name", r.get("KernelName", ""))
        if "hdlc_repair_kernel" in name or "hdlc_crc_kernel" in name:
            out["kernels"].append(dict(kernel=name.split("(")[0], calls=int(r.get("Calls", 0)),
                                       mean_ms=round(float(r.get("AverageNs", r.get("Average", 0))) / 1e6, 4),
                                       min_ms=round(float(r.get("MinNs", 0)) / 1e6, 4),
                                       max_ms=round(float(r.get("MaxNs", 0)) / 1e6, 4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="C3")
    ap.add_argument("--calls", type=int, default=20, help="calls per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating on / off leg pairs")
    ap.add_argument("--sigma", type=float, default=1000.0, help="noise of the base streams (amplitude 12000)")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--summarise", metavar="STATS_CSV")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.summarise:
        res = summarise(a.summarise)
    else:
        import torch
        assert torch.cuda.is_available(), "time_repair.py measures on the GPU"
        n_ch, total, sps = SHAPES[a.shape]
        xd = device_audio(n_ch, total, sps, a.sigma)
        on = batch_for(a.shape, n_ch, total)
        on.repair(True)

        def leg(batch, calls):
            for _ in range(3):                       # warm-up
                batch.run(xd, sync=False)
                batch.discard_frames()
            batch.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                batch.run(xd, sync=False)
                batch.discard_frames()
            batch.sync()
            return (time.perf_counter() - t0) * 1e3 / calls

        if a.kernel_only:
            leg(on, a.calls)
            print(f"{a.calls + 3} timed calls at {a.shape}")
            return
        off = batch_for(a.shape, n_ch, total)
        on_ms, off_ms = [], []
        for _ in range(a.legs):
            on_ms.append(leg(on, a.calls))
            off_ms.append(leg(off, a.calls))
        calls = a.legs * (a.calls + 3)
        res = dict(shape=a.shape, n_channels=n_ch, samples=total, sigma=a.sigma, calls_per_leg=a.calls,
                   on_ms=[round(v, 4) for v in on_ms], off_ms=[round(v, 4) for v in off_ms],
                   on_median_ms=round(float(np.median(on_ms)), 4), off_median_ms=round(float(np.median(off_ms)), 4),
                   added_ms=round(float(np.median(on_ms) - np.median(off_ms)), 4),
                   off_spread_ms=round(float(max(off_ms) - min(off_ms)), 4),
                   frames_per_call=int(on.counters()["receivedframes"].sum() // calls),
                   failed_candidates_per_call=int(on.counters()["lostframes"].sum() // calls),
                   repaired_per_call=int(on.repaired().sum() // calls),
                   failed_candidates_per_call_off=int(off.counters()["lostframes"].sum() // calls))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
