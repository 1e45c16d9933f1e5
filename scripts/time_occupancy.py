"""What the channels' load figures (gnuais_batch_occupancy, occupancy.hip) cost at BASELINE shapes (C3: 16384 x 48000 at
48 kHz; C5: 16384 x 192000 at 192 kHz), device-resident I/Q tiled from 256 base streams as time_iq.py tiles it.

  python scripts/time_occupancy.py --shape C3       ms per run_iq call with the feature on against off (frame times and
                                                    frame signal on in both), two batches on the same box, alternating legs
                                                    of --calls calls; one JSON line (--out FILE)
  python scripts/time_occupancy.py --shape C3 --kernel-only --calls 20
                                                    timed calls alone, for `rocprofv3 --kernel-trace --stats
                                                    --output-format csv -- ...`
  python scripts/time_occupancy.py --summarise STATS.csv [--shape C3]
                                                    occ_code_kernel, occ_cover_kernel and occ_epoch_kernel beside
                                                    frame_signal_kernel and iq_power_kernel, from such a stats file
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

from time_iq import SHAPES, batch_for, device_iq

KERNELS = ("occ_code_kernel", "occ_cover_kernel", "occ_epoch_kernel", "frame_signal_kernel", "iq_power_kernel",
           "frame_time_kernel", "hdlc_crc_kernel", "iq_discriminator_kernel")


def summarise(path, shape):
    out = dict(shape=shape, kernels=[])
    by = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name", r.get("KernelName", ""))
        k = next((k for k in KERNELS if k in name), None)
        if k is None:
            continue
        row = dict(kernel=k, calls=int(r.get("Calls", 0)), mean_ms=round(float(r.get("AverageNs", r.get("Average", 0))) / 1e6, 4),
                   min_ms=round(float(r.get("MinNs", 0)) / 1e6, 4), max_ms=round(float(r.get("MaxNs", 0)) / 1e6, 4),
                   total_ms=round(float(r.get("TotalDurationNs", 0)) / 1e6, 3))
        out["kernels"].append(row)
        by.setdefault(k, row)
    if "frame_signal_kernel" in by:
        fs = by["frame_signal_kernel"]
        out["against_frame_signal_kernel"] = {k: round(by[k]["total_ms"] / max(fs["total_ms"], 1e-9), 2)
                                              for k in KERNELS[:3] if k in by}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="C3")
    ap.add_argument("--calls", type=int, default=20, help="calls per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating on / off leg pairs")
    ap.add_argument("--epoch", type=int, default=1024, help="blocks of an epoch")
    ap.add_argument("--margin", type=int, default=16)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--summarise", metavar="STATS_CSV")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.summarise:
        res = summarise(a.summarise, a.shape)
    else:
        import torch
        assert torch.cuda.is_available(), "time_occupancy.py measures on the GPU"
        n_ch, total, sps = SHAPES[a.shape]
        xd = device_iq(n_ch, total, sps)
        on = batch_for(a.shape, n_ch, total)
        on.frame_times(True)
        on.frame_signal(True)
        on.occupancy(a.epoch, a.margin)

        def leg(batch, calls):
            for _ in range(3):                       # warm-up
                batch.run_iq(xd, sync=False)
                batch.discard_frames()
            batch.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                batch.run_iq(xd, sync=False)
                batch.discard_frames()
            batch.sync()
            return (time.perf_counter() - t0) * 1e3 / calls

        if a.kernel_only:
            leg(on, a.calls)
            first, rec = on.drain_occupancy()
            print(f"{a.calls + 3} timed calls at {a.shape}, {len(first)} epochs final, {on.occupancy_lost()} lost")
            return
        off = batch_for(a.shape, n_ch, total)
        off.frame_times(True)
        off.frame_signal(True)
        on_ms, off_ms = [], []
        for _ in range(a.legs):
            on_ms.append(leg(on, a.calls))
            off_ms.append(leg(off, a.calls))
        first, rec = on.drain_occupancy()
        res = dict(shape=a.shape, n_channels=n_ch, samples=total, calls_per_leg=a.calls, epoch_blocks=a.epoch,
                   on_ms=[round(v, 4) for v in on_ms], off_ms=[round(v, 4) for v in off_ms],
                   on_median_ms=round(float(np.median(on_ms)), 4), off_median_ms=round(float(np.median(off_ms)), 4),
                   added_ms=round(float(np.median(on_ms) - np.median(off_ms)), 4),
                   off_spread_ms=round(float(max(off_ms) - min(off_ms)), 4),
                   epochs_held=int(len(first)), epochs_lost=int(on.occupancy_lost()),
                   mean_load=round(float(rec["busy"].mean() / a.epoch), 4) if len(first) else None)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
