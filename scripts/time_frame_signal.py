"""What the frames' signal records (gnuais_batch_frame_signal, frame_signal.hip) cost at BASELINE shapes (C3: 16384 x 48000
at 48 kHz; C5: 16384 x 192000 at 192 kHz), device-resident I/Q tiled from 256 base streams as time_iq.py tiles it.

  python scripts/time_frame_signal.py --shape C3    ms per run_iq call with the feature on against off (frame times on in
                                                    both), two batches on the same box, alternating legs of --calls calls;
                                                    one JSON line (--out FILE)
  python scripts/time_frame_signal.py --shape C3 --kernel-only --calls 20
                                                    timed calls alone, with the AFC on so that afc_apply_kernel runs beside
                                                    the ingest kernel, for `rocprofv3 --kernel-trace --stats
                                                    --output-format csv -- ...`
  python scripts/time_frame_signal.py --summarise STATS.csv [--shape C3]
                                                    iq_power_kernel against afc_apply_kernel (both move 4 bytes a sample; the
                                                    gate: mean <= afc_apply's mean + its own min-max spread) and
                                                    frame_signal_kernel beside hdlc_crc_kernel, from such a stats file
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

KERNELS = ("iq_power_kernel", "afc_apply_kernel", "frame_signal_kernel", "hdlc_crc_kernel", "frame_time_kernel",
           "iq_discriminator_kernel")


def summarise(path, shape):
    n_ch, total, _ = SHAPES[shape]
    out = dict(shape=shape, kernels=[])
    by = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name", r.get("KernelName", ""))
        k = next((k for k in KERNELS if k in name), None)
        if k is None:
            continue
        row = dict(kernel=k, instance=name.split("(")[0] if "anonymous" not in name else k, calls=int(r.get("Calls", 0)),
                   mean_ms=round(float(r.get("AverageNs", r.get("Average", 0))) / 1e6, 4),
                   min_ms=round(float(r.get("MinNs", 0)) / 1e6, 4), max_ms=round(float(r.get("MaxNs", 0)) / 1e6, 4))
        out["kernels"].append(row)
        by.setdefault(k, row)
    if "iq_power_kernel" in by and "afc_apply_kernel" in by:
        p, a = by["iq_power_kernel"], by["afc_apply_kernel"]
        bound = a["mean_ms"] + (a["max_ms"] - a["min_ms"])
        out["ingest"] = dict(mean_ms=p["mean_ms"], tb_per_s=round(n_ch * total * 4 / (p["mean_ms"] / 1e3) / 1e12, 3),
                             afc_apply_mean_ms=a["mean_ms"], afc_apply_spread_ms=round(a["max_ms"] - a["min_ms"], 4),
                             gate_ms=round(bound, 4), within_gate=bool(p["mean_ms"] <= bound))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="C3")
    ap.add_argument("--calls", type=int, default=20, help="calls per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating on / off leg pairs")
    ap.add_argument("--afc", type=int, default=2048, help="--kernel-only: the AFC window (afc_apply_kernel is the yardstick)")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--summarise", metavar="STATS_CSV")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.summarise:
        res = summarise(a.summarise, a.shape)
    else:
        import torch
        assert torch.cuda.is_available(), "time_frame_signal.py measures on the GPU"
        n_ch, total, sps = SHAPES[a.shape]
        xd = device_iq(n_ch, total, sps)
        on = batch_for(a.shape, n_ch, total)
        if a.kernel_only and a.afc:
            on.afc(a.afc)
        on.frame_times(True)
        on.frame_signal(True)

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
            print(f"{a.calls + 3} timed calls at {a.shape}")
            return
        off = batch_for(a.shape, n_ch, total)
        off.frame_times(True)
        on_ms, off_ms = [], []
        for _ in range(a.legs):
            on_ms.append(leg(on, a.calls))
            off_ms.append(leg(off, a.calls))
        res = dict(shape=a.shape, n_channels=n_ch, samples=total, calls_per_leg=a.calls,
                   on_ms=[round(v, 4) for v in on_ms], off_ms=[round(v, 4) for v in off_ms],
                   on_median_ms=round(float(np.median(on_ms)), 4), off_median_ms=round(float(np.median(off_ms)), 4),
                   added_ms=round(float(np.median(on_ms) - np.median(off_ms)), 4),
                   off_spread_ms=round(float(max(off_ms) - min(off_ms)), 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
