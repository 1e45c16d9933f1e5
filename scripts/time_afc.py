"""The carrier-error stage (AFC) at BASELINE shapes (C3: 16384 x 48000 at 48 kHz; C5: 16384 x 192000 at 192 kHz),
device-resident I/Q tiled from 256 base streams as scripts/time_iq.py tiles it (gated bursts, 3 kHz off).

  python scripts/time_afc.py --shape C3            ms per run_iq call with the AFC on against the AFC off, two batches
                                                  on the same box, alternating legs; one JSON line (and --out FILE)
  python scripts/time_afc.py --shape C3 --kernel-only --calls 20
                                                  discriminator + AFC alone (gnuais_batch_afc_apply), for `rocprofv3
                                                  --kernel-trace --stats --output-format csv -- ...`
  python scripts/time_afc.py --summarise STATS.csv --shape C3
                                                  the three kernels' mean times from a rocprofv3 stats file beside their
                                                  byte floors at 8 TB/s
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

from time_iq import SHAPES, PEAK_TBS, batch_for

WINDOW = {"C3": 2048, "C5": 8192}
EST_CHUNK = 64                   # afc.hip: estimates per thread (the first window summed, the others slid)


def kernel_bytes(window):
    """bytes a sample: the discriminator reads a pair and writes a sample (the block sums are 16 bytes per 64 samples);
    the apply kernel reads a sample and writes one; the estimate reads W/64 + 2 (chunk - 1) block sums of 16 bytes per
    chunk of blocks and writes 2 bytes per block of 64 samples"""
    est = ((window // 64 + 2 * (EST_CHUNK - 1)) * 16 / EST_CHUNK + 2) / 64
    return {"iq_discriminator_kernel": 6 + 16 / 64, "afc_apply_kernel": 4, "afc_estimate_kernel": est}


def device_iq(n_ch, total, sps, k=256):
    import torch
    from gnuais_amd import synth
    base = np.stack([synth.make_iq_stream(total, channel=c, sps=sps, occupancy=0.8, gated=True, offset_hz=3000.0,
                                          rate_hz=9600 * sps)[0] for c in range(k)], axis=1)
    bd = torch.from_numpy(base).cuda()
    rot = torch.tensor([synth.rotation_of(c, total) for c in range(n_ch)], device=bd.device)
    out = torch.empty((total, n_ch, 2), dtype=torch.int16, device=bd.device)
    cols = torch.arange(n_ch, device=bd.device) % k
    for lo in range(0, total, 4096):                 # row bands: the index tensor stays small
        r = (torch.arange(lo, min(lo + 4096, total), device=bd.device)[:, None] + rot[None, :]) % total
        out[lo:lo + r.shape[0]] = bd[r, cols[None, :]]
    return out


def summarise(path, shape):
    n_ch, total, _ = SHAPES[shape]
    samples = n_ch * total
    rows = list(csv.DictReader(open(path)))
    out = dict(shape=shape, window=WINDOW[shape], kernels=[])
    for r in rows:
        name = r.get("Name", r.get("KernelName", ""))
        for k, bytes_per_sample in kernel_bytes(WINDOW[shape]).items():
            if k in name:
                ms = float(r.get("AverageNs", r.get("Average", 0))) / 1e6
                floor = samples * bytes_per_sample / (PEAK_TBS * 1e12) * 1e3
                out["kernels"].append(dict(kernel=name, calls=int(r.get("Calls", 0)), kernel_ms=round(ms, 4),
                                           min_ms=round(float(r.get("MinNs", 0)) / 1e6, 4),
                                           max_ms=round(float(r.get("MaxNs", 0)) / 1e6, 4),
                                           bytes_per_sample=round(bytes_per_sample, 3), byte_floor_ms=round(floor, 4),
                                           times_the_floor=round(ms / floor, 2) if floor else None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="C3")
    ap.add_argument("--window", type=int, default=0, help="default: 2048 at C3, 8192 at C5")
    ap.add_argument("--calls", type=int, default=20, help="calls per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating AFC on / AFC off leg pairs")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--summarise", metavar="STATS_CSV")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.summarise:
        res = summarise(a.summarise, a.shape)
    else:
        import torch
        assert torch.cuda.is_available(), "time_afc.py measures on the GPU"
        n_ch, total, sps = SHAPES[a.shape]
        W = a.window or WINDOW[a.shape]
        xd = device_iq(n_ch, total, sps)
        on = batch_for(a.shape, n_ch, total)
        on.afc(W)
        if a.kernel_only:
            for _ in range(a.calls):
                on.afc_apply(xd)
            torch.cuda.synchronize()
            print(f"{a.calls} discriminator + AFC calls at {a.shape}, window {W}")
            return
        off = batch_for(a.shape, n_ch, total)

        def leg(batch):
            for _ in range(3):                       # warm-up
                batch.run_iq(xd, sync=False)
                batch.discard_frames()
            batch.sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                batch.run_iq(xd, sync=False)
                batch.discard_frames()
            batch.sync()
            return (time.perf_counter() - t0) * 1e3 / a.calls

        on_ms, off_ms = [], []
        for _ in range(a.legs):
            on_ms.append(leg(on))
            off_ms.append(leg(off))
        est = on.afc_estimate().astype(np.float64) * (9600 * sps) / 65536.0
        res = dict(shape=a.shape, n_channels=n_ch, samples=total, window=W, calls_per_leg=a.calls,
                   afc_on_ms=[round(v, 4) for v in on_ms], afc_off_ms=[round(v, 4) for v in off_ms],
                   afc_on_median_ms=round(float(np.median(on_ms)), 4), afc_off_median_ms=round(float(np.median(off_ms)), 4),
                   added_ms=round(float(np.median(on_ms) - np.median(off_ms)), 4),
                   frames_per_call_on=int(on.counters()["receivedframes"].sum() // (a.legs * (a.calls + 3))),
                   frames_per_call_off=int(off.counters()["receivedframes"].sum() // (a.legs * (a.calls + 3))),
                   estimate_hz_median=round(float(np.median(est)), 1))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
