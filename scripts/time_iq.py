"""Complex baseband in at BASELINE shapes (C3: 16384 x 48000 at 48 kHz; C5: 16384 x 192000 at 192 kHz), device-resident
I/Q tiled from 256 base streams as bench.py tiles audio.

  python scripts/time_iq.py --shape C3            ms per call of run_iq against run on the same box, alternating legs;
                                                 one JSON line (and --out FILE)
  python scripts/time_iq.py --shape C3 --kernel-only --calls 20
                                                 the discriminator alone, for `rocprofv3 --kernel-trace --stats
                                                 --output-format csv -- ...` (its kernel_stats.csv feeds --summarise)
  python scripts/time_iq.py --summarise STATS.csv --shape C3
                                                 the kernel's mean time from a rocprofv3 stats file -> TB/s at 6 bytes a
                                                 sample and the share of 8 TB/s; VALU issue estimate beside it
"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = {"C3": (16384, 48000, 5), "C5": (16384, 192000, 20)}
PEAK_TBS = 8.0
VALU_PER_SAMPLE = 46            # counted in the gfx950 ISA of the 4-channel loop (736 for 16 samples), the division included
LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9    # 256 CUs x 4 SIMDs x 16 lanes per cycle x 2.4 GHz (wave64 over 4 cycles)


def device_iq(n_ch, total, sps, k=256):
    import torch
    from gnuais_amd import synth
    base = np.stack([synth.make_iq_stream(total, channel=c, sps=sps, occupancy=0.8)[0] for c in range(k)], axis=1)
    bd = torch.from_numpy(base).cuda()
    rot = torch.tensor([synth.rotation_of(c, total) for c in range(n_ch)], device=bd.device)
    out = torch.empty((total, n_ch, 2), dtype=torch.int16, device=bd.device)
    cols = torch.arange(n_ch, device=bd.device) % k
    for lo in range(0, total, 4096):                 # row bands: the index tensor stays small
        r = (torch.arange(lo, min(lo + 4096, total), device=bd.device)[:, None] + rot[None, :]) % total
        out[lo:lo + r.shape[0]] = bd[r, cols[None, :]]
    return out


def batch_for(shape, n_ch, total):
    from gnuais_amd import ReceiverBatch, params
    kw = dict(taps=params.taps_192k(), pllinc=params.PLLINC_192K) if shape == "C5" else {}
    return ReceiverBatch(n_ch, max_len=total, **kw)


def summarise(path, shape):
    n_ch, total, _ = SHAPES[shape]
    rows = list(csv.DictReader(open(path)))
    row = next(r for r in rows if "iq_discriminator_kernel" in r.get("Name", r.get("KernelName", "")))
    ms = float(row.get("AverageNs", row.get("Average", 0))) / 1e6
    samples = n_ch * total
    tbs = samples * 6 / (ms / 1e3) / 1e12
    t_bytes = samples * 6 / (PEAK_TBS * 1e12) * 1e3
    t_valu = samples * VALU_PER_SAMPLE / LANE_OPS_PER_S * 1e3
    return dict(shape=shape, kernel=row.get("Name", row.get("KernelName")), calls=int(row.get("Calls", 0)),
                kernel_ms=round(ms, 4), min_ms=round(float(row.get("MinNs", 0)) / 1e6, 4),
                max_ms=round(float(row.get("MaxNs", 0)) / 1e6, 4), bytes_per_call=samples * 6, tb_per_s=round(tbs, 3),
                share_of_8tbs=round(tbs / PEAK_TBS, 3), bound_bytes_ms=round(t_bytes, 3),
                bound_valu_issue_ms=round(t_valu, 3),
                governs="bytes" if t_bytes >= t_valu else "VALU issue")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="C3")
    ap.add_argument("--calls", type=int, default=20, help="calls per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating run_iq / run leg pairs")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--summarise", metavar="STATS_CSV")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.summarise:
        res = summarise(a.summarise, a.shape)
    else:
        import torch
        assert torch.cuda.is_available(), "time_iq.py measures on the GPU"
        n_ch, total, sps = SHAPES[a.shape]
        xd = device_iq(n_ch, total, sps)
        b = batch_for(a.shape, n_ch, total)
        if a.kernel_only:
            for _ in range(a.calls):
                b.discriminate(xd)
            torch.cuda.synchronize()
            print(f"{a.calls} discriminator calls at {a.shape}")
            return
        audio = b.discriminate(xd)
        b.reset()
        r = batch_for(a.shape, n_ch, total)

        def leg(batch, fn, x):
            for _ in range(3):                       # warm-up
                fn(x, sync=False)
                batch.discard_frames()
            batch.sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn(x, sync=False)
                batch.discard_frames()
            batch.sync()
            return (time.perf_counter() - t0) * 1e3 / a.calls

        iq_ms, au_ms = [], []
        for _ in range(a.legs):
            iq_ms.append(leg(b, b.run_iq, xd))
            au_ms.append(leg(r, r.run, audio))
        res = dict(shape=a.shape, n_channels=n_ch, samples=total, calls_per_leg=a.calls,
                   run_iq_ms=[round(v, 4) for v in iq_ms], run_ms=[round(v, 4) for v in au_ms],
                   run_iq_median_ms=round(float(np.median(iq_ms)), 4), run_median_ms=round(float(np.median(au_ms)), 4),
                   added_ms=round(float(np.median(iq_ms) - np.median(au_ms)), 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
