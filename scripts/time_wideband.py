"""Wideband in at two shapes, device-resident wide I/Q tiled from 64 synthetic base streams:
  W3: 8192 streams x K = 2 offsets x D = 6, 288 000 wide samples per call (C3's 16 384 receivers x 48 000 out)
  W2: 128 streams x K = 2 x D = 6, 288 000 wide samples (C2's 256 receivers x 48 000 out)

  python scripts/time_wideband.py --shape W3      ms per call of run_wideband, run_iq (on the channelised I/Q) and run
                                                  (on its audio), alternating legs on one box; one JSON line (--out FILE)
  python scripts/time_wideband.py --shape W3 --kernel-only --calls 20
                                                  the channeliser alone, for `rocprofv3 --kernel-trace --stats
                                                  --output-format csv -- ...` (its kernel_stats.csv feeds --summarise)
  python scripts/time_wideband.py --summarise STATS.csv --shape W3
                                                  the kernel's mean time from a rocprofv3 stats file -> TB/s and the
                                                  share of the byte and issue bounds
"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = {"W3": (8192, 2, 6, 288000), "W2": (128, 2, 6, 288000)}
OFFSETS = [-25000, 25000]
PEAK_TBS = 8.0
LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9    # as scripts/time_iq.py


def valu_per_row(K, D, NA=17):
    """lane instructions per output row per stream in the fast form's loop (counted from its structure): per pair of wide
    samples, 2 loads' address math aside, K * (2 mixes of ~9 + 2 packs) and 2 * K * NA v_dot2c; per row, K * 2 * NA
    accumulator moves and the K rounded stores"""
    pairs = (D + 1) // 2
    return pairs * (K * (2 * 9 + 2) + 2 * K * NA) + 2 * K * NA + 6 * K


def device_wide(M, n, D, k=64):
    import torch
    from gnuais_amd import synth
    base = np.stack([synth.make_wideband_stream(n, D, 48000 * D, OFFSETS, stream=c, occupancy=0.8)[0] for c in range(k)],
                    axis=1)
    bd = torch.from_numpy(base).cuda()
    out = torch.empty((n, M, 2), dtype=torch.int16, device=bd.device)
    cols = torch.arange(M, device=bd.device) % k
    for lo in range(0, n, 8192):                 # row bands, each stream a rotated copy of its base
        rot = (torch.arange(M, device=bd.device) * 977) % n
        r = (torch.arange(lo, min(lo + 8192, n), device=bd.device)[:, None] + rot[None, :]) % n
        out[lo:lo + r.shape[0]] = bd[r, cols[None, :]]
    return out


def summarise(path, shape):
    M, K, D, n = SHAPES[shape]
    rows = list(csv.DictReader(open(path)))
    row = next(r for r in rows if "channeliser_kernel" in r.get("Name", r.get("KernelName", "")))
    ms = float(row.get("AverageNs", row.get("Average", 0))) / 1e6
    nbytes = M * n * 4 + (n // D) * M * K * 4
    t_bytes = nbytes / (PEAK_TBS * 1e12) * 1e3
    t_valu = M * (n // D) * valu_per_row(K, D) / LANE_OPS_PER_S * 1e3
    return dict(shape=shape, kernel=row.get("Name", row.get("KernelName")), calls=int(row.get("Calls", 0)),
                kernel_ms=round(ms, 4), min_ms=round(float(row.get("MinNs", 0)) / 1e6, 4),
                max_ms=round(float(row.get("MaxNs", 0)) / 1e6, 4), bytes_per_call=nbytes,
                tb_per_s=round(nbytes / (ms / 1e3) / 1e12, 3), bound_bytes_ms=round(t_bytes, 3),
                bound_valu_issue_ms=round(t_valu, 3), share_of_byte_bound=round(t_bytes / ms, 3),
                share_of_issue_bound=round(t_valu / ms, 3), valu_per_row_per_stream=valu_per_row(K, D))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="W3")
    ap.add_argument("--calls", type=int, default=10, help="calls per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating run_wideband / run_iq / run leg triples")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--summarise", metavar="STATS_CSV")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.summarise:
        res = summarise(a.summarise, a.shape)
    else:
        import torch
        from gnuais_amd import ReceiverBatch
        assert torch.cuda.is_available(), "time_wideband.py measures on the GPU"
        M, K, D, n = SHAPES[a.shape]
        N, rows = M * K, n // D
        xd = device_wide(M, n, D)
        w = ReceiverBatch(N, max_len=rows)
        w.channeliser(D, 48000 * D, OFFSETS)
        if a.kernel_only:
            for _ in range(a.calls):
                w.channelise(xd)
            torch.cuda.synchronize()
            print(f"{a.calls} channeliser calls at {a.shape}")
            return
        iq = w.channelise(xd)
        w.reset()
        q = ReceiverBatch(N, max_len=rows)
        audio = q.discriminate(iq)
        q.reset()
        r = ReceiverBatch(N, max_len=rows)

        def leg(batch, fn, x):
            for _ in range(2):                       # warm-up
                fn(x, sync=False)
                batch.discard_frames()
            batch.sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn(x, sync=False)
                batch.discard_frames()
            batch.sync()
            return (time.perf_counter() - t0) * 1e3 / a.calls

        wb, iqm, au = [], [], []
        for _ in range(a.legs):
            wb.append(leg(w, w.run_wideband, xd))
            iqm.append(leg(q, q.run_iq, iq))
            au.append(leg(r, r.run, audio))
        med = lambda v: round(float(np.median(v)), 4)
        res = dict(shape=a.shape, streams=M, offsets=K, decim=D, wide_samples=n, receivers=N, rows=rows,
                   calls_per_leg=a.calls, run_wideband_ms=[round(v, 4) for v in wb], run_iq_ms=[round(v, 4) for v in iqm],
                   run_ms=[round(v, 4) for v in au], run_wideband_median_ms=med(wb), run_iq_median_ms=med(iqm),
                   run_median_ms=med(au), added_over_run_iq_ms=round(med(wb) - med(iqm), 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
