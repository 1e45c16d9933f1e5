"""What delivering each transmission once (gnuais_batch_unique, frame_unique.hip) costs against delivering every copy, at
C3's shape (16384 x 48000 at 48 kHz): --copies receivers hear each stream, with delays below 41 rows.

  python scripts/time_unique.py --copies 8          ms per drain, alternating legs in one job on one batch and one ring
                                                    content per drain (a C3 call, not timed):
                                                      leg A  gnuais_batch_drain_frames_timed()   every copy crosses PCIe
                                                      leg B  gnuais_batch_drain_frames_unique()  one record per cluster
                                                    both through the C ABI into buffers allocated and touched once; one
                                                    JSON line (--out FILE)
  python scripts/time_unique.py --copies 8 --kernel-only --drains 20
                                                    leg B's drains alone, for `rocprofv3 --kernel-trace --stats
                                                    --output-format csv -- ...`
  python scripts/time_unique.py --summarise STATS.csv
                                                    the stage's kernels (its own and rocPRIM's) from such a stats file

The input: 2048 base streams (the bench's generator); stream i of the call is base stream i % 2048 rotated by
(i // 2048) * 9600 rows -- the same payloads at another time are other transmissions -- and receiver c hears stream
c // copies, DELAYS[c % copies] rows late."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_CH, TOTAL, N_BASE = 16384, 48000, 2048
DELAYS = [0, 7, 11, 18, 23, 29, 34, 40]
WINDOW = 128


def device_receivers(copies):
    import torch
    from gnuais_amd import synth
    base, _ = synth.make_base_streams(N_BASE, TOTAL, occupancy=0.8)
    bt = torch.from_numpy(base).cuda()
    x = torch.empty((TOTAL, N_CH), dtype=torch.int16, device=bt.device)
    n_streams = N_CH // copies
    for r in range(n_streams // N_BASE):
        rot = torch.roll(bt, r * 9600, dims=1)
        for j in range(copies):
            cols = torch.arange(r * N_BASE, (r + 1) * N_BASE, device=bt.device) * copies + j
            x[:, cols] = torch.roll(rot, DELAYS[j], dims=1).t()
    return x


def summarise(path):
    out = dict(kernels=[])
    for r in csv.DictReader(open(path)):
        name = r.get("Name", r.get("KernelName", ""))
        if any(k in name for k in ("uniq_", "rocprim", "frames_gather", "nmea_keys", "frame_time_gather")):
            out["kernels"].append(dict(kernel=name.split("(")[0][-60:], calls=int(r.get("Calls", 0)),
                                       total_ms=round(float(r.get("TotalDurationNs", 0)) / 1e6, 4),
                                       mean_ms=round(float(r.get("AverageNs", r.get("Average", 0))) / 1e6, 4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, choices=[1, 2, 4, 8], default=8)
    ap.add_argument("--drains", type=int, default=20, help="drains per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating A / B leg pairs")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--summarise", metavar="STATS_CSV")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.summarise:
        res = summarise(a.summarise)
    else:
        import torch
        from gnuais_amd import ReceiverBatch
        from gnuais_amd.lib import FRAME_DTYPE, check
        assert torch.cuda.is_available(), "time_unique.py measures on the GPU"
        xd = device_receivers(a.copies)
        b = ReceiverBatch(N_CH, max_len=TOTAL)
        b.frame_times(True)
        b.unique(WINDOW)
        cap = 1 << 19
        frames, times, copies = np.ones(cap, dtype=FRAME_DTYPE), np.ones(cap, dtype=np.int64), np.ones(cap, dtype=np.int32)
        got = C.c_int()
        counts = dict(A=[], B=[])

        def drain(which):
            b.run(xd)                                   # the ring's content: one C3 call, synchronised, not timed
            assert b.pending_frames() <= cap
            t0 = time.perf_counter()
            if which == "A":
                check(b._lib.gnuais_batch_drain_frames_timed(b._h, frames.ctypes.data, times.ctypes.data, cap, C.byref(got)))
            else:
                check(b._lib.gnuais_batch_drain_frames_unique(b._h, frames.ctypes.data, times.ctypes.data,
                                                              copies.ctypes.data, cap, C.byref(got)))
            ms = (time.perf_counter() - t0) * 1e3
            counts[which].append(got.value)
            return ms

        def leg(which, n):
            for _ in range(3):                          # warm-up: the stage's buffers grow on first use
                drain(which)
            return float(np.median([drain(which) for _ in range(n)]))

        if a.kernel_only:
            leg("B", a.drains)
            print(f"{a.drains + 3} unique drains at C3, {a.copies} copies")
            return
        a_ms, b_ms = [], []
        for _ in range(a.legs):
            a_ms.append(leg("A", a.drains))
            b_ms.append(leg("B", a.drains))
        res = dict(shape="C3", n_channels=N_CH, samples=TOTAL, copies=a.copies, window=WINDOW, drains_per_leg=a.drains,
                   timed_ms=[round(v, 4) for v in a_ms], unique_ms=[round(v, 4) for v in b_ms],
                   timed_median_ms=round(float(np.median(a_ms)), 4), unique_median_ms=round(float(np.median(b_ms)), 4),
                   ratio=round(float(np.median(b_ms) / np.median(a_ms)), 4),
                   frames_per_drain=int(np.median(counts["A"])), records_per_drain=int(np.median(counts["B"])),
                   late=b.unique_late())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
