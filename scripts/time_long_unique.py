"""What delivering each long transmission once on the device (gnuais_batch_long_unique, frame_unique.hip) costs
against the merge a user could do with the host object alone, at C3's width (16384 channels): --copies receivers hear
each stream of long bursts, with delays below 41 rows.

  python scripts/time_long_unique.py --copies 8     ms per drain, alternating legs in one job on one batch and one ring
                                                    content per drain (a reset and one call, not timed):
                                                      leg A  gnuais_batch_drain_long_frames() + gnuais_long_uniq_push()
                                                             every copy crosses PCIe, 152 bytes each; the host merges
                                                      leg B  gnuais_batch_drain_long_frames_unique()
                                                             one record per cluster crosses, 156 bytes each
                                                    both through the C ABI into buffers allocated and touched once, timed by
                                                    a host clock around calls that end in a synchronise; one JSON line
                                                    (--out FILE, default profiles/long_unique_time_C3.json)

The input: 256 base streams of three long bursts (54, 100 and 126 bytes, one every six slots, payloads of the stream's
own); stream i of the call is base stream i % 256 rotated by (i // 256) * 2560 rows -- the same payloads at another time
are other transmissions -- and receiver c hears stream c // copies, DELAYS[c % copies] rows late."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_CH, N_BASE, ROT = 16384, 256, 2560
SIZES = (54, 100, 126)
TOTAL = len(SIZES) * 6 * 1280
DELAYS = [0, 7, 11, 18, 23, 29, 34, 40]
WINDOW = 128


def base_streams():
    from gnuais_amd import synth

    def payloads(i):
        def pick(rng, slot):
            if slot % 6 or slot // 6 >= len(SIZES):
                return None
            n = SIZES[slot // 6]
            return bytes(np.random.default_rng([5, i, n]).integers(0, 256, n, dtype=np.uint8))
        return pick
    return np.stack([synth.make_stream(TOTAL, seed=5, channel=i, sigma=500.0, payloads=payloads(i))[0] for i in range(N_BASE)])


def device_receivers(copies):
    import torch
    bt = torch.from_numpy(base_streams()).cuda()
    x = torch.empty((TOTAL, N_CH), dtype=torch.int16, device=bt.device)
    n_streams = N_CH // copies
    for r in range(n_streams // N_BASE):
        rot = torch.roll(bt, r * ROT, dims=1)
        for j in range(copies):
            cols = torch.arange(r * N_BASE, (r + 1) * N_BASE, device=bt.device) * copies + j
            x[:, cols] = torch.roll(rot, DELAYS[j], dims=1).t()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, choices=[1, 2, 4, 8], default=8)
    ap.add_argument("--drains", type=int, default=10, help="drains per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating A / B leg pairs")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "long_unique_time_C3.json"))
    a = ap.parse_args()
    import torch
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import LONG_FRAME_DTYPE, check
    from gnuais_amd.receiver import LongUniq
    assert torch.cuda.is_available(), "time_long_unique.py measures on the GPU"
    xd = device_receivers(a.copies)
    b = ReceiverBatch(N_CH, max_len=TOTAL)
    b.long_frames(True)
    b.long_unique(WINDOW)
    host = LongUniq(WINDOW)
    cap = int(b.info("long_frame_cap"))
    frames, merged = np.ones(cap, dtype=LONG_FRAME_DTYPE), np.ones(cap, dtype=LONG_FRAME_DTYPE)
    copies = np.ones(cap, dtype=np.int32)
    got, out = C.c_int(), C.c_int()
    counts = dict(A=[], A_out=[], B=[])

    def drain(which):
        b.reset()                                   # every drain sees the same call from the same state: no copy of a
        host.reset()                                # burst that straddles two calls reaches the other leg's merge as a late one
        b.run(xd)                                   # the ring's content: one call, synchronised, not timed
        rows = int(b.info("rows"))
        t0 = time.perf_counter()
        if which == "A":
            check(b._lib.gnuais_batch_drain_long_frames(b._h, frames.ctypes.data, cap, C.byref(got)))
            rc = b._lib.gnuais_long_uniq_push(host._h, frames.ctypes.data, got.value, rows, merged.ctypes.data,
                                              copies.ctypes.data, cap, C.byref(out))
            assert rc == 0
        else:
            check(b._lib.gnuais_batch_drain_long_frames_unique(b._h, merged.ctypes.data, copies.ctypes.data, cap, C.byref(got)))
        ms = (time.perf_counter() - t0) * 1e3
        counts[which].append(got.value)
        if which == "A":
            counts["A_out"].append(out.value)
        return ms

    def leg(which, n):
        for _ in range(2):                          # warm-up: the stage's buffers grow on first use
            drain(which)
        return float(np.median([drain(which) for _ in range(n)]))

    a_ms, b_ms = [], []
    for _ in range(a.legs):
        a_ms.append(leg("A", a.drains))
        b_ms.append(leg("B", a.drains))
    n_frames, n_records = int(np.median(counts["A"])), int(np.median(counts["B"]))
    assert n_records == int(np.median(counts["A_out"])), "the two merges disagree on the number of transmissions"
    res = dict(shape="C3 width", n_channels=N_CH, rows=TOTAL, copies=a.copies, window=WINDOW, drains_per_leg=a.drains,
               host_merge_ms=[round(v, 4) for v in a_ms], device_merge_ms=[round(v, 4) for v in b_ms],
               host_merge_median_ms=round(float(np.median(a_ms)), 4), device_merge_median_ms=round(float(np.median(b_ms)), 4),
               difference_ms=round(float(np.median(b_ms) - np.median(a_ms)), 4),
               host_merge_spread_ms=round(float(max(a_ms) - min(a_ms)), 4),
               frames_per_drain=n_frames, records_per_drain=n_records,
               pcie_bytes_host_merge=152 * n_frames, pcie_bytes_device_merge=156 * n_records,
               late=b.long_unique_late())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
