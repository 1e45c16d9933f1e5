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
  ... --format cu8|cs8|cf32                       the same legs, --kernel-only and --summarise on wide samples of that format
                                                  (the int16 streams quantised to it), converted where the kernel loads them
  python scripts/time_wideband.py --ratio U/D --kernel-only [--streams M] [--wide N] [--format F] [--offsets K] --calls 20
                                                  the wide stage alone at out rate = in rate * U / D on random samples, for
                                                  rocprofv3 as above; 1/D with D <= 64 is the integer form, so `--ratio 1/21`
                                                  and `--ratio 3/64` compare the two at nearly the same wide samples per
                                                  output row; --offsets 5 (K > 4) times the direct form
  python scripts/time_wideband.py --summarise STATS.csv --ratio U/D [--streams M] [--wide N]
                                                  the wide stage's kernels of that stats file (fast, direct, carry) as ns per
                                                  wide sample per stream
  python scripts/time_wideband.py --shape W2 --host-path [--streams M]
                                                  run_wideband_fmt_host on cu8 against run_wideband_host on the same samples
                                                  widened to int16, alternating legs: ms per call and GB/s over the bus
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
RATIO_OFFSETS = [-25000, 25000, 12000, 0, -7000]     # --ratio --offsets K: the first K
PAIR_BYTES = {"cs16": 4, "cu8": 2, "cs8": 2, "cf32": 8}
PEAK_TBS = 8.0
LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9    # as scripts/time_iq.py


CONVERT_VALU = {"cs16": 0, "cs8": 1, "cu8": 2, "cf32": 14}     # lane instructions per wide sample to convert it (ISA)


def valu_per_row(K, D, NA=17, fmt="cs16"):
    """lane instructions per output row per stream in the fast form's loop (counted from its structure): per pair of wide
    samples, 2 loads' address math aside, K * (2 mixes of ~9 + 2 packs) and 2 * K * NA v_dot2c; per row, K * 2 * NA
    accumulator moves and the K rounded stores; and the format's conversion of each of the row's D wide samples (cs8
    one v_perm_b32, cu8 that and a v_xor_b32, cf32 six per component and two to pack)"""
    pairs = (D + 1) // 2
    return pairs * (K * (2 * 9 + 2) + 2 * K * NA) + 2 * K * NA + 6 * K + D * CONVERT_VALU[fmt]


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


def quantise(xd, fmt):
    """the int16 wide samples in format fmt, round to nearest: cu8 (v + 32640) / 256, cs8 v / 256, cf32 v / 32768"""
    import torch
    if fmt == "cs16":
        return xd
    if fmt == "cf32":
        return xd.to(torch.float32) / 32768.0
    out = torch.empty(xd.shape, dtype=torch.uint8 if fmt == "cu8" else torch.int8, device=xd.device)
    for lo in range(0, xd.shape[0], 8192):
        v = xd[lo:lo + 8192].to(torch.int32)
        if fmt == "cu8":
            out[lo:lo + 8192] = ((v + 32640 + 128) >> 8).clamp(0, 255).to(torch.uint8)
        else:
            out[lo:lo + 8192] = ((v + 128) >> 8).clamp(-128, 127).to(torch.int8)
    return out


def fmt_name(kernel_name, fmt):
    """whether a rocprofv3 kernel name is the fast form's kernel of format fmt: channeliser_kernel<K, NA, F, RATIONAL>"""
    f = {"cs16": 0, "cu8": 1, "cs8": 2, "cf32": 3}[fmt]
    if "channeliser_kernel<" not in kernel_name:
        return False
    args = kernel_name.replace(" ", "").split("channeliser_kernel<")[1].split(">")[0].split(",")
    return len(args) == 4 and args[2] == str(f)


def summarise(path, shape, fmt="cs16"):
    M, K, D, n = SHAPES[shape]
    rows = list(csv.DictReader(open(path)))
    row = next(r for r in rows if fmt_name(r.get("Name", r.get("KernelName", "")), fmt))
    ms = float(row.get("AverageNs", row.get("Average", 0))) / 1e6
    nbytes = M * n * PAIR_BYTES[fmt] + (n // D) * M * K * 4
    t_bytes = nbytes / (PEAK_TBS * 1e12) * 1e3
    t_valu = M * (n // D) * valu_per_row(K, D, fmt=fmt) / LANE_OPS_PER_S * 1e3
    return dict(shape=shape, format=fmt, kernel=row.get("Name", row.get("KernelName")), calls=int(row.get("Calls", 0)),
                kernel_ms=round(ms, 4), min_ms=round(float(row.get("MinNs", 0)) / 1e6, 4),
                max_ms=round(float(row.get("MaxNs", 0)) / 1e6, 4), bytes_per_call=nbytes,
                tb_per_s=round(nbytes / (ms / 1e3) / 1e12, 3), bound_bytes_ms=round(t_bytes, 3),
                bound_valu_issue_ms=round(t_valu, 3), share_of_byte_bound=round(t_bytes / ms, 3),
                share_of_issue_bound=round(t_valu / ms, 3), valu_per_row_per_stream=valu_per_row(K, D, fmt=fmt))


def ratio_shape(a):
    """--ratio U/D: (U, D, streams, wide samples per call: --wide rounded down to a multiple of D)"""
    U, D = (int(v) for v in a.ratio.split("/"))
    return U, D, a.streams or 8192, a.wide // D * D


def ratio_kernel_only(a):
    import torch
    from gnuais_amd import ReceiverBatch
    U, D, M, n = ratio_shape(a)
    offsets = RATIO_OFFSETS[:a.offsets]
    K, rows = len(offsets), n // D * U
    dt = {"cs16": torch.int16, "cu8": torch.uint8, "cs8": torch.int8}.get(a.format)
    if a.format == "cf32":
        x = torch.rand((n, M, 2), device="cuda") * 2.0 - 1.0
    else:
        info = torch.iinfo(dt)
        x = torch.randint(info.min, info.max + 1, (n, M, 2), dtype=dt, device="cuda")
    b = ReceiverBatch(M * K, max_len=rows)
    b.resampler(U, D, 1000 * D, offsets)          # the mixer periods depend on the rate; any rate times the kernel alike
    fmt = None if a.format == "cs16" else a.format
    for _ in range(a.calls):
        b.channelise(x, fmt=fmt)
    torch.cuda.synchronize()
    print(f"{a.calls} calls at {U}/{D}, {M} streams x {K} offsets, {n} wide samples -> {rows} rows, {a.format}")


def summarise_ratio(a):
    U, D, M, n = ratio_shape(a)
    out = []
    for r in csv.DictReader(open(a.summarise)):
        name = r.get("Name", r.get("KernelName", ""))
        if "channeliser_kernel" in name or "channeliser_direct_kernel" in name or "channeliser_carry_kernel" in name:
            per = lambda key: round(float(r.get(key, 0)) / (float(n) * M), 6)
            out.append(dict(kernel=name, calls=int(r.get("Calls", 0)), ratio=a.ratio, streams=M, wide_samples=n,
                            mean_ms=round(float(r.get("AverageNs", 0)) / 1e6, 4),
                            ns_per_wide_sample_per_stream=dict(mean=per("AverageNs"), min=per("MinNs"), max=per("MaxNs"))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="W3")
    ap.add_argument("--calls", type=int, default=10, help="calls per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternating run_wideband / run_iq / run leg triples")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--summarise", metavar="STATS_CSV")
    ap.add_argument("--format", choices=sorted(PAIR_BYTES) + ["all"], default="cs16",
                    help="the wide samples' format; all (--kernel-only): the four formats in turn, call by call, so that "
                         "one profiler run holds them side by side on one box and clock")
    ap.add_argument("--host-path", action="store_true", help="cu8 in native bytes against the same widened to int16")
    ap.add_argument("--streams", type=int, default=0, help="--host-path: streams instead of the shape's")
    ap.add_argument("--ratio", metavar="U/D", help="the rational channeliser at this ratio (--kernel-only, --summarise)")
    ap.add_argument("--offsets", type=int, default=2, choices=range(1, len(RATIO_OFFSETS) + 1),
                    help="--ratio: offsets per stream; 5 takes the direct form")
    ap.add_argument("--wide", type=int, default=262144, help="--ratio: wide samples per call (rounded down to a multiple of D)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.ratio and a.summarise:
        res = summarise_ratio(a)
    elif a.ratio:
        assert a.kernel_only, "--ratio times the kernel alone: with --kernel-only or --summarise"
        return ratio_kernel_only(a)
    elif a.summarise:
        res = summarise(a.summarise, a.shape, a.format)
    else:
        import torch
        from gnuais_amd import ReceiverBatch
        assert torch.cuda.is_available(), "time_wideband.py measures on the GPU"
        M, K, D, n = SHAPES[a.shape]
        N, rows = M * K, n // D
        if a.host_path:
            return host_path(a)
        fmt = None if a.format == "cs16" else a.format      # None: the entries without a format
        if a.format == "all":
            assert a.kernel_only, "--format all is for --kernel-only"
            x16 = device_wide(M, n, D)
            xs = [(None, x16)] + [(f, quantise(x16, f)) for f in ("cu8", "cs8", "cf32")]
            w = ReceiverBatch(N, max_len=rows)
            w.channeliser(D, 48000 * D, OFFSETS)
            for _ in range(a.calls):
                for f, x in xs:
                    w.channelise(x, fmt=f)
            torch.cuda.synchronize()
            print(f"{a.calls} channeliser calls of each format in turn at {a.shape}")
            return
        xd = quantise(device_wide(M, n, D), a.format)
        w = ReceiverBatch(N, max_len=rows)
        w.channeliser(D, 48000 * D, OFFSETS)
        if a.kernel_only:
            for _ in range(a.calls):
                w.channelise(xd, fmt=fmt)
            torch.cuda.synchronize()
            print(f"{a.calls} channeliser calls at {a.shape}, {a.format}")
            return
        iq = w.channelise(xd, fmt=fmt)
        w.reset()
        q = ReceiverBatch(N, max_len=rows)
        audio = q.discriminate(iq)
        q.reset()
        r = ReceiverBatch(N, max_len=rows)

        def leg(batch, fn, x, **kw):
            for _ in range(2):                       # warm-up
                fn(x, sync=False, **kw)
                batch.discard_frames()
            batch.sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn(x, sync=False, **kw)
                batch.discard_frames()
            batch.sync()
            return (time.perf_counter() - t0) * 1e3 / a.calls

        wb, iqm, au = [], [], []
        for _ in range(a.legs):
            wb.append(leg(w, w.run_wideband, xd, **({"fmt": fmt} if fmt else {})))
            iqm.append(leg(q, q.run_iq, iq))
            au.append(leg(r, r.run, audio))
        med = lambda v: round(float(np.median(v)), 4)
        res = dict(shape=a.shape, format=a.format, streams=M, offsets=K, decim=D, wide_samples=n, receivers=N, rows=rows,
                   calls_per_leg=a.calls, run_wideband_ms=[round(v, 4) for v in wb], run_iq_ms=[round(v, 4) for v in iqm],
                   run_ms=[round(v, 4) for v in au], run_wideband_median_ms=med(wb), run_iq_median_ms=med(iqm),
                   run_median_ms=med(au), added_over_run_iq_ms=round(med(wb) - med(iqm), 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def host_path(a):
    """run_wideband_fmt_host on cu8 against run_wideband_host on the same samples widened to int16 on the host"""
    import torch
    from gnuais_amd import ReceiverBatch
    M, K, D, n = SHAPES[a.shape]
    M = a.streams or M
    u8 = quantise(device_wide(M, n, D), "cu8").cpu().numpy()
    wide = ((u8.astype(np.int32) << 8) - 32640).astype(np.int16)
    b = ReceiverBatch(M * K, max_len=n // D)
    b.channeliser(D, 48000 * D, OFFSETS)

    def leg(x, fmt):
        b.run_wideband(x, fmt=fmt)                   # warm-up: staging allocation
        b.discard_frames()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            b.run_wideband(x, fmt=fmt)
            b.discard_frames()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    t8, t16 = [], []
    for _ in range(a.legs):
        t8.append(leg(u8, "cu8"))
        t16.append(leg(wide, None))
    med = lambda v: float(np.median(v))
    res = dict(shape=f"{a.shape}/{M}" if a.streams else a.shape, streams=M, wide_samples=n, calls_per_leg=a.calls, cu8_ms=[round(v, 3) for v in t8],
               cs16_widened_ms=[round(v, 3) for v in t16], cu8_median_ms=round(med(t8), 3),
               cs16_widened_median_ms=round(med(t16), 3), cu8_bytes=int(u8.nbytes), cs16_bytes=int(wide.nbytes),
               cu8_gb_per_s_whole_call=round(u8.nbytes / med(t8) / 1e6, 2),
               cs16_gb_per_s_whole_call=round(wide.nbytes / med(t16) / 1e6, 2))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
