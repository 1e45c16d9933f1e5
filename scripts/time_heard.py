"""What the member lists of the unique drain (gnuais_batch_drain_frames_heard, frame_unique.hip) cost, at
scripts/time_unique.py's shape and input (C3, 16384 x 48000 at 48 kHz; --copies receivers hear each stream):

  python scripts/time_heard.py --copies 8       ms per drain, alternating legs in one job on one batch (frame times,
                                                frame signal and the merge on) and one ring content per drain (a C3
                                                call, not timed):
                                                  leg A  gnuais_batch_drain_frames_signal()  every copy, 80 bytes each:
                                                         the only way to the same information without the lists
                                                  leg B  gnuais_batch_drain_frames_heard()   records + member lists
                                                  leg C  gnuais_batch_drain_frames_unique()  records + counts
                                                3 warm-up and --drains timed drains a leg, --legs alternations; all
                                                through the C ABI into buffers allocated and touched once; one JSON
                                                line (--out FILE)
  python scripts/time_heard.py --copies 8 --only C
                                                leg C alone: runs on a build that does not have the lists yet, for the
                                                comparison of leg C with the commit before"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from time_unique import N_CH, TOTAL, WINDOW, device_receivers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, choices=[1, 2, 4, 8], default=8)
    ap.add_argument("--drains", type=int, default=20, help="timed drains per leg")
    ap.add_argument("--legs", type=int, default=3, help="alternations of the legs")
    ap.add_argument("--only", choices=["A", "B", "C"], help="one leg alone")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from gnuais_amd import ReceiverBatch
    from gnuais_amd.lib import FRAME_DTYPE, SIGNAL_DTYPE, check
    assert torch.cuda.is_available(), "time_heard.py measures on the GPU"
    xd = device_receivers(a.copies)
    b = ReceiverBatch(N_CH, max_len=TOTAL)
    b.frame_times(True)
    b.frame_signal(True)
    b.unique(WINDOW)
    cap = 1 << 19
    frames, times, copies = np.ones(cap, dtype=FRAME_DTYPE), np.ones(cap, dtype=np.int64), np.ones(cap, dtype=np.int32)
    signal, first = np.ones(cap, dtype=SIGNAL_DTYPE), np.ones(cap + 1, dtype=np.int32)
    members = np.ones(3 * cap, dtype=np.int64)              # cap members of 24 bytes
    got, nm = C.c_int(), C.c_int()
    which = [a.only] if a.only else ["A", "B", "C"]
    counts = {w: [] for w in which}
    listed = []

    def drain(w):
        b.run(xd)                                   # the ring's content: one C3 call, synchronised, not timed
        assert b.pending_frames() <= cap
        t0 = time.perf_counter()
        if w == "A":
            check(b._lib.gnuais_batch_drain_frames_signal(b._h, frames.ctypes.data, times.ctypes.data, signal.ctypes.data,
                                                          cap, C.byref(got)))
        elif w == "B":
            check(b._lib.gnuais_batch_drain_frames_heard(b._h, frames.ctypes.data, times.ctypes.data, copies.ctypes.data,
                                                         cap, C.byref(got), first.ctypes.data, members.ctypes.data,
                                                         C.byref(nm)))
        else:
            check(b._lib.gnuais_batch_drain_frames_unique(b._h, frames.ctypes.data, times.ctypes.data, copies.ctypes.data,
                                                          cap, C.byref(got)))
        ms = (time.perf_counter() - t0) * 1e3
        counts[w].append(got.value)
        if w == "B":
            listed.append(nm.value)
        return ms

    def leg(w):
        for _ in range(3):                          # warm-up: the stage's buffers grow on first use
            drain(w)
        return float(np.median([drain(w) for _ in range(a.drains)]))

    ms = {w: [] for w in which}
    for _ in range(a.legs):
        for w in which:
            ms[w].append(leg(w))
    names = dict(A="signal", B="heard", C="unique")
    res = dict(shape="C3", n_channels=N_CH, samples=TOTAL, copies=a.copies, window=WINDOW, drains_per_leg=a.drains)
    for w in which:
        res[names[w] + "_ms"] = [round(v, 4) for v in ms[w]]
        res[names[w] + "_median_ms"] = round(float(np.median(ms[w])), 4)
        res[names[w] + "_per_drain"] = int(np.median(counts[w]))
    if "A" in ms:
        res["signal_spread_ms"] = round(max(ms["A"]) - min(ms["A"]), 4)
    if "A" in ms and "B" in ms:
        res["heard_minus_signal_ms"] = round(float(np.median(ms["B"]) - np.median(ms["A"])), 4)
        res["members_per_drain"] = int(np.median(listed))
    if "B" in ms and "C" in ms:
        res["heard_minus_unique_ms"] = round(float(np.median(ms["B"]) - np.median(ms["C"])), 4)
    res["late"] = b.unique_late()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
