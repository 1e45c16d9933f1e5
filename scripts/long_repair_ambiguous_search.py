#!/usr/bin/env python3
"""Finds long candidates that two different trials of the long-frame repair both pass (include/gnuais_hip.h,
gnuais_batch_long_repair: such a candidate stays lost) and writes them to tests/golden/long_repair_ambiguous.json.

Two passing trials need a change of stuffing, so the payloads are biased towards 1s (many runs of five).  A payload of
54 to 64 bytes is drawn, framed as D' records it (tests/long_repair_ref.py: candidate_raw), and one pair is inverted at
p1, every p1 in turn.  The search itself is cheap: the library's host function (gnuais_long_repair_candidate, a popcount
per word and a table CRC per trial) counts the passing trials of each record, about half a second per payload.  It only
points: every hit is then confirmed by the restatement's bit-by-bit brute force, which also names the trials, and a hit
the two disagree on stops the search.

usage: long_repair_ambiguous_search.py [hits wanted, default 3] [seed, default 1]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import long_repair_ref as lrr  # noqa: E402
from gnuais_amd import lib  # noqa: E402


def main():
    want = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    L = lib.load()
    pl = np.zeros(126, dtype=np.uint8)
    n, pos = C.c_int(), C.c_int()
    found, tried = [], 0
    while len(found) < want:
        nbytes = int(rng.integers(54, 65))
        bits = (rng.random(8 * nbytes) < 0.8).astype(np.uint8)
        payload = np.packbits(bits, bitorder="little").tobytes()
        raw0 = lrr.candidate_raw(payload)
        tried += 1
        for p1 in range(raw0.size - 1):
            rec = np.ascontiguousarray(lrr.flipped(raw0, p1))
            k = L.gnuais_long_repair_candidate(rec.ctypes.data, int(rec.size), pl.ctypes.data, C.byref(n), C.byref(pos))
            if k > 1:
                passing = lrr.brute_force(rec)
                assert len(passing) == k, (payload.hex(), p1, k, passing)
                found.append({"payload": payload.hex(), "p1": int(p1), "passes_at": [t[0] for t in passing],
                              "nbits": [t[1] for t in passing]})
                print(tried, found[-1], flush=True)
                break
    with open(os.path.join(ROOT, "tests", "golden", "long_repair_ambiguous.json"), "w") as f:
        json.dump(found, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
