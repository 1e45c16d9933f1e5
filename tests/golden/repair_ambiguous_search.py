#!/usr/bin/env python3
"""Finds candidates that two different trials of the single-symbol repair both pass (include/gnuais_hip.h,
gnuais_batch_repair: such a candidate stays lost) and writes them to repair_ambiguous.json beside this file.

Two passing trials need a change of stuffing, so the payloads are biased towards 1s (many runs of five).  A payload is
drawn, framed as the deframer records it (tests/repair_ref.py: candidate_raw), one pair is inverted at p1 -- every p1 in
turn -- and the restatement's brute force counts the passing trials.  Each hit is a few tens of seconds of search.

usage: repair_ambiguous_search.py [hits wanted, default 4] [seed, default 1]"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import repair_ref  # noqa: E402


def main():
    want = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    found = []
    while len(found) < want:
        bits = (rng.random(168) < 0.8).astype(np.uint8)
        payload = np.packbits(bits, bitorder="little").tobytes()
        raw0 = repair_ref.candidate_raw(payload)
        recs = np.tile(raw0, (raw0.size - 1, 1))
        p1 = np.arange(raw0.size - 1)
        recs[p1, p1] ^= 1
        recs[p1, p1 + 1] ^= 1
        for p, passing in zip(p1, repair_ref.brute_force_many(recs)):
            if len(passing) > 1:
                found.append({"payload": payload.hex(), "p1": int(p), "passes_at": [t[0] for t in passing]})
                print(found[-1], flush=True)
                break
    with open(os.path.join(HERE, "repair_ambiguous.json"), "w") as f:
        json.dump(found, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
