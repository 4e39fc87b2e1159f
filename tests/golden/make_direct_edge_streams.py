#!/usr/bin/env python3
"""Find the RNG streams whose FOURTH draw is exactly 0.0 and write them to direct_edge_streams.json.

A direct-light sample (tinyrt.h trt_direct, steps 2-3) takes one draw for the emitter and then two (quad) or three (sphere): the fourth
draw of stream (seed, j, 1) is the u3 of a sphere's random unit vector, and where it is 0.0 the vector is 0/0 - the sample is dead by
NaN.  draw_edge_streams.json holds the streams whose first, second or third draw is 0; this scans the same streams (SEED, j, 1) for
j < 2^SCAN_LOG2 for the fourth with make_draw_edge_streams.py's vectorised restatement of trt-rng v1 and records the first PER_CASE.
tests/test_direct_draw_cases.py confirms every recorded stream with the oracle's own orc_rng_seed + orc_rng_random.

    python tests/golden/make_direct_edge_streams.py        # ~15 s for 2^27 streams
"""
import json
import os

import numpy as np

import make_draw_edge_streams as M

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "direct_edge_streams.json")
SEED, SAMPLE = M.SEED, M.SAMPLE
SCAN_LOG2, CHUNK_LOG2 = 27, 22
PER_CASE = 8
U = np.uint32


def scan():
    found = []
    with np.errstate(over="ignore"):
        for c in range(1 << (SCAN_LOG2 - CHUNK_LOG2)):
            j = (np.arange(1 << CHUNK_LOG2, dtype=np.uint64) + (c << CHUNK_LOG2)).astype(U)
            s0, s1 = M.rng_seed(SEED, j, SAMPLE)
            zero_before = np.zeros(len(j), bool)
            for draw in range(4):
                r, s0, s1 = M.rng_next(s0, s1)
                if draw < 3:
                    zero_before |= (r >> U(9)) == 0
            found += [int(x) for x in j[((r >> U(9)) == 0) & ~zero_before]]
    return found


if __name__ == "__main__":
    found = scan()
    doc = {"seed": SEED, "sample": SAMPLE, "scanned_streams": 1 << SCAN_LOG2, "found": {"u4_zero": len(found)}, "u4_zero": found[:PER_CASE]}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(doc)
