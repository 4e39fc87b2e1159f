#!/usr/bin/env python3
"""Find the RNG streams whose first, second or third draw is exactly 0.0 and write them to draw_edge_streams.json.

A sample's first ray is drawn from stream (seed, j, 1) (tinyrt.h trt_gather / trt_ambient / trt_probe / trt_passes).  random::<f32>() is
0.0 when the top 23 bits of the generator's output are 0: 2^-23 per draw, so none of the few thousand streams the other tests use has one.
This scans streams (SEED, j, 1) for j < 2^SCAN_LOG2 with a vectorised numpy restatement of trt-rng v1 (rng_seed, rng_next: xoroshiro64*
seeded through mix32) and records the first PER_CASE streams of each kind.  tests/test_draw_cases.py confirms every recorded stream with
the oracle's own orc_rng_seed + orc_rng_random, so a stale or wrong file fails there.

    python tests/golden/make_draw_edge_streams.py        # ~10 s for 2^27 streams
"""
import json
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "draw_edge_streams.json")
SEED, SAMPLE = 5, 1
SCAN_LOG2, CHUNK_LOG2 = 27, 22
PER_CASE = 8
U = np.uint32


def mix32(x):
    x = x ^ (x >> U(16))
    x = x * U(0x7FEB352D)
    x = x ^ (x >> U(15))
    x = x * U(0x846CA68B)
    return x ^ (x >> U(16))


def rotl(x, k):
    return (x << U(k)) | (x >> U(32 - k))


def rng_seed(seed, pixel, sample):
    """trt-rng v1: (s0, s1) of stream (seed, pixel, sample); pixel is a uint32 array."""
    key = mix32(np.array([(seed + 0x9E3779B9) & 0xFFFFFFFF], U))[0]
    s0 = mix32(U(sample) + mix32(pixel ^ key))
    s1 = mix32(pixel + mix32(np.array([sample], U) ^ ~key))
    s1 = np.where((s0 | s1) == 0, U(0x6C078965), s1)
    return s0, s1


def rng_next(s0, s1):
    """(output, s0', s1')"""
    r = s0 * U(0x9E3779BB)
    s1 = s1 ^ s0
    return r, rotl(s0, 26) ^ s1 ^ (s1 << U(9)), rotl(s1, 13)


def scan():
    found = {"u1_zero": [], "u2_zero": [], "u3_zero": []}
    with np.errstate(over="ignore"):
        for c in range(1 << (SCAN_LOG2 - CHUNK_LOG2)):
            j = (np.arange(1 << CHUNK_LOG2, dtype=np.uint64) + (c << CHUNK_LOG2)).astype(U)
            s0, s1 = rng_seed(SEED, j, SAMPLE)
            for name in found:
                r, s0, s1 = rng_next(s0, s1)
                found[name] += [int(x) for x in j[(r >> U(9)) == 0]]
    return found


if __name__ == "__main__":
    found = scan()
    doc = {"seed": SEED, "sample": SAMPLE, "scanned_streams": 1 << SCAN_LOG2, "found": {k: len(v) for k, v in found.items()}}
    doc.update({k: v[:PER_CASE] for k, v in found.items()})
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(doc)
