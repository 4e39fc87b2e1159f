#!/usr/bin/env python3
"""What the sample-parallel route costs the next-event queries on the device beside the folding queries.  Needs a GPU.

  python tools/nee_samples_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/nee_samples_bench.json]

Items, K, seed, depth and scenes are tools/nee_pick_bench.py's: 1024 x 1024 floor surfels with the axis up, K = 16, seed 5,
the cosine source with B = 5 and source_is_diffuse = 1, on the Cornell floor (lamp lowered to y = 99, E = 1), the many-light room (E = 61)
and the 100 k-sphere grid under 64 virtual lamps.  Contenders, the same paths each, in two groups that alternate:
  nee             trt_nee_device(n, K)                                  a lane owns an item for its K samples; 24 bytes written per item
  pair            trt_nee_samples_device(n, K) + trt_fold_samples_device     a lane owns a sample; 12 bytes per SAMPLE written, read again, folded
  mis_pick        trt_nee_mis_pick_device(n, K), balance
  pair_mis_pick   trt_nee_samples_device(weighted, pick) + trt_fold_samples_device
  split_samples   the same pair as two calls over [0, 8) and [8, 16), the second fold with accumulate
  split_items     the same pair as two calls over the two halves of the items (first_stream advanced), ONE record buffer of half the size
                  used twice: what a caller short of the 192 MB of records does
  samples_pair    trt_samples_device(n, K, COSINE) + trt_fold_samples_device with the same depth: the paths without shadow rays
Before anything is timed every pair's sums, second moments and counters are compared by bits (a NaN by NaN-ness) with the folding
query's.  Method: tools/samples_bench.py's, unchanged - one process, every contender warmed, then timed in windows of at least --window-s
seconds of repeated calls between two device events, the contenders of a group alternating, --rounds windows each; the figure is the
median window, the spread (max - min) / median.  Prints one JSON line; --out also writes it to a file."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from direct_bench import cornell                                            # the same items and tables as the other emitter benches  # noqa: E402
from direct_pick_bench import grid_64_lamps, many_light_room                 # noqa: E402
from gather_bench import SEED, SIDE, K                                       # noqa: E402
from samples_bench import PLAN_FIELDS, counted, same_bits, timed             # the method, unchanged  # noqa: E402

BOUNCES = 5
HALF = K // 2


def bench_items(trt, torch, name, scene, items, table, args):
    dev = torch.device("cuda:0")
    n = len(items)
    h = n // 2
    pick, total = trt.lights.pick_table(table)
    d_items = torch.from_numpy(items).to(dev)
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    d_pick = torch.from_numpy(pick.view(np.uint8).copy()).to(dev)
    d_s, d_m, d_s2, d_m2 = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(4))
    d_c = torch.zeros(n * K * 3, dtype=torch.float32, device=dev)
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)
    nee_kw = dict(samples_per_item=K, seed=SEED, source="cosine", source_is_diffuse=True, max_bounces=BOUNCES)
    background = (0.0, 0.0, 0.0)

    def folding(mis, with_pick):
        arg = None if not with_pick else d_pick.data_ptr() if mis is None else (d_pick.data_ptr(), total)

        def call(counters=0):
            scene.nee_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), d_s.data_ptr(), d_m.data_ptr(), d_counters_ptr=counters, mis=mis,
                             pick=arg, **nee_kw)
        return call

    def pair_of(mis, with_pick, ranges=((0, K),), halves=((0, n),)):
        arg = None if not with_pick else d_pick.data_ptr() if mis is None else (d_pick.data_ptr(), total)

        def call(counters=0):
            for first, count in halves:
                # one half of the items reuses the record buffer's start: the records of a half are its own
                rec = d_c.data_ptr() if len(halves) > 1 else d_c.data_ptr() + first * K * 12
                for k, (b, e) in enumerate(ranges):
                    scene.nee_samples_device(d_items.data_ptr() + first * 24, count, d_table.data_ptr(), len(table), rec, d_counters_ptr=counters, mis=mis,
                                             pick=arg, sample_begin=b, sample_end=e, first_stream=first * K, **nee_kw)
                    trt.fold_samples_device(rec, count, K, d_s2.data_ptr() + first * 12, d_m2.data_ptr() + first * 12, sample_begin=b, sample_end=e,
                                            accumulate=k > 0)
        return call

    def samples_pair(counters=0):
        scene.samples_device(d_items.data_ptr(), n, d_c.data_ptr(), d_counters_ptr=counters, samples_per_item=K, source="cosine", max_bounces=BOUNCES,
                             background=background, seed=SEED)
        trt.fold_samples_device(d_c.data_ptr(), n, K, d_s2.data_ptr(), d_m2.data_ptr())

    groups = [{"nee": folding(None, False), "pair": pair_of(None, False)},
              {"mis_pick": folding("balance", True), "pair_mis_pick": pair_of("balance", True),
               "split_samples": pair_of("balance", True, ranges=((0, HALF), (HALF, K))),
               "split_items": pair_of("balance", True, halves=((0, h), (h, n - h))), "samples_pair": samples_pair}]
    out = {"items": n, "emitters": len(table), "paths_per_job": n * K, "record_bytes": n * K * 12, "record_bytes_split_items": (n - h) * K * 12}
    rays = {}
    for group in groups:
        reference = next(iter(group))
        want = counted(torch, ctr, group[reference])
        rays[reference] = want[1]
        for key, call in group.items():
            if key in (reference, "samples_pair"):
                continue
            d_s2.fill_(7.5)
            d_m2.fill_(7.5)
            got = counted(torch, ctr, call)
            if got != want or not same_bits(torch, d_s2, d_s) or not same_bits(torch, d_m2, d_m):
                raise SystemExit("%s: the fold of %s is not %s" % (name, key, reference))
            rays[key] = got[1]
    rays["samples_pair"] = counted(torch, ctr, samples_pair)[1]
    plans = {"nee": scene.nee_plan(n), "pair": scene.nee_samples_plan(n, K), "mis_pick": scene.nee_plan(n, mis="balance", pick=True),
             "pair_mis_pick": scene.nee_samples_plan(n, K, mis="balance", pick=True),
             "split_samples": scene.nee_samples_plan(n, HALF, mis="balance", pick=True),
             "split_items": scene.nee_samples_plan(h, K, mis="balance", pick=True), "samples_pair": scene.samples_plan(n, K)}
    for group in groups:
        t = timed(torch, group, args)
        for key in t:
            t[key]["rays"] = rays[key]
            t[key]["rays_per_sample"] = round(rays[key] / (n * K), 4)
            t[key]["mpaths_per_s"] = round(n * K / t[key]["ms_per_job_median"] / 1e3, 2)
            t[key]["plan"] = {f: v for f, v in plans[key].items() if f in PLAN_FIELDS}
        out.update(t)

    def ratio(tag, a, b):
        out["time_%s_over_%s" % (a, b)] = round(out[a]["ms_per_job_median"] / out[b]["ms_per_job_median"], 4)
        out["%s_faster_beyond_the_spreads" % tag] = bool(out[a]["ms_per_job_max"] < out[b]["ms_per_job_min"])

    ratio("pair", "pair", "nee")
    ratio("pair_mis_pick", "pair_mis_pick", "mis_pick")
    ratio("split_samples", "split_samples", "mis_pick")
    ratio("split_items", "split_items", "mis_pick")
    ratio("pair_mis_pick_against_samples_pair", "pair_mis_pick", "samples_pair")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3 or args.window_s < 1.0:
        ap.error("at least 3 windows of at least 1 s per contender")
    import torch
    trt = importlib.import_module("tiny-raytracer_amd")
    trt._lib.check(trt.lib.trt_set_device(0))
    out = {"metric": "ms per job of n x K samples (device events around a window of jobs, median window)", "rounds": args.rounds,
           "window_s": args.window_s, "device": torch.cuda.get_device_name(0), "library": os.path.basename(trt._lib.LIB_PATH),
           "samples_per_item": K, "seed": SEED, "side": SIDE, "max_bounces": BOUNCES, "source": "cosine", "source_is_diffuse": 1,
           "ratios": "time_A_over_B = median ms of A / median ms of B: below 1, A is faster; spread = (max - min) / median; every pair includes its "
                     "fold; samples_pair traces the same first rays without shadow rays",
           "shapes_timed": "whatever shape each scene's plan names (see the plans); the other shapes were run by the tests only and were not timed"}
    for name, make in (("cornell_floor", lambda: cornell(trt, 99.0)), ("many_light_room", lambda: many_light_room(trt)),
                       ("sphere_grid_64_lamps", lambda: grid_64_lamps(trt))):
        scene, items, table = make()
        out[name] = bench_items(trt, torch, name, scene, items, table, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
