#!/usr/bin/env python3
"""What choosing the emitter of every vertex's shadow ray through an alias table (trt_nee_pick, trt_nee_mis_pick) costs on the device beside
the uniform choice, and what it buys where the emitters' powers differ.  Needs a GPU.

  python tools/nee_pick_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/nee_pick_bench.json]

Items, K, seed and protocol are tools/direct_pick_bench.py's: 1024 x 1024 floor surfels with the axis up, K = 16, seed 5; the next-event
queries run the cosine source with B = 5 and source_is_diffuse = 1, the indirect half of a bake.  Three sets:
  cornell_one_lamp     the Cornell box with the lamp lowered to y = 99, its own table (E = 1) and the power table of it: both queries
                       choose record 0, so the extra draw and the two loads per vertex are the only difference - THE TIME OF THE DRAW
  many_light_room      the lowered box with sixty sphere lights of radius 1 and 0.05 x the lamp's colour along three walls (E = 61, the
                       lamp 94 % of the power): THE GAIN, for trt_nee_pick against trt_nee and trt_nee_mis_pick against trt_nee_mis
                       (balance), and for the bake pair trt_direct_mis_pick + trt_nee_mis_pick against trt_direct_mis + trt_nee_mis
  sphere_grid_64_lamps the 100 k-sphere grid under 8 x 8 virtual quad lamps of one size whose colours, hence powers, span 1 : 1000 (no
                       light is geometry, so the weighted queries return the unweighted bytes and are left out; the bake pair is
                       trt_direct_pick + trt_nee_pick against trt_direct + trt_nee)
Timing: each contender is warmed, then timed in windows of at least --window-s seconds of repeated calls between two device events on
the stream; the contenders alternate in one process, --rounds windows each; the figure is the median window, the spread (max - min) /
median.  Reported per set and contender: the time, rays per sample, the mean and the per-item sample variance of the red channel from
moment2, K / (K - 1) x (moment2 - radiance^2) averaged over the items; per pair time_pick_over_uniform and the equal-time efficiency
(var_uniform x t_uniform) / (var_pick x t_pick), section 6.13's measure: above 1 the table reaches a given noise sooner, below 1 it does
not pay.  A bake's two halves draw from different streams: its variance and its time are the halves' sums.  Prints one JSON line; --out
also writes it to a file."""
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

from direct_bench import PLAN_KEYS, cornell                                 # the same items and tables as the direct-light benches  # noqa: E402
from direct_pick_bench import grid_64_lamps, many_light_room                 # noqa: E402
from gather_bench import SEED, SIDE, K, window                               # the same K, seed and window as the other query benches  # noqa: E402

BOUNCES = 5


def bench_items(trt, torch, scene, items, table, weighted, args):
    dev = torch.device("cuda:0")
    n = len(items)
    pick, total = trt.lights.pick_table(table)
    d_items = torch.from_numpy(items).to(dev)
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    d_pick = torch.from_numpy(pick.view(np.uint8).copy()).to(dev)
    mis = "balance" if weighted else None
    # (contender, query, mis, through the table?): the next-event pairs, and the direct half of the bake pair
    contenders = [("uniform", "nee", None, False), ("pick", "nee", None, True)]
    if weighted:
        contenders += [("mis_uniform", "nee", mis, False), ("mis_pick", "nee", mis, True)]
    contenders += [("direct_uniform", "direct", mis, False), ("direct_pick", "direct", mis, True)]
    sums = {c[0]: tuple(torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2)) for c in contenders}
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)

    def make(key, query, how, with_pick):
        def call(counters=0):
            s, m = sums[key]
            table_arg = None if not with_pick else (d_pick.data_ptr() if how is None else (d_pick.data_ptr(), total))
            head = (d_items.data_ptr(), n, d_table.data_ptr(), len(table), s.data_ptr(), m.data_ptr())
            if query == "nee":
                scene.nee_device(*head, d_counters_ptr=counters, samples_per_item=K, seed=SEED, source="cosine", source_is_diffuse=True,
                                 max_bounces=BOUNCES, mis=how, pick=table_arg)
            else:
                scene.direct_device(*head, d_counters_ptr=counters, samples_per_item=K, seed=SEED, mis=how, pick=table_arg)
        return call

    calls = {key: make(key, query, how, with_pick) for key, query, how, with_pick in contenders}
    plans = {key: (scene.nee_plan if query == "nee" else scene.direct_plan)(n, mis=how, pick=True if with_pick else None)
             for key, query, how, with_pick in contenders}
    rays = {}
    for key, call in calls.items():                                         # the rays of a job; also the first launch
        ctr.zero_()
        call(ctr.data_ptr())
        torch.cuda.synchronize()
        assert int(ctr[0]) == n * K
        rays[key] = int(ctr[1])
    out = {"items": n, "emitters": len(table), "samples_per_job": n * K, "largest_prob": round(float(pick["prob"].max()), 5),
           "smallest_prob": float(pick["prob"].min())}
    stats = {}
    for key in calls:
        s, m = (t.view(n, 3)[:, 0].double() for t in sums[key])
        var = torch.clamp(m - s * s, min=0.0) * (K / (K - 1.0))
        stats[key] = {"mean_red": round(float(s.mean()), 5), "mean_sample_variance_red": float(var.mean()),
                      "largest_item_sample_variance_red": round(float(var.max()), 4)}
    reps, windows = {}, {k: [] for k in calls}
    for key, call in calls.items():                                         # warm-up and the repetitions of a window
        call()
        torch.cuda.synchronize()
        reps[key] = max(1, int(np.ceil(1000.0 * args.window_s / window(torch, call, 1))))
    for _ in range(args.rounds):
        for key, call in calls.items():
            windows[key].append(window(torch, call, reps[key]))
    med = {}
    for key in calls:
        ms = sorted(windows[key])
        med[key] = ms[len(ms) // 2]
        q = plans[key]
        out[key] = dict(stats[key], ms_per_job_median=round(med[key], 3), ms_per_job_min=round(ms[0], 3), ms_per_job_max=round(ms[-1], 3),
                        spread=round((ms[-1] - ms[0]) / med[key], 4), jobs_per_window=reps[key], windows=len(ms),
                        msamples_per_s=round(n * K / med[key] / 1e3, 2), rays=rays[key], rays_per_sample=round(rays[key] / (n * K), 4),
                        plan={k: q[k] for k in PLAN_KEYS})

    def compare(tag, uniform, picked):
        """uniform, picked: tuples of contenders whose times and variances add (one query, or the two halves of a bake)."""
        tu, tp = sum(med[k] for k in uniform), sum(med[k] for k in picked)
        vu = sum(stats[k]["mean_sample_variance_red"] for k in uniform)
        vp = sum(stats[k]["mean_sample_variance_red"] for k in picked)
        out["time_%s_over_uniform" % tag] = round(tp / tu, 4)
        if vp > 0.0:
            out["variance_uniform_over_%s" % tag] = round(vu / vp, 3)
            eff = (vu * tu) / (vp * tp)
            out["equal_time_efficiency_%s_against_uniform" % tag] = round(eff, 3)
            out["%s_pays" % tag] = bool(eff > 1.0)

    compare("pick", ("uniform",), ("pick",))
    if weighted:
        compare("mis_pick", ("mis_uniform",), ("mis_pick",))
    compare("bake_pick", ("direct_uniform", "mis_uniform" if weighted else "uniform"), ("direct_pick", "mis_pick" if weighted else "pick"))
    out["bake_pair"] = ("trt_direct_mis_pick + trt_nee_mis_pick against trt_direct_mis + trt_nee_mis (balance)" if weighted else
                        "trt_direct_pick + trt_nee_pick against trt_direct + trt_nee")
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
           "ratios": "time_X_over_uniform = median ms of X / median ms of its uniform partner; equal_time_efficiency_X_against_uniform = "
                     "(var_uniform * t_uniform) / (var_X * t_X): above 1, X reaches a given noise sooner; a bake's times and variances are "
                     "the sums of its two halves; spread = (max - min) / median",
           "shapes_timed": "the lock-step list from LDS (cornell_one_lamp), the 16-byte-node walk from global memory (the grid set) and "
                           "whatever shape the many-light room's 79 primitives get (see its plan); the other shapes were run by the tests "
                           "only and were not timed"}
    scene, items, table = cornell(trt, 99.0)
    out["cornell_one_lamp"] = bench_items(trt, torch, scene, items, table, True, args)
    scene, items, table = many_light_room(trt)
    out["many_light_room"] = bench_items(trt, torch, scene, items, table, True, args)
    scene, items, table = grid_64_lamps(trt)
    out["sphere_grid_64_lamps"] = bench_items(trt, torch, scene, items, table, False, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
