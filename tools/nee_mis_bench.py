#!/usr/bin/env python3
"""What a weighted next-event query (trt_nee_mis) costs on the device beside the plain one and the gather query of the same items, and
what the weights buy.  Needs a GPU.

  python tools/nee_mis_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/nee_mis_bench.json]

Items, tables, K, seed and protocol are tools/nee_bench.py's: 1024 x 1024 floor surfels with the axis up over the floor of the Cornell box
with the lamp lowered to y = 99 and over the 100 k-sphere grid's ground, K = 16, seed 5, cosine source, max_bounces = 5; the box's own lamp,
and for the grid, which has no light, direct_bench's virtual quad lamp (there every contender but the gather adds light no path can hit,
the weighted queries return trt_nee's bytes - a virtual emitter's wl is 1 - and only times and rays are compared).  Contenders, n x K
samples each, in one process:
  mis_balance, mis_power   trt_nee_mis_device(n, K, table, source_is_diffuse = 0) with either heuristic
  nee                      trt_nee_device, the same call unweighted
  gather                   trt_gather_device(n, K, cosine)
  bake_balance, bake_power trt_direct_device(n, K, table) with seed + 1, then trt_nee_mis_device(source_is_diffuse = 1): the full bake of
                           tinyrt.h; independent streams, so the sample variance of the sum is the sum of the sample variances
Timing: each contender is warmed, then timed in windows of at least --window-s seconds of repeated calls between two device events; the
contenders alternate, --rounds windows each; the figure is the median window.

Reported per scene and contender: the time, rays per sample, the per-item sample variance of the red channel from moment2,
K / (K - 1) x (moment2 - radiance^2) averaged over the items, and the mean; per scene the times over trt_nee_device's and over the
gather's, and DESIGN.md 6.13's equal-time efficiency (var_gather x t_gather) / (var x t) for every contender that estimates the gather's
integral: above 1, the contender reaches a given noise sooner.  Prints one JSON line; --out also writes it to a file."""
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

from direct_bench import PLAN_KEYS, cornell, grid                            # the same items and tables as the direct-light bench  # noqa: E402
from gather_bench import SEED, SIDE, K, window                               # the same K, seed and window as the other query benches  # noqa: E402
from nee_bench import MAX_BOUNCES                                            # noqa: E402

BAKES = ("bake_balance", "bake_power")


def bench_scene(trt, torch, scene, items, table, background, same_integral, args):
    dev = torch.device("cuda:0")
    n = len(items)
    d_items = torch.from_numpy(items).to(dev)
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    keys = ("mis_balance", "mis_power", "nee", "gather") + BAKES
    sums = {key: tuple(torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2)) for key in keys + ("bake_direct",)}
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)
    path = dict(samples_per_item=K, max_bounces=MAX_BOUNCES, background=background, seed=SEED)

    def nee_call(key, **kw):
        def call(counters=0):
            s, m = sums[key]
            scene.nee_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), s.data_ptr(), m.data_ptr(), d_counters_ptr=counters,
                             source="cosine", **kw, **path)
        return call

    def gather(counters=0):
        s, m = sums["gather"]
        scene.gather_device(d_items.data_ptr(), n, s.data_ptr(), m.data_ptr(), d_counters_ptr=counters, lobe="cosine", **path)

    def bake_call(key, mis):
        indirect = nee_call(key, mis=mis, source_is_diffuse=True)

        def call(counters=0):
            s, m = sums["bake_direct"]
            scene.direct_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), s.data_ptr(), m.data_ptr(), d_counters_ptr=counters,
                                samples_per_item=K, seed=SEED + 1)
            indirect(counters)
        return call

    calls = {"mis_balance": nee_call("mis_balance", mis="balance"), "mis_power": nee_call("mis_power", mis="power"), "nee": nee_call("nee"),
             "gather": gather, "bake_balance": bake_call("bake_balance", "balance"), "bake_power": bake_call("bake_power", "power")}
    plans = {key: scene.nee_plan(n, mis="balance") for key in keys}
    plans["nee"], plans["gather"] = scene.nee_plan(n), scene.gather_plan(n)
    rays = {}
    for key, call in calls.items():                                         # the rays of a job; also the first launch
        ctr.zero_()
        call(ctr.data_ptr())
        torch.cuda.synchronize()
        assert int(ctr[0]) == n * K * (2 if key in BAKES else 1)
        rays[key] = int(ctr[1])
    assert rays["mis_balance"] == rays["mis_power"] == rays["nee"]         # the walks are trt_nee's
    out = {"items": n, "emitters": len(table), "samples_per_job": n * K, "max_bounces": MAX_BOUNCES, "background": list(background),
           "same_integral": same_integral}
    stats = {}
    for key in calls:
        s, m = (t.view(n, 3)[:, 0].double() for t in sums[key])
        var = torch.clamp(m - s * s, min=0.0) * (K / (K - 1.0))
        if key in BAKES:                                                    # + the direct light: independent streams, the variances add
            ds, dm = (t.view(n, 3)[:, 0].double() for t in sums["bake_direct"])
            var = var + torch.clamp(dm - ds * ds, min=0.0) * (K / (K - 1.0))
            s = s + ds
        stats[key] = {"mean_red": round(float(s.mean()), 5), "mean_sample_variance_red": round(float(var.mean()), 6),
                      "mean_sample_sd_over_mean": round(float(var.sqrt().mean() / s.mean()), 4)}
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
    vg = stats["gather"]["mean_sample_variance_red"]
    for key in calls:
        if key == "gather":
            continue
        if key != "nee":
            out["time_%s_over_nee" % key] = round(med[key] / med["nee"], 4)
        out["time_%s_over_gather" % key] = round(med[key] / med["gather"], 4)
        v = stats[key]["mean_sample_variance_red"]
        if same_integral and v > 0.0:
            out["variance_gather_over_%s" % key] = round(vg / v, 3)
            out["equal_time_efficiency_%s" % key] = round((vg * med["gather"]) / (v * med[key]), 3)
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
           "samples_per_item": K, "seed": SEED, "side": SIDE,
           "ratios": "time_X_over_Y = median ms of X / median ms of Y; equal_time_efficiency_X = (var_gather * t_gather) / (var_X * t_X): "
                     "above 1, X reaches a given noise sooner; spread = (max - min) / median"}
    scene, items, table = cornell(trt, 99.0)
    out["cornell_lamp_lowered"] = bench_scene(trt, torch, scene, items, table, (0.0, 0.0, 0.0), True, args)
    scene, items, table = grid(trt)
    sky = tuple(float(c) for c in trt.scenes.sphere_grid(100000, 2, 2)["background"])
    out["sphere_grid_100k"] = bench_scene(trt, torch, scene, items, table, sky, False, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
