#!/usr/bin/env python3
"""What a direct-light query costs on the device beside an ambient query over the same items, and what it buys beside a gather.  Needs a GPU.

  python tools/direct_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/direct_bench.json]

Items: 1024 x 1024 floor surfels with the axis up - bake.quad_texels over the Cornell box's floor quad, and a square lattice over the
100 k-sphere grid's ground, 1 mm above it.  K = 16 samples per item, seed 5.  Tables: the Cornell box's own lamp (Scene.emitters()); for
the grid, which has no light, one virtual quad lamp of a quarter of the field's side, 30 above it (lights.quad).  Contenders, n x K
samples each:
  direct    trt_direct_device(n, K, table)                      24 bytes read per item, 24 written; a walk per live sample
  ambient   trt_ambient_device(n, K, cosine, max_distance inf)  24 bytes read per item, 16 written; a walk per sample
Timing: each contender is warmed, then timed in windows of at least --window-s seconds of repeated calls between two device events; the
contenders alternate, --rounds windows each, in one process; the figure is the median window and the spread of a contender is
(max - min) / median of its windows.  The expectation direct <= 1.25 x ambient - the draw adds one table read, a division and some twenty
vector instructions to a walk of hundreds - is recorded as true or false; it is no condition.

Variance: on the Cornell box with the lamp lowered to y = 99 (the stock lamp is coplanar with the ceiling, which hides it from the
reference's own paths about three times in four: a property of that scene) the per-item sample variance of the red channel,
K / (K - 1) x (moment2 - radiance^2) averaged over the items, of direct and of trt_gather_device with max_bounces = 1 and a black
background - the same integral found by chance - and the two means.  Prints one JSON line; --out also writes it to a file."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gather_bench import SEED, SIDE, K, window                               # the same K, seed and window as the other query benches  # noqa: E402

PLAN_KEYS = ("scene_mode", "walk", "threads_per_workgroup", "kernel_waves_per_simd", "workgroups_per_cu", "rays_per_wave", "waves", "wave_slots",
             "workgroups")
MARGIN = 1.25


def cornell(trt, lamp_y=None):
    desc = trt.scenes.cornell(2, 2)
    if lamp_y is not None:
        geos = list(desc["geometries"])
        kind, corner, u, v, material = geos[2]
        assert kind == "quad" and material == "light"
        geos[2] = (kind, (corner[0], lamp_y, corner[2]), u, v, material)
        desc = dict(desc, geometries=geos)
    scene = trt.world_from_description(desc)[0].get_bvh()
    kind, corner, u, v, _ = desc["geometries"][3]
    assert kind == "quad"
    return scene, trt.bake.quad_texels(corner, u, v, SIDE, SIDE, flip=True), scene.emitters()


def grid(trt):
    n = 100000
    scene = trt.world_from_description(trt.scenes.sphere_grid(n, 2, 2))[0].get_bvh()
    half = math.sqrt(n) / 2.0
    c = ((np.arange(SIDE) + 0.5) / SIDE * 2.0 - 1.0) * half
    items = np.zeros((SIDE, SIDE, 6), np.float32)
    items[..., 0], items[..., 2] = c[None, :], c[:, None]
    items[..., 1], items[..., 4] = 1e-3, 1.0
    q = half / 4.0
    return scene, np.ascontiguousarray(items.reshape(-1, 6)), trt.lights.quad((-q, 30.0, -q), (2.0 * q, 0.0, 0.0), (0.0, 0.0, 2.0 * q), (10.0, 10.0, 10.0))


def bench_scene(trt, torch, scene, items, table, args):
    dev = torch.device("cuda:0")
    n = len(items)
    d_items = torch.from_numpy(items).to(dev)
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    d_s, d_m, d_bent = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(3))
    d_vis = torch.zeros(n, dtype=torch.float32, device=dev)
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)

    def direct(counters=0):
        scene.direct_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), d_s.data_ptr(), d_m.data_ptr(), d_counters_ptr=counters,
                            samples_per_item=K, seed=SEED)

    def ambient(counters=0):
        scene.ambient_device(d_items.data_ptr(), n, d_vis.data_ptr(), d_bent.data_ptr(), d_counters_ptr=counters, samples_per_item=K, lobe="cosine",
                             seed=SEED)

    calls = {"direct": direct, "ambient": ambient}
    plans = {"direct": scene.direct_plan(n), "ambient": scene.ambient_plan(n)}
    walks = {}
    for key, call in calls.items():                                         # the walks of a job; also the first launch
        ctr.zero_()
        call(ctr.data_ptr())
        torch.cuda.synchronize()
        assert int(ctr[0]) == n * K
        walks[key] = int(ctr[1])
    out = {"items": n, "emitters": len(table), "samples_per_job": n * K, "mean_direct_red": round(float(d_s.view(n, 3)[:, 0].double().mean()), 5),
           "mean_visibility": round(float(d_vis.double().mean()), 5)}
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
        out[key] = {"ms_per_job_median": round(med[key], 3), "ms_per_job_min": round(ms[0], 3), "ms_per_job_max": round(ms[-1], 3),
                    "spread": round((ms[-1] - ms[0]) / med[key], 4), "jobs_per_window": reps[key], "windows": len(ms),
                    "msamples_per_s": round(n * K / med[key] / 1e3, 2), "walks": walks[key], "plan": {k: q[k] for k in PLAN_KEYS}}
    out["time_direct_over_ambient"] = round(med["direct"] / med["ambient"], 4)
    out["direct_within_1.25x_of_ambient"] = bool(med["direct"] <= MARGIN * med["ambient"])
    return out


def variance(trt, torch, scene, items, table):
    dev = torch.device("cuda:0")
    n = len(items)
    d_items = torch.from_numpy(items).to(dev)
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    out = {"lamp_y": 99.0, "items": n, "samples_per_item": K, "channel": "red"}
    for key in ("direct", "gather1"):
        d_s, d_m = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2))
        if key == "direct":
            scene.direct_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), d_s.data_ptr(), d_m.data_ptr(), samples_per_item=K, seed=SEED)
        else:
            scene.gather_device(d_items.data_ptr(), n, d_s.data_ptr(), d_m.data_ptr(), samples_per_item=K, lobe="cosine", max_bounces=1,
                                background=(0.0, 0.0, 0.0), seed=SEED)
        torch.cuda.synchronize()
        s, m = d_s.view(n, 3)[:, 0].double(), d_m.view(n, 3)[:, 0].double()
        var = torch.clamp(m - s * s, min=0.0) * (K / (K - 1.0))
        out[key] = {"mean": round(float(s.mean()), 5), "mean_sample_variance": round(float(var.mean()), 5),
                    "mean_sample_sd_over_mean": round(float(var.sqrt().mean() / s.mean()), 4)}
    out["variance_gather1_over_direct"] = round(out["gather1"]["mean_sample_variance"] / out["direct"]["mean_sample_variance"], 2)
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
           "ratios": "time_direct_over_ambient = median ms of direct / median ms of ambient: below 1, direct is faster; spread = (max - min) / median",
           "expectation": "direct <= 1.25 x ambient, recorded per scene; not a condition"}
    out["cornell"] = bench_scene(trt, torch, *cornell(trt), args)
    out["sphere_grid_100k"] = bench_scene(trt, torch, *grid(trt), args)
    out["cornell_lamp_lowered_variance"] = variance(trt, torch, *cornell(trt, 99.0))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
