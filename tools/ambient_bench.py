#!/usr/bin/env python3
"""What an ambient query costs on the device, beside the two routes to the same estimate that existed before it.  Needs a GPU.

  python tools/ambient_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/ambient_bench.json]

Cornell and the 100 k-sphere grid.  Items: the surfel list of tools/gather_bench.py - the render's own rays for sample 0 at 1024 x 1024
(trt_primary_rays_device) through Scene.intersect; a ray that hits gives the surfel (hit point, normal), a ray that misses stays as a
probe; the axis of every third item is scaled by 0.25 and of the next by 3.  K = 16 samples per item, seed 5, cosine lobe, and two
distances: +inf, and one finite distance D = the median finite hit distance of a million of the explicit rays below (about half of the
hits at +inf lie beyond it).  Contenders, n x K samples each:
  ambient   trt_ambient_device(n, K, max_distance)             24 bytes read per item, 16 written
  gather1   trt_gather_device(n, K, max_bounces = 1, white)    the workaround before trt_ambient: a closest-hit walk and a shade per sample,
            no distance (the same job at both distances), lights add their colour instead of blocking, no direction; 24 bytes written
  occluded  trt_occluded_device(n x K rays, t_max)             the first rays already resident in HBM, 24 (+ 4 with a t_max) bytes read and
            1 written per SAMPLE; the upload of the rays, the download of the bytes and the fold on the host that this route also needs
            are NOT timed
The explicit rays are drawn here by the same rule (Lambertian::scatter about the item's axis) with numpy, from a generator of numpy's:
the same distribution, not the same rays, so the mean visibility of the two routes agrees to sampling noise and is in the line.  Timing:
every contender is warmed, then timed in windows of at least --window-s seconds of repeated calls between two device events; the
contenders alternate, --rounds windows each, in one process; the figure is the median window, and the spread of a contender is
(max - min) / median of its windows.  No ratio is fixed in advance; the expectation that ambient is not slower than gather1 beyond
gather1's own spread is recorded as true or false.  Prints one JSON line; --out also writes it to a file."""
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

from gather_bench import SEED, SIDE, K, cosine_rays, surfels, window                     # the same items, the same explicit draw  # noqa: E402

PLAN_KEYS = ("scene_mode", "walk", "threads_per_workgroup", "kernel_waves_per_simd", "workgroups_per_cu", "rays_per_wave", "waves", "wave_slots",
             "workgroups")


def bench_scene(trt, torch, name, desc, args):
    dev = torch.device("cuda:0")
    world, cam = trt.world_from_description(desc)
    scene = world.get_bvh()
    n = SIDE * SIDE
    items, n_surfels = surfels(trt, torch, scene, cam, n)
    d_items = torch.from_numpy(items).to(dev)
    rays = cosine_rays(items, K, SEED)
    # the finite distance: the median finite hit distance of a million of the explicit rays (every 16th)
    t = scene.intersect(rays[::K])["t"]
    finite = float(np.float32(np.median(t[np.isfinite(t)].astype(np.float64))))
    d_rays = torch.from_numpy(rays).to(dev)
    del rays
    d_tmax = torch.full((n * K,), finite, dtype=torch.float32, device=dev)
    d_vis = torch.zeros(n, dtype=torch.float32, device=dev)
    d_bent = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    d_s, d_m = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2))
    d_occ = torch.zeros(n * K, dtype=torch.uint8, device=dev)
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)
    out = {"items": n, "surfels": n_surfels, "probes": n - n_surfels, "samples_per_job": n * K, "finite_distance": finite}
    plans = {"ambient": scene.ambient_plan(n), "gather1": scene.gather_plan(n), "occluded": scene.query_plan(n * K)}
    for label, dist in (("inf", float("inf")), ("finite", finite)):

        def ambient(counters=0):
            scene.ambient_device(d_items.data_ptr(), n, d_vis.data_ptr(), d_bent.data_ptr(), d_counters_ptr=counters, samples_per_item=K, lobe="cosine",
                                 max_distance=dist, seed=SEED)

        def gather1(counters=0):
            scene.gather_device(d_items.data_ptr(), n, d_s.data_ptr(), d_m.data_ptr(), d_counters_ptr=counters, samples_per_item=K, lobe="cosine",
                                max_bounces=1, background=(1.0, 1.0, 1.0), seed=SEED)

        def occluded(counters=0):
            scene.occluded_device(d_rays.data_ptr(), n * K, d_occ.data_ptr(), d_t_max_ptr=0 if label == "inf" else d_tmax.data_ptr())

        calls = {"ambient": ambient, "gather1": gather1, "occluded": occluded}
        walks = {}
        for key in ("ambient", "gather1"):                                  # the walks of a job; also the first launch
            ctr.zero_()
            calls[key](ctr.data_ptr())
            torch.cuda.synchronize()
            assert int(ctr[0]) == n * K
            walks[key] = int(ctr[1])
        occluded()
        torch.cuda.synchronize()
        walks["occluded"] = n * K
        # the routes estimate the same thing: the mean visibility over all items agrees to sampling noise
        mean_vis = {"ambient": float(d_vis.double().mean()), "occluded": float(1.0 - d_occ.double().mean())}
        if abs(mean_vis["ambient"] - mean_vis["occluded"]) > 0.005:
            raise SystemExit("%s %s: the mean visibility of ambient and of the explicit rays differ: %r" % (name, label, mean_vis))
        reps, windows = {}, {k: [] for k in calls}
        for key, call in calls.items():                                     # warm-up and the repetitions of a window
            call()
            torch.cuda.synchronize()
            once = window(torch, call, 1)
            reps[key] = max(1, int(np.ceil(1000.0 * args.window_s / once)))
        for _ in range(args.rounds):
            for key, call in calls.items():
                windows[key].append(window(torch, call, reps[key]))
        res = {"max_distance": "inf" if label == "inf" else finite, "mean_visibility": {k: round(v, 5) for k, v in mean_vis.items()}}
        med, spread = {}, {}
        for key in calls:
            ms = sorted(windows[key])
            med[key] = ms[len(ms) // 2]
            spread[key] = (ms[-1] - ms[0]) / med[key]
            q = plans[key]
            res[key] = {"ms_per_job_median": round(med[key], 3), "ms_per_job_min": round(ms[0], 3), "ms_per_job_max": round(ms[-1], 3),
                        "spread": round(spread[key], 4), "jobs_per_window": reps[key], "windows": len(ms),
                        "msamples_per_s": round(n * K / med[key] / 1e3, 2), "walks": walks[key], "plan": {k: q[k] for k in PLAN_KEYS}}
        res["time_ambient_over_gather1"] = round(med["ambient"] / med["gather1"], 4)
        res["time_ambient_over_occluded"] = round(med["ambient"] / med["occluded"], 4)
        res["ambient_not_slower_than_gather1_beyond_its_spread"] = bool(med["ambient"] <= med["gather1"] * (1.0 + spread["gather1"]))
        out[label] = res
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
           "samples_per_item": K, "seed": SEED, "lobe": "cosine", "width": SIDE, "height": SIDE,
           "ratios": "time_ambient_over_gather1 = median ms of ambient / median ms of gather1: below 1, ambient is faster; spread = (max - min) / median"}
    for name, desc in (("cornell", trt.scenes.cornell(SIDE, SIDE)), ("sphere_grid_100k", trt.scenes.sphere_grid(100000, SIDE, SIDE))):
        out[name] = bench_scene(trt, torch, name, desc, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
