#!/usr/bin/env python3
"""What a passes query costs on the device beside a gather query of the same items.  Needs a GPU.

  python tools/passes_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/passes_bench.json]

Items: 1024 x 1024 surfels on the floor of each scene, axis = the floor's unit normal.  Cornell: bake.quad_texels over the floor quad, as
examples/bake_passes.py lays them.  The 100 k-sphere grid: a regular grid over the square the spheres are scattered on, each point on the
ground sphere with its outward normal.  K = 16 samples per item, cosine lobe, max_bounces 50, seed 5, the scene's own background:
tools/gather_bench.py's parameters.  Contenders, n x K paths each, THE SAME paths (a passes query draws and traces what the gather does;
the tool checks that the reference's ray counts are equal):
  passes1   trt_passes_device(n, K), 1 depth bin     24 bytes read per item, 24 + 4 written; the kernels that carry 2 bins
  passes2   trt_passes_device(n, K), 2 depth bins    24 bytes read per item, 48 + 4 written; the same kernels
  passes4   trt_passes_device(n, K), 4 depth bins    24 bytes read per item, 96 + 4 written; the kernels that carry 4 bins
  gather    trt_gather_device(n, K), cosine lobe     24 bytes read per item, 24 written (radiance and second moments); the same launch
            shape, the gather kernels' own launch bound
Timing (tools/gather_bench.py's): every contender is warmed, then timed in windows of at least --window-s seconds of repeated calls between
two device events; the contenders alternate, --rounds windows each, in one process; the figure is the median window, and the spread of a
contender is (max - min) / median of its windows.  Prints one JSON line; --out also writes it to a file."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import gather_bench as GB  # noqa: E402

K, DEPTH, SEED, SIDE = GB.K, GB.DEPTH, GB.SEED, GB.SIDE
PLAN_FIELDS = ("scene_mode", "walk", "threads_per_workgroup", "kernel_waves_per_simd", "workgroups_per_cu", "rays_per_wave", "waves", "wave_slots",
               "workgroups")
BINS = (1, 2, 4)


def cornell_floor(trt, desc):
    kind, corner, u, v, _ = desc["geometries"][3]
    assert kind == "quad"
    return trt.bake.quad_texels(corner, u, v, SIDE, SIDE, flip=True)         # cross(u, v) points down


def grid_floor(desc):
    """SIDE x SIDE points of the ground sphere over the square of the small spheres, each with the ground's outward unit normal."""
    kind, centre, radius, _ = desc["geometries"][0]
    assert kind == "sphere" and radius == 1000.0
    half = np.sqrt(len(desc["geometries"]) - 1) / 2.0
    a = ((np.arange(SIDE, dtype=np.float64) + 0.5) / SIDE * 2.0 - 1.0) * half
    x, z = np.meshgrid(a, a)
    normal = np.stack([x, np.sqrt(radius * radius - x * x - z * z), z], axis=-1) / radius
    point = np.asarray(centre, np.float64) + radius * normal
    return np.ascontiguousarray(np.concatenate([point, normal], axis=-1).reshape(-1, 6).astype(np.float32))


def bench_scene(trt, torch, name, desc, items, args):
    dev = torch.device("cuda:0")
    scene = trt.world_from_description(desc)[0].get_bvh()
    n = len(items)
    assert n == SIDE * SIDE
    bg = tuple(desc["background"])
    d_items = torch.from_numpy(items).to(dev)
    d_p = {b: torch.zeros(n * 6 * b, dtype=torch.float32, device=dev) for b in BINS}
    d_spent = torch.zeros(n, dtype=torch.float32, device=dev)
    d_s, d_m = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2))
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)
    path = dict(max_bounces=DEPTH, background=bg, seed=SEED)

    def passes(bins):
        def call(counters=0):
            scene.passes_device(d_items.data_ptr(), n, d_p[bins].data_ptr(), d_spent.data_ptr(), d_counters_ptr=counters, samples_per_item=K,
                                depth_bins=bins, source="cosine", **path)
        return call

    def gather(counters=0):
        scene.gather_device(d_items.data_ptr(), n, d_s.data_ptr(), d_m.data_ptr(), d_counters_ptr=counters, samples_per_item=K, lobe="cosine", **path)

    calls = {"passes%d" % b: passes(b) for b in BINS}
    calls["gather"] = gather
    rays = {}
    for key, call in calls.items():                                         # the reference's ray count of a job; also the first launch
        ctr.zero_()
        call(ctr.data_ptr())
        torch.cuda.synchronize()
        assert int(ctr[0]) == n * K
        rays[key] = int(ctr[1])
    if len(set(rays.values())) != 1:
        raise SystemExit("%s: the contenders did not trace the same paths: %r" % (name, rays))
    # the slots at depth 0 do not depend on the bins (tinyrt.h, identity 2)
    p2, p4 = d_p[2].view(n, 4, 3), d_p[4].view(n, 8, 3)
    if not (torch.equal(p2[:, 0].contiguous().view(torch.int32), p4[:, 0].contiguous().view(torch.int32)) and
            torch.equal(p2[:, 2].contiguous().view(torch.int32), p4[:, 4].contiguous().view(torch.int32))):
        raise SystemExit("%s: the depth-0 slots of 2 and 4 bins differ" % name)
    share = {"direct": float(p4[:, [0, 4]].sum(dim=1).mean()), "indirect": float(p4[:, [1, 2, 3, 5, 6, 7]].sum(dim=1).mean()),
             "spent": float(d_spent.mean())}
    reps, windows = {}, {k: [] for k in calls}
    for key, call in calls.items():                                         # warm-up and the repetitions of a window
        call()
        torch.cuda.synchronize()
        once = GB.window(torch, call, 1)
        reps[key] = max(1, int(np.ceil(1000.0 * args.window_s / once)))
    for _ in range(args.rounds):
        for key, call in calls.items():
            windows[key].append(GB.window(torch, call, reps[key]))
    plans = {"passes%d" % b: scene.passes_plan(n, b) for b in BINS}
    plans["gather"] = scene.gather_plan(n)
    out = {"items": n, "paths_per_job": n * K, "reference_rays": rays["gather"],
           "mean_over_items_and_channels": {k: round(v, 6) for k, v in share.items()}}
    med = {}
    for key in calls:
        ms = sorted(windows[key])
        med[key] = ms[len(ms) // 2]
        out[key] = {"ms_per_job_median": round(med[key], 3), "ms_per_job_min": round(ms[0], 3), "ms_per_job_max": round(ms[-1], 3),
                    "spread": round((ms[-1] - ms[0]) / med[key], 4), "jobs_per_window": reps[key], "windows": len(ms),
                    "mpaths_per_s": round(n * K / med[key] / 1e3, 2), "reference_mrays_per_s": round(rays[key] / med[key] / 1e3, 2),
                    "plan": {k: plans[key][k] for k in PLAN_FIELDS}}
    for b in BINS:
        out["time_passes%d_over_gather" % b] = round(med["passes%d" % b] / med["gather"], 4)
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
    out = {"metric": "ms per job of n x K paths (device events around a window of jobs, median window)", "rounds": args.rounds,
           "window_s": args.window_s, "device": torch.cuda.get_device_name(0), "library": os.path.basename(trt._lib.LIB_PATH),
           "samples_per_item": K, "max_bounces": DEPTH, "seed": SEED, "source": "cosine", "lobe": "cosine", "items": "%d x %d floor surfels" % (SIDE, SIDE),
           "ratios": "time_passesB_over_gather = median ms of passes with B depth bins / median ms of gather, the same paths: above 1, the "
                     "passes query is slower; spread = (max - min) / median"}
    cornell = trt.scenes.cornell(SIDE, SIDE)
    grid = trt.scenes.sphere_grid(100000, SIDE, SIDE)
    for name, desc, items in (("cornell", cornell, cornell_floor(trt, cornell)), ("sphere_grid_100k", grid, grid_floor(grid))):
        out[name] = bench_scene(trt, torch, name, desc, items, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
