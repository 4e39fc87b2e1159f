#!/usr/bin/env python3
"""What a probe query costs on the device beside a gather query of the same items.  Needs a GPU.

  python tools/probe_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/probe_bench.json]

tools/gather_bench.py's method and items: Cornell and the 100 k-sphere grid, 1 M surfels (the render's own rays at 1024 x 1024 turned into
surfels where they hit), K = 16 samples per item, max_bounces 50, seed 5.  Contenders, n x K paths each:
  probe3    trt_probe_device(n, K), bands 3, sphere     24 bytes read per item, 108 written; the 9-coefficient kernels
  probe2    trt_probe_device(n, K), bands 2, sphere     24 bytes read per item, 48 written; the 4-coefficient kernels
  probe3h   trt_probe_device(n, K), bands 3, hemisphere  the same kernels; the first rays leave the surfel on the side of its axis, as the
            gather's do, so the paths are of the gather's kind: it separates what the kernel costs from what the whole sphere's paths cost
  gather    trt_gather_device(n, K), cosine lobe        24 bytes read per item, 24 written (radiance and second moments); the same launch
            shape, the gather kernels' own launch bound
The paths differ - a probe draws over the whole sphere, a gather about the axis - so the reference's ray count of every job is in the line
and the ratios are given per job and per reference ray.  Timing: every contender is warmed, then timed in windows of at least --window-s
seconds of repeated calls between two device events; the contenders alternate, --rounds windows each, in one process; the figure is the
median window, and the spread of a contender is (max - min) / median of its windows.  Prints one JSON line; --out also writes it to a
file."""
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


def bench_scene(trt, torch, name, desc, args):
    dev = torch.device("cuda:0")
    world, cam = trt.world_from_description(desc)
    scene = world.get_bvh()
    n = SIDE * SIDE
    bg = tuple(desc["background"])
    items, n_surfels = GB.surfels(trt, torch, scene, cam, n)
    d_items = torch.from_numpy(items).to(dev)
    d_sh9 = torch.zeros(n * 27, dtype=torch.float32, device=dev)
    d_sh9h = torch.zeros(n * 27, dtype=torch.float32, device=dev)
    d_sh4 = torch.zeros(n * 12, dtype=torch.float32, device=dev)
    d_s, d_m = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2))
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)
    path = dict(max_bounces=DEPTH, background=bg, seed=SEED)

    def probe3(counters=0):
        scene.probe_device(d_items.data_ptr(), n, d_sh9.data_ptr(), d_counters_ptr=counters, samples_per_item=K, bands=3, domain="sphere", **path)

    def probe3h(counters=0):
        scene.probe_device(d_items.data_ptr(), n, d_sh9h.data_ptr(), d_counters_ptr=counters, samples_per_item=K, bands=3, domain="hemisphere", **path)

    def probe2(counters=0):
        scene.probe_device(d_items.data_ptr(), n, d_sh4.data_ptr(), d_counters_ptr=counters, samples_per_item=K, bands=2, domain="sphere", **path)

    def gather(counters=0):
        scene.gather_device(d_items.data_ptr(), n, d_s.data_ptr(), d_m.data_ptr(), d_counters_ptr=counters, samples_per_item=K, lobe="cosine", **path)

    calls = {"probe3": probe3, "probe2": probe2, "probe3h": probe3h, "gather": gather}
    rays = {}
    for key, call in calls.items():                                         # the reference's ray count of a job; also the first launch
        ctr.zero_()
        call(ctr.data_ptr())
        torch.cuda.synchronize()
        assert int(ctr[0]) == n * K
        rays[key] = int(ctr[1])
    # the two probes trace the same paths, and the leading coefficients do not depend on the bands
    if rays["probe2"] != rays["probe3"] or not torch.equal(d_sh9.view(n, 9, 3)[:, :4, :].contiguous().view(torch.int32), d_sh4.view(n, 4, 3).view(torch.int32)):
        raise SystemExit("%s: bands 2 is not the head of bands 3" % name)
    reps, windows = {}, {k: [] for k in calls}
    for key, call in calls.items():                                         # warm-up and the repetitions of a window
        call()
        torch.cuda.synchronize()
        once = GB.window(torch, call, 1)
        reps[key] = max(1, int(np.ceil(1000.0 * args.window_s / once)))
    for _ in range(args.rounds):
        for key, call in calls.items():
            windows[key].append(GB.window(torch, call, reps[key]))
    plans = {"probe3": scene.probe_plan(n, 3), "probe2": scene.probe_plan(n, 2), "probe3h": scene.probe_plan(n, 3), "gather": scene.gather_plan(n)}
    out = {"items": n, "surfels": n_surfels, "probes": n - n_surfels, "paths_per_job": n * K}
    med, spread = {}, {}
    for key in calls:
        ms = sorted(windows[key])
        med[key] = ms[len(ms) // 2]
        spread[key] = (ms[-1] - ms[0]) / med[key]
        out[key] = {"ms_per_job_median": round(med[key], 3), "ms_per_job_min": round(ms[0], 3), "ms_per_job_max": round(ms[-1], 3),
                    "spread": round(spread[key], 4), "jobs_per_window": reps[key], "windows": len(ms),
                    "mpaths_per_s": round(n * K / med[key] / 1e3, 2), "reference_rays": rays[key],
                    "reference_mrays_per_s": round(rays[key] / med[key] / 1e3, 2), "plan": {k: plans[key][k] for k in PLAN_FIELDS}}
    for key in ("probe3", "probe2", "probe3h"):
        out["time_%s_over_gather" % key] = round(med[key] / med["gather"], 4)
        out["rays_%s_over_gather" % key] = round(rays[key] / rays["gather"], 4)
        out["time_per_ray_%s_over_gather" % key] = round((med[key] / rays[key]) / (med["gather"] / rays["gather"]), 4)
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
           "samples_per_item": K, "max_bounces": DEPTH, "seed": SEED, "domain": "sphere (probe3, probe2), hemisphere (probe3h)", "lobe": "cosine", "width": SIDE, "height": SIDE,
           "ratios": "time_probe3_over_gather = median ms of probe3 / median ms of gather: above 1, the probe is slower; time_per_ray_* divides "
                     "each by the reference's ray count of its job first; spread = (max - min) / median"}
    for name, desc in (("cornell", trt.scenes.cornell(SIDE, SIDE)), ("sphere_grid_100k", trt.scenes.sphere_grid(100000, SIDE, SIDE))):
        out[name] = bench_scene(trt, torch, name, desc, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
