#!/usr/bin/env python3
"""Throughput of the first-hit feature buffers (trt_render_aov_device) beside the unfused way to the same hits.  Needs a GPU.

  python tools/aov_bench.py [--reps 20] [--warmup 5] [--out profiles/aov_bench.json]

Workloads: Cornell at 2048 x 2048 and sphere_grid(100000) at 3840 x 2160, each at 1 and at 8 samples per pixel, seed 1.
 - fused: ONE trt_render_aov_device call with all six buffers wanted (ray generation, walk and fold in one kernel; 40 bytes written per
   pixel, whatever the sample count);
 - unfused: per sample, trt_primary_rays_device into a device buffer and trt_intersect_device on it (24 bytes written and read and 28
   bytes written per primary ray) - and that leaves the fold over the samples still to do, which is not timed.
Both are timed on device buffers with a pair of device events around EACH repetition, `reps` repetitions after `warmup` untimed ones; the
figure is primary rays (pixels x samples) per second from the median repetition, and the ratio fused / unfused.  Before timing, the two
ways are checked against each other at sample 0: the geometry buffer must equal the records' geometry.  Prints one JSON line; --out also
writes it to a file.  --compact-nodes 0 compiles the sphere grid without its 16-byte nodes (the register-slot kernel then runs).  TRT_LIB_PATH (tiny-raytracer_amd/_lib.py) selects another build of the library: its name and the launch plan of
every workload are recorded, so that two builds can be compared in one GPU visit."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.query_bench import time_case  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="image side scale (smaller images for a quick look; the stored figures use 1)")
    ap.add_argument("--only", default=None, help="run the workloads whose name contains this text")
    ap.add_argument("--compact-nodes", type=int, default=-1, help="trt_scene_options.compact_nodes of the sphere grid (0: no 16-byte nodes, "
                    "so the register-slot kernel for scenes in global memory runs; the stored figures use the default)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20 or args.warmup < 5:
        ap.error("at least 20 repetitions after 5 warm-ups")
    import torch
    trt = importlib.import_module("tiny-raytracer_amd")
    trt._lib.check(trt.lib.trt_set_device(0))
    dev = torch.device("cuda:0")
    k = args.scale
    workloads = [("cornell_2048x2048", trt.scenes.cornell(int(2048 * k), int(2048 * k))),
                 ("sphere_grid100000_3840x2160", trt.scenes.sphere_grid(100000, int(3840 * k), int(2160 * k)))]
    out = {"metric": "primary rays/s", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(trt._lib.LIB_PATH),
           "what": "whole-call device time (median of the repetitions): fused = one trt_render_aov_device with six buffers; unfused = per sample "
                   "trt_primary_rays_device + trt_intersect_device, the fold over the samples not included",
           "plans": {}, "cases": {}, "ratios": {}}
    for name, desc in workloads:
        if args.only and args.only not in name:
            continue
        world, cam = trt.world_from_description(desc)
        scene = world.get_bvh(compact_nodes=args.compact_nodes) if name.startswith("sphere_grid") and args.compact_nodes != -1 else world.get_bvh()
        w, h = cam.get_image_size()
        n = w * h
        plan = scene.aov_plan(n)
        out["plans"][name] = {f: plan[f] for f in ("scene_mode", "walk", "threads_per_workgroup", "kernel_waves_per_simd", "workgroups_per_cu",
                                                   "leaf_slots", "fallback", "rays_per_wave", "workgroups")}
        bufs = {ch: torch.empty(n * per * 4, dtype=torch.uint8, device=dev) for ch, (_, per) in trt.AOV_CHANNELS.items()}
        ptrs = {ch: t.data_ptr() for ch, t in bufs.items()}
        rays = torch.empty(n * 24, dtype=torch.uint8, device=dev)
        hits = torch.empty(n * 28, dtype=torch.uint8, device=dev)
        for spp in (1, 8):
            renderer = trt.Renderer(spp, 1, 50, False, desc["background"], seed=1)

            def fused():
                renderer.render_aov_device(cam, scene, ptrs)

            def unfused():
                for s in range(spp):
                    cam.primary_rays_device(s, spp, rays.data_ptr(), seed=1)
                    scene.intersect_device(rays.data_ptr(), n, hits.data_ptr())

            # the two ways see the same first hits at sample 0
            fused()
            cam.primary_rays_device(0, spp, rays.data_ptr(), seed=1)
            scene.intersect_device(rays.data_ptr(), n, hits.data_ptr())
            torch.cuda.synchronize()
            geometry = hits.view(torch.int32).reshape(n, 7)[:, 1]
            if not torch.equal(bufs["geometry"].view(torch.int32), geometry):
                raise SystemExit(f"{name}/spp{spp}: the geometry buffer differs from trt_intersect on the exported rays")
            for kind, call in (("fused", fused), ("unfused", unfused)):
                med, lo, hi = time_case(torch, call, args.reps, args.warmup)
                out["cases"][f"{name}/spp{spp}/{kind}"] = {"primary_rays": n * spp, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                                                          "ms_max": round(hi, 4), "rays_per_s": round(n * spp / (med * 1e-3), 1)}
            c = out["cases"]
            c[f"{name}/spp{spp}/fused"]["hit_share_sample0"] = round(float((geometry != -1).sum()) / n, 4)
            out["ratios"][f"{name}/spp{spp}/fused_over_unfused"] = round(c[f"{name}/spp{spp}/fused"]["rays_per_s"] / c[f"{name}/spp{spp}/unfused"]["rays_per_s"], 3)
        del scene, world, bufs, rays, hits
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
