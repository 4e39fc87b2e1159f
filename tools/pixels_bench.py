#!/usr/bin/env python3
"""What the sparse render and the selection cost on the device.  Needs a GPU.

  python tools/pixels_bench.py [--reps 20] [--warmup 5] [--out profiles/pixels_bench.json]

Cornell at 1024 x 1024, 64 spp, max_bounces 50, seed 5.
 1. trt_render_pixels_device over ALL pixels (listed row-major, and listed 8 x 8 tile by tile) beside trt_render_moments_device of the
    same frame: the same samples traced by the sparse kernel (a lane owns a pixel, folds in registers) and by the streamed kernels
    (samples as work items, radiance records through HBM, a fold pass).  The two frames and second moments must be equal bit for bit:
    checked before timing.
 2. Lists of 50 %, 10 % and 1 % of the pixels, once as whole 8 x 8 tiles chosen at random (listed tile by tile) and once scattered
    (single pixels chosen at random, listed ascending), as time per traced sample relative to the full render's:
    (t_list / entries) / (t_full / pixels).  Below the share 1 / that ratio, refining sparsely beats tracing the whole frame again.
 3. trt_select_pixels_device over the frame (all pixels as candidates) at a tolerance that keeps about half.
Timing: a pair of device events around EACH call, `reps` repetitions after `warmup` untimed ones, the median (tools/query_bench.py
time_case).  Prints one JSON line; --out also writes it to a file."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.query_bench import time_case  # noqa: E402


def tile_major(side, tiles):
    """The pixels of the given 8 x 8 tiles (indices into the tiles_x x tiles_y grid), tile by tile, row-major within a tile."""
    tiles_x = side // 8
    ty, tx = np.divmod(np.asarray(tiles, np.int64), tiles_x)
    dy, dx = np.divmod(np.arange(64, dtype=np.int64), 8)
    y = ty[:, None] * 8 + dy[None, :]
    x = tx[:, None] * 8 + dx[None, :]
    return (y * side + x).reshape(-1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="image side scale (smaller images for a quick look; the stored figures use 1)")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20 or args.warmup < 5:
        ap.error("at least 20 repetitions after 5 warm-ups")
    import torch
    trt = importlib.import_module("tiny-raytracer_amd")
    trt._lib.check(trt.lib.trt_set_device(0))
    dev = torch.device("cuda:0")
    side = int(1024 * args.scale) // 8 * 8
    desc = trt.scenes.cornell(side, side)
    world, cam = trt.world_from_description(desc)
    scene = world.get_bvh()
    n = side * side
    r = trt.Renderer(args.spp, 1, 50, False, desc["background"], seed=5)
    d_s, d_m = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2))
    d_s2, d_m2 = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2))
    rng = np.random.default_rng(1)
    n_tiles = n // 64
    lists = {"all_row_major": np.arange(n, dtype=np.uint32), "all_tile_major": tile_major(side, np.arange(n_tiles))}
    for share in (0.5, 0.1, 0.01):
        k_tiles = max(1, int(round(n_tiles * share)))
        lists["tiles_%g" % share] = tile_major(side, np.sort(rng.permutation(n_tiles)[:k_tiles]))
        lists["scattered_%g" % share] = np.sort(rng.permutation(n)[:k_tiles * 64]).astype(np.uint32)
    d_lists = {k: torch.from_numpy(v.astype(np.int64)).to(torch.int32).to(dev) for k, v in lists.items()}

    def full():
        r.render_moments_device(cam, scene, d_s.data_ptr(), d_m.data_ptr())

    def sparse(key):
        t = d_lists[key]
        r.render_pixels_device(cam, scene, t.data_ptr(), t.numel(), d_s2.data_ptr(), d_m2.data_ptr())

    full()
    for key in ("all_row_major", "all_tile_major"):
        d_s2.zero_()
        d_m2.zero_()
        sparse(key)
        torch.cuda.synchronize()
        if not (torch.equal(d_s.view(torch.int32), d_s2.view(torch.int32)) and torch.equal(d_m.view(torch.int32), d_m2.view(torch.int32))):
            raise SystemExit("the sparse render of all pixels (%s) differs from trt_render_moments_device" % key)
    plan = scene.pixels_plan(n)
    out = {"metric": "ms per call (device events, median)", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(trt._lib.LIB_PATH), "scene": "cornell", "width": side, "height": side, "spp": args.spp, "max_bounces": 50,
           "plan": {k: plan[k] for k in ("walk", "threads_per_workgroup", "kernel_waves_per_simd", "workgroups_per_cu", "rays_per_wave", "workgroups")}}
    med, lo, hi = time_case(torch, full, args.reps, args.warmup)
    out["render_moments_device"] = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
    per_sample_full = med / n
    for key in lists:
        med, lo, hi = time_case(torch, lambda: sparse(key), args.reps, args.warmup)
        entries = len(lists[key])
        ratio = (med / entries) / per_sample_full
        out["pixels_" + key] = {"entries": entries, "share": round(entries / n, 4), "ms_median": round(med, 4), "ms_min": round(lo, 4),
                                "ms_max": round(hi, 4), "per_sample_over_full": round(ratio, 4), "break_even_share": round(min(1.0, 1.0 / ratio), 4)}
    out["sparse_all_over_moments"] = round(out["pixels_all_row_major"]["ms_median"] / out["render_moments_device"]["ms_median"], 4)

    # selection over the frame, at the relative tolerance that keeps about half of the pixels
    d_sel = torch.zeros(n, dtype=torch.int32, device=dev)
    d_count = torch.zeros(1, dtype=torch.int32, device=dev)
    need = trt.select_scratch_bytes(n)
    scratch = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    s, m = d_s.cpu().numpy().reshape(-1, 3), d_m.cpu().numpy().reshape(-1, 3)
    d = np.maximum(m - s * s, 0).sum(axis=1) / np.float32(args.spp - 1)
    rel = np.sqrt(d) / np.maximum(s.sum(axis=1), 1e-20)
    rel_tol = float(np.median(rel))

    def select():
        trt.select_pixels_device(d_s.data_ptr(), d_m.data_ptr(), n, args.spp, args.spp, n, rel_tol, 0.0, d_sel.data_ptr(), d_count.data_ptr(),
                                 scratch.data_ptr(), need)

    select()
    torch.cuda.synchronize()
    med, lo, hi = time_case(torch, select, args.reps, args.warmup)
    out["select_pixels_device"] = {"candidates": n, "kept_share": round(int(d_count.cpu()[0]) / n, 4), "rel_tol": round(rel_tol, 6),
                                   "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
