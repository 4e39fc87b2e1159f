#!/usr/bin/env python3
"""Throughput of the ray queries (trt_intersect_device / trt_occluded_device) on workloads of the size users run.  Needs a GPU.

  python tools/query_bench.py [--reps 20] [--warmup 5] [--bench-line FILE] [--out profiles/query_bench.json]

Rays: the pinhole camera rays through the pixel centres of Cornell at 2048 x 2048 and of sphere_grid(100000) at 3840 x 2160, each in image
order (row-major) and in a fixed random permutation; closest hit and occlusion, both with t_max = NULL (+inf).  Every case is timed on
device buffers with a pair of device events around EACH repetition, `reps` repetitions after `warmup` untimed ones; the figure is rays per
second from the median repetition.  These are whole-call device times (launch to last store, the 24-byte ray read and the 28- / 1-byte
answer written included), not a share of any peak.  Prints one JSON line; --out also writes it to a file.  --bench-line: a file holding
bench.py's JSON line of the same build and GPU visit, recorded under "render_headline" for orientation only (a rendered ray includes
ray generation and shading: the two are not a ratio to pass or fail)."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def camera_rays(torch, pod, device):
    """float32 [h * w, 6], row-major: origin = the camera position, direction towards the centre of pixel (x, y) on the viewport
    (camera.rs:58-66 with the pixel centre in place of the random offset and no defocus), normalised."""
    w, h = pod.width, pod.height
    f = lambda v: torch.tensor(v.tolist(), dtype=torch.float32, device=device)
    pos, ul, hor, ver = f(pod.position), f(pod.viewport_upper_left), f(pod.horizontal), f(pod.vertical)
    u = (torch.arange(w, dtype=torch.float32, device=device) + 0.5) / float(w - 1)
    v = (torch.arange(h, dtype=torch.float32, device=device) + 0.5) / float(h - 1)
    target = ul[None, None, :] + u[None, :, None] * hor[None, None, :] - v[:, None, None] * ver[None, None, :]
    d = target - pos[None, None, :]
    d = d / d.norm(dim=2, keepdim=True)
    rays = torch.cat([pos.expand(h, w, 3), d], dim=2).reshape(h * w, 6).contiguous()
    return rays


def time_case(torch, call, reps, warmup):
    for _ in range(warmup):
        call()
    pairs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="image side scale (smaller images for a quick look; the stored figures use 1)")
    ap.add_argument("--bench-line", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20 or args.warmup < 5:
        ap.error("at least 20 repetitions after 5 warm-ups")
    import torch
    trt = importlib.import_module("tiny-raytracer_amd")
    trt._lib.check(trt.lib.trt_set_device(0))
    dev = torch.device("cuda:0")
    s = args.scale
    workloads = [("cornell_2048x2048", trt.scenes.cornell(int(2048 * s), int(2048 * s))),
                 ("sphere_grid100000_3840x2160", trt.scenes.sphere_grid(100000, int(3840 * s), int(2160 * s)))]
    out = {"metric": "rays/s", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "what": "whole-call device time of trt_intersect_device / trt_occluded_device (median of the repetitions), t_max = NULL; not a share of peak",
           "cases": {}, "ratios": {}}
    for name, desc in workloads:
        world, cam = trt.world_from_description(desc)
        scene = world.get_bvh()
        image = camera_rays(torch, cam.pod, dev)
        n = image.shape[0]
        g = torch.Generator(device="cpu")
        g.manual_seed(12345)
        perm = torch.randperm(n, generator=g).to(dev)
        orders = {"image_order": image, "permuted": image[perm].contiguous()}
        hits = torch.empty(n * 28, dtype=torch.uint8, device=dev)
        occ = torch.empty(n, dtype=torch.uint8, device=dev)
        for order, rays in orders.items():
            kinds = {"closest_hit": lambda r=rays: scene.intersect_device(r.data_ptr(), n, hits.data_ptr()),
                     "occluded": lambda r=rays: scene.occluded_device(r.data_ptr(), n, occ.data_ptr())}
            for kind, call in kinds.items():
                med, lo, hi = time_case(torch, call, args.reps, args.warmup)
                out["cases"][f"{name}/{order}/{kind}"] = {"rays": n, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                                                         "rays_per_s": round(n / (med * 1e-3), 1)}
            # the two kinds answered the same rays: the flags are the records' hit?
            geometry = hits.view(torch.int32).reshape(n, 7)[:, 1]
            n_hit, n_occ = int((geometry != -1).sum()), int(occ.sum())
            if n_hit != n_occ:
                raise SystemExit(f"{name}/{order}: {n_hit} hits but {n_occ} occluded rays")
            out["cases"][f"{name}/{order}/closest_hit"]["hit_share"] = round(n_hit / n, 4)
            c = out["cases"]
            out["ratios"][f"{name}/{order}/occluded_over_closest_hit"] = round(c[f"{name}/{order}/occluded"]["rays_per_s"] / c[f"{name}/{order}/closest_hit"]["rays_per_s"], 3)
        for kind in ("closest_hit", "occluded"):
            c = out["cases"]
            out["ratios"][f"{name}/{kind}/permuted_over_image_order"] = round(c[f"{name}/permuted/{kind}"]["rays_per_s"] / c[f"{name}/image_order/{kind}"]["rays_per_s"], 3)
        del scene, world, image, perm, orders, hits, occ
    if args.bench_line:
        with open(args.bench_line) as f:
            lines = [l for l in f.read().splitlines() if l.strip().startswith("{")]
        b = json.loads(lines[-1])
        out["render_headline"] = {k: b.get(k) for k in ("metric", "value", "scene", "width", "height", "gpus") if k in b}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
