#!/usr/bin/env python3
"""What a gather query costs on the device, beside the only other route to the same estimate.  Needs a GPU.

  python tools/gather_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/gather_bench.json]

Cornell and the 100 k-sphere grid.  Items: the surfel list of tests/test_gpu_gather.py scaled up - the render's own rays for sample 0 at
1024 x 1024 (trt_primary_rays_device) through Scene.intersect; a ray that hits gives the surfel (hit point, normal), a ray that misses
stays as a probe; the axis of every third item is scaled by 0.25 and of the next by 3.  K = 16 samples per item, max_bounces 50, seed 5
(the budget of tools/radiance_bench.py), cosine lobe.  Contenders, n x K paths each:
  gather    trt_gather_device(n, K)                   24 bytes read per item, 24 written
  explicit  trt_radiance_device(n x K rays, K = 1)    the first rays already resident in HBM, 24 bytes read and 24 written per SAMPLE;
            the upload of the rays, the download of the samples and the fold on the host that this route also needs are NOT timed
  unfolded  trt_gather_device(n x K items, K = 1)     every item repeated K times: sample s of item i is item i * K + s with the same
            stream, so these are gather's own paths, drawn on the device, but launched as the explicit route is (n x K runs entries, no
            fold).  It separates what the draw costs (unfolded against explicit) from what the launch of n items with K samples each
            costs (gather against unfolded); its bytes must fold to gather's, and do before anything is timed
The explicit rays are drawn here by the same rule (Lambertian::scatter about the item's axis) with numpy, from a generator of numpy's:
the same distribution, not the same paths.  The reference's ray count of both jobs is in the line, so that the reader sees how equal the
work is.  Timing: every contender is warmed, then timed in windows of at least --window-s seconds of repeated calls between two device
events; the contenders alternate, --rounds windows each, in one process; the figure is the median window, and the spread of a contender is
(max - min) / median of its windows.  Prints one JSON line; --out also writes it to a file."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K, DEPTH, SEED, SIDE = 16, 50, 5, 1024
AXIS_SCALES = (1.0, 0.25, 3.0)


def window(torch, call, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def surfels(trt, torch, scene, cam, n):
    """float32 [n, 6]: see the module's text."""
    d_rays = torch.zeros(n * 6, dtype=torch.float32, device="cuda:0")
    cam.primary_rays_device(0, K, d_rays.data_ptr(), seed=SEED)
    torch.cuda.synchronize()
    rays = d_rays.cpu().numpy().reshape(n, 6)
    hits = scene.intersect(rays)
    hit = np.isfinite(hits["t"])
    items = rays.copy()
    items[hit, 0:3] = (rays[hit, 0:3] + hits["t"][hit, None] * rays[hit, 3:6]).astype(np.float32)
    items[hit, 3:6] = hits["normal"][hit]
    items[:, 3:6] *= np.array(AXIS_SCALES, np.float32)[np.arange(n) % 3][:, None]
    return np.ascontiguousarray(items), int(hit.sum())


def cosine_rays(items, k, seed):
    """float32 [n * k, 6]: Ray::new(point, axis + unit vector), the unit vector uniform on the sphere; numpy's generator, float64."""
    g = np.random.default_rng(seed)
    n = len(items)
    out = np.empty((n, k, 6), np.float32)
    for a in range(0, n, 65536):                                            # in pieces: the float64 temporaries of 16 M rays are large
        part = items[a:a + 65536]
        u = g.standard_normal((len(part), k, 3))
        u /= np.linalg.norm(u, axis=2, keepdims=True)
        d = part[:, None, 3:6].astype(np.float64) + u
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        out[a:a + 65536, :, 0:3] = part[:, None, 0:3]
        out[a:a + 65536, :, 3:6] = d
    return out.reshape(n * k, 6)


def bench_scene(trt, torch, name, desc, args):
    dev = torch.device("cuda:0")
    world, cam = trt.world_from_description(desc)
    scene = world.get_bvh()
    n = SIDE * SIDE
    bg = tuple(desc["background"])
    items, n_surfels = surfels(trt, torch, scene, cam, n)
    d_items = torch.from_numpy(items).to(dev)
    d_rays = torch.from_numpy(cosine_rays(items, K, SEED)).to(dev)
    d_s, d_m = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2))
    d_s1, d_m1 = (torch.zeros(n * K * 3, dtype=torch.float32, device=dev) for _ in range(2))
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)
    path = dict(max_bounces=DEPTH, background=bg, seed=SEED)

    def gather(counters=0):
        scene.gather_device(d_items.data_ptr(), n, d_s.data_ptr(), d_m.data_ptr(), d_counters_ptr=counters, samples_per_item=K, lobe="cosine", **path)

    def explicit(counters=0):
        scene.radiance_device(d_rays.data_ptr(), n * K, d_s1.data_ptr(), d_m1.data_ptr(), d_counters_ptr=counters, samples_per_ray=1, **path)

    d_items_k = d_items.view(n, 6).repeat_interleave(K, dim=0).contiguous()
    d_s2, d_m2 = (torch.zeros(n * K * 3, dtype=torch.float32, device=dev) for _ in range(2))

    def unfolded(counters=0):
        scene.gather_device(d_items_k.data_ptr(), n * K, d_s2.data_ptr(), d_m2.data_ptr(), d_counters_ptr=counters, samples_per_item=1, lobe="cosine",
                            **path)

    calls = {"gather": gather, "explicit": explicit, "unfolded": unfolded}
    rays = {}
    for key, call in calls.items():                                         # the reference's ray count of a job; also the first launch
        ctr.zero_()
        call(ctr.data_ptr())
        torch.cuda.synchronize()
        assert int(ctr[0]) == n * K
        rays[key] = int(ctr[1])
    # unfolded holds gather's samples: folded in gather's order (f32, one operation per operator) they are gather's bytes
    inv = torch.tensor(1.0 / K, dtype=torch.float32, device=dev)
    acc = torch.zeros(n, 3, dtype=torch.float32, device=dev)
    for s in range(K):
        acc = acc + d_s2.view(n, K, 3)[:, s, :] * inv
    if not torch.equal(acc.view(torch.int32), d_s.view(n, 3).view(torch.int32)) or rays["unfolded"] != rays["gather"]:
        raise SystemExit("%s: the unfolded gather does not fold to the gather" % name)
    # the two routes estimate the same thing: the mean over all items agrees to sampling noise
    mean_g = d_s.view(n, 3).double().mean(dim=0)
    mean_e = (d_s1.view(n, K, 3).double().sum(dim=1) / K).mean(dim=0)
    reps, windows = {}, {k: [] for k in calls}
    for key, call in calls.items():                                         # warm-up and the repetitions of a window
        call()
        torch.cuda.synchronize()
        once = window(torch, call, 1)
        reps[key] = max(1, int(np.ceil(1000.0 * args.window_s / once)))
    for _ in range(args.rounds):
        for key, call in calls.items():
            windows[key].append(window(torch, call, reps[key]))
    plans = {"gather": scene.gather_plan(n), "explicit": scene.radiance_plan(n * K), "unfolded": scene.gather_plan(n * K)}
    out = {"items": n, "surfels": n_surfels, "probes": n - n_surfels, "paths_per_job": n * K,
           "mean_radiance": {"gather": [round(float(x), 5) for x in mean_g], "explicit": [round(float(x), 5) for x in mean_e]}}
    med, spread = {}, {}
    for key in calls:
        ms = sorted(windows[key])
        med[key] = ms[len(ms) // 2]
        spread[key] = (ms[-1] - ms[0]) / med[key]
        q = plans[key]
        out[key] = {"ms_per_job_median": round(med[key], 3), "ms_per_job_min": round(ms[0], 3), "ms_per_job_max": round(ms[-1], 3),
                    "spread": round(spread[key], 4), "jobs_per_window": reps[key], "windows": len(ms),
                    "mpaths_per_s": round(n * K / med[key] / 1e3, 2), "reference_rays": rays[key],
                    "reference_mrays_per_s": round(rays[key] / med[key] / 1e3, 2),
                    "plan": {k: q[k] for k in ("scene_mode", "walk", "threads_per_workgroup", "kernel_waves_per_simd", "workgroups_per_cu",
                                               "rays_per_wave", "waves", "wave_slots", "workgroups")}}
    out["time_gather_over_explicit"] = round(med["gather"] / med["explicit"], 4)
    out["time_unfolded_over_explicit"] = round(med["unfolded"] / med["explicit"], 4)
    out["time_gather_over_unfolded"] = round(med["gather"] / med["unfolded"], 4)
    out["rays_gather_over_explicit"] = round(rays["gather"] / rays["explicit"], 4)
    out["gather_not_slower_beyond_the_explicit_spread"] = bool(med["gather"] <= med["explicit"] * (1.0 + spread["explicit"]))
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
           "samples_per_item": K, "max_bounces": DEPTH, "seed": SEED, "lobe": "cosine", "width": SIDE, "height": SIDE,
           "ratios": "time_gather_over_explicit = median ms of gather / median ms of explicit: below 1, gather is faster; spread = (max - min) / median"}
    for name, desc in (("cornell", trt.scenes.cornell(SIDE, SIDE)), ("sphere_grid_100k", trt.scenes.sphere_grid(100000, SIDE, SIDE))):
        out[name] = bench_scene(trt, torch, name, desc, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
