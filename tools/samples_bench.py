#!/usr/bin/env python3
"""What the sample-parallel route costs on the device beside the folding queries.  Needs a GPU.

  python tools/samples_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/samples_bench.json]

Cornell and the 100 k-sphere grid with the surfels of tools/gather_bench.py (1 M items, K = 16, max_bounces 50, seed 5), and 64 probes in
the Cornell box with 256 and with 16 384 samples.  Contenders, the same paths each:
  gather    trt_gather_device(n, K), cosine                          a lane owns an item for its K samples; 24 bytes written per item
  pair      trt_samples_device(n, K, COSINE) + trt_fold_samples_device    a lane owns a sample; 12 bytes per SAMPLE written, read again and folded
  radiance  trt_radiance_device(n rays, K)                            the same items taken as rays; the first segment walked once per ray
  pair_rays trt_samples_device(n, K, RAYS) + trt_fold_samples_device      the first segment walked once per sample
  probe     trt_probe_device(64, K, sphere, bands 3)                  64 items: one wave
  samples   trt_samples_device(64, K, SPHERE) with directions          64 x K lanes; the projection (sh.project, numpy on the host) is NOT timed
  fold      trt_fold_samples_device alone, beside copy: a device-to-device copy of the same colour bytes
Before anything is timed the outputs are compared: the pair's sums with the folding query's by bits (a NaN by NaN-ness), the projection of
the samples with the probe's coefficients, and the reference's ray counts.  Timing: every contender is warmed, then timed in windows of at
least --window-s seconds of repeated calls between two device events; the contenders of a group alternate, --rounds windows each, in one
process; the figure is the median window, the spread (max - min) / median.  Prints one JSON line; --out also writes it to a file."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gather_bench import surfels, window  # noqa: E402

K, DEPTH, SEED, SIDE = 16, 50, 5, 1024
PROBES, PROBE_K = 64, (256, 16384)
PLAN_FIELDS = ("scene_mode", "walk", "threads_per_workgroup", "kernel_waves_per_simd", "workgroups_per_cu", "rays_per_wave", "waves", "wave_slots",
               "workgroups")


def same_bits(torch, a, b):
    a, b = a.view(-1), b.view(-1)
    return bool(torch.where(torch.isnan(b), torch.isnan(a), a.view(torch.int32) == b.view(torch.int32)).all())


def timed(torch, calls, args):
    """{name: {median, min, max, spread, jobs}} of contenders that alternate."""
    reps, windows = {}, {k: [] for k in calls}
    for key, call in calls.items():
        call()
        torch.cuda.synchronize()
        once = window(torch, call, 1)
        reps[key] = max(1, int(np.ceil(1000.0 * args.window_s / once)))
    for _ in range(args.rounds):
        for key, call in calls.items():
            windows[key].append(window(torch, call, reps[key]))
    out = {}
    for key in calls:
        ms = sorted(windows[key])
        med = ms[len(ms) // 2]
        out[key] = {"ms_per_job_median": round(med, 4), "ms_per_job_min": round(ms[0], 4), "ms_per_job_max": round(ms[-1], 4),
                    "spread": round((ms[-1] - ms[0]) / med, 4), "jobs_per_window": reps[key], "windows": len(ms)}
    return out


def counted(torch, ctr, call):
    ctr.zero_()
    call(ctr.data_ptr())
    torch.cuda.synchronize()
    return int(ctr[0]), int(ctr[1])


def bench_scene(trt, torch, name, desc, args):
    dev = torch.device("cuda:0")
    world, cam = trt.world_from_description(desc)
    scene = world.get_bvh()
    n = SIDE * SIDE
    items, n_surfels = surfels(trt, torch, scene, cam, n)
    d_items = torch.from_numpy(items).to(dev)
    d_s, d_m, d_s2, d_m2 = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(4))
    d_c = torch.zeros(n * K * 3, dtype=torch.float32, device=dev)
    d_copy = torch.zeros_like(d_c)
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)
    path = dict(max_bounces=DEPTH, background=tuple(desc["background"]), seed=SEED)

    def gather(counters=0):
        scene.gather_device(d_items.data_ptr(), n, d_s.data_ptr(), d_m.data_ptr(), d_counters_ptr=counters, samples_per_item=K, lobe="cosine", **path)

    def radiance(counters=0):
        scene.radiance_device(d_items.data_ptr(), n, d_s.data_ptr(), d_m.data_ptr(), d_counters_ptr=counters, samples_per_ray=K, **path)

    def fold():
        trt.fold_samples_device(d_c.data_ptr(), n, K, d_s2.data_ptr(), d_m2.data_ptr())

    def pair_of(source):
        def pair(counters=0):
            scene.samples_device(d_items.data_ptr(), n, d_c.data_ptr(), d_counters_ptr=counters, samples_per_item=K, source=source, **path)
            fold()
        return pair

    out = {"items": n, "surfels": n_surfels, "probes": n - n_surfels, "paths_per_job": n * K}
    for folding, source, key in ((gather, "cosine", "pair"), (radiance, "rays", "pair_rays")):
        pair = pair_of(source)
        want = counted(torch, ctr, folding)
        got = counted(torch, ctr, pair)
        if got != want or not same_bits(torch, d_s2, d_s) or not same_bits(torch, d_m2, d_m):
            raise SystemExit("%s: the fold of the %s samples is not the folding query" % (name, source))
        fname = folding.__name__
        t = timed(torch, {fname: folding, key: pair}, args)
        for k in t:
            t[k]["reference_rays"] = want[1]
            t[k]["mpaths_per_s"] = round(n * K / t[k]["ms_per_job_median"] / 1e3, 2)
        t[fname]["plan"] = {k: v for k, v in (scene.gather_plan(n) if source == "cosine" else scene.radiance_plan(n)).items() if k in PLAN_FIELDS}
        t[key]["plan"] = {k: v for k, v in scene.samples_plan(n, K).items() if k in PLAN_FIELDS}
        out.update(t)
        ratio = t[key]["ms_per_job_median"] / t[fname]["ms_per_job_median"]
        out["time_%s_over_%s" % (key, fname)] = round(ratio, 4)
        out["%s_faster_beyond_the_spreads" % key] = bool(t[key]["ms_per_job_max"] < t[fname]["ms_per_job_min"])
    # the fold alone, the records of the last pair resident, beside a copy of the same bytes
    t = timed(torch, {"fold": fold, "copy": lambda: d_copy.copy_(d_c)}, args)
    for k in t:
        t[k]["gbytes_per_s_read"] = round(n * K * 12 / t[k]["ms_per_job_median"] / 1e6, 1)
    out.update(t)
    out["time_fold_over_copy"] = round(t["fold"]["ms_per_job_median"] / t["copy"]["ms_per_job_median"], 4)
    return out


def bench_probes(trt, torch, desc, k, args):
    dev = torch.device("cuda:0")
    world, _ = trt.world_from_description(desc)
    scene = world.get_bvh()
    # an 8 x 8 grid of probes across the box (side 100) at half height: examples/bake_probes.py's
    g = ((np.arange(8) + 0.5) * (100.0 / 8)).astype(np.float32)
    items = np.zeros((PROBES, 6), np.float32)
    items[:, 0], items[:, 1], items[:, 2] = np.tile(g, 8), 50.0, np.repeat(g[::-1], 8)
    items[:, 4] = 1.0
    d_items = torch.from_numpy(items).to(dev)
    d_sh = torch.zeros(PROBES * 27, dtype=torch.float32, device=dev)
    d_c, d_d = (torch.zeros(PROBES * k * 3, dtype=torch.float32, device=dev) for _ in range(2))
    d_s, d_m, d_copy = torch.zeros(PROBES * 3, dtype=torch.float32, device=dev), torch.zeros(PROBES * 3, dtype=torch.float32, device=dev), torch.zeros_like(d_c)
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)
    path = dict(samples_per_item=k, max_bounces=DEPTH, background=tuple(desc["background"]), seed=SEED)

    def probe(counters=0):
        scene.probe_device(d_items.data_ptr(), PROBES, d_sh.data_ptr(), d_counters_ptr=counters, bands=3, domain="sphere", **path)

    def samples(counters=0):
        scene.samples_device(d_items.data_ptr(), PROBES, d_c.data_ptr(), d_d.data_ptr(), d_counters_ptr=counters, source="sphere", **path)

    want, got = counted(torch, ctr, probe), counted(torch, ctr, samples)
    sh = trt.sh.project(d_c.cpu().numpy().reshape(PROBES, k, 3), d_d.cpu().numpy().reshape(PROBES, k, 3), 3, points=items[:, 0:3])
    if got != want or not same_bits(torch, torch.from_numpy(sh).to(dev), d_sh):
        raise SystemExit("probes, K = %d: the projection of the samples is not the probe query" % k)
    out = {"items": PROBES, "samples_per_item": k, "paths_per_job": PROBES * k}
    t = timed(torch, {"probe": probe, "samples": samples}, args)
    for key in t:
        t[key]["reference_rays"] = want[1]
    t["probe"]["plan"] = {f: v for f, v in scene.probe_plan(PROBES, 3).items() if f in PLAN_FIELDS}
    t["samples"]["plan"] = {f: v for f, v in scene.samples_plan(PROBES, k).items() if f in PLAN_FIELDS}
    out.update(t)
    out["time_samples_over_probe"] = round(t["samples"]["ms_per_job_median"] / t["probe"]["ms_per_job_median"], 4)
    f = timed(torch, {"fold": lambda: trt.fold_samples_device(d_c.data_ptr(), PROBES, k, d_s.data_ptr(), d_m.data_ptr()),
                      "copy": lambda: d_copy.copy_(d_c)}, args)
    out["fold"], out["copy"] = f["fold"], f["copy"]
    out["time_fold_over_copy"] = round(f["fold"]["ms_per_job_median"] / f["copy"]["ms_per_job_median"], 4)
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
    out = {"metric": "ms per job (device events around a window of jobs, median window)", "rounds": args.rounds, "window_s": args.window_s,
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(trt._lib.LIB_PATH), "samples_per_item": K, "max_bounces": DEPTH,
           "seed": SEED, "width": SIDE, "height": SIDE,
           "ratios": "time_pair_over_gather = median ms of samples + fold / median ms of gather: below 1, the pair is faster; spread = (max - min) / median"}
    for name, desc in (("cornell", trt.scenes.cornell(SIDE, SIDE)), ("sphere_grid_100k", trt.scenes.sphere_grid(100000, SIDE, SIDE))):
        out[name] = bench_scene(trt, torch, name, desc, args)
    for k in PROBE_K:
        out["probes_64x%d" % k] = bench_probes(trt, torch, trt.scenes.cornell(SIDE, SIDE), k, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
