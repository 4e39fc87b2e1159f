#!/usr/bin/env python3
"""What the probe projection and the K-aware probe query cost on the device.  Needs a GPU.

  python tools/project_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/project_bench.json]

Shapes (items x samples): 1 M x 16 - the surfels of tools/gather_bench.py as probes, where the projection folds a lane per item - and
64 x 256 and 64 x 16 384 - an 8 x 8 grid of probes in the Cornell box, a wave per item.  max_bounces 50, seed 5, bands 3.
  project   trt_project_samples_device over the records of trt_samples_device (sphere), beside
  fold      trt_fold_samples_device over the same colours (six chains an item where the projection has 27), and
  copy      a device-to-device copy of the record bytes the projection reads: the colours and the directions
            (Cornell, sphere domain, all three shapes)
  probe     trt_probe_device: a lane owns an item for its K samples, beside
  parallel  trt_probe_parallel_device with a record buffer for all items (one chunk): a lane owns a sample, 24 bytes per SAMPLE written,
            read again and projected
            (Cornell: all three shapes on the sphere, 1 M x 16 on the hemisphere too; the 100 k-sphere grid: 1 M x 16, both domains)
Before anything is timed the outputs are compared by bits (a NaN by NaN-ness): the parallel query's sums and counters with the probe
query's, and the projection of the samples' records with the same sums.  Timing is tools/samples_bench.py's: every contender is warmed,
then timed in windows of at least --window-s seconds of repeated calls between two device events; the contenders of a group alternate,
--rounds windows each, in one process; the figure is the median window, the spread (max - min) / median.  Prints one JSON line; --out
also writes it to a file."""
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

from gather_bench import surfels  # noqa: E402
from samples_bench import PLAN_FIELDS, counted, same_bits, timed  # noqa: E402

DEPTH, SEED, SIDE, BANDS = 50, 5, 1024, 3
PROBES = 64


def probe_grid():
    """An 8 x 8 grid of probes across the box (side 100) at half height: examples/bake_probes.py's."""
    g = ((np.arange(8) + 0.5) * (100.0 / 8)).astype(np.float32)
    items = np.zeros((PROBES, 6), np.float32)
    items[:, 0], items[:, 1], items[:, 2] = np.tile(g, 8), 50.0, np.repeat(g[::-1], 8)
    items[:, 4] = 1.0
    return items


def bench_shape(trt, torch, scene, items, k, domain, bg, args, alone):
    dev = torch.device("cuda:0")
    n = len(items)
    d_items = torch.from_numpy(items).to(dev)
    d_sh, d_sh2, d_sh3 = (torch.zeros(n * 27, dtype=torch.float32, device=dev) for _ in range(3))
    record_bytes = 24 * k * n
    d_rec = torch.zeros(record_bytes // 4, dtype=torch.float32, device=dev)
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)
    path = dict(samples_per_item=k, max_bounces=DEPTH, background=bg, seed=SEED)

    def probe(counters=0):
        scene.probe_device(d_items.data_ptr(), n, d_sh.data_ptr(), d_counters_ptr=counters, bands=BANDS, domain=domain, **path)

    def parallel(counters=0):
        scene.probe_parallel_device(d_items.data_ptr(), n, d_sh2.data_ptr(), d_rec.data_ptr(), record_bytes, d_counters_ptr=counters, bands=BANDS,
                                    domain=domain, **path)

    want, got = counted(torch, ctr, probe), counted(torch, ctr, parallel)
    if got != want or not same_bits(torch, d_sh2, d_sh):
        raise SystemExit("%d x %d, %s: the parallel probe query is not the probe query" % (n, k, domain))
    out = {"items": n, "samples_per_item": k, "domain": domain, "paths_per_job": n * k, "record_bytes": record_bytes}
    t = timed(torch, {"probe": probe, "parallel": parallel}, args)
    for key in t:
        t[key]["reference_rays"] = want[1]
        t[key]["mpaths_per_s"] = round(n * k / t[key]["ms_per_job_median"] / 1e3, 2)
    t["probe"]["plan"] = {f: v for f, v in scene.probe_plan(n, BANDS).items() if f in PLAN_FIELDS}
    t["parallel"]["plan"] = {f: v for f, v in scene.probe_parallel_plan(n, k).items() if f in PLAN_FIELDS}
    out.update(t)
    out["time_parallel_over_probe"] = round(t["parallel"]["ms_per_job_median"] / t["probe"]["ms_per_job_median"], 4)
    out["parallel_faster_beyond_the_spreads"] = bool(t["parallel"]["ms_per_job_max"] < t["probe"]["ms_per_job_min"])
    out["probe_faster_beyond_the_spreads"] = bool(t["probe"]["ms_per_job_max"] < t["parallel"]["ms_per_job_min"])
    if alone:
        # the projection alone over the records of the sample query, beside the six-chain fold of the colours and a copy of the bytes
        d_c, d_d = (torch.zeros(n * k * 3, dtype=torch.float32, device=dev) for _ in range(2))
        d_copy = torch.zeros(2 * n * k * 3, dtype=torch.float32, device=dev)
        d_s, d_m = torch.zeros(n * 3, dtype=torch.float32, device=dev), torch.zeros(n * 3, dtype=torch.float32, device=dev)
        scene.samples_device(d_items.data_ptr(), n, d_c.data_ptr(), d_d.data_ptr(), source=domain, **path)

        def project():
            trt.project_samples_device(d_c.data_ptr(), d_d.data_ptr(), n, k, d_sh3.data_ptr(), bands=BANDS, d_items_ptr=d_items.data_ptr())

        def fold():
            trt.fold_samples_device(d_c.data_ptr(), n, k, d_s.data_ptr(), d_m.data_ptr())

        def copy():
            d_copy[:n * k * 3].copy_(d_c)
            d_copy[n * k * 3:].copy_(d_d)

        project()
        torch.cuda.synchronize()
        if not same_bits(torch, d_sh3, d_sh):
            raise SystemExit("%d x %d, %s: the projection of the samples is not the probe query" % (n, k, domain))
        f = timed(torch, {"project": project, "fold": fold, "copy": copy}, args)
        f["project"]["gbytes_per_s_read"] = round(n * k * 24 / f["project"]["ms_per_job_median"] / 1e6, 1)
        f["fold"]["gbytes_per_s_read"] = round(n * k * 12 / f["fold"]["ms_per_job_median"] / 1e6, 1)
        f["copy"]["gbytes_per_s_read"] = round(n * k * 24 / f["copy"]["ms_per_job_median"] / 1e6, 1)
        out.update(f)
        out["regime"] = "wave per item" if k >= 64 and n <= 4096 else "lane per item"
        out["time_project_over_fold"] = round(f["project"]["ms_per_job_median"] / f["fold"]["ms_per_job_median"], 4)
        out["time_project_over_copy"] = round(f["project"]["ms_per_job_median"] / f["copy"]["ms_per_job_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_bench.json"))
    args = ap.parse_args()
    if args.rounds < 3 or args.window_s < 1.0:
        ap.error("at least 3 windows of at least 1 s per contender")
    import torch
    trt = importlib.import_module("tiny-raytracer_amd")
    trt._lib.check(trt.lib.trt_set_device(0))
    out = {"metric": "ms per job (device events around a window of jobs, median window)", "rounds": args.rounds, "window_s": args.window_s,
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(trt._lib.LIB_PATH), "bands": BANDS, "max_bounces": DEPTH, "seed": SEED,
           "ratios": "time_parallel_over_probe = median ms of trt_probe_parallel_device / median ms of trt_probe_device: below 1, the parallel "
                     "query is faster; spread = (max - min) / median"}
    n = SIDE * SIDE
    for name, desc in (("cornell", trt.scenes.cornell(SIDE, SIDE)), ("sphere_grid_100k", trt.scenes.sphere_grid(100000, SIDE, SIDE))):
        world, cam = trt.world_from_description(desc)
        scene = world.get_bvh()
        bg = tuple(desc["background"])
        items, n_surfels = surfels(trt, torch, scene, cam, n)
        res = {"surfels": n_surfels}
        for domain in ("sphere", "hemisphere"):
            res["1Mx16_%s" % domain] = bench_shape(trt, torch, scene, items, 16, domain, bg, args, alone=(name == "cornell" and domain == "sphere"))
            print("done", name, domain, file=sys.stderr, flush=True)
        if name == "cornell":
            for k in (256, 16384):
                res["64x%d_sphere" % k] = bench_shape(trt, torch, scene, probe_grid(), k, "sphere", bg, args, alone=True)
                print("done", name, k, file=sys.stderr, flush=True)
        out[name] = res
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
