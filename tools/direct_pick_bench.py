#!/usr/bin/env python3
"""What choosing the emitter through an alias table (trt_direct_pick, trt_direct_mis_pick) costs on the device beside the uniform choice,
and what it buys where the emitters' powers differ.  Needs a GPU.

  python tools/direct_pick_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/direct_pick_bench.json]

Items, K, seed and protocol are tools/direct_bench.py's: 1024 x 1024 floor surfels with the axis up, K = 16, seed 5.  Four sets:
  cornell_one_lamp     the Cornell box with the lamp lowered to y = 99, its own table (E = 1) and the power table of it: both queries
                       choose record 0, so the extra draw and the two loads are the only difference - THE TIME OF THE DRAW
  sphere_grid_one_lamp the 100 k-sphere grid with direct_bench's virtual quad lamp (E = 1): the same, on the walk from global memory
  many_light_room      the lowered box with sixty sphere lights of radius 1 and 0.05 x the lamp's colour along three walls (E = 61, the
                       lamp 94 % of the power): THE GAIN, for trt_direct_pick against trt_direct and trt_direct_mis_pick against
                       trt_direct_mis (balance)
  sphere_grid_64_lamps the grid under 8 x 8 virtual quad lamps of one size whose colours, hence powers, span 1 : 1000 (no light is
                       geometry, so the weighted queries return the unweighted bytes and are left out)
Timing: each contender is warmed, then timed in windows of at least --window-s seconds of repeated calls between two device events on
the stream; the contenders alternate in one process, --rounds windows each; the figure is the median window, the spread (max - min) /
median.  Reported per set and contender: the time, rays per sample, the mean and the per-item sample variance of the red channel from
moment2, K / (K - 1) x (moment2 - radiance^2) averaged over the items; per set time_pick_over_uniform and the equal-time efficiency
(var_uniform x t_uniform) / (var_pick x t_pick), section 6.13's measure: above 1 the table reaches a given noise sooner, below 1 it does
not pay.  Prints one JSON line; --out also writes it to a file."""
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

from direct_bench import PLAN_KEYS, cornell, grid                            # the same items and tables as the direct-light bench  # noqa: E402
from gather_bench import SEED, SIDE, K, window                               # the same K, seed and window as the other query benches  # noqa: E402


def many_light_room(trt):
    """(scene, floor texels, the scene's own table of 61): the lowered box with 20 dim sphere lights on each of three walls."""
    desc = trt.scenes.cornell(2, 2)
    geos = list(desc["geometries"])
    kind, corner, u, v, material = geos[2]
    assert kind == "quad" and material == "light"
    geos[2] = (kind, (corner[0], 99.0, corner[2]), u, v, material)
    lamp = [m for m in desc["materials"] if m[0] == "light"][0]
    materials = list(desc["materials"]) + [("dim_light", lamp[1], tuple(0.05 * c for c in lamp[2]), 0.0)]
    for y in (20.0, 40.0, 60.0, 80.0):
        for a in (10.0, 30.0, 50.0, 70.0, 90.0):
            geos += [("sphere", (2.0, y, a), 1.0, "dim_light"), ("sphere", (98.0, y, a), 1.0, "dim_light"), ("sphere", (a, y, 98.0), 1.0, "dim_light")]
    scene = trt.world_from_description(dict(desc, materials=materials, geometries=geos))[0].get_bvh()
    kind, corner, u, v, _ = desc["geometries"][3]
    table = scene.emitters()
    assert len(table) == 61
    return scene, trt.bake.quad_texels(corner, u, v, SIDE, SIDE, flip=True), table


def grid_64_lamps(trt):
    """(scene, ground surfels, 64 virtual quad lamps) of the 100 k-sphere grid: direct_bench's lamp cut into 8 x 8 with gaps, colours
    10 x 1000^(-k / 63) in table order."""
    scene, items, one = grid(trt)
    corner, u, v = one["a"][0].astype(np.float64), one["b"][0].astype(np.float64), one["c"][0].astype(np.float64)
    lamps = []
    for k in range(64):
        i, j = k % 8, k // 8
        c = 10.0 * 1000.0 ** (-k / 63.0)
        lamps.append(trt.lights.quad(tuple(corner + u * (i / 8.0) + v * (j / 8.0)), tuple(u / 16.0), tuple(v / 16.0), (c, c, c)))
    return scene, items, trt.lights.table(*lamps)


def bench_items(trt, torch, scene, items, table, weighted, args):
    dev = torch.device("cuda:0")
    n = len(items)
    pick, total = trt.lights.pick_table(table)
    d_items = torch.from_numpy(items).to(dev)
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    d_pick = torch.from_numpy(pick.view(np.uint8).copy()).to(dev)
    keys = ("uniform", "pick") + (("mis_uniform", "mis_pick") if weighted else ())
    sums = {key: tuple(torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2)) for key in keys}
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)

    def direct_call(key, mis, with_pick):
        def call(counters=0):
            s, m = sums[key]
            table_arg = None if not with_pick else (d_pick.data_ptr() if mis is None else (d_pick.data_ptr(), total))
            scene.direct_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), s.data_ptr(), m.data_ptr(), d_counters_ptr=counters,
                                samples_per_item=K, seed=SEED, mis=mis, pick=table_arg)
        return call

    calls = {"uniform": direct_call("uniform", None, False), "pick": direct_call("pick", None, True)}
    plans = {"uniform": scene.direct_plan(n), "pick": scene.direct_plan(n, pick=True)}
    if weighted:
        calls.update(mis_uniform=direct_call("mis_uniform", "balance", False), mis_pick=direct_call("mis_pick", "balance", True))
        plans.update(mis_uniform=scene.direct_plan(n, mis="balance"), mis_pick=scene.direct_plan(n, mis="balance", pick=True))
    rays = {}
    for key, call in calls.items():                                         # the rays of a job; also the first launch
        ctr.zero_()
        call(ctr.data_ptr())
        torch.cuda.synchronize()
        assert int(ctr[0]) == n * K
        rays[key] = int(ctr[1])
    out = {"items": n, "emitters": len(table), "samples_per_job": n * K, "largest_prob": round(float(pick["prob"].max()), 5),
           "smallest_prob": float(pick["prob"].min())}
    stats = {}
    for key in calls:
        s, m = (t.view(n, 3)[:, 0].double() for t in sums[key])
        var = torch.clamp(m - s * s, min=0.0) * (K / (K - 1.0))
        stats[key] = {"mean_red": round(float(s.mean()), 5), "mean_sample_variance_red": float(var.mean()),
                      "largest_item_sample_variance_red": round(float(var.max()), 4)}
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
        out[key] = dict(stats[key], ms_per_job_median=round(med[key], 3), ms_per_job_min=round(ms[0], 3), ms_per_job_max=round(ms[-1], 3),
                        spread=round((ms[-1] - ms[0]) / med[key], 4), jobs_per_window=reps[key], windows=len(ms),
                        msamples_per_s=round(n * K / med[key] / 1e3, 2), rays=rays[key], rays_per_sample=round(rays[key] / (n * K), 4),
                        plan={k: q[k] for k in PLAN_KEYS})
    for tag, uniform, picked in (("pick", "uniform", "pick"),) + ((("mis_pick", "mis_uniform", "mis_pick"),) if weighted else ()):
        out["time_%s_over_%s" % (picked, uniform)] = round(med[picked] / med[uniform], 4)
        vu, vp = stats[uniform]["mean_sample_variance_red"], stats[picked]["mean_sample_variance_red"]
        if vp > 0.0:
            out["variance_%s_over_%s" % (uniform, picked)] = round(vu / vp, 3)
            eff = (vu * med[uniform]) / (vp * med[picked])
            out["equal_time_efficiency_%s_against_%s" % (picked, uniform)] = round(eff, 3)
            out["%s_pays" % tag] = bool(eff > 1.0)
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
           "ratios": "time_X_over_Y = median ms of X / median ms of Y; equal_time_efficiency_X_against_Y = (var_Y * t_Y) / (var_X * t_X): "
                     "above 1, X reaches a given noise sooner; spread = (max - min) / median",
           "shapes_timed": "the lock-step list from LDS (cornell_one_lamp), the 16-byte-node walk from global memory (both grid sets) and "
                           "whatever shape the many-light room's 79 primitives get (see its plan); the other shapes were run by the tests "
                           "only and were not timed"}
    scene, items, table = cornell(trt, 99.0)
    out["cornell_one_lamp"] = bench_items(trt, torch, scene, items, table, True, args)
    scene, items, table = grid(trt)
    out["sphere_grid_one_lamp"] = bench_items(trt, torch, scene, items, table, False, args)
    scene, items, table = many_light_room(trt)
    out["many_light_room"] = bench_items(trt, torch, scene, items, table, True, args)
    scene, items, table = grid_64_lamps(trt)
    out["sphere_grid_64_lamps"] = bench_items(trt, torch, scene, items, table, False, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
