#!/usr/bin/env python3
"""What a weighted direct-light query (trt_direct_mis) costs on the device beside the plain one and a one-bounce gather of the same items,
and what the weights buy.  Needs a GPU.

  python tools/direct_mis_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/direct_mis_bench.json]

Items, tables, K, seed and protocol are tools/direct_bench.py's and tools/nee_mis_bench.py's: 1024 x 1024 floor surfels with the axis up
over the floor of the Cornell box with the lamp lowered to y = 99 and over the 100 k-sphere grid's ground, K = 16, seed 5; the box's own
lamp, and for the grid, which has no light, direct_bench's virtual quad lamp (there trt_direct_mis returns trt_direct's bytes - a virtual
emitter's wl is 1 and no lobe ray finds a light - so the extra time is the lobe walk alone).  A third set of items is a bake of all five
room quads of the lowered box (floor, ceiling, both side walls, the back wall; the box has no front wall), 458 x 458 texels each with the
axis into the room: the ceiling and the top rows of the walls lie beside the lamp.  Contenders, n x K samples each, in one process:
  mis_balance, mis_power   trt_direct_mis_device(n, K, table) with either heuristic
  direct                   trt_direct_device, the same call unweighted
  gather1                  trt_gather_device(n, K, cosine, max_bounces = 1, black background): the lobe ray's walk alone
and on the all-surfaces bake besides
  indirect                 trt_nee_mis_device(source_is_diffuse = 1, BALANCE, max_bounces = 5) with seed + 1: the other half of a bake
  gather                   trt_gather_device(n, K, cosine, max_bounces = 5, black background): the whole bake found by chance
Timing: each contender is warmed, then timed in windows of at least --window-s seconds of repeated calls between two device events; the
contenders alternate, --rounds windows each; the figure is the median window.

Reported per item set and contender: the time, rays per sample, the per-item sample variance of the red channel from moment2,
K / (K - 1) x (moment2 - radiance^2) averaged over the items, and the mean.  Per item set: the time of the weighted query over the sum of
trt_direct's and the one-bounce gather's (the expectation: at most 1 - it walks exactly their rays and saves a launch and an item load),
and the equal-time efficiency against trt_direct, (var_direct x t_direct) / (var_mis x t_mis).  For the bake trio the times of the two
halves add and, the halves being on independent streams, so do their variances; efficiency is against the gather.  Prints one JSON line;
--out also writes it to a file."""
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

BAKE_SIDE = 458                                                              # 5 x 458^2 = 1 048 820 texels: the floor set's size
BLACK = (0.0, 0.0, 0.0)


def room_texels(trt):
    """(scene, items, table) of the lowered box: BAKE_SIDE^2 texels over each of its five room quads, the axis into the room."""
    scene, _, table = cornell(trt, 99.0)
    desc = trt.scenes.cornell(2, 2)
    out = []
    for g in (3, 4, 0, 1, 5):                                               # floor, ceiling, the two side walls, the back wall
        kind, corner, u, v, _ = desc["geometries"][g]
        assert kind == "quad"
        normal = np.cross(np.asarray(u, np.float64), np.asarray(v, np.float64))
        inward = np.dot(normal, np.array([50.0, 50.0, 50.0]) - np.asarray(corner, np.float64)) > 0.0
        out.append(trt.bake.quad_texels(corner, u, v, BAKE_SIDE, BAKE_SIDE, flip=not inward))
    return scene, np.ascontiguousarray(np.concatenate(out)), table


def bench_items(trt, torch, scene, items, table, bake, args):
    dev = torch.device("cuda:0")
    n = len(items)
    d_items = torch.from_numpy(items).to(dev)
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    keys = ("mis_balance", "mis_power", "direct", "gather1") + (("indirect", "gather") if bake else ())
    sums = {key: tuple(torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2)) for key in keys}
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)

    def direct_call(key, mis):
        def call(counters=0):
            s, m = sums[key]
            scene.direct_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), s.data_ptr(), m.data_ptr(), d_counters_ptr=counters,
                                samples_per_item=K, seed=SEED, mis=mis)
        return call

    def gather_call(key, bounces):
        def call(counters=0):
            s, m = sums[key]
            scene.gather_device(d_items.data_ptr(), n, s.data_ptr(), m.data_ptr(), d_counters_ptr=counters, samples_per_item=K, lobe="cosine",
                                max_bounces=bounces, background=BLACK, seed=SEED)
        return call

    def indirect(counters=0):
        s, m = sums["indirect"]
        scene.nee_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), s.data_ptr(), m.data_ptr(), d_counters_ptr=counters,
                         samples_per_item=K, source="cosine", source_is_diffuse=True, mis="balance", max_bounces=5, background=BLACK, seed=SEED + 1)

    calls = {"mis_balance": direct_call("mis_balance", "balance"), "mis_power": direct_call("mis_power", "power"),
             "direct": direct_call("direct", None), "gather1": gather_call("gather1", 1)}
    plans = {"mis_balance": scene.direct_plan(n, mis="balance"), "mis_power": scene.direct_plan(n, mis="power"), "direct": scene.direct_plan(n),
             "gather1": scene.gather_plan(n)}
    if bake:
        calls.update(indirect=indirect, gather=gather_call("gather", 5))
        plans.update(indirect=scene.nee_plan(n, mis="balance"), gather=scene.gather_plan(n))
    rays = {}
    for key, call in calls.items():                                         # the rays of a job; also the first launch
        ctr.zero_()
        call(ctr.data_ptr())
        torch.cuda.synchronize()
        assert int(ctr[0]) == n * K
        rays[key] = int(ctr[1])
    assert rays["mis_balance"] == rays["mis_power"] == rays["direct"] + rays["gather1"]          # identity 3: exactly their rays
    out = {"items": n, "emitters": len(table), "samples_per_job": n * K}
    stats, var = {}, {}
    for key in calls:
        s, m = (t.view(n, 3)[:, 0].double() for t in sums[key])
        var[key] = torch.clamp(m - s * s, min=0.0) * (K / (K - 1.0))
        stats[key] = {"mean_red": round(float(s.mean()), 5), "mean_sample_variance_red": round(float(var[key].mean()), 6),
                      "largest_item_sample_variance_red": round(float(var[key].max()), 3)}
    out["same_bytes_as_direct"] = bool(torch.equal(sums["mis_balance"][0], sums["direct"][0]) and torch.equal(sums["mis_power"][1], sums["direct"][1]))
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
    vd = stats["direct"]["mean_sample_variance_red"]
    for key in ("mis_balance", "mis_power"):
        out["time_%s_over_direct" % key] = round(med[key] / med["direct"], 4)
        out["time_%s_over_direct_plus_gather1" % key] = round(med[key] / (med["direct"] + med["gather1"]), 4)
        out["expectation_%s_at_most_direct_plus_gather1" % key] = bool(med[key] <= med["direct"] + med["gather1"])
        v = stats[key]["mean_sample_variance_red"]
        if v > 0.0:
            out["variance_direct_over_%s" % key] = round(vd / v, 3)
            out["equal_time_efficiency_%s_against_direct" % key] = round((vd * med["direct"]) / (v * med[key]), 3)
    if bake:
        vg, tg = stats["gather"]["mean_sample_variance_red"], med["gather"]
        trio = {}
        for name, first in (("direct_mis_plus_nee_mis", "mis_balance"), ("direct_plus_nee_mis", "direct")):
            v = float((var[first] + var["indirect"]).mean())
            t = med[first] + med["indirect"]
            mean = float((sums[first][0].view(n, 3)[:, 0].double() + sums["indirect"][0].view(n, 3)[:, 0].double()).mean())
            trio[name] = {"mean_red": round(mean, 5), "mean_sample_variance_red": round(v, 6), "ms_per_bake": round(t, 3),
                          "time_over_gather": round(t / tg, 4), "variance_gather_over_bake": round(vg / v, 3),
                          "equal_time_efficiency_against_gather": round((vg * tg) / (v * t), 3)}
        trio["gather"] = {"mean_red": stats["gather"]["mean_red"], "mean_sample_variance_red": vg, "ms_per_bake": round(tg, 3)}
        out["bake_trio"] = trio
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
           "samples_per_item": K, "seed": SEED, "side": SIDE, "bake_side": BAKE_SIDE,
           "ratios": "time_X_over_Y = median ms of X / median ms of Y; equal_time_efficiency_X_against_Y = (var_Y * t_Y) / (var_X * t_X): "
                     "above 1, X reaches a given noise sooner; spread = (max - min) / median",
           "shapes_timed": "the lock-step list from LDS (both Cornell sets) and the 16-byte-node walk from global memory (the grid); the "
                           "two LDS-stack shapes and the two register-slot shapes were run by the tests only and were not timed"}
    scene, items, table = cornell(trt, 99.0)
    out["cornell_lamp_lowered_floor"] = bench_items(trt, torch, scene, items, table, False, args)
    scene, items, table = grid(trt)
    out["sphere_grid_100k"] = bench_items(trt, torch, scene, items, table, False, args)
    scene, items, table = room_texels(trt)
    out["cornell_lamp_lowered_all_surfaces"] = bench_items(trt, torch, scene, items, table, True, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
