#!/usr/bin/env python3
"""Quality of the adaptive sampling driver at equal budget, on the CPU.  Needs no GPU: the product's bytes are the oracle's
(tests/test_gpu_adaptive.py), so the restatement of Renderer.render_adaptive over the CPU oracle (tests/adaptive_cases.py) IS the driver.

  python tools/adaptive_quality.py [--cap 256] [--min-spp 8] [--step-spp 8] [--out profiles/adaptive_quality.json]

Cornell 64 x 64, max_bounces 8, seed 5, against the 65536-spp reference of seed 77 (the harness of DESIGN.md 6.4's consistency table).
For each tolerance: the tonemapped mean squared error of the adaptive frame, the samples it spent, and the error of a UNIFORM render of
the same total number of samples rounded UP to a whole spp (so the uniform frame never has fewer samples).  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap", type=int, default=256, help="samples_per_pixel N, a power of two")
    ap.add_argument("--min-spp", type=int, default=8)
    ap.add_argument("--step-spp", type=int, default=8)
    ap.add_argument("--tolerances", default="0.2:0,0.1:0,0.05:0,0.1:0.01", help="rel_tol:abs_tol,...")
    ap.add_argument("--ref-spp", type=int, default=65536)
    ap.add_argument("--threads", type=int, default=min(32, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    trt = importlib.import_module("tiny-raytracer_amd")
    from oracle import orc
    import adaptive_cases as A
    import denoise_color_cases as D
    side, bounces = 64, 8
    desc = trt.scenes.cornell(side, side)
    ow, ocam = orc.world_from_description(desc)
    bg = desc["background"]
    ref, _ = orc.render(ow, ocam, args.ref_spp, bounces, bg, seed=77, nthreads=args.threads)
    samples = D.oracle_samples(orc, ow, ocam, args.cap, bounces, bg, 5, nthreads=args.threads)
    out = {"metric": "tonemapped MSE against the reference", "scene": "cornell", "width": side, "height": side, "max_bounces": bounces, "seed": 5,
           "reference": {"spp": args.ref_spp, "seed": 77}, "cap": args.cap, "min_spp": args.min_spp, "step_spp": args.step_spp, "rows": []}
    uniform_cache = {}

    def uniform(spp):
        if spp not in uniform_cache:
            frame, _ = orc.render(ow, ocam, spp, bounces, bg, seed=5, nthreads=args.threads)
            uniform_cache[spp] = D.tonemapped_mse(frame, ref)
        return uniform_cache[spp]

    for item in args.tolerances.split(","):
        rel_tol, abs_tol = (float(v) for v in item.split(":"))
        frame, _, _, count, history = A.restated_adaptive(samples, args.min_spp, args.step_spp, rel_tol, abs_tol)
        total = int(count.astype(np.int64).sum())
        spp_u = -(-total // (side * side))
        row = {"rel_tol": rel_tol, "abs_tol": abs_tol, "mean_spp": round(total / (side * side), 3), "share_at_min": round(float((count == args.min_spp).mean()), 4),
               "share_at_cap": round(float((count == args.cap).mean()), 4), "rounds": len(history) - 1,
               "mse_adaptive": D.tonemapped_mse(frame, ref), "uniform_spp": spp_u, "mse_uniform": uniform(spp_u)}
        row["adaptive_over_uniform"] = round(row["mse_adaptive"] / row["mse_uniform"], 4)
        out["rows"].append(row)
    out["mse_uniform_at_min"] = uniform(args.min_spp)
    out["mse_uniform_at_cap"] = uniform(args.cap)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
