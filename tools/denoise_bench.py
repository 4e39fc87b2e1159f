#!/usr/bin/env python3
"""Device time of the a-trous denoiser (trt_denoise_device), per pass and in total, for every form of its kernel.  Needs a GPU.

  python tools/denoise_bench.py [--reps 20] [--warmup 5] [--out profiles/denoise_bench.json]

Workloads: Cornell at 2048 x 2048 (the bench frame) and sphere_grid(100000) at 3840 x 2160; the frame is a 4-spp render, the guides are
its feature buffers (albedo, normal, depth: all three terms on), default parameters (4 iterations).
Forms (TRT_DENOISE_VARIANT, read by the library at every call): `shipped` (unset: the library's choice per step), `plain` (dword loads
from the caller's buffers, no packing, no LDS), `packed` (16-byte records from global memory at every step), `lds` (the LDS tile at
every step it can serve - 1, 2, 4 - and the packed records beyond).  All forms must give the same bytes: checked before timing.
Timing: a pair of device events around EACH call, `reps` repetitions after `warmup` untimed ones, the median.  A call with k iterations
is timed for k = 1 .. 4; "pass_ms"[k-1] is T(k) - T(k-1), so pass 1 of the tuned forms carries the packing prologue and pass k of a
k-iteration call writes 12-byte pixels where a middle pass writes 16.
Yardstick: a device-to-device copy (torch, 16-byte vectors) that moves as many bytes as one pass must: per pixel 28 B of guides and
12 B of colour read and 12 B written = 52 B, timed as a copy of 26 B per pixel (26 read + 26 written).
Prints one JSON line; --out also writes it to a file."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.query_bench import time_case  # noqa: E402

FORMS = (("shipped", None), ("plain", "plain"), ("packed", "packed"), ("lds", "lds"))


def set_form(value):
    if value is None:
        os.environ.pop("TRT_DENOISE_VARIANT", None)
    else:
        os.environ["TRT_DENOISE_VARIANT"] = value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="image side scale (smaller images for a quick look; the stored figures use 1)")
    ap.add_argument("--only", default=None, help="run the workloads whose name contains this text")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20 or args.warmup < 5:
        ap.error("at least 20 repetitions after 5 warm-ups")
    import torch
    trt = importlib.import_module("tiny-raytracer_amd")
    trt._lib.check(trt.lib.trt_set_device(0))
    dev = torch.device("cuda:0")
    k = args.scale
    iterations = trt.denoise_params().iterations
    workloads = [("cornell_2048x2048", trt.scenes.cornell(int(2048 * k), int(2048 * k))),
                 ("sphere_grid100000_3840x2160", trt.scenes.sphere_grid(100000, int(3840 * k), int(2160 * k)))]
    out = {"metric": "ms per call (device events, median)", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(trt._lib.LIB_PATH), "iterations": iterations,
           "what": "trt_denoise_device, 4-spp frame + albedo, normal, depth, default parameters; total_ms[k-1] = a call with k iterations, "
                   "pass_ms[k-1] = total_ms[k-1] - total_ms[k-2] (pass 1 of the tuned forms includes the packing prologue); copy = a "
                   "device-to-device copy moving the 52 bytes per pixel one pass must move (26 read + 26 written)",
           "cases": {}, "shipped_vs": {}}
    for name, desc in workloads:
        if args.only and args.only not in name:
            continue
        world, cam = trt.world_from_description(desc)
        w, h = cam.get_image_size()
        n = w * h
        r = trt.Renderer(4, 1, 50, False, desc["background"], seed=5)
        frame = r.render(cam, world).data
        aov = r.render_aov(cam, world, channels=("albedo", "normal", "depth"))
        d = {"color": torch.from_numpy(frame).to(dev)}
        d.update({ch: torch.from_numpy(a).to(dev) for ch, a in aov.items()})
        d_out = torch.zeros(n * 3, dtype=torch.float32, device=dev)
        need = trt.denoise_scratch_bytes(w, h)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        del world, frame, aov

        def call(its):
            trt.denoise_device(d["color"].data_ptr(), w, h, d_out.data_ptr(), scratch.data_ptr(), need, d_albedo_ptr=d["albedo"].data_ptr(),
                               d_normal_ptr=d["normal"].data_ptr(), d_depth_ptr=d["depth"].data_ptr(), iterations=its)

        # all forms give the same bytes
        results = {}
        for form, value in FORMS:
            set_form(value)
            call(iterations)
            torch.cuda.synchronize()
            results[form] = d_out.clone()
        set_form(None)
        for form in results:
            if not torch.equal(results[form].view(torch.int32), results["shipped"].view(torch.int32)):
                raise SystemExit(f"{name}: the {form} form differs from the shipped one")
        del results
        case = {"pixels": n, "scratch_bytes": need}
        for form, value in FORMS:
            set_form(value)
            totals = [time_case(torch, lambda its=its: call(its), args.reps, args.warmup) for its in range(1, iterations + 1)]
            med = [t[0] for t in totals]
            case[form] = {"total_ms": [round(t, 4) for t in med], "total_ms_min": [round(t[1], 4) for t in totals],
                          "total_ms_max": [round(t[2], 4) for t in totals],
                          "pass_ms": [round(med[i] - (med[i - 1] if i else 0.0), 4) for i in range(iterations)]}
        set_form(None)
        src = torch.empty((n * 26 + 15) // 16 * 4, dtype=torch.float32, device=dev).view(-1, 4)
        dst = torch.empty_like(src)
        copy_ms, lo, hi = time_case(torch, lambda: dst.copy_(src), args.reps, args.warmup)
        case["copy"] = {"bytes_moved": int(src.numel()) * 8, "ms_median": round(copy_ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                        "gb_per_s": round(src.numel() * 8 / (copy_ms * 1e-3) / 1e9, 1)}
        out["cases"][name] = case
        full = case["shipped"]["total_ms"][-1]
        out["shipped_vs"][name] = {"plain_over_shipped": round(case["plain"]["total_ms"][-1] / full, 3),
                                   "packed_over_shipped": round(case["packed"]["total_ms"][-1] / full, 3),
                                   "lds_over_shipped": round(case["lds"]["total_ms"][-1] / full, 3),
                                   "shipped_over_copy_of_all_passes": round(full / (iterations * copy_ms), 2)}
        del d, d_out, scratch, src, dst
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
