#!/usr/bin/env python3
"""What the second moments and the variance-guided colour stop cost on the device.  Needs a GPU.

  python tools/moments_bench.py [--reps 20] [--warmup 5] [--out profiles/moments_bench.json]

 1. trt_render_moments_device beside trt_render_device: Cornell at 2048 x 2048, 64 spp, max_bounces 50 (the bench frame's scene and size).
    The moments come out of the fold that forms the frame anyway: 12 more bytes written per pixel (and read, where a render continues
    its buffers), against 768 bytes of radiance records read per pixel at 64 spp and the trace before it.
 2. trt_variance_device on that frame.
 3. trt_denoise_ex_device with the colour term on beside off (= trt_denoise_device), on the 64-spp frame with its feature buffers, default
    parameters.
Both frames and both denoised images must agree where they have to (the frame of 1 is trt_render_device's bit for bit; the term off is
trt_denoise_device bit for bit): checked before timing.
Timing: a pair of device events around EACH call, `reps` repetitions after `warmup` untimed ones, the median (tools/query_bench.py
time_case).  Prints one JSON line; --out also writes it to a file."""
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
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20 or args.warmup < 5:
        ap.error("at least 20 repetitions after 5 warm-ups")
    import torch
    trt = importlib.import_module("tiny-raytracer_amd")
    trt._lib.check(trt.lib.trt_set_device(0))
    dev = torch.device("cuda:0")
    side = int(2048 * args.scale)
    desc = trt.scenes.cornell(side, side)
    world, cam = trt.world_from_description(desc)
    scene = world.get_bvh()
    n = side * side
    r = trt.Renderer(args.spp, 1, 50, False, desc["background"], seed=5)
    d_frame = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    d_frame2 = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    d_m2 = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    d_var = torch.zeros(n, dtype=torch.float32, device=dev)

    def render():
        r.render_device(cam, scene, d_frame.data_ptr())

    def render_moments():
        r.render_moments_device(cam, scene, d_frame2.data_ptr(), d_m2.data_ptr())

    def variance():
        trt.variance_device(d_frame2.data_ptr(), d_m2.data_ptr(), n, args.spp, d_var.data_ptr())

    render()
    render_moments()
    variance()
    torch.cuda.synchronize()
    if not torch.equal(d_frame.view(torch.int32), d_frame2.view(torch.int32)):
        raise SystemExit("the frame of trt_render_moments_device differs from trt_render_device's")
    out = {"metric": "ms per call (device events, median)", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(trt._lib.LIB_PATH), "scene": "cornell", "width": side, "height": side, "spp": args.spp, "max_bounces": 50,
           "variance_positive_share": round(float((d_var > 0).float().mean()), 4)}
    for key, fn in (("render_device", render), ("render_moments_device", render_moments), ("variance_device", variance)):
        med, lo, hi = time_case(torch, fn, args.reps, args.warmup)
        out[key] = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
    out["moments_over_render"] = round(out["render_moments_device"]["ms_median"] / out["render_device"]["ms_median"], 4)

    aov = r.render_aov(cam, scene, channels=("albedo", "normal", "depth"))
    d = {ch: torch.from_numpy(a).to(dev) for ch, a in aov.items()}
    del aov
    d_out = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    d_out2 = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    need = trt.denoise_scratch_bytes(side, side)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)

    def denoise(out_t, **colour):
        trt.denoise_device(d_frame2.data_ptr(), side, side, out_t.data_ptr(), scratch.data_ptr(), need, d_albedo_ptr=d["albedo"].data_ptr(),
                           d_normal_ptr=d["normal"].data_ptr(), d_depth_ptr=d["depth"].data_ptr(), **colour)

    denoise(d_out)
    denoise(d_out2, d_variance_ptr=d_var.data_ptr(), sigma_color=0.0)
    torch.cuda.synchronize()
    if not torch.equal(d_out.view(torch.int32), d_out2.view(torch.int32)):
        raise SystemExit("trt_denoise_ex_device with the term off differs from trt_denoise_device")
    denoise(d_out2, d_variance_ptr=d_var.data_ptr())
    torch.cuda.synchronize()
    out["denoise_changed_share"] = round(float((d_out.view(-1, 3) != d_out2.view(-1, 3)).any(dim=1).float().mean()), 4)
    for key, fn in (("denoise_term_off", lambda: denoise(d_out)), ("denoise_term_on", lambda: denoise(d_out2, d_variance_ptr=d_var.data_ptr()))):
        med, lo, hi = time_case(torch, fn, args.reps, args.warmup)
        out[key] = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
    out["term_on_over_off"] = round(out["denoise_term_on"]["ms_median"] / out["denoise_term_off"]["ms_median"], 4)
    out["sigma_color"] = trt.denoise_color().sigma_color
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
