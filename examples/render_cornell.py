#!/usr/bin/env python3
"""The reference binary (src/main.rs) through the Python mirror: Cornell box -> output.png.
   python examples/render_cornell.py [width height spp] [--aov DIR] [--denoise] [--adaptive REL_TOL]
--aov DIR also writes the frame's first-hit feature buffers (Renderer.render_aov: same seed, samples and primary rays as the render) to
DIR: albedo.png, normal.png ((n + 1) / 2), depth.png (scaled to the farthest hit), coverage.png, and all six as arrays in aov.npz.
--denoise also writes denoised.png beside output.png: the frame through trt.denoise (the a-trous filter of tinyrt.h, default parameters)
guided by the albedo, normal and depth buffers of the same seed and samples and, from 2 spp on, by the variance of every pixel's estimate
(Renderer.render_moments + trt.variance: the colour stop of trt_denoise_ex); and variance.png, the standard error per pixel (the square
root of that variance, white = 0.25 and more).
--adaptive REL_TOL samples adaptively instead (Renderer.render_adaptive: 8 samples everywhere, then 8 more at a time where the standard
error of a pixel still exceeds REL_TOL x its r + g + b, with an absolute floor of 0.01, up to spp): output.png is every pixel's estimate
at its own sample count, samples.png the count map (white = spp).  DESIGN.md 6.5 has the error at equal budget: 0.05 is a sound value."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinyrt_amd as trt

argv = sys.argv[1:]
aov_dir = None
if "--aov" in argv:
    at = argv.index("--aov")
    aov_dir = argv[at + 1]
    del argv[at:at + 2]
adaptive = None
if "--adaptive" in argv:
    at = argv.index("--adaptive")
    adaptive = float(argv[at + 1])
    del argv[at:at + 2]
denoise = "--denoise" in argv
if denoise:
    argv.remove("--denoise")
w, h, spp = (int(a) for a in argv[:3]) if len(argv) >= 3 else (300, 300, 300)
world, camera = trt.world_from_description(trt.scenes.cornell(w, h))          # build_world + Camera::new, src/main.rs:7-16
instance = trt.Renderer(spp, 8, 20, True, (0.001, 0.001, 0.001))             # Renderer::new(300, 8, 20, true, Some(0.001))
if adaptive is not None:
    import numpy as np
    t0 = time.perf_counter()
    frame, accum, moment2, count = instance.render_adaptive(camera, world, min(8, spp), 8, adaptive, 0.01)
    dt = time.perf_counter() - t0
    trt.Image(frame).save("output.png")
    trt.Image(np.ascontiguousarray(np.repeat((count.astype(np.float32) / spp)[:, :, None], 3, axis=2)), gamma=1.0).save("samples.png")
    print(f"{w}x{h}, adaptive to {spp} spp at rel_tol {adaptive:g}: {float(count.mean()):.1f} samples per pixel on average, "
          f"{float((count == count.min()).mean()):.0%} of the pixels at {int(count.min())}, {float((count == spp).mean()):.0%} at {spp}, "
          f"call {dt * 1e3:.1f} ms -> output.png, samples.png")
    sys.exit(0)
t0 = time.perf_counter()
if denoise:                                                                  # the same frame, bit for bit, with its second moments
    accum, moment2, _ = instance.render_moments(camera, world)
    image = trt.Image(accum)
else:
    image = instance.render(camera, world)
dt = time.perf_counter() - t0
image.save("output.png")
st = instance.last_stats
print(f"{w}x{h}, {spp} spp: {st['rays']} rays, kernel {st['kernel_ms']:.1f} ms ({st['rays'] / st['kernel_ms'] / 1e3:.0f} Mray/s), "
      f"call {dt * 1e3:.1f} ms -> output.png")
if aov_dir:
    import numpy as np
    os.makedirs(aov_dir, exist_ok=True)
    aov = instance.render_aov(camera, world)
    np.savez(os.path.join(aov_dir, "aov.npz"), **aov)
    grey = lambda a: np.repeat(a[:, :, None], 3, axis=2)                         # noqa: E731
    far = float(aov["depth"].max()) or 1.0
    for name, linear in (("albedo", aov["albedo"]), ("normal", (aov["normal"] + 1.0) * 0.5), ("depth", grey(aov["depth"] / far)),
                         ("coverage", grey(aov["coverage"]))):
        trt.Image(np.ascontiguousarray(linear, np.float32), gamma=1.0).save(os.path.join(aov_dir, name + ".png"))
    hit = aov["geometry"] != 0xFFFFFFFF
    print(f"feature buffers -> {aov_dir}: coverage {float(aov['coverage'].mean()):.3f}, {len(np.unique(aov['geometry'][hit]))} geometries seen by sample 0")
if denoise:
    guides = instance.render_aov(camera, world, channels=("albedo", "normal", "depth"))
    t0 = time.perf_counter()
    import numpy as np
    var = trt.variance(accum, moment2, spp)                                  # +inf at 1 spp: unknown
    clean = trt.denoise(image.data, guides["albedo"], guides["normal"], guides["depth"], variance=var if spp >= 2 else None)
    dt = time.perf_counter() - t0
    trt.Image(clean).save("denoised.png")
    err = np.sqrt(np.where(np.isfinite(var), var, 0.0)).astype(np.float32)
    trt.Image(np.ascontiguousarray(np.repeat((err / 0.25)[:, :, None], 3, axis=2), np.float32), gamma=1.0).save("variance.png")
    p = trt.denoise_params()
    print(f"denoised ({p.iterations} passes, sigma_color {trt.denoise_color().sigma_color:g}, call {dt * 1e3:.1f} ms with its copies) -> denoised.png; "
          f"standard error: median {float(np.median(err)):.4f}, 99th percentile {float(np.percentile(err, 99)):.4f} -> variance.png")
