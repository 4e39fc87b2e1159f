#!/usr/bin/env python3
"""Bake a lightmap: the light the floor of the Cornell box receives, texel by texel -> lightmap.png.
   python examples/bake_lightmap.py [texels samples] [--export]
bake.quad_texels lays texels x texels surfels (texel centre, unit normal) over the floor quad - the fourth quad of scenes.cornell, whose
cross(u, v) points down, hence flip - and Scene.gather (trt_gather) does the rest on the device: for every sample it draws a direction
about the normal with the cosine lobe (Lambertian::scatter's rule), traces its path and folds per texel.  The result is the radiance a
white diffuse floor would reflect, irradiance / pi; it goes through Image.save (the imager's tone map), and the second moments give the
standard error per texel (trt.variance), printed.  Only the surfels go up (24 bytes per texel) and the sums come down.
--export bakes through the sample-parallel route instead: Scene.samples_device (trt_samples_device) leaves every sample's colour in HBM,
where a caller's own estimator could read it, trt.fold_samples_device folds the records there, and the sums are asserted to be
Scene.gather's, bit for bit.  Needs torch for the device buffers."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinyrt_amd as trt

export = "--export" in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a != "--export"]
texels, spp = (int(a) for a in argv[:2]) if len(argv) >= 2 else (256, 64)
desc = trt.scenes.cornell(2, 2)                                              # the camera of the description is not used
world, _ = trt.world_from_description(desc)
scene = world.get_bvh()
kind, corner, u, v, _ = desc["geometries"][3]
assert kind == "quad"
items = trt.bake.quad_texels(corner, u, v, texels, texels, flip=True)        # the axis points up, into the box
t0 = time.perf_counter()
radiance, moment2, st = scene.gather(items, spp, lobe="cosine", max_bounces=20, background=desc["background"], moment2=True)
dt = time.perf_counter() - t0
if export:
    import torch
    n = len(items)
    d_items = torch.from_numpy(items).to("cuda:0")
    d_colors = torch.zeros(n * spp * 3, dtype=torch.float32, device="cuda:0")
    d_sums, d_sums2 = (torch.zeros(n * 3, dtype=torch.float32, device="cuda:0") for _ in range(2))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    scene.samples_device(d_items.data_ptr(), n, d_colors.data_ptr(), samples_per_item=spp, source="cosine", max_bounces=20,
                         background=desc["background"])
    trt.fold_samples_device(d_colors.data_ptr(), n, spp, d_sums.data_ptr(), d_sums2.data_ptr())
    b.record()
    torch.cuda.synchronize()
    for got, want in ((d_sums, radiance), (d_sums2, moment2)):
        got = got.cpu().numpy().reshape(n, 3)
        assert np.where(np.isnan(want), np.isnan(got), got.view(np.uint32) == want.view(np.uint32)).all(), "the folded samples are not Scene.gather's sums"
    print(f"--export: {n * spp} samples on {scene.samples_plan(n, spp)['waves']} waves (Scene.gather: {scene.gather_plan(n)['waves']}), "
          f"samples + fold {a.elapsed_time(b):.1f} ms against {st['kernel_ms']:.1f} ms; the sums are Scene.gather's bit for bit")
    radiance = d_sums.cpu().numpy().reshape(n, 3)
trt.Image(radiance.reshape(texels, texels, 3)).save("lightmap.png")
err = np.sqrt(trt.variance(radiance, moment2, spp)) if spp >= 2 else np.zeros(1, np.float32)
print(f"{texels}x{texels} texels of the floor, {spp} samples each: {st['rays']} rays, kernel {st['kernel_ms']:.1f} ms "
      f"({st['rays'] / st['kernel_ms'] / 1e3:.0f} Mray/s), call {dt * 1e3:.1f} ms, median standard error {float(np.median(err)):.4f} -> lightmap.png")
