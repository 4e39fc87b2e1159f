#!/usr/bin/env python3
"""Bake a lightmap: the light the floor of the Cornell box receives, texel by texel -> lightmap.png.
   python examples/bake_lightmap.py [texels samples]
bake.quad_texels lays texels x texels surfels (texel centre, unit normal) over the floor quad - the fourth quad of scenes.cornell, whose
cross(u, v) points down, hence flip - and Scene.gather (trt_gather) does the rest on the device: for every sample it draws a direction
about the normal with the cosine lobe (Lambertian::scatter's rule), traces its path and folds per texel.  The result is the radiance a
white diffuse floor would reflect, irradiance / pi; it goes through Image.save (the imager's tone map), and the second moments give the
standard error per texel (trt.variance), printed.  Only the surfels go up (24 bytes per texel) and the sums come down."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinyrt_amd as trt

argv = sys.argv[1:]
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
trt.Image(radiance.reshape(texels, texels, 3)).save("lightmap.png")
err = np.sqrt(trt.variance(radiance, moment2, spp)) if spp >= 2 else np.zeros(1, np.float32)
print(f"{texels}x{texels} texels of the floor, {spp} samples each: {st['rays']} rays, kernel {st['kernel_ms']:.1f} ms "
      f"({st['rays'] / st['kernel_ms'] / 1e3:.0f} Mray/s), call {dt * 1e3:.1f} ms, median standard error {float(np.median(err)):.4f} -> lightmap.png")
