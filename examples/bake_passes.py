#!/usr/bin/env python3
"""Bake the floor of the Cornell box in passes: direct light, indirect light and the share of spent paths -> direct.png, indirect.png,
spent.png.
   python examples/bake_passes.py [texels samples]
bake.quad_texels lays texels x texels surfels over the floor quad (as examples/bake_lightmap.py does) and Scene.passes (trt_passes) draws
and traces exactly the paths Scene.gather would, but keeps them apart by how they ended: with 2 depth bins slot 0 holds the light of the
paths that reached the lamp with their first ray, slot 2 those that left through the open front at once - together the direct light, which
an engine computes at run time - and slots 1 and 3 everything that scattered first: the indirect light a lightmap stores.  The two add up
to the lightmap of bake_lightmap.py (same seed, same paths) up to the rounding of another summation order.  `spent` is the share of each
texel's paths that ended by the bounce budget and so carry no light: the bias of the budget, texel by texel."""
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
passes, spent, st = scene.passes(items, spp, depth_bins=2, source="cosine", max_bounces=20, background=desc["background"])
dt = time.perf_counter() - t0
direct, indirect = trt.passes.direct(passes), trt.passes.indirect(passes)
trt.Image(direct.reshape(texels, texels, 3)).save("direct.png")
trt.Image(indirect.reshape(texels, texels, 3)).save("indirect.png")
trt.Image(np.repeat(spent[:, None], 3, axis=1).reshape(texels, texels, 3)).save("spent.png")
print(f"{texels}x{texels} texels of the floor, {spp} samples each: {st['rays']} rays, kernel {st['kernel_ms']:.1f} ms "
      f"({st['rays'] / st['kernel_ms'] / 1e3:.0f} Mray/s), call {dt * 1e3:.1f} ms; mean direct {float(direct.mean()):.4f}, "
      f"indirect {float(indirect.mean()):.4f}, spent share {float(spent.mean()):.4f} -> direct.png, indirect.png, spent.png")
