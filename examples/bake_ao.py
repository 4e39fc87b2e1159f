#!/usr/bin/env python3
"""Bake ambient occlusion: how much of the hemisphere above each texel of the Cornell box's floor is blocked -> ao.png.
   python examples/bake_ao.py [texels samples distance]
bake.quad_texels lays texels x texels surfels (texel centre, unit normal) over the floor quad exactly as examples/bake_lightmap.py does,
and Scene.ambient (trt_ambient) does the rest on the device: for every sample it draws a direction about the normal with the cosine lobe,
asks whether anything lies within `distance` along it (default 50, half the side of the box; "inf" counts everything, and then only the
open front of the box is visible) and folds per texel.  The image is the visibility, white = open; 1 - it
is cosine-weighted ambient occlusion.  The bent normal - the mean open direction - comes back with it and its mean tilt is printed.  Only
the surfels go up (24 bytes per texel) and 16 bytes per texel come down."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinyrt_amd as trt

argv = sys.argv[1:]
texels, spp = (int(a) for a in argv[:2]) if len(argv) >= 2 else (256, 64)
distance = float(argv[2]) if len(argv) >= 3 else 50.0
desc = trt.scenes.cornell(2, 2)                                              # the camera of the description is not used
world, _ = trt.world_from_description(desc)
scene = world.get_bvh()
kind, corner, u, v, _ = desc["geometries"][3]
assert kind == "quad"
items = trt.bake.quad_texels(corner, u, v, texels, texels, flip=True)        # the axis points up, into the box
t0 = time.perf_counter()
visibility, bent, st = scene.ambient(items, spp, lobe="cosine", max_distance=distance, bent=True)
dt = time.perf_counter() - t0
grey = np.repeat(visibility.reshape(texels, texels, 1), 3, axis=2)
trt.Image(np.ascontiguousarray(grey)).save("ao.png")
length = np.linalg.norm(bent.astype(np.float64), axis=1)
open_ = length > 0.0
tilt = np.degrees(np.arccos(np.clip(bent[open_, 1] / length[open_], -1.0, 1.0)))       # against the floor's normal (0, 1, 0)
print(f"{texels}x{texels} texels of the floor, {spp} samples each within {distance:g}: {st['rays']} rays, kernel {st['kernel_ms']:.1f} ms "
      f"({st['rays'] / st['kernel_ms'] / 1e3:.0f} Mray/s), call {dt * 1e3:.1f} ms, mean occlusion {1.0 - float(visibility.mean()):.4f}, "
      f"mean tilt of the bent normal {float(tilt.mean()):.1f} degrees -> ao.png")
