#!/usr/bin/env python3
"""Bake the direct light of the Cornell box's floor with shadow rays -> direct_nee.png, beside the same light found by chance.
   python examples/bake_direct.py [texels samples] [--mis balance|power] [--pick]
bake.quad_texels lays texels x texels surfels over the floor quad (as examples/bake_passes.py does).  Scene.direct (trt_direct) aims every
sample at a point on the lamp - the table is Scene.emitters(), the scene's own lights - and asks whether the segment is blocked;
Scene.passes (trt_passes) draws cosine-distributed first rays, of which about one in 200 reaches the lamp, and keeps those in its depth-0
slot.  Both estimate the same integral, so the two means agree to sampling noise, and the standard error of a texel (trt_variance's
square root) says at what price: at the same number of samples the shadow rays are about two orders of magnitude quieter.

--mis sends one cosine-lobe ray from every texel besides and weights the two against each other (trt_direct_mis): the same mean; on the
floor, far from the lamp, it buys nothing and costs a walk, beside the lamp (a ceiling, the top of a wall) it removes the 1/d2 tail.

--pick adds sixty small sphere lights of a twentieth of the lamp's colour along the walls and chooses the emitter of every sample through
lights.pick_table's alias table (trt_direct_pick; with --mis trt_direct_mis_pick): by power, where the uniform choice sends sixty of
sixty-one shadow rays to a few percent of the light.  It prints the standard error of a texel both ways.

The lamp is lowered from y = 100 to y = 99 here.  In the stock box it lies in the ceiling's plane, and the reference's own paths - hence
trt_gather and trt_passes - see it only where rounding lets the lamp win the tie with the ceiling, about a quarter of the time; a shadow
ray aims at the lamp and stops short of it, so it sees the lamp fully.  That is a property of that scene, not of either query."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinyrt_amd as trt

argv = sys.argv[1:]
mis = None
if "--mis" in argv:
    at = argv.index("--mis")
    mis = argv[at + 1]
    del argv[at:at + 2]
pick = "--pick" in argv
if pick:
    argv.remove("--pick")
texels, spp = (int(a) for a in argv[:2]) if len(argv) >= 2 else (256, 64)
desc = trt.scenes.cornell(2, 2)                                              # the camera of the description is not used
geos = list(desc["geometries"])
kind, corner, u, v, material = geos[2]
assert kind == "quad" and material == "light"
geos[2] = (kind, (corner[0], 99.0, corner[2]), u, v, material)
materials = list(desc["materials"])
if pick:                                                                    # the many-light room: 20 dim spheres on each of three walls
    lamp = [m for m in materials if m[0] == "light"][0]
    materials.append(("dim_light", lamp[1], tuple(0.05 * c for c in lamp[2]), 0.0))
    for y in (20.0, 40.0, 60.0, 80.0):
        for a in (10.0, 30.0, 50.0, 70.0, 90.0):
            geos += [("sphere", (2.0, y, a), 1.0, "dim_light"), ("sphere", (98.0, y, a), 1.0, "dim_light"), ("sphere", (a, y, 98.0), 1.0, "dim_light")]
desc = dict(desc, materials=materials, geometries=geos)
world, _ = trt.world_from_description(desc)
scene = world.get_bvh()
kind, corner, u, v, _ = desc["geometries"][3]
assert kind == "quad"
items = trt.bake.quad_texels(corner, u, v, texels, texels, flip=True)        # the axis points up, into the box
table = scene.emitters()
t0 = time.perf_counter()
direct, moment2, st = scene.direct(items, table, spp, moment2=True, mis=mis, pick=trt.lights.pick_table(table) if pick else None)
dt = time.perf_counter() - t0
passes, _, pst = scene.passes(items, spp, depth_bins=2, source="cosine", max_bounces=1, background=(0.0, 0.0, 0.0), spent=False)
by_chance = trt.passes.direct(passes)
trt.Image(direct.reshape(texels, texels, 3)).save("direct_nee.png")
with np.errstate(invalid="ignore"):
    err = np.sqrt(np.maximum(moment2 - direct * direct, 0.0) / max(spp - 1, 1))[:, 0]
print(f"{texels}x{texels} texels of the floor, {spp} samples each, {len(table)} emitter: {st['rays']} {'shadow' if mis is None else 'shadow and lobe'} rays of "
      f"{st['samples']} samples, "
      f"kernel {st['kernel_ms']:.1f} ms, call {dt * 1e3:.1f} ms; mean direct light {float(direct[:, 0].mean()):.4f} "
      f"(standard error of a texel {float(err.mean()):.4f}) beside passes.direct {float(by_chance[:, 0].mean()):.4f} "
      f"from {pst['rays']} rays found by chance -> direct_nee.png")
if pick:
    uniform, um2, _ = scene.direct(items, table, spp, moment2=True, mis=mis)
    with np.errstate(invalid="ignore"):
        uerr = np.sqrt(np.maximum(um2 - uniform * uniform, 0.0) / max(spp - 1, 1))[:, 0]
    print(f"{len(table)} emitters chosen by power: standard error of a texel {float(err.mean()):.4f}, chosen uniformly {float(uerr.mean()):.4f} "
          f"(mean {float(uniform[:, 0].mean()):.4f})")
