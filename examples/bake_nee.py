#!/usr/bin/env python3
"""Bake the full light of the Cornell box's floor with the lights aimed at at every bounce -> nee.png, beside the same light found by
chance -> gather.png.
   python examples/bake_nee.py [SIZE K] [--mis balance|power] [--direct-mis balance|power] [--pick] [--export]
bake.quad_texels lays SIZE x SIZE surfels over the floor quad.  Scene.direct (trt_direct) aims every sample at the lamp from the texel
itself; Scene.nee (trt_nee) with source_is_diffuse=True traces the cosine-distributed paths Scene.gather traces, hides the lamp where a
path reaches it by a diffuse bounce and sends one shadow ray to it from every diffuse vertex instead: the texel's indirect light.  Their sum
and Scene.gather at the same K estimate the same integral; the standard error of a texel says at what price.

--mis weights every shadow ray against the hit the path makes anyway (trt_nee_mis): the same mean, without the 1/d2 tail of the shadow
rays sent from vertices beside the lamp.

--direct-mis takes the direct part from trt_direct_mis, which weights the texel's own shadow ray against a cosine-lobe ray from the texel:
with both flags no term of the bake is unbounded, which matters for texels beside the lamp (not the floor's).

--pick bakes the many-light room of examples/bake_direct.py --pick - sixty small sphere lights of a twentieth of the lamp's colour along
the walls - and chooses the emitter of every shadow ray, the texel's own and those of the path's vertices, through lights.pick_table's alias
table (trt_direct_pick and trt_nee_pick; with the mis flags trt_direct_mis_pick and trt_nee_mis_pick): by power, where the uniform choice
sends sixty of sixty-one shadow rays to six percent of the light.  The same bake with the uniform choice is printed beside it.

--export bakes the indirect part a second time, a sample to a GPU lane: Scene.nee_samples_device (trt_nee_samples_device) writes every
sample's colour into K records per texel in HBM and fold_samples_device (trt_fold_samples_device) folds them.  The sums are asserted equal
to Scene.nee's by their bits, and the records are what a robust estimator of the caller's own would read: the median of the texels' means
of eight groups is printed beside the mean.

The lamp is lowered from y = 100 to y = 99 here, as in examples/bake_direct.py: in the stock box it lies in the ceiling's plane."""
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
direct_mis = None
if "--direct-mis" in argv:
    at = argv.index("--direct-mis")
    direct_mis = argv[at + 1]
    del argv[at:at + 2]
pick = "--pick" in argv
if pick:
    argv.remove("--pick")
export = "--export" in argv
if export:
    argv.remove("--export")
size, spp = (int(a) for a in argv[:2]) if len(argv) >= 2 else (256, 64)
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
scene = trt.world_from_description(desc)[0].get_bvh()
kind, corner, u, v, _ = desc["geometries"][3]
assert kind == "quad"
items = trt.bake.quad_texels(corner, u, v, size, size, flip=True)            # the axis points up, into the box
table = scene.emitters()
path = dict(max_bounces=5, background=(0.0, 0.0, 0.0))
t0 = time.perf_counter()
pick_table = trt.lights.pick_table(table) if pick else None
direct, d_m2, dst = scene.direct(items, table, spp, moment2=True, mis=direct_mis, pick=pick_table)
indirect, i_m2, ist = scene.nee(items, table, spp, source="cosine", source_is_diffuse=True, moment2=True, mis=mis, pick=pick_table, **path)
t1 = time.perf_counter()
gather, g_m2, gst = scene.gather(items, spp, lobe="cosine", moment2=True, **path)
t2 = time.perf_counter()
full = direct + indirect
trt.Image(full.reshape(size, size, 3)).save("nee.png")
trt.Image(gather.reshape(size, size, 3)).save("gather.png")


def texel_error(mean, m2):
    return np.sqrt(np.maximum(m2 - mean * mean, 0.0) / max(spp - 1, 1))[:, 0]


# the two estimates are drawn from different streams of a sample: their variances add
err_nee = np.sqrt(texel_error(direct, d_m2) ** 2 + texel_error(indirect, i_m2) ** 2)
err_gather = texel_error(gather, g_m2)
print(f"{size}x{size} texels of the floor, {spp} samples each: direct + nee mean {float(full[:, 0].mean()):.4f} "
      f"(standard error of a texel {float(err_nee.mean()):.4f}; {dst['rays'] + ist['rays']} rays, {(t1 - t0) * 1e3:.1f} ms) -> nee.png; "
      f"gather mean {float(gather[:, 0].mean()):.4f} (standard error {float(err_gather.mean()):.4f}; {gst['rays']} rays, "
      f"{(t2 - t1) * 1e3:.1f} ms) -> gather.png")
if pick:
    # the same bake with the uniform choice: the same expectation, the noise the table is for
    u_direct, u_d_m2, _ = scene.direct(items, table, spp, moment2=True, mis=direct_mis)
    u_indirect, u_i_m2, _ = scene.nee(items, table, spp, source="cosine", source_is_diffuse=True, moment2=True, mis=mis, **path)
    err_uniform = np.sqrt(texel_error(u_direct, u_d_m2) ** 2 + texel_error(u_indirect, u_i_m2) ** 2)
    print(f"{len(table)} emitters, the lamp {float(pick_table[0]['prob'].max()):.3f} of the power: uniform choice mean "
          f"{float((u_direct + u_indirect)[:, 0].mean()):.4f} (standard error of a texel {float(err_uniform.mean()):.4f}); of the indirect part alone "
          f"{float(texel_error(u_indirect, u_i_m2).mean()):.4f} uniform, {float(texel_error(indirect, i_m2).mean()):.4f} by power")
if export:
    import torch
    n = len(items)
    d_items = torch.from_numpy(np.ascontiguousarray(items)).to("cuda:0")
    d_table = torch.from_numpy(table.view("uint8").copy()).to("cuda:0")
    d_records = torch.zeros(n * spp * 3, dtype=torch.float32, device="cuda:0")
    d_sum, d_m2 = torch.zeros(n * 3, dtype=torch.float32, device="cuda:0"), torch.zeros(n * 3, dtype=torch.float32, device="cuda:0")
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    pick_arg = None
    if pick:
        d_pick = torch.from_numpy(pick_table[0].view("uint8").copy()).to("cuda:0")
        pick_arg = d_pick.data_ptr() if mis is None else (d_pick.data_ptr(), pick_table[1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scene.nee_samples_device(d_items.data_ptr(), n, d_table.data_ptr(), len(table), d_records.data_ptr(), d_counters_ptr=ctr.data_ptr(),
                             samples_per_item=spp, source="cosine", source_is_diffuse=True, mis=mis, pick=pick_arg, **path)
    trt.fold_samples_device(d_records.data_ptr(), n, spp, d_sum.data_ptr(), d_m2.data_ptr())
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    folded, folded_m2 = d_sum.view(n, 3).cpu().numpy(), d_m2.view(n, 3).cpu().numpy()
    assert folded.tobytes() == indirect.tobytes() and folded_m2.tobytes() == i_m2.tobytes(), "the folded records are not Scene.nee's sums"
    assert (int(ctr[0]), int(ctr[1])) == (ist["samples"], ist["rays"])
    records = d_records.view(n, spp, 3).cpu().numpy()
    groups = 8 if spp % 8 == 0 else 1
    robust = np.median(records.reshape(n, groups, spp // groups, 3).mean(axis=2), axis=1)
    print(f"--export: {n * spp} records of the indirect part in {(t1 - t0) * 1e3:.1f} ms with their fold, the sums equal to Scene.nee's by bits; "
          f"mean {float(folded[:, 0].mean()):.4f}, median of {groups} group means {float(robust[:, 0].mean()):.4f}")
