#!/usr/bin/env python3
"""Bake light probes: a G x G grid of points in the horizontal plane y = 50 of the Cornell box, the radiance arriving at each projected
onto 9 spherical-harmonic coefficients per channel -> probes.png.
   python examples/bake_probes.py [G K] [--export] [--parallel]
Scene.probe (trt_probe) does it on the device: for every one of K samples it draws a direction uniformly over the sphere, traces its path
and adds colour * Y_k(direction) / K to the probe's coefficients; 24 bytes per probe go up and 108 come down.  Each probe is drawn as a
small white diffuse ball seen from the open front of the box and lit by sh.irradiance of its own coefficients - the irradiance about the
normal, over pi: what a dynamic object placed there would look like.  Far probes are at the top, the red wall's side on the left.
--export bakes through the sample-parallel route instead - Scene.samples_device (trt_samples_device, source "sphere") leaves every
sample's colour and direction in HBM, a sample to a lane where Scene.probe gives the K samples of a probe one lane, and sh.project folds
them on the host - and asserts that the coefficients are Scene.probe's, bit for bit.  Needs torch for the device buffers.
--parallel bakes the same probes through Scene.probe_parallel (trt_probe_parallel) as well - the same sample-parallel paths with the
projection on the device too, in one call with host buffers - asserts the coefficients equal to Scene.probe's by their bits and prints
both kernel times: few probes with many samples (say 4 4096) are where it pays."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinyrt_amd as trt

export = "--export" in sys.argv[1:]
parallel = "--parallel" in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a not in ("--export", "--parallel")]
grid, spp = (int(a) for a in argv[:2]) if len(argv) >= 2 else (8, 256)
TILE = 48                                                                    # pixels per ball
desc = trt.scenes.cornell(2, 2)                                              # the camera of the description is not used
world, _ = trt.world_from_description(desc)
scene = world.get_bvh()
centre = (np.arange(grid) + 0.5) * (100.0 / grid)
items = np.zeros((grid, grid, 6), np.float32)                               # [row = far to near, column = x]
items[..., 0] = centre[None, :]
items[..., 1] = 50.0
items[..., 2] = centre[::-1, None]
items[..., 4] = 1.0                                                         # the axis: not read by the sphere domain
items = np.ascontiguousarray(items.reshape(-1, 6))
t0 = time.perf_counter()
coeffs, st = scene.probe(items, spp, bands=3, domain="sphere", max_bounces=20, background=desc["background"])
dt = time.perf_counter() - t0
if export:
    import torch
    n = len(items)
    d_items = torch.from_numpy(items).to("cuda:0")
    d_colors, d_dirs = (torch.zeros(n * spp * 3, dtype=torch.float32, device="cuda:0") for _ in range(2))
    ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    scene.samples_device(d_items.data_ptr(), n, d_colors.data_ptr(), d_dirs.data_ptr(), d_counters_ptr=ctr.data_ptr(), samples_per_item=spp,
                         source="sphere", max_bounces=20, background=desc["background"])
    b.record()
    torch.cuda.synchronize()
    exported = trt.sh.project(d_colors.cpu().numpy().reshape(n, spp, 3), d_dirs.cpu().numpy().reshape(n, spp, 3), 3, points=items[:, 0:3])
    same = np.where(np.isnan(coeffs), np.isnan(exported), exported.view(np.uint32) == coeffs.view(np.uint32))
    assert same.all() and int(ctr[1]) == st["rays"], "the projected samples are not Scene.probe's coefficients"
    q = scene.samples_plan(n, spp)
    print(f"--export: {n * spp} samples on {q['waves']} waves (Scene.probe: {scene.probe_plan(n)['waves']}), kernel {a.elapsed_time(b):.1f} ms "
          f"against {st['kernel_ms']:.1f} ms; projected on the host, the coefficients are Scene.probe's bit for bit")
    coeffs = exported
if parallel:
    baked, stp = scene.probe_parallel(items, spp, bands=3, domain="sphere", max_bounces=20, background=desc["background"])
    same = np.where(np.isnan(coeffs), np.isnan(baked), baked.view(np.uint32) == coeffs.view(np.uint32))
    assert same.all() and stp["rays"] == st["rays"] and stp["samples"] == st["samples"], "Scene.probe_parallel's coefficients are not Scene.probe's"
    q = scene.probe_parallel_plan(len(items), spp)
    print(f"--parallel: {len(items) * spp} samples on {q['waves']} waves (Scene.probe: {scene.probe_plan(len(items))['waves']}), kernels "
          f"{stp['kernel_ms']:.1f} ms against Scene.probe's {st['kernel_ms']:.1f} ms; the coefficients are Scene.probe's bit for bit")
    coeffs = baked
# the normals of a ball seen along +z: image x is world x, image y (up) is world y, and the visible side faces the viewer at -z
p = (np.arange(TILE) + 0.5) / TILE * 2.0 - 1.0
nx, ny = np.meshgrid(p, -p)
inside = nx * nx + ny * ny < 0.9
nz = -np.sqrt(np.clip(1.0 - nx * nx - ny * ny, 0.0, 1.0))
normals = np.stack([nx, ny, nz], axis=-1).astype(np.float32)                # [TILE, TILE, 3]
image = np.zeros((grid * TILE, grid * TILE, 3), np.float32)
for k in range(grid * grid):
    ball = trt.sh.irradiance(coeffs[k][None, None], normals, "sphere") / np.pi
    r, c = divmod(k, grid)
    image[r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE] = np.where(inside[..., None], np.maximum(ball, 0.0), 0.0)
trt.Image(np.ascontiguousarray(image)).save("probes.png")
mean = coeffs[:, 0, :].astype(np.float64).mean(axis=0) / float(trt.sh.C0)   # coefficient 0 is the mean of L * c0: over sphere and probes
print(f"{grid}x{grid} probes at y = 50, {spp} samples each: {st['rays']} rays, kernel {st['kernel_ms']:.1f} ms "
      f"({st['rays'] / st['kernel_ms'] / 1e3:.0f} Mray/s), call {dt * 1e3:.1f} ms, mean arriving radiance "
      f"({mean[0]:.3f}, {mean[1]:.3f}, {mean[2]:.3f}) -> probes.png")
