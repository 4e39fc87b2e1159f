#!/usr/bin/env python3
"""A camera the library does not have: a 360 degree equirectangular view from inside the Cornell box -> panorama.png.
   python examples/panorama.py [width height spp [spread]]
The rays are made here in numpy - column = longitude, row = latitude, from the middle of the box - and handed to Scene.radiance
(trt_radiance), which path traces caller-supplied rays with spp samples each and returns the mean colour and the mean of its square; the
frame goes through Image.save (the imager's tone map), and the second moments give the standard error per ray (trt.variance), printed.
Any other projection - fisheye, orthographic, a lens model of one's own - is another way to fill `rays`.
All spp samples of a pixel pass through the pixel centre, so edges stay aliased however many there are.  With a fourth argument, a cone
spread (about the angle of a pixel in radians: 2 pi / width), the frame is traced with Scene.gather(lobe="cone") instead: the device
jitters every sample's direction inside that cone, which anti-aliases the view."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinyrt_amd as trt

argv = sys.argv[1:]
w, h, spp = (int(a) for a in argv[:3]) if len(argv) >= 3 else (1024, 512, 64)
spread = float(argv[3]) if len(argv) >= 4 else None
world, _ = trt.world_from_description(trt.scenes.cornell(2, 2))              # the pinhole camera of the description is not used
scene = world.get_bvh()
lon = ((np.arange(w) + 0.5) / w * 2.0 - 1.0) * np.pi                         # -pi .. pi, 0 looks down +z
lat = (0.5 - (np.arange(h) + 0.5) / h) * np.pi                               # pi/2 (up) .. -pi/2
lon, lat = np.meshgrid(lon, lat)
rays = np.empty((h, w, 6), np.float32)
rays[..., 0:3] = (50.0, 50.0, 45.0)                                          # between the two boxes
rays[..., 3] = np.cos(lat) * np.sin(lon)
rays[..., 4] = np.sin(lat)
rays[..., 5] = np.cos(lat) * np.cos(lon)
t0 = time.perf_counter()
if spread is None:
    radiance, moment2, st = scene.radiance(rays.reshape(-1, 6), spp, max_bounces=20, background=(0.001, 0.001, 0.001), moment2=True)
else:
    radiance, moment2, st = scene.gather(rays.reshape(-1, 6), spp, lobe="cone", spread=spread, max_bounces=20, background=(0.001, 0.001, 0.001),
                                         moment2=True)
dt = time.perf_counter() - t0
trt.Image(radiance.reshape(h, w, 3)).save("panorama.png")
err = np.sqrt(trt.variance(radiance, moment2, spp)) if spp >= 2 else np.zeros(1, np.float32)
print(f"{w}x{h} equirectangular, {spp} samples per ray: {st['rays']} rays, kernel {st['kernel_ms']:.1f} ms "
      f"({st['rays'] / st['kernel_ms'] / 1e3:.0f} Mray/s), call {dt * 1e3:.1f} ms, median standard error {float(np.median(err)):.4f} -> panorama.png")
