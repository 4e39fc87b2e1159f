#!/usr/bin/env python3
"""A frame of the Cornell box through the queries, with the lamp aimed at at every diffuse hit -> nee_frame.png.
   python examples/render_nee.py [W H SPP] [--mis balance|power] [--pick] [--export]
Everything stays in HBM.  For sample s of SPP the camera writes the frame's primary rays (trt_primary_rays_device: the rays the render
traces for that sample) and Scene.nee_device (trt_nee_device, source "rays") folds one sample per pixel into the running sums: K = SPP,
the sample range [s, s + 1), accumulate from the second pass on - the frame in passes that tinyrt.h describes for trt_passes.  The first
hit of a camera ray is no diffuse vertex (source_is_diffuse = 0): the lamp is seen where the camera looks at it, and hidden where a path
reaches it by a diffuse bounce, because the shadow ray from that bounce has already counted it.  With --mis (trt_nee_mis_device) the
shadow ray and that hit are both counted, weighted by their densities.  (The stock box's lamp is coplanar with the ceiling, where the two
disagree about visibility: tinyrt.h, limits.)  With --pick the emitter of every shadow ray is chosen through lights.pick_table's alias table
(trt_nee_pick_device; with --mis trt_nee_mis_pick_device): the box has one lamp, so the frame's expectation and noise are the same and the
run shows what the extra draw costs.  With --export the same frame is traced a second time a sample to a GPU lane:
Scene.nee_samples_device (trt_nee_samples_device) writes every pass's colours into SPP records per pixel and fold_samples_device folds them
pass by pass; the sums and counters are asserted equal to the first frame's by their bits."""
import os
import sys
import time

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
export = "--export" in argv
if export:
    argv.remove("--export")
w, h, spp = (int(a) for a in argv[:3]) if len(argv) >= 3 else (300, 300, 64)
import torch

world, camera = trt.world_from_description(trt.scenes.cornell(w, h))
scene = world.get_bvh()
table = scene.emitters()
n = w * h
d_rays = torch.zeros(n * 6, dtype=torch.float32, device="cuda:0")
d_sum = torch.zeros(n * 3, dtype=torch.float32, device="cuda:0")
d_m2 = torch.zeros(n * 3, dtype=torch.float32, device="cuda:0")
d_table = torch.from_numpy(table.view("uint8").copy()).to("cuda:0")
ctr = torch.zeros(16, dtype=torch.int64, device="cuda:0")
pick_arg = None
if pick:
    records, total = trt.lights.pick_table(table)
    d_pick = torch.from_numpy(records.view("uint8").copy()).to("cuda:0")
    pick_arg = d_pick.data_ptr() if mis is None else (d_pick.data_ptr(), total)
torch.cuda.synchronize()
t0 = time.perf_counter()
for s in range(spp):
    camera.primary_rays_device(s, spp, d_rays.data_ptr(), seed=1)
    scene.nee_device(d_rays.data_ptr(), n, d_table.data_ptr(), len(table), d_sum.data_ptr(), d_m2.data_ptr(), d_counters_ptr=ctr.data_ptr(),
                     samples_per_item=spp, source="rays", max_bounces=20, background=(0.001, 0.001, 0.001), seed=1, sample_begin=s,
                     sample_end=s + 1, accumulate=s > 0, mis=mis, pick=pick_arg)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
frame = d_sum.view(h, w, 3).cpu().numpy()
trt.Image(frame).save("nee_frame.png")
print(f"{w}x{h}, {spp} spp in {spp} passes: {int(ctr[1])} rays of {int(ctr[0])} samples in {dt * 1e3:.1f} ms, mean {float(frame.mean()):.4f} "
      "-> nee_frame.png")
if export:
    d_records = torch.zeros(n * spp * 3, dtype=torch.float32, device="cuda:0")
    d_sum2, d_m22 = torch.zeros_like(d_sum), torch.zeros_like(d_m2)
    ctr2 = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(spp):
        camera.primary_rays_device(s, spp, d_rays.data_ptr(), seed=1)
        scene.nee_samples_device(d_rays.data_ptr(), n, d_table.data_ptr(), len(table), d_records.data_ptr(), d_counters_ptr=ctr2.data_ptr(),
                                 samples_per_item=spp, source="rays", max_bounces=20, background=(0.001, 0.001, 0.001), seed=1, sample_begin=s,
                                 sample_end=s + 1, mis=mis, pick=pick_arg)
        trt.fold_samples_device(d_records.data_ptr(), n, spp, d_sum2.data_ptr(), d_m22.data_ptr(), sample_begin=s, sample_end=s + 1, accumulate=s > 0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert bool((d_sum2.view(torch.int32) == d_sum.view(torch.int32)).all()) and bool((d_m22.view(torch.int32) == d_m2.view(torch.int32)).all()), \
        "the folded records are not the frame"
    assert ctr2.tolist() == ctr.tolist()
    print(f"--export: {n * spp} records in {spp} passes, folded pass by pass, in {dt * 1e3:.1f} ms: the frame and the counters of before, by bits")
