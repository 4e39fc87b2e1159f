#!/usr/bin/env python3
"""What a radiance query costs on the device, beside the ways the same paths can be traced.  Needs a GPU.

  make -C tiny-raytracer_amd/csrc plainwalk        (the second library: contender c)
  python tools/radiance_bench.py [--rounds 3] [--window-s 1.0] [--out profiles/radiance_bench.json]

Cornell at 1024 x 1024 and the 100 k-sphere grid at 1024 x 1024; the rays are the render's own for sample 0 (trt_primary_rays_device),
K = 16 samples per ray, max_bounces 50, seed 5.  Contenders, n x K paths each:
  a  trt_radiance_device                      the shipped kernel
  b  trt_render_pixels_device                 every pixel listed, 16 spp: as many paths through a kernel this change does not touch
  c  trt_radiance_device of build/libtinyrt_plainwalk.so: the same kernel with TRT_RADIANCE_PLAIN_WALK=1 - every sample walks its
     first segment instead of re-using the ray's first hit (on the lock-step list, Cornell, the shipped kernel does that too: a and c
     are then the same code)
  d  K calls of trt_sample_batch              what the job cost before: host buffers, an allocation per call, one sample per point
     (call k with seed 5 + k, so that the K samples differ; host-synchronous, copies included)
Before timing, a and c must leave the same bytes.  Timing: every contender is warmed, then timed in windows of at least --window-s
seconds of repeated calls between two device events (d: whole K-call jobs); the contenders alternate, --rounds windows each, in one
process; the figure is the median window.  Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K, DEPTH, SEED, SIDE = 16, 50, 5, 1024
PLAIN_LIB = os.path.join(ROOT, "build", "libtinyrt_plainwalk.so")


def load_second_library(trt, path):
    lib = C.CDLL(path)
    for name, (res, args) in trt._lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class RawWorld:
    """A world and its scene in a second copy of the library (handles of one copy are not handed to another)."""

    def __init__(self, trt, lib, desc):
        self.trt, self.lib = trt, lib
        self.w, self.scene = C.c_void_p(), C.c_void_p()
        self.ok(lib.trt_world_create(C.byref(self.w)))
        trt.scenes.build_world(desc, self, lambda kind, albedo, param: trt.Material(kind, trt.Vec3(*albedo), param),
                               lambda c, r, m: ("sphere", c, r, m), lambda c, u, v, m: ("quad", c, u, v, m))
        self.ok(lib.trt_scene_create(self.w, C.byref(self.scene)))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError("second library: %d %s" % (rc, self.lib.trt_last_error().decode()))

    def add_material(self, name, m):
        self.ok(self.lib.trt_world_add_material(self.w, name.encode(), C.byref(m)))

    def get_material(self, name):
        idx = C.c_uint32()
        self.ok(self.lib.trt_world_get_material(self.w, name.encode(), C.byref(idx)))
        return idx.value

    def add_geometry(self, g):
        V = self.trt.Vec3
        if g[0] == "sphere":
            self.ok(self.lib.trt_world_add_sphere(self.w, V(*g[1]), g[2], g[3]))
        else:
            self.ok(self.lib.trt_world_add_quad(self.w, V(*g[1]), V(*g[2]), V(*g[3]), g[4]))

    def add_spheres(self, cr, mat):
        cr = np.ascontiguousarray(cr, np.float32).reshape(-1, 4)
        mat = np.ascontiguousarray(mat, np.uint32)
        self.ok(self.lib.trt_world_add_spheres(self.w, len(cr), cr.ctypes.data, mat.ctypes.data))

    def close(self):
        self.lib.trt_scene_destroy(self.scene)
        self.lib.trt_world_destroy(self.w)


def window(torch, call, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def bench_scene(trt, torch, lib2, name, desc, args):
    dev = torch.device("cuda:0")
    world, cam = trt.world_from_description(desc)
    scene = world.get_bvh()
    n = SIDE * SIDE
    bg = tuple(desc["background"])
    d_rays = torch.zeros(n * 6, dtype=torch.float32, device=dev)
    cam.primary_rays_device(0, K, d_rays.data_ptr(), seed=SEED)
    d_s, d_m, d_s2, d_m2 = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(4))
    ctr = torch.zeros(16, dtype=torch.int64, device=dev)
    kw = dict(samples_per_ray=K, max_bounces=DEPTH, background=bg, seed=SEED)
    p = scene._radiance_params(**kw)
    raw = RawWorld(trt, lib2, desc)
    r = trt.Renderer(K, 1, DEPTH, False, bg, seed=SEED)
    d_list = torch.arange(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    h_rays = d_rays.cpu().numpy().reshape(n, 6)
    points = np.zeros(n, np.dtype([("x", np.uint32), ("y", np.uint32), ("ray", np.float32, (6,))]))
    points["ray"] = h_rays
    h_points = (trt.SamplePoint * n).from_buffer(points)
    h_out = (trt.SampledColor * n)()

    def a(counters=0):
        scene.radiance_device(d_rays.data_ptr(), n, d_s.data_ptr(), d_m.data_ptr(), d_counters_ptr=counters, **kw)

    def b(counters=0):
        r.render_pixels_device(cam, scene, d_list.data_ptr(), n, d_s2.data_ptr(), d_m2.data_ptr(), d_counters_ptr=counters)

    def c(counters=None):
        raw.ok(lib2.trt_radiance_device(raw.scene, C.c_void_p(d_rays.data_ptr()), n, C.byref(p), C.c_void_p(d_s2.data_ptr()),
                                        C.c_void_p(d_m2.data_ptr()), counters, None))

    def d():
        for k in range(K):
            trt._lib.check(trt.lib.trt_sample_batch(scene._h, C.byref(h_points), n, C.byref(h_out), DEPTH, trt.Vec3(*bg), SEED + k, None))

    # the two forms of the new kernel leave the same bytes
    ctr_c = torch.zeros(16, dtype=torch.int64, device=dev)
    a(ctr.data_ptr())
    c(C.c_void_p(ctr_c.data_ptr()))
    torch.cuda.synchronize()
    if not (torch.equal(d_s.view(torch.int32), d_s2.view(torch.int32)) and torch.equal(d_m.view(torch.int32), d_m2.view(torch.int32))):
        raise SystemExit("%s: the plain-walk build differs from the shipped kernel" % name)
    rays = {"a": int(ctr[1]), "c": int(ctr_c[1])}
    ctr.zero_()
    b(ctr.data_ptr())
    torch.cuda.synchronize()
    rays["b"] = int(ctr[1])
    # d: call k traces streams (seed 5 + k, j, 0) - a K = 1 radiance query from stream 0 with that seed (bit for bit: tests/test_gpu_radiance.py)
    ctr.zero_()
    for k in range(K):
        scene.radiance_device(d_rays.data_ptr(), n, d_s2.data_ptr(), d_counters_ptr=ctr.data_ptr(), samples_per_ray=1, max_bounces=DEPTH,
                              background=bg, seed=SEED + k)
    torch.cuda.synchronize()
    rays["d"] = int(ctr[1])

    calls = {"a": a, "b": b, "c": c, "d": d}
    reps, windows = {}, {k: [] for k in calls}
    for key, call in calls.items():                                         # warm-up and the repetitions of a window
        call()
        torch.cuda.synchronize()
        once = window(torch, call, 1)
        reps[key] = max(1, int(np.ceil(1000.0 * args.window_s / once)))
    for _ in range(args.rounds):
        for key, call in calls.items():
            windows[key].append(window(torch, call, reps[key]))
    raw.close()
    plan = scene.radiance_plan(n)
    out = {"rays_in_batch": n, "paths_per_job": n * K,
           "plan": {k: plan[k] for k in ("scene_mode", "walk", "threads_per_workgroup", "kernel_waves_per_simd", "workgroups_per_cu", "rays_per_wave",
                                         "workgroups")}}
    names = {"a": "radiance_device", "b": "render_pixels_device_all_pixels", "c": "radiance_device_plain_walk", "d": "sample_batch_x%d" % K}
    med = {}
    for key in calls:
        ms = sorted(windows[key])
        med[key] = ms[len(ms) // 2]
        out[names[key]] = {"ms_per_job_median": round(med[key], 3), "ms_per_job_min": round(ms[0], 3), "ms_per_job_max": round(ms[-1], 3),
                           "jobs_per_window": reps[key], "windows": len(ms), "mpaths_per_s": round(n * K / med[key] / 1e3, 2),
                           "reference_rays": rays[key], "reference_mrays_per_s": round(rays[key] / med[key] / 1e3, 2)}
    for x, y in (("a", "b"), ("a", "c"), ("a", "d")):
        out["time_%s_over_%s" % (x, y)] = round(med[x] / med[y], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3 or args.window_s < 1.0:
        ap.error("at least 3 windows of at least 1 s per contender")
    if not os.path.exists(PLAIN_LIB):
        raise SystemExit(PLAIN_LIB + " is missing: make -C tiny-raytracer_amd/csrc plainwalk")
    import torch
    trt = importlib.import_module("tiny-raytracer_amd")
    trt._lib.check(trt.lib.trt_set_device(0))
    lib2 = load_second_library(trt, PLAIN_LIB)
    out = {"metric": "ms per job of n x K paths (device events around a window of jobs, median window)", "rounds": args.rounds,
           "window_s": args.window_s, "device": torch.cuda.get_device_name(0), "library": os.path.basename(trt._lib.LIB_PATH),
           "samples_per_ray": K, "max_bounces": DEPTH, "seed": SEED, "width": SIDE, "height": SIDE,
           "ratios": "time_x_over_y = median ms of x / median ms of y: below 1, x is faster"}
    for name, desc in (("cornell", trt.scenes.cornell(SIDE, SIDE)), ("sphere_grid_100k", trt.scenes.sphere_grid(100000, SIDE, SIDE))):
        out[name] = bench_scene(trt, torch, lib2, name, desc, args)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    sys.exit(main())
