#!/usr/bin/env python3
"""Scene compile time, host compiler vs device compiler (trt_scene_create_on_device), one JSON line per scene:
  host_s            trt_scene_create_ex, median of 3
  device_s          trt_scene_create_on_device returning (end to end), median of 3 after one warm-up device build
  device_kernels_ms the device passes alone (HIP events from the first kernel to the last packing copy, trt_kernel_timing_*)
  device_rest_ms    device_s - kernels: geometry upload, copy-back of the blob and node dumps, host layout work
  bytes_equal       Scene.packed() of both are the same bytes
  python tools/scene_build_time.py [--out profiles/scene_build_device.json] [--only NAME] [--device-only]
Per-kernel and per-copy times: run it under rocprofv3 --kernel-trace --memory-copy-trace --stats with --only --device-only."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = [("cornell", "cornell", ()), ("random_spheres", "random_spheres", ()), ("sphere_grid100k", "sphere_grid", (100000,)),
          ("sphere_field1m", "sphere_field", (1_000_000,)), ("sphere_field4m", "sphere_field", (4_000_000,))]


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--device-only", action="store_true", help="one warm-up and one timed device build, no host builds (for a trace)")
    a = ap.parse_args()
    import tinyrt_amd as trt
    trt._lib.check(trt.lib.trt_set_device(0))
    rows = []
    for name, gen, args in SCENES:
        if a.only and name != a.only:
            continue
        world, _ = trt.world_from_description(getattr(trt.scenes, gen)(*args))
        n = world.num_geometries()
        if a.device_only:
            trt.Scene(world, on_device=True)
            dt, _ = timed(lambda: trt.Scene(world, on_device=True))
            row = {"scene": name, "primitives": n, "device_s": round(dt, 5)}
        else:
            host_times, host = [], None
            for _ in range(3):
                dt, host = timed(lambda: trt.Scene(world))
                host_times.append(dt)
            dev = trt.Scene(world, on_device=True)                   # warm-up (module load, first allocations)
            del dev
            dev_times, kern = [], []
            for _ in range(3):
                trt._lib.check(trt.lib.trt_kernel_timing_begin())
                dt, dev = timed(lambda: trt.Scene(world, on_device=True))
                ms, cnt = C.c_double(), C.c_uint32()
                trt._lib.check(trt.lib.trt_kernel_timing_end(C.byref(ms), C.byref(cnt)))
                dev_times.append(dt)
                kern.append(ms.value)
            host_s, dev_s, kern_ms = statistics.median(host_times), statistics.median(dev_times), statistics.median(kern)
            row = {"scene": name, "primitives": n, "host_s": round(host_s, 5), "device_s": round(dev_s, 5),
                   "device_kernels_ms": round(kern_ms, 3), "device_rest_ms": round(1e3 * dev_s - kern_ms, 3),
                   "speedup": round(host_s / dev_s, 2), "device_bytes": host.info()["device_bytes"],
                   "bytes_equal": bool((host.packed() == dev.packed()).all())}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        json.dump({"_about": "tools/scene_build_time.py: host vs device scene compile, one MI355X, same process",
                   "host_threads": min(16, os.cpu_count() or 1), "scenes": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
