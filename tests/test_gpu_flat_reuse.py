"""Interval reuse in the lock-step leaf walk (rt_path.h box_loop_flat, flat_reuse.h) against the CPU oracle: scenes of at most 32
primitives with many shared slab planes - Cornell, stacked boxes sharing faces, thin coplanar and parallel sheets that many rays
pass at once (the box loop is left and re-entered mid-list), planes at +-0 - give the oracle's frame bit for bit through the
production kernel (hand-written loop) and the counting kernel (C++ loop), with the oracle's counters; and a full-size Cornell frame
with reuse is the frame with TRT_FLAT_REUSE=0."""
import os
import subprocess
import sys

import numpy as np
import pytest
from test_gpu_parity import STAT_KEYS, assert_bit_equal

pytestmark = pytest.mark.gpu
STREAMED = 3
WALK_FLAT = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MATS = [("white", 0, (0.73, 0.73, 0.73), 0.0), ("red", 0, (0.65, 0.05, 0.05), 0.0), ("metal", 1, (0.8, 0.85, 0.88), 0.05),
        ("glass", 2, (1.0, 1.0, 1.0), 1.5), ("light", 3, (15.0, 15.0, 15.0), 0.0)]


def _scene(trt, name, geos, cam, background=(0.02, 0.02, 0.03)):
    mats = [(n, k, a, p) for n, k, a, p in MATS]
    kinds = {0: trt.scenes.LAMBERTIAN, 1: trt.scenes.METAL, 2: trt.scenes.DIELECTRIC, 3: trt.scenes.LIGHT}
    mats = [(n, kinds[k], a, p) for n, k, a, p in mats]
    return dict(name=name, materials=mats, geometries=geos, camera=cam, background=background)


def box_stacks(trt, w=96, h=80):
    """Four boxes stacked and side by side, sharing whole faces, on a floor under a light: 26 quads."""
    b = trt.scenes._box
    geos = b((0.0, 0.0, 0.0), (10.0, 10.0, 10.0), "white") + b((0.0, 10.0, 0.0), (10.0, 20.0, 10.0), "metal")
    geos += b((10.0, 0.0, 0.0), (20.0, 10.0, 10.0), "red") + b((0.0, 20.0, 0.0), (10.0, 30.0, 10.0), "glass")
    geos += [("quad", (-20.0, 0.0, -20.0), (60.0, 0.0, 0.0), (0.0, 0.0, 60.0), "white"),
             ("quad", (0.0, 45.0, 0.0), (10.0, 0.0, 0.0), (0.0, 0.0, 10.0), "light")]
    cam = dict(focus_distance=60.0, defocus_angle=0.0, position=(35.0, 25.0, -40.0), look_at=(8.0, 12.0, 5.0),
               up=(0.0, 1.0, 0.0), vertical_fov=45.0, width=w, height=h)
    return _scene(trt, "box_stacks", geos, cam)


def thin_sheets(trt, w=80, h=80):
    """Twelve parallel glass and metal sheets with the same x / y extent one behind another, seen face on, in front of a 4 x 4 grid
    of coplanar tiles, under a light: 29 quads.  A primary ray's box passes for most of them at once, so the leaf stack fills and
    the box loop is left and re-entered in the middle of the list."""
    geos = []
    for k in range(12):
        geos.append(("quad", (-5.0, -5.0, 2.0 + 0.5 * k), (10.0, 0.0, 0.0), (0.0, 10.0, 0.0), "glass" if k % 3 else "metal"))
    for i in range(4):
        for j in range(4):
            geos.append(("quad", (-8.0 + 4.0 * i, -8.0 + 4.0 * j, 12.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0), "white" if (i + j) % 2 else "red"))
    geos.append(("quad", (-3.0, 9.0, 4.0), (6.0, 0.0, 0.0), (0.0, 0.0, 6.0), "light"))
    cam = dict(focus_distance=10.0, defocus_angle=0.0, position=(0.0, 0.0, -12.0), look_at=(0.0, 0.0, 0.0),
               up=(0.0, 1.0, 0.0), vertical_fov=50.0, width=w, height=h)
    return _scene(trt, "thin_sheets", geos, cam, background=(0.5, 0.6, 0.7))


def signed_zero_planes(trt, w=64, h=64):
    """Quads whose corners sit on the planes x = +0 / -0, y = +0 / -0 and z = +0 / -0, seen from a camera on the x = 0 and y = 0
    planes (primary rays start with o.x = o.y = 0): 9 quads."""
    geos = [("quad", (0.0, -4.0, 2.0), (0.0, 8.0, 0.0), (0.0, 0.0, 6.0), "red"),
            ("quad", (-0.0, -4.0, 2.0), (-0.0, 8.0, -0.0), (0.0, 0.0, 6.0), "white"),
            ("quad", (-4.0, 0.0, 2.0), (8.0, 0.0, 0.0), (0.0, 0.0, 6.0), "metal"),
            ("quad", (-4.0, -0.0, 2.0), (8.0, -0.0, 0.0), (0.0, -0.0, 6.0), "white"),
            ("quad", (-3.0, -3.0, 0.0), (3.0, 0.0, 0.0), (0.0, 3.0, 0.0), "glass"),
            ("quad", (0.0, 0.0, -0.0), (3.0, 0.0, 0.0), (0.0, 3.0, -0.0), "glass"),
            ("quad", (-0.0, -3.0, 0.0), (3.0, 0.0, 0.0), (0.0, 3.0, 0.0), "metal"),
            ("quad", (-6.0, -6.0, 9.0), (12.0, 0.0, 0.0), (0.0, 12.0, 0.0), "white"),
            ("quad", (-2.0, 5.0, 3.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), "light")]
    cam = dict(focus_distance=8.0, defocus_angle=0.0, position=(0.0, 0.0, -8.0), look_at=(0.0, 0.0, 4.0),
               up=(0.0, 1.0, 0.0), vertical_fov=60.0, width=w, height=h)
    return _scene(trt, "signed_zero_planes", geos, cam, background=(0.3, 0.3, 0.4))


SCENES = {"cornell": lambda trt: trt.scenes.cornell(96, 96), "box_stacks": box_stacks, "thin_sheets": thin_sheets,
          "signed_zero_planes": signed_zero_planes}


@pytest.mark.parametrize("slots", [0, 2])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_flat_walk_with_reuse_equals_oracle(trt, orc, scene, slots):
    """slots 0: the launch plan's leaf stack; 2: a lane that put one leaf aside stops the box loop at the end of the pair, so the
    loop is re-entered after nearly every pair (the first box of every entry computes all three axes)."""
    desc = SCENES[scene](trt)
    spp, depth, seed = 6, 12, 5
    ow, ocam = orc.world_from_description(desc)
    cpu, cst = orc.render(ow, ocam, spp, depth, desc["background"], seed=seed, nthreads=8)
    pw, pcam = trt.world_from_description(desc)
    r = trt.Renderer(spp, 1, depth, False, desc["background"], seed=seed, backend=STREAMED)
    r.tuning = {"leaf_slots": slots}
    plan = r.launch_plan(pcam, pw.get_bvh())
    assert plan["walk"] == WALK_FLAT and plan["kernel_walk"] == WALK_FLAT, plan
    n_leaves = len(desc["geometries"])
    assert n_leaves <= 32
    plain = r.render(pcam, pw)                                          # production kernel: the hand-written loop
    assert_bit_equal(plain.data, cpu, f"{scene} slots {slots}: production kernel vs oracle")
    counted = r.render(pcam, pw, collect_stats=2)                       # counting kernel: the C++ loop, same schedule
    assert_bit_equal(counted.data, cpu, f"{scene} slots {slots}: counting kernel (lock-step walk) vs oracle")
    st = r.last_stats
    for k in ("samples", "rays", "sphere_tests", "quad_plane_tests", "quad_inside_tests", "shades"):
        assert st[k] == cst[k], (scene, slots, k)
    assert abs(st["node_tests"] - n_leaves * st["rays"]) < 1e-3 * st["node_tests"]     # every ray steps every leaf box (bar NaN-prone rays)
    ref = r.render(pcam, pw, collect_stats=1)                            # the reference tree: every counter the oracle's
    assert_bit_equal(ref.data, cpu, f"{scene} slots {slots}: reference-tree counting kernel vs oracle")
    for k in STAT_KEYS:
        assert r.last_stats[k] == cst[k], (scene, slots, k)


def test_device_compiled_scene_renders_the_same(trt, orc):
    """A scene compiled on the device carries the same reuse schedule (derived from the same bytes): same frame."""
    desc = box_stacks(trt, 64, 48)
    ow, ocam = orc.world_from_description(desc)
    cpu, _ = orc.render(ow, ocam, 4, 10, desc["background"], seed=2, nthreads=8)
    pw, pcam = trt.world_from_description(desc)
    r = trt.Renderer(4, 1, 10, False, desc["background"], seed=2, backend=STREAMED)
    img = r.render(pcam, pw.get_bvh(on_device=True))
    assert_bit_equal(img.data, cpu, "device-compiled scene vs oracle")


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
trt = __import__("tiny-raytracer_amd")
desc = trt.scenes.cornell(2048, 2048)
pw, pcam = trt.world_from_description(desc)
r = trt.Renderer(2, 1, 50, False, desc["background"], seed=7, backend=3)
np.save(sys.argv[2], r.render(pcam, pw).data)
"""


def test_cornell_2048_reuse_on_equals_off(trt, tmp_path):
    """The bench frame size: the frame with interval reuse (the default) is the frame with TRT_FLAT_REUSE=0 (every leaf box computed
    in full), bit for bit.  The switch is read once when the library loads, so each setting renders in a fresh child process."""
    frames = {}
    for reuse in ("1", "0"):
        out = tmp_path / f"frame_{reuse}.npy"
        env = dict(os.environ, TRT_FLAT_REUSE=reuse)
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        frames[reuse] = np.load(out)
    assert frames["1"].shape == (2048, 2048, 3)
    assert np.any(frames["1"] > 0)
    assert_bit_equal(frames["1"], frames["0"], "Cornell 2048x2048, reuse on vs TRT_FLAT_REUSE=0")
