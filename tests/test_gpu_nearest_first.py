"""The nearest-first leaf phase on the GPU (nearest_first.h; rt_path.h leaf_phase_nearest): on scenes of axis-exact quads only, the
production lock-step kernel tests the nearest pending leaf first and skips the others by the margin - and gives the CPU oracle's frame
bit for bit, which is also the frame of the same kernel with TRT_NEAREST_FIRST=0 (the walk-order phase).  With leaf_slots 2 and 3 a walk
has several phases with a finite carried t_best.  A scene with a sphere or a rotated quad keeps the walk-order phase and the oracle's
frame.  The closest-hit query runs the same walk: the recorded rays that take the residual loop and the walk-order re-run
(tests/golden/nearest_first_cold_rays.txt, written by tests/native/nearest_first_check.c) and the ray classes of walk_ray_cases get the
oracle's (t bits, geometry), also with a caller t_max between the first and the second hit.  The switch is read once when the library
loads, so every environment variant renders in a fresh child process under its own time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import walk_ray_cases as W
from test_gpu_axis_quads import SCENES as AQ_SCENES, child_frame
from test_gpu_parity import assert_bit_equal
from test_gpu_queries import MISS, oracle_records
from test_nearest_first import EXTRA_SCENES, recorded_cold_rays

pytestmark = pytest.mark.gpu
STREAMED, WALK_FLAT = 3, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPP, DEPTH, SEED = 16, 50, 9


def with_sphere(trt):
    desc = AQ_SCENES["box_stacks"](trt)
    return dict(desc, name="box_stacks_sphere", geometries=desc["geometries"] + [("sphere", (5.0, 36.0, 5.0), 3.0, "metal")])


SCENES = dict(AQ_SCENES, **EXTRA_SCENES)                  # cornell 96 x 96 ... box_stacks_rotated (switch off), and this pull request's five
SCENES["box_stacks_sphere"] = with_sphere                 # switch off
SWITCH_OFF = ("box_stacks_rotated", "box_stacks_sphere")

# argv: repository root, scene name, output .npy, leaf_slots (0: the plan's)
CHILD = r"""
import os
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
trt = __import__("tiny-raytracer_amd")
import test_gpu_nearest_first as T
desc = T.SCENES[sys.argv[2]](trt)
pw, pcam = trt.world_from_description(desc)
r = trt.Renderer(T.SPP, 1, T.DEPTH, False, desc["background"], seed=T.SEED, backend=3)
if int(sys.argv[4]):
    r.tuning = {"leaf_slots": int(sys.argv[4])}
np.save(sys.argv[3], r.render(pcam, pw).data)
"""


def switched_off_frame(tmp_path, scene, slots=0):
    """The production frame of `scene` from a fresh process with TRT_NEAREST_FIRST=0."""
    out = tmp_path / f"{scene}_{slots}_off.npy"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, scene, str(out), str(slots)], env=dict(os.environ, TRT_NEAREST_FIRST="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def oracle_frames(trt, orc):
    """scene name -> (description, oracle frame); each rendered once."""
    cache = {}

    def get(scene):
        if scene not in cache:
            desc = SCENES[scene](trt)
            ow, ocam = orc.world_from_description(desc)
            cpu, _ = orc.render(ow, ocam, SPP, DEPTH, desc["background"], seed=SEED, nthreads=8)
            cpu.setflags(write=False)
            cache[scene] = (desc, cpu)
        return cache[scene]
    return get


def production_frame(trt, desc, slots=0):
    pw, pcam = trt.world_from_description(desc)
    r = trt.Renderer(SPP, 1, DEPTH, False, desc["background"], seed=SEED, backend=STREAMED)
    if slots:
        r.tuning = {"leaf_slots": slots}
    plan = r.launch_plan(pcam, pw.get_bvh())
    assert plan["walk"] == WALK_FLAT and plan["specialised"] == 1, plan
    return r.render(pcam, pw).data


@pytest.mark.parametrize("scene", sorted(s for s in SCENES if s not in SWITCH_OFF))
def test_frame_equals_oracle_and_switch_off(trt, oracle_frames, tmp_path, scene):
    desc, cpu = oracle_frames(scene)
    frame = production_frame(trt, desc)
    assert_bit_equal(frame, cpu, f"{scene}: production kernel vs oracle")
    assert_bit_equal(frame, switched_off_frame(tmp_path, scene), f"{scene}: production kernel vs TRT_NEAREST_FIRST=0")
    assert np.any(cpu > 0) or scene == "far_room"                       # (far_room: the reference never reaches a quad without thickness)


@pytest.mark.parametrize("slots", [2, 3])
def test_cornell_with_several_phases_per_walk(trt, oracle_frames, tmp_path, slots):
    """leaf_slots 2 and 3: the box loop is left after nearly every pair, so most phases start from a finite (T0, P0)."""
    desc, cpu = oracle_frames("cornell")
    frame = production_frame(trt, desc, slots)
    assert_bit_equal(frame, cpu, f"Cornell, leaf_slots {slots}: production kernel vs oracle")
    assert_bit_equal(frame, switched_off_frame(tmp_path, "cornell", slots), f"Cornell, leaf_slots {slots}: production kernel vs TRT_NEAREST_FIRST=0")


@pytest.mark.parametrize("scene", SWITCH_OFF)
def test_scenes_without_the_switch_keep_the_oracles_frame(trt, oracle_frames, scene):
    desc, cpu = oracle_frames(scene)
    assert_bit_equal(production_frame(trt, desc), cpu, f"{scene}: production kernel vs oracle")


def rays_of(lines):
    return np.array([[int(w, 16) for w in l.split()[:6]] for l in lines], np.uint32).view(np.float32)


def check_queries(trt, orc, desc, rays, what):
    """intersect() against the oracle's closest hit: t bits and geometry index, for t_max = inf and for ends around the first two hits."""
    ow, _ = orc.world_from_description(desc)
    sc = trt.world_from_description(desc)[0].get_bvh()
    hit, t, geo = ow.hit_index_batch(rays)
    got = sc.intersect(rays)
    assert np.array_equal(got["geometry"] != MISS, hit), what
    assert np.array_equal(got["t"].view(np.uint32), t.view(np.uint32)), what
    assert np.array_equal(got["geometry"][hit].astype(np.int64), geo[hit].astype(np.int64)), what
    # the second hit: the oracle again from just behind the first
    hr = rays[hit]
    assert len(hr) >= 32, what
    t1 = t[hit]
    t2 = np.array([ow.hit_index_batch(r[None, :], t0=float(np.nextafter(a, np.float32(np.inf))))[1][0] for r, a in zip(hr, t1)], np.float32)
    between = np.where(np.isfinite(t2), (t1 + (t2 - t1) * np.float32(0.5)).astype(np.float32), (t1 * np.float32(2.0)).astype(np.float32))
    for name, tm in (("between the first and the second hit", between), ("just behind the first hit", np.nextafter(t1, np.float32(np.inf))),
                     ("the first hit itself", t1), ("the second hit itself", np.where(np.isfinite(t2), t2, np.float32(1e30)).astype(np.float32))):
        want, _ = oracle_records(trt, orc, ow, hr, tm)
        got = sc.intersect(hr, tm)
        assert np.array_equal(got["t"].view(np.uint32), want["t"].view(np.uint32)), (what, name)
        assert np.array_equal(got["geometry"], want["geometry"]), (what, name)
    return int(hit.sum())


def test_recorded_cold_path_rays_get_the_oracles_hit(trt, orc):
    """The 64 recorded rays that take the residual loop (Cornell) and the 64 that take the walk-order re-run (wide_room)."""
    rec = recorded_cold_rays()
    assert sorted(rec) == ["cornell", "wide_room"] and all(len(v) == 64 for v in rec.values())
    assert all(l.endswith(" 1") for l in rec["cornell"]) and all(l.endswith(" 2") for l in rec["wide_room"])
    for scene in rec:
        assert check_queries(trt, orc, SCENES[scene](trt), rays_of(rec[scene]), scene) >= 60


def test_walk_ray_cases_on_cornell_get_the_oracles_hit(trt, orc):
    desc = W.scene(trt, "cornell")
    ow, _ = orc.world_from_description(desc)
    bbox, prim, _ = ow.bvh_dump()
    classes = W.RayMaker(desc, bbox, prim).classes(48)
    rays = np.ascontiguousarray(np.concatenate(list(classes.values())).astype(np.float32))
    rays = rays[~np.isnan(rays).any(axis=1)]
    assert check_queries(trt, orc, desc, rays, "walk_ray_cases, Cornell") >= 100


def test_cornell_2048_switch_on_equals_off(tmp_path):
    """The bench frame size, one step of 8 spp: the frame with the switch on is the frame with TRT_NEAREST_FIRST=0, bit for bit."""
    on = child_frame(tmp_path, "cornell2048", "nf_on", TRT_NEAREST_FIRST="1")
    off = child_frame(tmp_path, "cornell2048", "nf_off", TRT_NEAREST_FIRST="0")
    assert on.shape == (2048, 2048, 3) and np.any(on > 0)
    assert_bit_equal(on, off, "Cornell 2048x2048, 8 spp: switch on vs TRT_NEAREST_FIRST=0")
