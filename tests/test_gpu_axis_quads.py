"""Axis-exact quads on the GPU (axis_quads.h; rt_path.h axis_quads_to_lds, trav_leaf): scenes whose quads are all axis-aligned run the
two-dot-product inside test on rewritten LDS records in the production lock-step kernel, and give the CPU oracle's frame bit for
bit - which is also the counting kernel's (generic test, with the oracle's counters), the megakernel's (generic test) and the frame
of the same kernel with TRT_AXIS_QUADS=0.  A scene with one rotated quad keeps the generic test and the oracle's frame.  The switch is
read once when the library loads, so every environment variant renders in a fresh child process under its own time limit.  The one
slow step is a fixture: the C++-loops build of the library (its six sources compiled side by side, about ten seconds), which no other file
of a clean checkout provides."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
from test_gpu_flat_reuse import MATS, SCENES as REUSE_SCENES, _scene, box_stacks
from test_gpu_parity import STAT_KEYS, assert_bit_equal
from test_gpu_walk_rays import CSRC, HIPCC, library_cxxflags

pytestmark = pytest.mark.gpu
MEGAKERNEL, STREAMED = 1, 3
WALK_FLAT = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
assert [m[0] for m in MATS] == ["white", "red", "metal", "glass", "light"]


def twelve_combinations(trt, w=88, h=80):
    """Twelve quads, each with another (normal axis, u / v order, sign of u, sign of v): a closed box of six faces at +-10 (the top
    one a light) and six panels floating at +-6 inside it, seen from inside."""
    geos = []
    signs = [(1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0)]
    combos = set()
    for k in range(12):
        a, level, order = k % 3, k // 3, (k // 3) % 2
        su, sv = signs[k % 4]
        plane = (-10.0, 10.0, -6.0, 6.0)[level]
        half = 10.0 if level < 2 else 4.0
        b, c = (a + 1) % 3, (a + 2) % 3
        ub, vc = (b, c) if order == 0 else (c, b)                        # which in-plane axis u runs along, and v
        u, v, corner = [0.0] * 3, [0.0] * 3, [0.0] * 3
        u[ub], v[vc] = su * 2.0 * half, sv * 2.0 * half
        corner[a], corner[ub], corner[vc] = plane, -su * half, -sv * half
        mat = "light" if (a, level) == (1, 1) else ("white", "red", "metal", "glass")[(k + level) % 4] if level >= 2 else ("white", "red")[k % 2]
        geos.append(("quad", tuple(corner), tuple(u), tuple(v), mat))
        combos.add((a, order, su, sv))
    assert len(combos) == 12
    cam = dict(focus_distance=9.0, defocus_angle=0.0, position=(7.5, 2.0, -8.5), look_at=(-2.0, -1.0, 3.0), up=(0.0, 1.0, 0.0),
               vertical_fov=70.0, width=w, height=h)
    return _scene(trt, "twelve_combinations", geos, cam)


def box_stacks_rotated(trt):
    """box_stacks plus one quad turned by a milliradian about z: not axis-exact, so the whole scene keeps the generic test."""
    desc = box_stacks(trt)
    a = 1e-3
    desc["geometries"] = desc["geometries"] + [("quad", (22.0, 0.0, -5.0), (8.0 * math.cos(a), 8.0 * math.sin(a), 0.0), (0.0, 0.0, 8.0), "metal")]
    desc["name"] = "box_stacks_rotated"
    return desc


SCENES = {"cornell": lambda trt: trt.scenes.cornell(96, 96), "box_stacks": REUSE_SCENES["box_stacks"], "thin_sheets": REUSE_SCENES["thin_sheets"],
          "signed_zero_planes": REUSE_SCENES["signed_zero_planes"], "twelve_combinations": twelve_combinations,
          "box_stacks_rotated": box_stacks_rotated}
SPP, DEPTH, SEED = 16, 50, 9

# argv: repository root, scene name ("cornell2048": the bench frame), output .npy
CHILD = r"""
import os
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
trt = __import__("tiny-raytracer_amd")
if sys.argv[2] == "cornell2048":
    desc, spp, depth, seed = trt.scenes.cornell(2048, 2048), 8, 50, 7
else:
    import test_gpu_axis_quads as T
    desc, spp, depth, seed = T.SCENES[sys.argv[2]](trt), T.SPP, T.DEPTH, T.SEED
pw, pcam = trt.world_from_description(desc)
r = trt.Renderer(spp, 1, depth, False, desc["background"], seed=seed, backend=3)
np.save(sys.argv[3], r.render(pcam, pw).data)
"""


def child_frame(tmp_path, scene, tag, **env):
    """The production (streamed) frame of `scene` from a fresh process with `env` on top of the current environment."""
    out = tmp_path / f"{scene}_{tag}.npy"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, scene, str(out)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def oracle_frames(trt, orc):
    """scene name -> (description, oracle frame, oracle counters); each rendered once."""
    cache = {}

    def get(scene):
        if scene not in cache:
            desc = SCENES[scene](trt)
            ow, ocam = orc.world_from_description(desc)
            cpu, cst = orc.render(ow, ocam, SPP, DEPTH, desc["background"], seed=SEED, nthreads=8)
            cpu.setflags(write=False)
            cache[scene] = (desc, cpu, cst)
        return cache[scene]
    return get


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_production_kernel_equals_oracle_counting_kernel_megakernel_and_switch_off(trt, oracle_frames, tmp_path, scene):
    desc, cpu, cst = oracle_frames(scene)
    assert len(desc["geometries"]) <= 32
    pw, pcam = trt.world_from_description(desc)
    r = trt.Renderer(SPP, 1, DEPTH, False, desc["background"], seed=SEED, backend=STREAMED)
    plan = r.launch_plan(pcam, pw.get_bvh())
    assert plan["walk"] == WALK_FLAT and plan["kernel_walk"] == WALK_FLAT, plan
    plain = r.render(pcam, pw)                                          # production kernel: the switch is on wherever the scene allows it
    assert_bit_equal(plain.data, cpu, f"{scene}: production kernel vs oracle")
    counted = r.render(pcam, pw, collect_stats=2)                       # counting kernel, lock-step walk: always the generic test
    assert_bit_equal(counted.data, cpu, f"{scene}: counting kernel (lock-step walk) vs oracle")
    st = r.last_stats
    assert st["rays"] == cst["rays"], scene
    for k in ("samples", "sphere_tests", "quad_plane_tests", "quad_inside_tests", "shades"):
        assert st[k] == cst[k], (scene, k)
    ref = r.render(pcam, pw, collect_stats=1)                            # the reference tree: every counter the oracle's
    assert_bit_equal(ref.data, cpu, f"{scene}: reference-tree counting kernel vs oracle")
    for k in STAT_KEYS:
        assert r.last_stats[k] == cst[k], (scene, k)
    mega = trt.Renderer(SPP, 1, DEPTH, False, desc["background"], seed=SEED, backend=MEGAKERNEL).render(pcam, pw)
    assert_bit_equal(plain.data, mega.data, f"{scene}: production kernel vs megakernel")
    off = child_frame(tmp_path, scene, "off", TRT_AXIS_QUADS="0")
    assert_bit_equal(plain.data, off, f"{scene}: production kernel vs TRT_AXIS_QUADS=0")
    on = child_frame(tmp_path, scene, "on", TRT_AXIS_QUADS="1")
    assert_bit_equal(on, cpu, f"{scene}: production kernel in a fresh process (TRT_AXIS_QUADS=1) vs oracle")


def test_device_compiled_scene_takes_the_switch_too(trt, oracle_frames):
    """The switch is derived from the host copy of the blob, which the device scene compiler leaves as well: same frame."""
    desc, cpu, _ = oracle_frames("twelve_combinations")
    pw, pcam = trt.world_from_description(desc)
    r = trt.Renderer(SPP, 1, DEPTH, False, desc["background"], seed=SEED, backend=STREAMED)
    assert_bit_equal(r.render(pcam, pw.get_bvh(on_device=True)).data, cpu, "device-compiled scene vs oracle")


def test_cornell_2048_switch_on_equals_off(tmp_path):
    """The bench frame size, one step of 8 spp: the frame with the switch on is the frame with TRT_AXIS_QUADS=0, bit for bit."""
    on = child_frame(tmp_path, "cornell2048", "on", TRT_AXIS_QUADS="1")
    off = child_frame(tmp_path, "cornell2048", "off", TRT_AXIS_QUADS="0")
    assert on.shape == (2048, 2048, 3) and np.any(on > 0)
    assert_bit_equal(on, off, "Cornell 2048x2048, 8 spp: switch on vs TRT_AXIS_QUADS=0")


@pytest.fixture(scope="module")
def cxxloops_library(tmp_path_factory):
    """The library with the C++ box-step loops (-DTRT_ASM_BOX_LOOP=0, what `make cxxloops` builds), its sources compiled side by side."""
    out = tmp_path_factory.mktemp("cxxloops")
    with open(os.path.join(CSRC, "Makefile")) as f:
        src = next(line.split("=", 1)[1].split() for line in f if line.startswith("SRC"))
    objs, procs = [], []
    for s in src:
        objs.append(str(out / (s + ".o")))
        procs.append(subprocess.Popen([HIPCC, "--offload-arch=gfx950", *library_cxxflags(), "-DTRT_ASM_BOX_LOOP=0", "-c", os.path.join(CSRC, s), "-o", objs[-1]]))
    codes = [p.wait(timeout=900) for p in procs]
    assert codes == [0] * len(src), "the C++-loops build does not compile"
    lib = str(out / "libtinyrt_cxxloops.so")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs], check=True, timeout=900)
    return lib


def test_cornell_on_the_cxx_loops_build(oracle_frames, cxxloops_library, tmp_path):
    """The same switch in the build whose lock-step walk is the C++ loop: Cornell 96 x 96 is the oracle's frame, switch on and off."""
    _, cpu, _ = oracle_frames("cornell")
    on = child_frame(tmp_path, "cornell", "cxx_on", TRT_LIB_PATH=cxxloops_library, TRT_AXIS_QUADS="1")
    assert_bit_equal(on, cpu, "Cornell 96x96, C++ loops, switch on vs oracle")
    off = child_frame(tmp_path, "cornell", "cxx_off", TRT_LIB_PATH=cxxloops_library, TRT_AXIS_QUADS="0")
    assert_bit_equal(off, cpu, "Cornell 96x96, C++ loops, TRT_AXIS_QUADS=0 vs oracle")
