"""The lock-step kernel compiled per scene at run time (flat_literal.h, streamed.hip; TRT_FLAT_LITERAL) on the GPU, against the CPU oracle
bit for bit.  The switch is read once when the library loads, so each setting renders in ONE fresh child process that renders every scene
of its setting and hands back frames, device counters and the library's count of compilations: TRT_FLAT_LITERAL=1 (every scene
compiles at its first streamed render), =0 and unset (nothing compiles at these sizes), and =1 with the test switch that hands the
compiler an empty source (the render falls back to the built-in kernel and says so in the diagnostic, not in the result).
Frames are 16 x 16 at 4 spp, depth 50; Cornell also 64 x 64 at 8 spp in the bands of two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
from test_gpu_flat_reuse import _scene
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
STREAMED, WALK_FLAT = 3, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPP, DEPTH, SEED, W, H = 4, 50, 11, 16, 16


def _cam(pos, at, fov=60.0, focus=10.0):
    return dict(focus_distance=focus, defocus_angle=0.0, position=pos, look_at=at, up=(0.0, 1.0, 0.0), vertical_fov=fov, width=W, height=H)


def one_quad(trt):
    return _scene(trt, "one_quad", [("quad", (-2.0, -2.0, 5.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0), "light")], _cam((0.0, 0.0, -4.0), (0.0, 0.0, 5.0)),
                  background=(0.4, 0.5, 0.6))


def three_quads(trt):
    """An odd tail: the last pair of the box loop has one leaf."""
    geos = [("quad", (-4.0, -2.0, -4.0), (8.0, 0.0, 0.0), (0.0, 0.0, 12.0), "white"), ("quad", (-4.0, -2.0, 8.0), (8.0, 0.0, 0.0), (0.0, 8.0, 0.0), "metal"),
            ("quad", (-2.0, 5.0, 1.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), "light")]
    return _scene(trt, "three_quads", geos, _cam((0.0, 1.0, -6.0), (0.0, 0.0, 4.0)), background=(0.2, 0.2, 0.3))


def thirty_two_quads(trt):
    """The longest list the walk takes: a floor of 5 x 5 tiles (coplanar, rows share their z planes, columns their x planes), four
    standing sheets, two shelves and a light."""
    geos = []
    for i in range(5):
        for j in range(5):
            geos.append(("quad", (-5.0 + 2.0 * i, 0.0, 2.0 * j), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), "white" if (i + j) % 2 else "red"))
    for k in range(4):
        geos.append(("quad", (-5.0 + 2.5 * k, 0.0, 9.0 - k), (2.5, 0.0, 0.0), (0.0, 4.0, 0.0), ("metal", "glass")[k % 2]))
    geos += [("quad", (-5.0, 2.0, 3.0), (0.0, 0.0, 4.0), (0.0, 2.0, 0.0), "red"), ("quad", (5.0, 2.0, 3.0), (0.0, 0.0, 4.0), (0.0, 2.0, 0.0), "metal"),
             ("quad", (-2.0, 7.0, 3.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), "light")]
    assert len(geos) == 32
    return _scene(trt, "thirty_two_quads", geos, _cam((0.0, 4.0, -7.0), (0.0, 1.0, 5.0)), background=(0.1, 0.1, 0.15))


def coplanar_and_signed_zero(trt):
    """Quads on the planes x, y, z = +0 / -0 seen from a camera on x = 0 and y = 0, in front of four coplanar tiles."""
    geos = [("quad", (0.0, -4.0, 2.0), (0.0, 8.0, 0.0), (0.0, 0.0, 6.0), "red"), ("quad", (-0.0, -4.0, 2.0), (-0.0, 8.0, -0.0), (0.0, 0.0, 6.0), "white"),
            ("quad", (-4.0, 0.0, 2.0), (8.0, 0.0, 0.0), (0.0, 0.0, 6.0), "metal"), ("quad", (-4.0, -0.0, 2.0), (8.0, -0.0, 0.0), (0.0, -0.0, 6.0), "white"),
            ("quad", (-3.0, -3.0, 0.0), (3.0, 0.0, 0.0), (0.0, 3.0, 0.0), "glass"), ("quad", (0.0, 0.0, -0.0), (3.0, 0.0, 0.0), (0.0, 3.0, -0.0), "glass")]
    for i in range(2):
        for j in range(2):
            geos.append(("quad", (-6.0 + 6.0 * i, -6.0 + 6.0 * j, 9.0), (6.0, 0.0, 0.0), (0.0, 6.0, 0.0), "white" if (i + j) % 2 else "red"))
    geos.append(("quad", (-2.0, 5.0, 3.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), "light"))
    return _scene(trt, "coplanar_and_signed_zero", geos, _cam((0.0, 0.0, -8.0), (0.0, 0.0, 4.0), focus=8.0), background=(0.3, 0.3, 0.4))


def wide_room(trt):
    """A closed room 2000 wide with ten glass and metal sheets across it: every ray's box passes for most leaves, and with two leaf slots
    per lane the box loop is left behind nearly every pair and entered again through the all-axes copies."""
    geos = trt.scenes._box((-1000.0, 0.0, -20.0), (1000.0, 40.0, 60.0), "white")
    for k in range(10):
        geos.append(("quad", (-1000.0, 0.0, 5.0 + 4.0 * k), (2000.0, 0.0, 0.0), (0.0, 40.0, 0.0), "glass" if k % 3 else "metal"))
    geos.append(("quad", (-900.0, 39.0, -10.0), (1800.0, 0.0, 0.0), (0.0, 0.0, 60.0), "light"))
    return _scene(trt, "wide_room", geos, _cam((0.0, 20.0, -15.0), (300.0, 15.0, 60.0), fov=80.0, focus=30.0))


def quads_and_a_sphere(trt):
    """A lock-step scene with one sphere: the generic leaf phase behind the specialised box phase."""
    geos = trt.scenes._box((-5.0, 0.0, 0.0), (5.0, 10.0, 10.0), "white")
    geos += [("sphere", (0.0, 3.0, 5.0), 2.0, "glass"), ("quad", (-2.0, 9.9, 3.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), "light")]
    return _scene(trt, "quads_and_a_sphere", geos, _cam((0.0, 5.0, 0.5), (0.0, 3.0, 5.0), fov=75.0, focus=5.0))


SCENES = {"cornell": lambda trt: trt.scenes.cornell(W, H), "one_quad": one_quad, "three_quads": three_quads, "thirty_two_quads": thirty_two_quads,
          "coplanar_and_signed_zero": coplanar_and_signed_zero, "wide_room": wide_room, "quads_and_a_sphere": quads_and_a_sphere}
TUNING = {"wide_room": {"leaf_slots": 2}}
BANDS = [dict(band_rows=8, band_stride=2, band_offset=k, rows_local=32) for k in (0, 1)]      # two ranks' rows of a 64-row frame

# argv: repository root, output .npz, scene names ...  ("bands": Cornell 64 x 64, 8 spp, one frame per rank; every scene is rendered twice)
CHILD = r"""
import ctypes
import os
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
trt = __import__("tiny-raytracer_amd")
import test_gpu_flat_literal as T
count = trt.lib.trt_flat_literal_compilations
count.restype, count.argtypes = ctypes.c_uint64, []
diag = trt.lib.trt_flat_literal_diagnostic
diag.restype, diag.argtypes = ctypes.c_char_p, []
out = {}
for name in sys.argv[3:]:
    before = count()
    if name == "bands":
        desc = trt.scenes.cornell(64, 64)
        pw, pcam = trt.world_from_description(desc)
        scene = pw.get_bvh()
        r = trt.Renderer(8, 1, T.DEPTH, False, desc["background"], seed=T.SEED, backend=T.STREAMED)
        for k, band in enumerate(T.BANDS):
            out["bands_frame%d" % k] = r.render(pcam, scene, **band).data
    else:
        desc = T.SCENES[name](trt)
        pw, pcam = trt.world_from_description(desc)
        scene = pw.get_bvh()
        r = trt.Renderer(T.SPP, 1, T.DEPTH, False, desc["background"], seed=T.SEED, backend=T.STREAMED)
        r.tuning = dict(T.TUNING.get(name, {}))
        plan = r.launch_plan(pcam, scene)
        assert plan["walk"] == T.WALK_FLAT and plan["kernel_walk"] == T.WALK_FLAT, plan
        out[name + "_frame"] = r.render(pcam, scene).data
        out[name + "_counters"] = np.array([r.last_stats["samples"], r.last_stats["rays"]], np.uint64)
        out[name + "_again"] = r.render(pcam, scene).data              # the same scene handle: nothing compiles a second time
    out[name + "_compilations"] = np.array([count() - before], np.uint64)
out["diagnostic"] = np.array([diag().decode()])
np.savez(sys.argv[2], **out)
"""


def run_child(tmp_path_factory, tag, names, **env):
    out = tmp_path_factory.mktemp("flat_literal_" + tag) / "out.npz"
    e = {k: v for k, v in os.environ.items() if k not in ("TRT_FLAT_LITERAL", "TRT_FLAT_LITERAL_TEST_FAIL")}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(out), *names], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def literal_on(tmp_path_factory):
    return run_child(tmp_path_factory, "on", sorted(SCENES) + ["bands"], TRT_FLAT_LITERAL="1")


@pytest.fixture(scope="module")
def literal_off(tmp_path_factory):
    return run_child(tmp_path_factory, "off", ["cornell", "bands"], TRT_FLAT_LITERAL="0")


@pytest.fixture(scope="module")
def oracle_frames(trt, orc):
    cache = {}

    def get(scene):
        if scene not in cache:
            desc = SCENES[scene](trt)
            assert len(desc["geometries"]) <= 32
            ow, ocam = orc.world_from_description(desc)
            cpu, cst = orc.render(ow, ocam, SPP, DEPTH, desc["background"], seed=SEED, nthreads=8)
            cpu.setflags(write=False)
            cache[scene] = (cpu, cst)
        return cache[scene]
    return get


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_compiled_kernel_gives_the_oracles_frame_and_ray_counts(literal_on, oracle_frames, scene):
    cpu, cst = oracle_frames(scene)
    assert literal_on["diagnostic"][0] == "", literal_on["diagnostic"][0]     # every scene really compiled: no fallback rendered these frames
    assert int(literal_on[scene + "_compilations"][0]) == 1, "one scene rendered twice compiles once"
    assert_bit_equal(literal_on[scene + "_frame"], cpu, f"{scene}: kernel compiled for the scene vs oracle")
    assert_bit_equal(literal_on[scene + "_again"], cpu, f"{scene}: second render vs oracle")
    samples, rays = (int(v) for v in literal_on[scene + "_counters"])
    assert (samples, rays) == (cst["samples"], cst["rays"]), scene
    assert np.any(cpu > 0)


def test_cornell_bands_equal_the_unspecialised_render(literal_on, literal_off):
    assert int(literal_on["bands_compilations"][0]) == 1 and int(literal_off["bands_compilations"][0]) == 0
    for k in range(len(BANDS)):
        on, off = literal_on["bands_frame%d" % k], literal_off["bands_frame%d" % k]
        assert on.shape == (32, 64, 3) and np.any(on > 0)
        assert on.tobytes() == off.tobytes(), f"band {k}: compiled kernel vs built-in kernel"


def test_switched_off_and_auto_at_these_sizes_compile_nothing(literal_off, oracle_frames, tmp_path_factory):
    cpu, _ = oracle_frames("cornell")
    auto = run_child(tmp_path_factory, "auto", ["cornell", "bands"])          # unset: far below the auto threshold
    for got in (literal_off, auto):
        assert int(got["cornell_compilations"][0]) == 0 and int(got["bands_compilations"][0]) == 0
        assert got["diagnostic"][0] == ""
        assert_bit_equal(got["cornell_frame"], cpu, "built-in kernel vs oracle")


def test_a_failed_compilation_renders_the_same_frame_through_the_builtin_kernel(oracle_frames, tmp_path_factory):
    cpu, cst = oracle_frames("cornell")
    got = run_child(tmp_path_factory, "fail", ["cornell"], TRT_FLAT_LITERAL="1", TRT_FLAT_LITERAL_TEST_FAIL="1")
    assert int(got["cornell_compilations"][0]) == 1                           # tried once, not again for the second render
    assert "built-in kernel runs" in got["diagnostic"][0]
    assert_bit_equal(got["cornell_frame"], cpu, "fallback after a failed compilation vs oracle")
    assert_bit_equal(got["cornell_again"], cpu, "fallback, second render vs oracle")
    assert int(got["cornell_counters"][1]) == cst["rays"]
