"""The interval cache of the lock-step kernel compiled per scene (flat_literal.h flat_literal_cached_asm; TRT_FLAT_LITERAL_PAIRS,
TRT_FLAT_LITERAL_PLANES) on the GPU, against the CPU oracle bit for bit.  The settings are read once when the library loads, so each one -
(3, 0): no cache, (4, 0), (8, 0), (8, 6) and the library's default - renders in ONE fresh child process with TRT_FLAT_LITERAL=1 (every scene
compiles its kernel at its first render).  Scenes, child script and frame size (16 x 16, 4 spp, depth 50) are those of
tests/test_gpu_flat_literal.py: one quad, three quads (an unpaired last leaf), 32 quads whose tiles share planes far apart in walk order,
coplanar and signed-zero planes, quads and a sphere, Cornell, and the wide room at two leaf slots per lane, which leaves the cached stream at
a stack-full ballot behind nearly every pair and comes back through the entry table.  What the generator does with each scene's own leaf
list at each setting - a cached stream at all, evictions, reuse from further back than the previous leaf - is asserted from its statistics
(the native checker, tests/native/flat_cache_check.cpp, on the list the product packs), so that a frame that matches is known to have come
through the code it is here for."""
import os
import subprocess
import sys

import numpy as np
import pytest
import test_gpu_flat_literal as T
from test_flat_literal_gen import leaves_of
from test_gpu_flat_literal import oracle_frames  # noqa: F401  (fixture)
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
ROOT = T.ROOT
SETTINGS = {"3_0": (3, 0), "4_0": (4, 0), "8_0": (8, 0), "8_6": (8, 6), "default": None}
KNOBS = ("TRT_FLAT_LITERAL", "TRT_FLAT_LITERAL_TEST_FAIL", "TRT_FLAT_LITERAL_PAIRS", "TRT_FLAT_LITERAL_PLANES", "TRT_FLAT_REUSE")


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """setting -> what the child of that setting rendered (one child per setting, started when first asked for)."""
    cache = {}

    def get(setting):
        if setting not in cache:
            out = tmp_path_factory.mktemp("flat_cache_" + setting) / "out.npz"
            env = {k: v for k, v in os.environ.items() if k not in KNOBS}
            env["TRT_FLAT_LITERAL"] = "1"
            if SETTINGS[setting] is not None:
                env["TRT_FLAT_LITERAL_PAIRS"], env["TRT_FLAT_LITERAL_PLANES"] = (str(v) for v in SETTINGS[setting])
            r = subprocess.run([sys.executable, "-c", T.CHILD, ROOT, str(out), *sorted(T.SCENES)], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            cache[setting] = dict(np.load(out))
        return cache[setting]
    return get


@pytest.fixture(scope="module")
def generator_stats(trt, tmp_path_factory):
    """(scene, pairs, planes) -> the generator's statistics for the scene's own leaf list."""
    d = tmp_path_factory.mktemp("flat_cache_stats")
    exe = str(d / "check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "tiny-raytracer_amd", "csrc"), os.path.join(ROOT, "tests", "native", "flat_cache_check.cpp"),
                    "-o", exe], check=True, timeout=300)

    def get(scene, pairs, planes):
        box, prim, _ = trt.Scene(trt.world_from_description(T.SCENES[scene](trt))[0]).nodes()
        w = leaves_of(box[prim >= 0])
        f = d / (scene + ".bin")
        f.write_bytes(w.tobytes())
        out = subprocess.run([exe, str(f), str(len(w)), "1", str(pairs), str(planes)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        v = [int(x) for x in out.stdout.split("\n")[1].split()[1:]]
        return dict(n=len(w), intervals=v[0], planes=v[1], evictions=v[2], far=v[3], extra=v[4], cached=bool(v[5]))
    return get


def test_the_scenes_reach_what_they_are_here_for(generator_stats):
    assert generator_stats("one_quad", 8, 6) == dict(n=1, intervals=3, planes=6, evictions=0, far=0, extra=0, cached=False)      # nothing to keep: the plain text
    assert generator_stats("three_quads", 4, 0)["n"] == 3
    st = generator_stats("thirty_two_quads", 4, 0)
    assert st["n"] == 32 and st["cached"] and st["evictions"] >= 1 and st["far"] >= 1, st
    assert generator_stats("thirty_two_quads", 8, 0)["intervals"] < st["intervals"]
    for scene in ("cornell", "wide_room", "coplanar_and_signed_zero", "quads_and_a_sphere", "thirty_two_quads"):
        for pairs, planes in ((4, 0), (8, 0), (8, 6)):
            assert generator_stats(scene, pairs, planes)["cached"], (scene, pairs, planes)
        assert not generator_stats(scene, 3, 0)["cached"]
    assert generator_stats("cornell", 8, 6)["planes"] < generator_stats("cornell", 8, 0)["planes"]
    assert generator_stats("wide_room", 8, 0)["n"] >= 6                      # several pairs: exits at the ballot with leaf_slots = 2 (T.TUNING)


@pytest.mark.parametrize("scene", sorted(T.SCENES))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_frame_and_ray_counts_are_the_oracles(frames, oracle_frames, setting, scene):  # noqa: F811
    cpu, cst = oracle_frames(scene)
    got = frames(setting)
    assert got["diagnostic"][0] == "", got["diagnostic"][0]                  # every scene really compiled: no fallback rendered these frames
    assert int(got[scene + "_compilations"][0]) == 1
    assert_bit_equal(got[scene + "_frame"], cpu, f"{scene} at {setting}: kernel compiled for the scene vs oracle")
    assert_bit_equal(got[scene + "_again"], cpu, f"{scene} at {setting}: second render vs oracle")
    samples, rays = (int(v) for v in got[scene + "_counters"])
    assert (samples, rays) == (cst["samples"], cst["rays"]), (scene, setting)
    assert np.any(cpu > 0)
