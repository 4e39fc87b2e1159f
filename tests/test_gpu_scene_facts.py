"""The lock-step kernel compiled per scene WITH scene facts (scene_facts.h; TRT_SCENE_FACTS) on the GPU, against the CPU oracle bit for bit.
The setting is read once when the library loads, so each one - the library's default (facts and the straight-line shade) and
TRT_SCENE_FACTS=0 (the unit without facts) - renders in ONE fresh child process with TRT_FLAT_LITERAL=1, every scene twice on one handle.
Scenes (tests/scene_facts_scenes.py): those of tests/test_gpu_flat_literal.py at 16 x 16, 4 spp, depth 50 - Cornell among them - and a
closed Lambertian room without a light at depth 3 (every path ends on the budget), one floor quad under a bright background (nearly every
ray leaves through the miss exit, the pool is refilled again and again), two lights alone (every hit ends), a room with a Metal quad and one
with a Dielectric quad (the general dispatch, less what the facts exclude) and a room with a tilted quad (not axis-exact: the walk-order
leaf phase with the straight-line shade); and Cornell at 128 x 128, 8 spp: several batches per wave, refills between rounds, idle lanes at
the tail.  Frame, second render, sample and ray counts are the oracle's; each scene compiles once; the diagnostic is empty; the facts each
scene's kernel was compiled with are the ones scene_facts_scenes.FACTS lists (0 with the setting off)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scene_facts_scenes as S
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
ROOT = S.T.ROOT
SETTINGS = {"default": None, "off": "0"}
KNOBS = ("TRT_FLAT_LITERAL", "TRT_FLAT_LITERAL_TEST_FAIL", "TRT_FLAT_LITERAL_PAIRS", "TRT_FLAT_LITERAL_PLANES", "TRT_FLAT_REUSE", "TRT_SCENE_FACTS",
         "TRT_AXIS_QUADS", "TRT_NEAREST_FIRST")
NAMES = sorted(S.SCENES) + [S.BIG["name"]]


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """setting -> what the child of that setting rendered (one child per setting, started when first asked for)."""
    cache = {}

    def get(setting):
        if setting not in cache:
            out = tmp_path_factory.mktemp("scene_facts_" + setting) / "out.npz"
            env = {k: v for k, v in os.environ.items() if k not in KNOBS}
            env["TRT_FLAT_LITERAL"] = "1"
            if SETTINGS[setting] is not None:
                env["TRT_SCENE_FACTS"] = SETTINGS[setting]
            r = subprocess.run([sys.executable, "-c", S.CHILD, ROOT, str(out), *NAMES], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            cache[setting] = dict(np.load(out))
        return cache[setting]
    return get


@pytest.fixture(scope="module")
def oracle(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            big = name == S.BIG["name"]
            desc = trt.scenes.cornell(S.BIG["width"], S.BIG["height"]) if big else S.SCENES[name](trt)
            ow, ocam = orc.world_from_description(desc)
            cpu, cst = orc.render(ow, ocam, S.BIG["spp"] if big else S.SPP, S.T.DEPTH if big else S.DEPTH[name], desc["background"], seed=S.SEED, nthreads=8)
            cpu.setflags(write=False)
            cache[name] = (cpu, cst)
        return cache[name]
    return get


@pytest.mark.parametrize("scene", NAMES)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_frame_counts_compilations_and_facts(frames, oracle, setting, scene):
    cpu, cst = oracle(scene)
    got = frames(setting)
    assert got["diagnostic"][0] == "", got["diagnostic"][0]                  # every scene really compiled: no fallback rendered these frames
    assert int(got[scene + "_compilations"][0]) == 1, "one scene rendered twice compiles once"
    want = S.FACTS["cornell" if scene == S.BIG["name"] else scene]
    assert int(got[scene + "_facts"][0]) == (want if setting == "default" else 0), (scene, setting, hex(int(got[scene + "_facts"][0])))
    # ... and they are the facts the compiled unit's source was written with (trt_flat_literal_facts: of the unit loaded last), not only
    # what the handle derived: a request that lost them on the way to the compiler would render the same frame through a unit without facts
    assert int(got[scene + "_unit_facts"][0]) == (want if setting == "default" else 0), (scene, setting, hex(int(got[scene + "_unit_facts"][0])))
    assert_bit_equal(got[scene + "_frame"], cpu, f"{scene} at {setting}: kernel compiled for the scene vs oracle")
    assert_bit_equal(got[scene + "_again"], cpu, f"{scene} at {setting}: second render vs oracle")
    samples, rays = (int(v) for v in got[scene + "_counters"])
    assert (samples, rays) == (cst["samples"], cst["rays"]), (scene, setting)
    if scene == "closed_room":
        assert not np.any(cpu != 0) and cst["rays"] == 3 * cst["samples"]      # every path spent its budget of three, every colour is +0
    else:
        assert np.any(cpu > 0)
