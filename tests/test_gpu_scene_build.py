"""The device scene compiler (trt_scene_create_on_device) against the host compiler: the same packed bytes, info, node
dumps, compact nodes and launch plans over the scene generators and a fuzz corpus (sizes around every power of two and
the compiler's own thresholds, ties, special values, deep SAH splits, every placement option); frames of device-built
scenes against the CPU oracle; concurrent builds; no device memory left behind."""
import threading

import numpy as np
import pytest

from scene_build_worlds import (cull_serial_max, few_keys_world, fuzz_world, growing_world, identical_world, ref_local_max,
                                sphere_world)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(trt):
    assert trt.lib.trt_device_count() >= 1
    trt._lib.check(trt.lib.trt_set_device(0))
    return trt


def _cam(trt):
    return trt.Camera(10.0, 0.0, (0, 0, -40), (0, 0, 0), (0, 1, 0), 40.0, 64, 48)


def assert_same_scene(trt, world, **opt):
    h = trt.Scene(world, **opt)
    d = trt.Scene(world, on_device=True, **opt)
    assert h.info() == d.info()
    hp, dp = h.packed(), d.packed()
    if not np.array_equal(hp, dp):
        bad = np.flatnonzero(hp != dp)
        raise AssertionError("packed scenes differ at %d bytes, first at %d of %d" % (len(bad), bad[0], len(hp)))
    for a, b in zip(h.nodes() + h.cull_nodes(), d.nodes() + d.cull_nodes()):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    hc, dc = h.compact_nodes(), d.compact_nodes()
    assert (hc is None) == (dc is None)
    if hc is not None:
        for a, b in zip(hc, dc):
            assert np.array_equal(a.view(np.uint16) if a.dtype == np.float16 else a, b.view(np.uint16) if b.dtype == np.float16 else b)
    r = trt.Renderer(4, 1, 8, False, (0.5, 0.7, 1.0), seed=1)
    cam = _cam(trt)
    assert r.launch_plan(cam, h) == r.launch_plan(cam, d)
    return d


@pytest.mark.parametrize("name,args", [("cornell", (64, 64)), ("dummy_spheres", ()), ("quad_test", ()), ("random_spheres", (64, 36)),
                                       ("sphere_grid", (100000, 64, 36)), ("sphere_field", (1_000_000, 64, 36)),
                                       ("sphere_field", (4_000_000, 64, 36))])
def test_scene_generators(dev, name, args):
    world, _ = dev.world_from_description(getattr(dev.scenes, name)(*args))
    assert_same_scene(dev, world)


def _sizes():
    T, S = ref_local_max(), cull_serial_max()
    n = {1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65}
    for k in range(1, 18):
        n |= {2 ** k - 1, 2 ** k + 1}
    for t in (T, 2 * T, 4 * T, S, 2 * S):
        n |= {t - 1, t, t + 1}
    return sorted(x for x in n if x >= 1)


@pytest.mark.parametrize("n", _sizes())
def test_fuzz_sizes(dev, n):
    assert_same_scene(dev, fuzz_world(dev, n, seed=n) if n <= 20000 else sphere_world(dev, n, seed=n))


@pytest.mark.parametrize("n", [2, 3, 7, 100, 1025, 3000])
def test_ties(dev, n):
    assert_same_scene(dev, identical_world(dev, n))
    assert_same_scene(dev, few_keys_world(dev, n, seed=n))


@pytest.mark.parametrize("seed", range(12))
def test_special_values(dev, seed):
    n = [5, 40, 300, 2500][seed % 4]
    assert_same_scene(dev, fuzz_world(dev, n, seed=100 + seed, special=0.05 + 0.05 * (seed % 3), quads=0.5), compact_nodes=1)


def test_huge_coordinates_not_finite(dev):
    w = fuzz_world(dev, 200, seed=5)
    w.add_geometry(dev.Sphere((3e30, 0, 0), 1.0, 0))
    d = assert_same_scene(dev, w, compact_nodes=1)
    assert d.info()["num_spheres"] >= 1


@pytest.mark.parametrize("n", [20, 70, 300, 1500])
def test_deep_uneven_splits(dev, n):
    assert_same_scene(dev, growing_world(dev, n))


@pytest.mark.parametrize("prune", [0.2, 0.5, 0.9, 1.0])
@pytest.mark.parametrize("compact", [-1, 0, 1])
@pytest.mark.parametrize("flat", [-1, 0, 1])
def test_options(dev, prune, compact, flat):
    for n in (9, 700, 5000):
        assert_same_scene(dev, fuzz_world(dev, n, seed=n + 7, special=0.02), cull_prune=prune, compact_nodes=compact, flat_walk=flat)


@pytest.mark.parametrize("name", ["cornell", "random_spheres"])
def test_frames_equal_oracle(dev, orc, name):
    desc = getattr(dev.scenes, name)(48, 32) if name == "random_spheres" else dev.scenes.cornell(48, 48)
    world, cam = dev.world_from_description(desc)
    scene = world.get_bvh(on_device=True)
    r = dev.Renderer(4, 1, 8, False, desc["background"], seed=1)
    gpu = r.render(cam, scene, collect_stats=True).data
    oworld, ocam = orc.world_from_description(desc)
    cpu, stats = orc.render(oworld, ocam, 4, 8, desc["background"], seed=1, nthreads=4)
    assert np.array_equal(gpu.view(np.uint32), cpu.view(np.uint32))
    assert r.last_stats["rays"] == stats["rays"] and r.last_stats["node_tests"] == stats["node_tests"]


def test_two_threads_build_at_once(dev):
    worlds = [sphere_world(dev, 600_000, seed=1), fuzz_world(dev, 20_000, seed=2, quads=0.5)]
    serial = [dev.Scene(w, on_device=True).packed() for w in worlds]
    out, errors = [None, None], []

    def build(i):
        try:
            dev._lib.check(dev.lib.trt_set_device(0))
            out[i] = dev.Scene(worlds[i], on_device=True).packed()
        except Exception as e:                                  # reported below
            errors.append(e)

    threads = [threading.Thread(target=build, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for a, b in zip(out, serial):
        assert np.array_equal(a, b)


def test_no_device_memory_left_behind(dev):
    import torch
    world = sphere_world(dev, 300_000, seed=3)
    dev.Scene(world, on_device=True)                            # warm-up: runtime and allocator state
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(3):
        s = dev.Scene(world, on_device=True)
        del s
    s = dev.Scene(world, on_device=True)
    r = dev.Renderer(1, 1, 2, False, (0.5, 0.7, 1.0), seed=1)
    r.render(_cam(dev), s)
    dev.lib.trt_scene_trim(s._h)
    del s
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free1 >= free0 - (4 << 20), (free0, free1)
