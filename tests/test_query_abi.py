"""The ray-query entry points (tinyrt.h trt_intersect / trt_occluded and their device forms) at the C boundary, without a GPU: the
symbols are declared, exported and bound, trt_hit has the documented layout, and misuse comes back as a code with a message before any
device work.  What the queries answer is checked on the GPU (tests/test_gpu_queries.py); the per-kind to insertion-index table they
report `geometry` through is not reachable from Python and is covered there too (mixed400 interleaves spheres and quads)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trt_intersect", "trt_occluded", "trt_intersect_device", "trt_occluded_device")


def test_the_four_symbols_are_declared_exported_and_bound(trt):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyrt.h")).read(), flags=re.S)
    raw = C.CDLL(trt._lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " is not declared in tinyrt.h"
        assert hasattr(raw, name), name + " is not exported"
        assert name in trt._lib.SIGNATURES and trt._lib.SIGNATURES[name][0] is C.c_int
    assert len(trt._lib.SIGNATURES["trt_intersect"][1]) == 5 and len(trt._lib.SIGNATURES["trt_intersect_device"][1]) == 6
    assert len(trt._lib.SIGNATURES["trt_occluded"][1]) == 5 and len(trt._lib.SIGNATURES["trt_occluded_device"][1]) == 6
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    assert "trt_intersect" in re.search(r"Later under 4[^/]*\*/", open(os.path.join(ROOT, "include", "tinyrt.h")).read(), flags=re.S).group(0)


def test_trt_hit_layout(trt):
    H = trt._lib.Hit
    assert C.sizeof(H) == 28 and H.t.offset == 0 and H.geometry.offset == 4 and H.material.offset == 8 and H.front_face.offset == 12
    assert H.normal.offset == 16
    d = trt.HIT_DTYPE
    assert d.itemsize == 28 and d.fields["normal"][1] == 16 and d.fields["geometry"][1] == 4 and d.names == ("t", "geometry", "material", "front_face", "normal")


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


@pytest.mark.parametrize("name", NAMES)
def test_misuse_is_invalid_arg_with_a_message_before_any_device_work(trt, name):
    fn = getattr(trt.lib, name)
    device = name.endswith("_device")
    rays = np.zeros((4, 6), np.float32)
    out = np.zeros(4 * 28, np.uint8)
    tail = (None,) if device else ()

    def call(scene, r, n, o):
        return fn(scene, r, None, n, o, *tail)

    s = _scene(trt)
    # (host pointers are handed to the device forms too: every one of these calls must return before anything is dereferenced)
    for args in ((None, rays.ctypes.data, 4, out.ctypes.data), (s._h, None, 4, out.ctypes.data), (s._h, rays.ctypes.data, 4, None),
                 (None, None, 0, None)):
        assert call(*args) == trt._lib.ERR_INVALID_ARG, args
        assert trt.lib.trt_last_error().decode() != ""


@pytest.mark.parametrize("name", ("trt_intersect", "trt_occluded"))
def test_a_well_formed_call_needs_a_device(trt, name):
    """Without a GPU: TRT_ERR_NO_DEVICE, also for n == 0 (the order of trt_sample_batch) - there is no CPU path.  With one: success."""
    fn = getattr(trt.lib, name)
    s = _scene(trt)
    rays = np.zeros((4, 6), np.float32)
    rays[:, 5] = 1.0
    out = np.full(4 * 28, 0xCD, np.uint8)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    assert fn(s._h, rays.ctypes.data, None, 4, out.ctypes.data) == want
    assert fn(s._h, None, None, 0, None) == want                            # n == 0 touches nothing
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (out == 0xCD).all()
        with pytest.raises(trt.TinyRTError) as e:
            s.intersect(rays)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
        with pytest.raises(trt.TinyRTError):
            s.occluded(rays, t_max=np.ones(4, np.float32))


def test_python_wrappers_check_their_arguments(trt):
    s = _scene(trt)
    with pytest.raises(ValueError):
        s.intersect(np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError):
        s.occluded(np.zeros((4, 6), np.float32), t_max=np.zeros(3, np.float32))


# ---- trt_query_launch_plan: the queries' launch arithmetic, checked without a device ----
def test_the_plan_symbol_is_declared_exported_and_bound(trt):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyrt.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+trt_query_launch_plan\s*\(", header) and hasattr(C.CDLL(trt._lib.LIB_PATH), "trt_query_launch_plan")
    assert trt._lib.SIGNATURES["trt_query_launch_plan"][0] is C.c_int and len(trt._lib.SIGNATURES["trt_query_launch_plan"][1]) == 4
    assert "trt_query_launch_plan" in re.search(r"Later under 4[^/]*\*/", open(os.path.join(ROOT, "include", "tinyrt.h")).read(), flags=re.S).group(0)
    s = _scene(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_query_launch_plan(None, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_query_launch_plan(s._h, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    # compute_units = 0 asks the current device; any other count needs none
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    assert trt.lib.trt_query_launch_plan(s._h, 1, 0, C.byref(out)) == want
    assert trt.lib.trt_query_launch_plan(s._h, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert s.query_plan(1, 304)["compute_units"] == 304


WALK_LDS_TREE, WALK_LOCK_STEP, WALK_NODES16, WALK_REGISTER_SLOTS = 1, 2, 3, 5       # trt_launch_plan.walk
# kQueryKernels (query.hip): (scene mode, walk, threads per workgroup)
QUERY_KERNEL_SHAPES = {(1, WALK_LOCK_STEP, 256), (1, WALK_LDS_TREE, 256), (1, WALK_LDS_TREE, 768), (1, WALK_REGISTER_SLOTS, 512),
                       (0, WALK_NODES16, 256), (0, WALK_REGISTER_SLOTS, 256)}


def _ceil_div(a, b):
    return (a + b - 1) // b


def _check_query_plan(q, n, cus, streamed, tag):
    """What launch_query and query_kernel assume (query.hip): LDS = scene copy | leaf stack (threads x slots x 8 B); wave w owns rays
    [w * rays_per_wave, ...), whole 64-ray rounds; the grid holds every wave."""
    assert q["has_kernel"] == 1, tag
    assert q["compute_units"] == cus, tag
    threads, slots = q["threads_per_workgroup"], q["leaf_slots"]
    assert (q["scene_mode"], q["walk"], threads) in QUERY_KERNEL_SHAPES, tag
    assert q["scene_mode"] == streamed["scene_mode"] and q["scene_lds_bytes"] == streamed["scene_lds_bytes"], tag
    assert (q["streamed_walk"], q["streamed_threads"]) == (streamed["walk"], streamed["threads_per_workgroup"]), tag
    if q["fallback"]:
        assert (q["streamed_walk"], q["streamed_threads"]) != (q["walk"], threads), tag
        assert (q["walk"], threads) == (WALK_REGISTER_SLOTS, 512 if q["scene_mode"] == 1 else 256), tag
    else:
        assert (q["walk"], threads) == (streamed["walk"], streamed["threads_per_workgroup"]), tag
        if q["walk"] != WALK_REGISTER_SLOTS:
            assert slots == streamed["leaf_slots"], tag
    # LDS
    al = (q["scene_lds_bytes"] + 15) & ~15
    if q["walk"] == WALK_REGISTER_SLOTS:
        assert slots == 0 and q["lds_bytes"] == q["scene_lds_bytes"], tag
    else:
        assert 1 <= slots <= 16 and q["lds_bytes"] == al + threads * slots * 8, tag
    assert q["lds_bytes"] <= 160 * 1024 and q["lds_bytes"] * q["workgroups_per_cu"] <= 160 * 1024, tag
    assert 1 <= q["workgroups_per_cu"] and q["workgroups_per_cu"] * threads <= q["kernel_waves_per_simd"] * 256, tag
    if slots < 2:
        assert q["stragglers"] == 0, tag
    if q["walk"] == WALK_LOCK_STEP:
        assert slots >= 2 and q["stragglers"] == 0, tag
    if q["walk"] == WALK_NODES16:
        assert q["scene_mode"] == 0, tag
    # the batch
    wave_slots, per_wave, waves = q["wave_slots"], q["rays_per_wave"], q["waves"]
    assert wave_slots == 4 * cus * q["workgroups_per_cu"] * (threads // 64), tag
    assert per_wave % 64 == 0 and per_wave >= 256, tag
    assert (per_wave == 256) == (_ceil_div(n, 256) <= wave_slots), tag
    if n == 0:
        assert waves == 0 and q["workgroups"] == 0, tag
    else:
        assert waves * per_wave >= n > (waves - 1) * per_wave, tag
    if per_wave > 256:
        assert waves <= wave_slots, tag
        assert per_wave - 64 < _ceil_div(n, wave_slots), tag                 # the shortest whole-round run that fits the slots
    assert q["workgroups"] == _ceil_div(waves, threads // 64) and q["workgroups"] < 2 ** 31, tag


def _plan_scenes(trt):
    """(tag, description): 1, 18, 32, 33, 400, 550, 600, 650, 700 and 3001 primitives - both sides of every threshold of the streamed
    plan the queries follow (lock-step list, LDS tree at 256 / 768 / 512 lanes, global memory)."""
    import walk_ray_cases as W
    from test_gpu_fuzz import random_scene
    out = [(name, W.scene(trt, name)) for name in ("one_primitive", "cornell", "prims32", "prims33", "mixed400")]
    out.append(("prims550", random_scene(1100, n_prims=550)))
    out.append(("prims600", W.scene(trt, "prims600")))
    out.append(("prims650", random_scene(1100, n_prims=650)))
    out.append(("prims700", random_scene(1100, n_prims=700)))
    out.append(("grid3000", W.scene(trt, "grid3000")))
    assert [len(d["geometries"]) for _, d in out] == [1, 18, 32, 33, 400, 550, 600, 650, 700, 3001]
    return out


def test_query_launch_plan_invariants_for_every_scene_size_option_and_batch(trt):
    """Every (scene size, flat_walk, compact_nodes, scene compiler, compute units, batch size) a caller can ask for yields a plan with a
    kernel instantiation, whose LDS parts add up, whose runs are whole 64-ray rounds that cover the batch exactly once, and whose walk
    and workgroup shape are the streamed plan's unless the register-slot fallback is reported."""
    import itertools
    compilers = (False, True) if trt.lib.trt_device_count() > 0 else (False,)      # the device compiler needs a device
    r = trt.Renderer(4, 1, 8, False, (0.1, 0.1, 0.1))
    n_checked, shapes, lengthened = 0, set(), 0
    for name, desc in _plan_scenes(trt):
        world, cam = trt.world_from_description(desc)
        for flat, compact, on_device in itertools.product((-1, 0, 1), (-1, 0, 1), compilers):
            sc = world.get_bvh(on_device=on_device, flat_walk=flat, compact_nodes=compact)
            streamed = r.launch_plan(cam, sc)
            for cus in (1, 64, 256, 304):
                slots = sc.query_plan(1, cus)["wave_slots"]
                for n in (0, 1, 63, 64, 65, 256, 257, 256 * slots, 256 * slots + 1, 320 * slots, 320 * slots + 1, 2 ** 31, 2 ** 32 - 1):
                    q = sc.query_plan(n, cus)
                    _check_query_plan(q, n, cus, streamed, (name, flat, compact, on_device, cus, n, q))
                    shapes.add((q["scene_mode"], q["walk"], q["threads_per_workgroup"], q["fallback"]))
                    lengthened += q["rays_per_wave"] > 256
                    n_checked += 1
                assert sc.query_plan(256 * slots, cus)["rays_per_wave"] == 256 and sc.query_plan(256 * slots + 1, cus)["rays_per_wave"] == 320
                assert sc.query_plan(320 * slots + 1, cus)["rays_per_wave"] == 384
    assert n_checked == 10 * 9 * len(compilers) * 4 * 13 and lengthened > n_checked // 4, (n_checked, lengthened)
    assert {s[:3] for s in shapes} == QUERY_KERNEL_SHAPES, sorted(shapes)


def test_the_gpu_tests_scene_list_reaches_every_kernel_and_every_route_to_the_fallback(trt):
    """tests/test_gpu_queries.py compares answers on PLAN_CASES; passed through the plan, those cases must launch all six instantiations of
    kQueryKernels and reach the register-slot fallback from an LDS tree plan, from a lock-step plan in LDS and from a lock-step plan in
    global memory - so that a later change to the plan cannot leave a kernel or a route untested without this test failing."""
    import walk_ray_cases as W
    import test_gpu_queries as G
    assert [name for name, options, _ in G.PLAN_CASES if not options] == G.SCENES and len(G.PLAN_CASES) == len(G.SCENES) + len(G.OTHER_WALKS)
    shapes, routes = set(), set()
    worlds = {}
    for name, options, shape in G.PLAN_CASES:
        if name not in worlds:
            worlds[name] = trt.world_from_description(W.scene(trt, name))[0]
        host_options = {k: v for k, v in options.items() if k != "on_device"}           # (both compilers give the same bytes: tests/test_gpu_scene_build.py)
        q = (worlds[name].get_bvh(**host_options) if host_options else worlds[name].get_bvh()).query_plan(408, 256)
        assert G.plan_shape(q) == shape, (name, options, G.plan_shape(q), shape)
        shapes.add(shape[:3])
        if q["fallback"]:
            routes.add((q["scene_mode"], q["streamed_walk"]))
    reached = sorted(shapes)
    print(f"\nquery kernel shapes reached by the GPU tests' scenes: {reached}; routes to the fallback (scene mode, streamed walk): {sorted(routes)}")
    assert shapes == QUERY_KERNEL_SHAPES, reached
    assert {(1, WALK_LDS_TREE), (1, WALK_LOCK_STEP), (0, WALK_LOCK_STEP)} <= routes, sorted(routes)
