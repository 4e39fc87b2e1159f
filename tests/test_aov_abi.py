"""The feature-buffer and primary-ray entry points (tinyrt.h trt_render_aov, trt_render_aov_device, trt_primary_rays,
trt_primary_rays_device, trt_aov_launch_plan) at the C boundary, without a GPU: the symbols are declared, exported and bound,
trt_aov_buffers has the documented layout, misuse comes back as TRT_ERR_INVALID_ARG with a message before any device work, and the launch
arithmetic holds its invariants for every scene and option the GPU tests use.  What the buffers hold is checked on the GPU
(tests/test_gpu_aov.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_query_abi import QUERY_KERNEL_SHAPES, WALK_LDS_TREE, WALK_LOCK_STEP, _check_query_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_primary_rays": 4, "trt_primary_rays_device": 5, "trt_render_aov": 4, "trt_render_aov_device": 5, "trt_aov_launch_plan": 4}
# kAovKernels (aov.hip): the (scene mode, walk, threads per workgroup) set of the queries' table
AOV_KERNEL_SHAPES = QUERY_KERNEL_SHAPES


def test_the_symbols_are_declared_exported_and_bound(trt):
    text = open(os.path.join(ROOT, "include", "tinyrt.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(trt._lib.LIB_PATH)
    later = re.search(r"Later under 4[^/]*\*/", text, flags=re.S).group(0)
    for name, nargs in NAMES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " is not declared in tinyrt.h"
        assert hasattr(raw, name), name + " is not exported"
        res, args = trt._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
        assert name in later, name + " is not listed under 'Later under 4'"
    assert "trt_aov_buffers" in later
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays


def test_trt_aov_buffers_layout(trt):
    B = trt._lib.AovBuffers
    assert C.sizeof(B) == 48
    assert [getattr(B, n).offset for n in ("albedo", "normal", "depth", "coverage", "geometry", "material")] == [0, 8, 16, 24, 32, 40]
    assert tuple(trt.AOV_CHANNELS) == B.FIELDS
    # the header declares one field per declaration, in this order
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyrt.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trt_aov_buffers\s*;", header).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["float *albedo", "float *normal", "float *depth", "float *coverage", "uint32_t *geometry", "uint32_t *material"]


def _scene_camera(trt):
    world, cam = trt.world_from_description(trt.scenes.cornell(8, 8))
    return world.get_bvh(), cam


def _params(trt, **over):
    return trt.Renderer(3, 1, 4, False, (0.1, 0.2, 0.3), seed=5).params(**over)


def _invalid(trt, rc):
    assert rc == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_last_error().decode() != ""


@pytest.mark.parametrize("device", (False, True))
def test_render_aov_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    fn = trt.lib.trt_render_aov_device if device else trt.lib.trt_render_aov
    tail = (None,) if device else ()
    sc, cam = _scene_camera(trt)
    p = _params(trt)
    depth = np.zeros(64, np.float32)
    bufs = trt._lib.AovBuffers()
    bufs.depth = depth.ctypes.data
    none = trt._lib.AovBuffers()
    _invalid(trt, fn(None, C.byref(cam.pod), C.byref(p), C.byref(bufs), *tail))
    _invalid(trt, fn(sc._h, None, C.byref(p), C.byref(bufs), *tail))
    _invalid(trt, fn(sc._h, C.byref(cam.pod), None, C.byref(bufs), *tail))
    _invalid(trt, fn(sc._h, C.byref(cam.pod), C.byref(p), None, *tail))
    _invalid(trt, fn(sc._h, C.byref(cam.pod), C.byref(p), C.byref(none), *tail))                  # all six NULL
    assert "all six" in trt.lib.trt_last_error().decode()
    # the parameters are validated as trt_render validates them
    for over in (dict(sample_begin=2, sample_end=1), dict(sample_end=4), dict(band_rows=4, band_stride=0),
                 dict(band_rows=4, band_stride=2, band_offset=2), dict(band_rows=4, band_stride=2, band_offset=1, rows_local=8)):
        q = _params(trt, **over)
        _invalid(trt, fn(sc._h, C.byref(cam.pod), C.byref(q), C.byref(bufs), *tail))
    q = _params(trt)
    q.samples_per_pixel = 0
    _invalid(trt, fn(sc._h, C.byref(cam.pod), C.byref(q), C.byref(bufs), *tail))
    assert (depth == 0).all()


@pytest.mark.parametrize("device", (False, True))
def test_primary_rays_misuse_is_invalid_arg_before_any_device_work(trt, device):
    fn = trt.lib.trt_primary_rays_device if device else trt.lib.trt_primary_rays
    tail = (None,) if device else ()
    _, cam = _scene_camera(trt)
    p = _params(trt)
    rays = np.zeros((64, 6), np.float32)
    _invalid(trt, fn(None, C.byref(p), 0, rays.ctypes.data, *tail))
    _invalid(trt, fn(C.byref(cam.pod), None, 0, rays.ctypes.data, *tail))
    _invalid(trt, fn(C.byref(cam.pod), C.byref(p), 0, None, *tail))
    _invalid(trt, fn(C.byref(cam.pod), C.byref(p), 3, rays.ctypes.data, *tail))                  # s >= samples_per_pixel
    _invalid(trt, fn(C.byref(cam.pod), C.byref(p), 0xFFFFFFFF, rays.ctypes.data, *tail))
    q = _params(trt, band_rows=4, band_stride=2, band_offset=2, rows_local=4)
    _invalid(trt, fn(C.byref(cam.pod), C.byref(q), 0, rays.ctypes.data, *tail))
    assert (rays == 0).all()


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path, neither for the buffers nor for the rays.  With one: success.  The sample
    range, max_bounces, the backend and the tuning are not looked at by the ray export; the backend not by the buffers."""
    sc, cam = _scene_camera(trt)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt, backend=77, sample_begin=9, sample_end=2)
    rays = np.full((64, 6), 7.0, np.float32)
    assert trt.lib.trt_primary_rays(C.byref(cam.pod), C.byref(p), 2, rays.ctypes.data) == want
    p = _params(trt, backend=77, max_bounces=0)
    depth = np.full(64, 7.0, np.float32)
    bufs = trt._lib.AovBuffers()
    bufs.depth = depth.ctypes.data
    assert trt.lib.trt_render_aov(sc._h, C.byref(cam.pod), C.byref(p), C.byref(bufs)) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (rays == 7.0).all() and (depth == 7.0).all()
        r = trt.Renderer(3, 1, 4, False, (0.1, 0.2, 0.3), seed=5)
        with pytest.raises(trt.TinyRTError) as e:
            r.render_aov(cam, sc)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
        with pytest.raises(trt.TinyRTError) as e:
            cam.primary_rays(0, 3, seed=5)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (rays == 7.0).any() and not (depth == 7.0).any()


def test_python_wrappers_check_their_arguments(trt):
    sc, cam = _scene_camera(trt)
    r = trt.Renderer(3, 1, 4, False, (0.1, 0.2, 0.3), seed=5)
    with pytest.raises(KeyError):
        r.render_aov(cam, sc, channels=("albedo", "radiance"))
    with pytest.raises(KeyError):
        r.render_aov_device(cam, sc, {"radiance": 64})
    with pytest.raises(TypeError):
        cam.primary_rays(0, 3, sample_end=2)


def test_the_plan_symbol_checks_its_arguments(trt):
    sc, _ = _scene_camera(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_aov_launch_plan(None, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_aov_launch_plan(sc._h, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_aov_launch_plan(sc._h, 1, 0, C.byref(out)) == want
    assert trt.lib.trt_aov_launch_plan(sc._h, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.aov_plan(1, 304)["compute_units"] == 304


PIXEL_COUNTS = (0, 1, 255, 256, 257, 2345, 9170, 2 ** 24)


def test_aov_launch_plan_invariants_on_every_scene_and_option_of_the_gpu_tests(trt):
    """Every (scene, options) of test_gpu_queries.PLAN_CASES at 256 compute units and every pixel count of PIXEL_COUNTS (nothing, one
    pixel, both sides of a run of 256, the two image sizes of tests/test_gpu_aov.py, a 4096 x 4096 frame): the invariants
    tests/test_query_abi.py checks for the queries - the LDS layout, runs that cover [0, n) once, workgroups = ceil(waves / waves per
    workgroup), the walk and workgroup shape of the streamed plan unless the fallback is reported - and the listed kernel shape; the
    cases reach every entry of the table and every route to the fallback."""
    import test_gpu_queries as G
    import walk_ray_cases as W
    cus = 256
    r = trt.Renderer(4, 1, 8, False, (0.1, 0.1, 0.1))
    shapes, routes, worlds, lengthened = set(), set(), {}, 0
    for name, options, shape in G.PLAN_CASES:
        if name not in worlds:
            worlds[name] = trt.world_from_description(W.scene(trt, name))
        world, cam = worlds[name]
        host_options = {k: v for k, v in options.items() if k != "on_device"}       # (both compilers give the same bytes: tests/test_gpu_scene_build.py)
        sc = world.get_bvh(**host_options) if host_options else world.get_bvh()
        streamed = r.launch_plan(cam, sc)
        for n in PIXEL_COUNTS:
            q = sc.aov_plan(n, cus)
            tag = (name, options, n, q)
            _check_query_plan(q, n, cus, streamed, tag)
            assert G.plan_shape(q) == shape, tag
            per_wave, waves = q["rays_per_wave"], q["waves"]
            # the runs [w * per_wave, min(n, (w + 1) * per_wave)) of waves 0 .. waves - 1 cover [0, n) once; the grid holds exactly them
            assert (waves - 1) * per_wave < n <= waves * per_wave if n else waves == 0, tag
            assert q["workgroups"] == -(-waves // (q["threads_per_workgroup"] // 64)), tag
            lengthened += per_wave > 256
            shapes.add(shape[:3])
            if q["fallback"]:
                routes.add((q["scene_mode"], q["streamed_walk"]))
        # the plan of the queries for as many rays is the same launch, but for the launch bound of the kernel (aov.hip kAovKernels)
        qq, qa = sc.query_plan(2345, cus), sc.aov_plan(2345, cus)
        for k in ("scene_mode", "walk", "threads_per_workgroup", "leaf_slots", "stragglers", "lds_bytes", "fallback", "rays_per_wave"):
            assert qq[k] == qa[k], (name, options, k)
        assert qa["kernel_waves_per_simd"] <= qq["kernel_waves_per_simd"]
    assert shapes == AOV_KERNEL_SHAPES, sorted(shapes)
    assert {(1, WALK_LDS_TREE), (1, WALK_LOCK_STEP), (0, WALK_LOCK_STEP)} <= routes, sorted(routes)
    assert lengthened > 0                                                    # 2^24 pixels lengthen the runs of some shape


def test_the_gpu_tests_case_lists_reach_every_kernel_and_every_route_to_the_fallback(trt):
    """tests/test_gpu_aov.py renders its SCENES with default options and its WALK_CASES with theirs; passed through the plan at the image
    size that module uses for them, the union must launch all six instantiations of kAovKernels and reach the register-slot fallback from
    an LDS tree plan, from a lock-step plan in LDS and from a lock-step plan in global memory - so that dropping a case there, or a later
    change to the plan, cannot leave a kernel or a route unrun without this test failing."""
    import test_gpu_aov as A
    import test_gpu_queries as G
    import walk_ray_cases as W
    cases = [(name, {}, G.DEFAULT_SHAPES[name]) for name in A.SCENES] + list(A.WALK_CASES)
    assert len(cases) == len(A.SCENES) + len(G.OTHER_WALKS)
    n = A.SIZES[0][0] * A.SIZES[0][1]
    shapes, routes, worlds = set(), set(), {}
    for name, options, shape in cases:
        if name not in worlds:
            worlds[name] = trt.world_from_description(W.scene(trt, name))[0]
        host_options = {k: v for k, v in options.items() if k != "on_device"}           # (both compilers give the same bytes: tests/test_gpu_scene_build.py)
        sc = worlds[name].get_bvh(**host_options) if host_options else worlds[name].get_bvh()
        q = sc.aov_plan(n, 256)
        assert G.plan_shape(q) == shape, (name, options, G.plan_shape(q), shape)
        shapes.add(shape[:3])
        if q["fallback"]:
            routes.add((q["scene_mode"], q["streamed_walk"]))
    # the default compilations alone miss the register-slot walk from global memory
    assert {G.DEFAULT_SHAPES[name][:3] for name in A.SCENES} == AOV_KERNEL_SHAPES - {(0, 5, 256)}
    assert shapes == AOV_KERNEL_SHAPES, sorted(shapes)
    assert {(1, WALK_LDS_TREE), (1, WALK_LOCK_STEP), (0, WALK_LOCK_STEP)} <= routes, sorted(routes)
