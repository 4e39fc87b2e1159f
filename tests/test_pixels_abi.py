"""The sparse render and selection entry points (tinyrt.h trt_render_pixels, trt_render_pixels_device, trt_pixels_launch_plan,
trt_select_pixels, trt_select_pixels_device, trt_select_scratch_bytes) at the C boundary, without a GPU: the symbols are declared,
exported and bound, misuse comes back as TRT_ERR_INVALID_ARG with a message before any device work, an empty list succeeds without a
device, and the launch arithmetic holds its invariants for every scene and option the GPU tests use.  What the buffers hold is checked on
the GPU (tests/test_gpu_pixels.py, tests/test_gpu_select.py, tests/test_gpu_adaptive.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_query_abi import QUERY_KERNEL_SHAPES, WALK_LDS_TREE, WALK_LOCK_STEP, _check_query_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_render_pixels": (C.c_int, 8), "trt_render_pixels_device": (C.c_int, 10), "trt_pixels_launch_plan": (C.c_int, 4),
         "trt_select_pixels": (C.c_int, 11), "trt_select_pixels_device": (C.c_int, 14), "trt_select_scratch_bytes": (C.c_uint64, 1)}
# kPixelsKernels (pixels.hip): one instantiation per walk of the feature buffers' table, which is the queries'
PIXELS_KERNEL_SHAPES = QUERY_KERNEL_SHAPES


def test_the_symbols_are_declared_exported_and_bound(trt):
    text = open(os.path.join(ROOT, "include", "tinyrt.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(trt._lib.LIB_PATH)
    later = re.search(r"Later under 4[^/]*\*/", text, flags=re.S).group(0)
    for name, (restype, nargs) in NAMES.items():
        ret = "uint64_t" if restype is C.c_uint64 else "int"
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", header), name + " is not declared in tinyrt.h"
        assert hasattr(raw, name), name + " is not exported"
        res, args = trt._lib.SIGNATURES[name]
        assert res is restype and len(args) == nargs, name
        assert name in later, name + " is not listed under 'Later under 4'"
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    # the plan struct is the queries' (no new struct)
    assert trt._lib.SIGNATURES["trt_pixels_launch_plan"][1][3] is trt._lib.SIGNATURES["trt_query_launch_plan"][1][3]
    assert C.sizeof(trt._lib.QueryPlan) == 16 * 4 + 2 * 8
    for name in ("select_pixels", "select_pixels_device", "select_scratch_bytes"):
        assert callable(getattr(trt, name))
    for name in ("render_pixels", "render_pixels_device", "render_adaptive"):
        assert callable(getattr(trt.Renderer, name))
    assert callable(trt.Scene.pixels_plan)


def _scene_camera(trt):
    world, cam = trt.world_from_description(trt.scenes.cornell(8, 8))
    return world.get_bvh(), cam


def _params(trt, **over):
    return trt.Renderer(4, 1, 4, False, (0.1, 0.2, 0.3), seed=5).params(**over)


def _invalid(trt, rc):
    assert rc == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_last_error().decode() != ""


@pytest.mark.parametrize("device", (False, True))
def test_render_pixels_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    sc, cam = _scene_camera(trt)
    p = _params(trt)
    px = np.array([0, 5, 63], np.uint32)
    accum = np.full((8, 8, 3), 7.0, np.float32)
    m2 = np.full((8, 8, 3), 7.0, np.float32)

    def call(s, c, q, pixels, n, a, m):
        if device:
            return trt.lib.trt_render_pixels_device(s, c, q, pixels, n, None, a, m, None, None)
        return trt.lib.trt_render_pixels(s, c, q, pixels, n, a, m, None)

    camp, pp = C.byref(cam.pod), C.byref(p)
    _invalid(trt, call(None, camp, pp, px.ctypes.data, 3, accum.ctypes.data, m2.ctypes.data))
    _invalid(trt, call(sc._h, None, pp, px.ctypes.data, 3, accum.ctypes.data, m2.ctypes.data))
    _invalid(trt, call(sc._h, camp, None, px.ctypes.data, 3, accum.ctypes.data, m2.ctypes.data))
    _invalid(trt, call(sc._h, camp, pp, None, 3, accum.ctypes.data, m2.ctypes.data))
    _invalid(trt, call(sc._h, camp, pp, px.ctypes.data, 3, None, m2.ctypes.data))
    q = _params(trt, collect_stats=1)
    _invalid(trt, call(sc._h, camp, C.byref(q), px.ctypes.data, 3, accum.ctypes.data, m2.ctypes.data))
    assert "collect_stats" in trt.lib.trt_last_error().decode()
    _invalid(trt, call(sc._h, camp, C.byref(_params(trt, collect_stats=2)), px.ctypes.data, 3, accum.ctypes.data, m2.ctypes.data))
    # the parameters are validated as trt_render validates them
    for over in (dict(sample_begin=2, sample_end=1), dict(sample_end=5), dict(band_rows=4, band_stride=0),
                 dict(band_rows=4, band_stride=2, band_offset=2), dict(band_rows=4, band_stride=2, band_offset=1, rows_local=8)):
        _invalid(trt, call(sc._h, camp, C.byref(_params(trt, **over)), px.ctypes.data, 3, accum.ctypes.data, m2.ctypes.data))
    q = _params(trt)
    q.samples_per_pixel = 0
    _invalid(trt, call(sc._h, camp, C.byref(q), px.ctypes.data, 3, accum.ctypes.data, m2.ctypes.data))
    if not device:
        # the host form validates the list with a bitmap: out of range (also for the rows a band shard owns), listed twice
        for bad in ([0, 64], [0xFFFFFFFF], [3, 9, 3], [63, 63]):
            b = np.array(bad, np.uint32)
            _invalid(trt, call(sc._h, camp, pp, b.ctypes.data, len(b), accum.ctypes.data, m2.ctypes.data))
        assert "twice" in trt.lib.trt_last_error().decode()
        b = np.array([32], np.uint32)
        shard = _params(trt, band_rows=4, band_stride=2, band_offset=1, rows_local=4)
        _invalid(trt, call(sc._h, camp, C.byref(shard), b.ctypes.data, 1, accum.ctypes.data, m2.ctypes.data))
        assert "outside" in trt.lib.trt_last_error().decode()
    assert (accum == 7.0).all() and (m2 == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_list_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc, cam = _scene_camera(trt)
    p = _params(trt)
    accum = np.full((8, 8, 3), 7.0, np.float32)
    if device:
        rc = trt.lib.trt_render_pixels_device(sc._h, C.byref(cam.pod), C.byref(p), None, 0, None, None, None, None, None)
    else:
        rc = trt.lib.trt_render_pixels(sc._h, C.byref(cam.pod), C.byref(p), None, 0, accum.ctypes.data, None, None)
    assert rc == trt._lib.TRT_OK
    assert (accum == 7.0).all()
    # ... but not before its arguments are checked
    _invalid(trt, trt.lib.trt_render_pixels(None, C.byref(cam.pod), C.byref(p), None, 0, accum.ctypes.data, None, None))
    r = trt.Renderer(4, 1, 4, False, (0.1, 0.2, 0.3), seed=5)
    st = r.render_pixels(cam, sc, np.zeros(0, np.uint32), accum)
    assert st["samples"] == 0 and st["rays"] == 0 and (accum == 7.0).all()


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path.  With one: success.  backend and tuning are not looked at."""
    sc, cam = _scene_camera(trt)
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt, backend=77)
    px = np.array([9, 3], np.uint32)
    accum = np.full((8, 8, 3), 7.0, np.float32)
    assert trt.lib.trt_render_pixels(sc._h, C.byref(cam.pod), C.byref(p), px.ctypes.data, 2, accum.ctypes.data, None, None) == want
    s = np.zeros((4, 3), np.float32)
    out = np.zeros(4, np.uint32)
    count = C.c_uint32(77)
    assert trt.lib.trt_select_pixels(s.ctypes.data, s.ctypes.data, 4, 8, 4, None, 4, 0.1, 0.0, out.ctypes.data, C.byref(count)) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (accum == 7.0).all() and count.value == 77
        r = trt.Renderer(4, 1, 4, False, (0.1, 0.2, 0.3), seed=5)
        with pytest.raises(trt.TinyRTError) as e:
            r.render_pixels(cam, sc, px, accum)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
        with pytest.raises(trt.TinyRTError) as e:
            trt.select_pixels(s, s, 8, 4, 0.1)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (accum.reshape(-1, 3)[[9, 3]] == 7.0).any() and (np.delete(accum.reshape(-1, 3), [9, 3], 0) == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_select_misuse_is_invalid_arg_before_any_device_work(trt, device):
    s = np.full((4, 3), 0.5, np.float32)
    out = np.full(4, 9, np.uint32)
    count = C.c_uint32(77)
    scratch = np.zeros(4, np.uint32)

    def call(a, m, npx, spp, done, cand, n, sel, cnt, scr=scratch.ctypes.data, scr_bytes=16):
        if device:
            return trt.lib.trt_select_pixels_device(a, m, npx, spp, done, cand, n, 0.1, 0.0, sel, cnt, scr, scr_bytes, None)
        return trt.lib.trt_select_pixels(a, m, npx, spp, done, cand, n, 0.1, 0.0, sel, cnt)

    sp, op, cp = s.ctypes.data, out.ctypes.data, C.byref(count)
    _invalid(trt, call(None, sp, 4, 8, 4, None, 4, op, cp))
    _invalid(trt, call(sp, None, 4, 8, 4, None, 4, op, cp))
    _invalid(trt, call(sp, sp, 4, 8, 4, None, 4, None, cp))
    _invalid(trt, call(sp, sp, 4, 8, 4, None, 4, op, None))
    _invalid(trt, call(sp, sp, 4, 0, 0, None, 4, op, cp))                  # samples_per_pixel == 0
    _invalid(trt, call(sp, sp, 4, 8, 9, None, 4, op, cp))                  # more samples done than the frame has
    _invalid(trt, call(None, None, 4, 8, 4, None, 0, None, None))          # an empty list still needs somewhere to write its count
    if device:
        _invalid(trt, call(sp, sp, 4, 8, 4, None, 4, op, cp, scr=None))
        _invalid(trt, call(sp, sp, 4, 8, 4, None, 4, op, cp, scr_bytes=15))
        assert "scratch" in trt.lib.trt_last_error().decode()
    assert count.value == 77 and (out == 9).all()


def test_select_of_nothing_succeeds_without_a_device(trt):
    count = C.c_uint32(77)
    assert trt.lib.trt_select_pixels(None, None, 0, 8, 4, None, 0, 0.1, 0.0, None, C.byref(count)) == trt._lib.TRT_OK
    assert count.value == 0
    got = trt.select_pixels(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 8, 4, 0.1)
    assert got.dtype == np.uint32 and len(got) == 0
    got = trt.select_pixels(np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32), 8, 4, 0.1, candidates=np.zeros(0, np.uint32))
    assert len(got) == 0
    if trt.lib.trt_device_count() == 0:
        # the device form has no buffer it could write without a device: it succeeds and writes nothing
        assert trt.lib.trt_select_pixels_device(None, None, 0, 8, 4, None, 0, 0.1, 0.0, None, C.byref(count), None, 0, None) == trt._lib.TRT_OK


def test_select_scratch_bytes_is_monotone_and_zero_safe(trt):
    assert trt.select_scratch_bytes(0) == 0
    assert trt.select_scratch_bytes(1) >= 4
    sizes = [trt.select_scratch_bytes(n) for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 2 ** 20, 2 ** 20 + 1, 2 ** 24,
                                                   2 ** 31, 2 ** 32 - 1)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[1]
    assert all(b % 4 == 0 for b in sizes)
    assert sizes[-1] < 2 ** 32 - 1                                          # far less than a word per candidate


def test_python_wrappers_check_their_arguments(trt):
    sc, cam = _scene_camera(trt)
    r = trt.Renderer(4, 1, 4, False, (0.1, 0.2, 0.3), seed=5)
    with pytest.raises(AssertionError):
        r.render_pixels(cam, sc, [0], np.zeros((8, 8, 3), np.float64))
    with pytest.raises(AssertionError):
        r.render_pixels(cam, sc, [0], np.zeros((8, 7, 3), np.float32))
    with pytest.raises(ValueError):
        trt.select_pixels(np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32), 8, 4, 0.1)
    for bad in (dict(min_spp=1, step_spp=1), dict(min_spp=5, step_spp=1), dict(min_spp=2, step_spp=0)):
        with pytest.raises(ValueError):
            r.render_adaptive(cam, sc, rel_tol=0.1, abs_tol=0.0, **bad)


def test_the_plan_symbol_checks_its_arguments(trt):
    sc, _ = _scene_camera(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_pixels_launch_plan(None, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_pixels_launch_plan(sc._h, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_pixels_launch_plan(sc._h, 1, 0, C.byref(out)) == want
    assert trt.lib.trt_pixels_launch_plan(sc._h, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.pixels_plan(1, 304)["compute_units"] == 304


PIXEL_COUNTS = (0, 1, 255, 256, 257, 2345, 9170, 2 ** 24)                   # tests/test_aov_abi.py


def test_pixels_launch_plan_invariants_on_every_scene_and_option_of_the_gpu_tests(trt):
    """Every (scene, options) of test_gpu_queries.PLAN_CASES at 256 compute units and every list length of PIXEL_COUNTS: the invariants
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
            q = sc.pixels_plan(n, cus)
            tag = (name, options, n, q)
            _check_query_plan(q, n, cus, streamed, tag)
            assert G.plan_shape(q) == shape, tag
            per_wave, waves = q["rays_per_wave"], q["waves"]
            assert (waves - 1) * per_wave < n <= waves * per_wave if n else waves == 0, tag
            assert q["workgroups"] == -(-waves // (q["threads_per_workgroup"] // 64)), tag
            lengthened += per_wave > 256
            shapes.add(shape[:3])
            if q["fallback"]:
                routes.add((q["scene_mode"], q["streamed_walk"]))
        # the plan of the feature buffers for as many pixels is the same kernel shape and LDS layout; the launch bound is this kernel's own
        # (a whole path and two sums live across the walk: pixels.hip kPixelsKernels), and with it the resident waves and a long list's runs
        qa, qp = sc.aov_plan(2345, cus), sc.pixels_plan(2345, cus)
        for k in ("scene_mode", "walk", "threads_per_workgroup", "leaf_slots", "stragglers", "lds_bytes", "fallback", "rays_per_wave"):
            assert qa[k] == qp[k], (name, options, k)
        assert 1 <= qp["kernel_waves_per_simd"] <= qa["kernel_waves_per_simd"]
    assert shapes == PIXELS_KERNEL_SHAPES, sorted(shapes)
    assert {(1, WALK_LDS_TREE), (1, WALK_LOCK_STEP), (0, WALK_LOCK_STEP)} <= routes, sorted(routes)
    assert lengthened > 0                                                    # 2^24 entries lengthen the runs of some shape


def test_the_gpu_tests_case_lists_reach_every_kernel_and_every_route_to_the_fallback(trt):
    """tests/test_gpu_pixels.py renders its SCENES with default options and tests/test_gpu_pixels_walks.py its CASES; passed through the
    plan at the image sizes those modules use, the union must launch all six instantiations of kPixelsKernels and reach the register-slot
    fallback from an LDS tree plan, from a lock-step plan in LDS and from a lock-step plan in global memory - so that dropping a case
    there, or a later change to the plan, cannot leave a kernel or a route unrun without this test failing."""
    import test_gpu_pixels as P
    import test_gpu_pixels_walks as PW
    import test_gpu_queries as G
    import walk_ray_cases as W
    cases = [(name, {}, G.DEFAULT_SHAPES[name]) for name in P.SCENES] + list(PW.CASES)
    assert len(cases) == len(P.SCENES) + len(G.OTHER_WALKS) + 2 and [c[0] for c in cases[-2:]] == ["degenerate", "nonfinite"]
    shapes, routes, worlds = set(), set(), {}
    for name, options, shape in cases:
        if name not in worlds:
            worlds[name] = trt.world_from_description(W.scene(trt, name))[0]
        host_options = {k: v for k, v in options.items() if k != "on_device"}           # (both compilers give the same bytes: tests/test_gpu_scene_build.py)
        sc = worlds[name].get_bvh(**host_options) if host_options else worlds[name].get_bvh()
        for w, h in PW.SIZES:
            q = sc.pixels_plan(w * h, 256)
            assert G.plan_shape(q) == shape, (name, options, G.plan_shape(q), shape)
            shapes.add(shape[:3])
            if q["fallback"]:
                routes.add((q["scene_mode"], q["streamed_walk"]))
    # the default compilations alone miss the register-slot walk from global memory: the reason tests/test_gpu_pixels_walks.py exists
    assert {G.DEFAULT_SHAPES[name][:3] for name in P.SCENES} == PIXELS_KERNEL_SHAPES - {(0, 5, 256)}
    assert shapes == PIXELS_KERNEL_SHAPES, sorted(shapes)
    assert {(1, WALK_LDS_TREE), (1, WALK_LOCK_STEP), (0, WALK_LOCK_STEP)} <= routes, sorted(routes)


def test_the_device_selection_refuses_overlapping_lists_before_any_device_work(trt):
    """select_write_kernel cannot compact in place, so trt_select_pixels_device returns TRT_ERR_INVALID_ARG when the n words at d_selected
    overlap the n words at d_candidates: equal pointers, a partial overlap on either side.  Adjacent ranges pass this check and reach the
    next one (here made to fail: a scratch that is too small - host pointers are handed in, so no call may get as far as a launch)."""
    n = 300
    s = np.full((n, 3), 0.5, np.float32)
    buf = np.full(3 * n, 9, np.uint32)
    count = C.c_uint32(77)
    scratch = np.zeros(64, np.uint32)
    assert trt.select_scratch_bytes(n) <= 4 * len(scratch)

    def call(cand_word, sel_word, scr_bytes=4 * len(scratch)):
        return trt.lib.trt_select_pixels_device(s.ctypes.data, s.ctypes.data, n, 8, 4, buf.ctypes.data + 4 * cand_word, n, 0.1, 0.0,
                                                buf.ctypes.data + 4 * sel_word, C.byref(count), scratch.ctypes.data, scr_bytes, None)

    for cand_word, sel_word in ((n, n), (n, n + 1), (n, n - 1), (n, 2 * n - 1), (n, 1), (0, n - 1), (n - 1, 0)):
        _invalid(trt, call(cand_word, sel_word))
        assert "overlap" in trt.lib.trt_last_error().decode(), (cand_word, sel_word)
        _invalid(trt, call(cand_word, sel_word, scr_bytes=0))              # ... and before the scratch is looked at
        assert "overlap" in trt.lib.trt_last_error().decode(), (cand_word, sel_word)
    for cand_word, sel_word in ((n, 2 * n), (n, 0), (0, n), (0, 2 * n)):
        _invalid(trt, call(cand_word, sel_word, scr_bytes=0))
        assert "scratch" in trt.lib.trt_last_error().decode(), (cand_word, sel_word)
    # candidates NULL (the pixels 0 .. n-1) has nothing to overlap; n == 0 reads and writes no list
    _invalid(trt, trt.lib.trt_select_pixels_device(s.ctypes.data, s.ctypes.data, n, 8, 4, None, n, 0.1, 0.0, buf.ctypes.data, C.byref(count),
                                                   scratch.ctypes.data, 0, None))
    assert "scratch" in trt.lib.trt_last_error().decode()
    if trt.lib.trt_device_count() == 0:
        assert trt.lib.trt_select_pixels_device(None, None, 0, 8, 4, buf.ctypes.data, 0, 0.1, 0.0, buf.ctypes.data, C.byref(count), None, 0,
                                                None) == trt._lib.TRT_OK
        # without a device the well-formed adjacent call gets as far as the device check
        assert call(n, 2 * n) == trt._lib.ERR_NO_DEVICE
    assert count.value == 77 and (buf == 9).all()
    with pytest.raises(trt.TinyRTError) as e:
        trt.select_pixels_device(s.ctypes.data, s.ctypes.data, n, 8, 4, n, 0.1, 0.0, buf.ctypes.data, C.addressof(count), scratch.ctypes.data,
                                 4 * len(scratch), d_candidates_ptr=buf.ctypes.data)
    assert e.value.code == trt._lib.ERR_INVALID_ARG
