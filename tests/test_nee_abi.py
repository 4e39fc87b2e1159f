"""The next-event entry points (tinyrt.h trt_nee, trt_nee_device, trt_nee_launch_plan, trt_nee_params_default) at the C boundary, without
a GPU: the symbols are declared, exported, bound and listed, the struct has the header's layout (ctypes, numpy, gcc), the defaults land in
a 0xCD-filled struct, misuse comes back as TRT_ERR_INVALID_ARG with a message before any device work, an empty batch succeeds without a
device, and the launch plan is the passes queries' but for the kernel's launch bound.  What the buffers hold is checked on the GPU
(tests/test_gpu_nee.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import direct_cases as D
from test_query_abi import _check_query_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trt_nee_params_default": (None, 1), "trt_nee": (C.c_int, 9), "trt_nee_device": (C.c_int, 10), "trt_nee_launch_plan": (C.c_int, 4)}
# tinyrt.h trt_nee_params as a numpy record (128 bytes)
PATH_DTYPE = np.dtype([("samples_per_ray", np.uint32), ("max_bounces", np.uint32), ("background", np.float32, (3,)), ("seed", np.uint32),
                       ("sample_begin", np.uint32), ("sample_end", np.uint32), ("accumulate", np.uint32), ("first_stream", np.uint32),
                       ("reserved", np.uint32, (6,))])
GATHER_DTYPE = np.dtype([("path", PATH_DTYPE), ("lobe", np.uint32), ("spread", np.float32), ("reserved", np.uint32, (6,))])
NEE_DTYPE = np.dtype([("gather", GATHER_DTYPE), ("shadow_end", np.float32), ("source_is_diffuse", np.uint32), ("reserved", np.uint32, (6,))])


def test_the_symbols_are_declared_exported_bound_and_listed(trt):
    text = open(os.path.join(ROOT, "include", "tinyrt.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(trt._lib.LIB_PATH)
    later = re.search(r"Later under 4[^/]*\*/", text, flags=re.S).group(0)
    for name, (restype, nargs) in NAMES.items():
        ret = "void" if restype is None else "int"
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", header), name + " is not declared in tinyrt.h"
        assert hasattr(raw, name), name + " is not exported"
        res, args = trt._lib.SIGNATURES[name]
        assert res is restype and len(args) == nargs, name
        assert name in later, name + " is not listed under 'Later under 4'"
    assert "trt_nee_params," in later
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    P = trt._lib.NeeParams
    assert C.sizeof(P) == 128
    assert (P.gather.offset, P.shadow_end.offset, P.source_is_diffuse.offset, P.reserved.offset) == (0, 96, 100, 104) and P.reserved.size == 24
    assert NEE_DTYPE.itemsize == 128 and [NEE_DTYPE.fields[n][1] for n in NEE_DTYPE.names] == [0, 96, 100, 104]
    assert C.sizeof(trt._lib.GatherParams) == 96 and C.sizeof(trt._lib.PassesParams) == 128     # unchanged
    # the signatures are the direct-light queries' with the other parameter struct
    for name in ("trt_nee", "trt_nee_device"):
        mine, theirs = trt._lib.SIGNATURES[name][1], trt._lib.SIGNATURES[name.replace("nee", "direct")][1]
        assert mine[5] is C.POINTER(P), name
        assert mine[:5] + mine[6:] == theirs[:5] + theirs[6:], name
    assert trt._lib.SIGNATURES["trt_nee_launch_plan"][1] == trt._lib.SIGNATURES["trt_direct_launch_plan"][1]
    for name in ("nee", "nee_device", "nee_plan"):
        assert callable(getattr(trt.Scene, name))
    # the struct in the header, field for field
    m = re.search(r"typedef struct \{([^}]*)\}\s*trt_nee_params\s*;", header)
    assert m and re.findall(r"(\w+)\s+(\w+)(\[\d+\])?\s*;", m.group(1)) == [
        ("trt_gather_params", "gather", ""), ("float", "shadow_end", ""), ("uint32_t", "source_is_diffuse", ""), ("uint32_t", "reserved", "[6]")]


def test_the_layout_matches_the_c_compiler(trt, tmp_path):
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tinyrt.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(trt_nee_params), offsetof(trt_nee_params, gather), offsetof(trt_nee_params, shadow_end), '
                   'offsetof(trt_nee_params, source_is_diffuse), offsetof(trt_nee_params, reserved)); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [128, 0, 96, 100, 104]


def test_the_default_parameters(trt):
    p = trt._lib.NeeParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    trt.lib.trt_nee_params_default(C.byref(p))
    want = trt._lib.PassesParams()
    trt.lib.trt_passes_params_default(C.byref(want))
    assert bytes(p.gather) == bytes(want.gather) and p.gather.lobe == trt._lib.PASSES_COSINE
    assert np.float32(p.shadow_end) == np.float32(0.999) and p.source_is_diffuse == 0 and list(p.reserved) == [0] * 6
    rec = np.frombuffer(bytes(p), NEE_DTYPE)[0]
    assert rec["shadow_end"] == np.float32(0.999) and rec["source_is_diffuse"] == 0 and rec["gather"]["path"]["max_bounces"] == 50
    trt.lib.trt_nee_params_default(None)                                   # tolerated


def _scene(trt):
    return trt.world_from_description(trt.scenes.cornell(8, 8))[0].get_bvh()


PATH_FIELDS = ("samples_per_ray", "max_bounces", "seed", "sample_begin", "sample_end", "accumulate", "first_stream")
GATHER_FIELDS = ("lobe", "spread")


def _params(trt, **over):
    """K = 4, seed 5; a keyword that names a field of the path or of the gather parameters sets it there."""
    p = trt._lib.NeeParams()
    trt.lib.trt_nee_params_default(C.byref(p))
    p.gather.path.samples_per_ray, p.gather.path.seed = 4, 5
    for k, v in over.items():
        setattr(p.gather.path if k in PATH_FIELDS else p.gather if k in GATHER_FIELDS else p, k, v)
    return p


def _invalid(trt, rc, word=None):
    assert rc == trt._lib.ERR_INVALID_ARG
    msg = trt.lib.trt_last_error().decode()
    assert msg != "" and (word is None or word in msg), msg


N = 3


def _call(trt, device, s, items, n, table, n_emitters, p, rad, m2):
    if device:
        return trt.lib.trt_nee_device(s, items, n, table, n_emitters, p, rad, m2, None, None)
    return trt.lib.trt_nee(s, items, n, table, n_emitters, p, rad, m2, None)


@pytest.mark.parametrize("device", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    rad = np.full((N, 3), 7.0, np.float32)
    m2 = np.full((N, 3), 7.0, np.float32)
    table = trt.lights.table(sc.emitters(), trt.lights.sphere((50.0, 50.0, 50.0), 2.0, (1.0, 1.0, 1.0)))
    E = len(table)
    assert E == 2
    ip, rp, mp, tp = items.ctypes.data, rad.ctypes.data, m2.ctypes.data, table.ctypes.data
    p = _params(trt)

    def call(s, r, n, q, a, b, t=tp, e=E):
        return _call(trt, device, s, r, n, t, e, C.byref(q) if q is not None else None, a, b)

    _invalid(trt, call(None, ip, N, p, rp, mp))
    _invalid(trt, call(sc._h, ip, N, None, rp, mp))
    _invalid(trt, call(sc._h, None, N, p, rp, mp))
    _invalid(trt, call(sc._h, ip, N, p, None, mp))
    # trt_passes' own errors on `gather`: everything trt_radiance reports on the path ...
    _invalid(trt, call(sc._h, ip, N, _params(trt, samples_per_ray=0), rp, mp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=3, sample_end=2), rp, mp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_end=5), rp, mp))                          # K + 1
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=5), rp, mp))                        # past K after the end == 0 rule
    for k in range(6):
        q = _params(trt)
        q.gather.path.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, rp, mp), "reserved")
    # ... the source, the cone's spread and the reserved words
    for lobe in (3, 4, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, lobe=lobe), rp, mp), "source")
    for spread in (-1.0, float("nan"), float("inf")):
        _invalid(trt, call(sc._h, ip, N, _params(trt, lobe=trt._lib.PASSES_CONE, spread=spread), rp, mp), "spread")
    for k in range(6):
        q = _params(trt)
        q.gather.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, rp, mp), "reserved")
    # trt_direct's on the table
    _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=None), "emitter")
    for e in (0, 2 ** 20 + 1, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, e=e), "n_emitters")
    if not device:                                                          # the device form cannot read the table
        for kind in (2, 3, 2 ** 32 - 1):
            bad = table.copy()
            bad["kind"][1] = kind
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=bad.ctypes.data), "kind")
        for k in range(2):
            bad = table.copy()
            bad["reserved"][0, k] = 1
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=bad.ctypes.data), "reserved")
    # ... and on shadow_end
    for end in (float("nan"), 0.0, -0.0, -1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0))), 2.0, float("inf"), -float("inf")):
        _invalid(trt, call(sc._h, ip, N, _params(trt, shadow_end=end), rp, mp), "shadow_end")
    # this struct's own
    for v in (2, 3, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, source_is_diffuse=v), rp, mp), "source_is_diffuse")
    for k in range(6):
        q = _params(trt)
        q.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, rp, mp), "reserved")
    # the RNG stream index must not wrap: first_stream + n * K <= 2^32, computed in 64 bits
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    edge = 2 ** 32 - N * 4
    if not device or want_ok != trt._lib.TRT_OK:                            # (the device form is given host pointers: never let it launch)
        assert call(sc._h, ip, N, _params(trt, first_stream=edge), rp, mp) == want_ok
        for kw in (dict(max_bounces=0), dict(shadow_end=1.0), dict(shadow_end=1e-30), dict(source_is_diffuse=1), dict(lobe=trt._lib.PASSES_RAYS),
                   dict(lobe=trt._lib.PASSES_RAYS, spread=float("nan")), dict(lobe=trt._lib.PASSES_CONE, spread=0.5)):
            assert call(sc._h, ip, N, _params(trt, **kw), rp, mp) == want_ok, kw
        assert call(sc._h, ip, N, p, rp, None) == want_ok                                          # moment2 is optional
        assert call(sc._h, ip, N, p, rp, mp, e=1) == want_ok
        rad[:] = 7.0
        m2[:] = 7.0
    _invalid(trt, call(sc._h, ip, N, _params(trt, first_stream=edge + 1), rp, mp), "2^32")
    _invalid(trt, call(sc._h, ip, 2 ** 32 - 1, _params(trt, samples_per_ray=2 ** 32 - 1, first_stream=2 ** 32 - 1), rp, mp))       # n * K needs 64 bits
    # ... and an empty batch is checked too, but for the table, which it does not need
    _invalid(trt, call(None, None, 0, p, None, None))
    _invalid(trt, call(sc._h, None, 0, None, None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, samples_per_ray=0), None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, shadow_end=float("nan")), None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, source_is_diffuse=2), None, None))
    q = _params(trt)
    q.reserved[5] = 1
    _invalid(trt, call(sc._h, None, 0, q, None, None))
    assert (rad == 7.0).all() and (m2 == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = _scene(trt)
    rad = np.full((N, 3), 7.0, np.float32)
    p = _params(trt, first_stream=2 ** 32 - 1, shadow_end=0.5, source_is_diffuse=1)     # n * K == 0: any first stream passes
    assert _call(trt, device, sc._h, None, 0, None, 0, C.byref(p), None, None) == trt._lib.TRT_OK
    assert _call(trt, device, sc._h, None, 0, None, 7, C.byref(p), rad.ctypes.data, rad.ctypes.data) == trt._lib.TRT_OK
    assert (rad == 7.0).all()
    got, m2, st = sc.nee(np.zeros((0, 6), np.float32), sc.emitters(), 4, moment2=True)
    assert got.shape == (0, 3) and m2.shape == (0, 3) and st["samples"] == 0 and st["rays"] == 0


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path.  With one: success."""
    sc = _scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 0:3] = (50.0, 0.0, 50.0)
    items[:, 4] = 1.0
    rad = np.full((N, 3), 7.0, np.float32)
    table = sc.emitters()
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt)
    assert trt.lib.trt_nee(sc._h, items.ctypes.data, N, table.ctypes.data, len(table), C.byref(p), rad.ctypes.data, None, None) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (rad == 7.0).all()
        assert trt.lib.trt_nee_device(sc._h, items.ctypes.data, N, table.ctypes.data, len(table), C.byref(p), rad.ctypes.data, None, None, None) == want
        with pytest.raises(trt.TinyRTError) as e:
            sc.nee(items, table, 4)
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (rad == 7.0).all()


def test_python_wrappers_check_their_arguments(trt):
    sc = _scene(trt)
    table = sc.emitters()
    with pytest.raises(ValueError):
        sc.nee(np.zeros((2, 5), np.float32), table, 4)
    with pytest.raises(ValueError):
        sc.nee(np.zeros((2, 6), np.float32), np.zeros((1, 20), np.float32), 4)
    with pytest.raises(ValueError):
        sc.nee(np.zeros((2, 6), np.float32), table, 4, source="sphere")
    with pytest.raises(AssertionError):
        sc.nee(np.zeros((2, 6), np.float32), table, 4, radiance=np.zeros((2, 3), np.float64))
    with pytest.raises(AssertionError):
        sc.nee(np.zeros((2, 6), np.float32), table, 4, moment2=np.zeros((3, 3), np.float32))
    for kw in (dict(samples_per_item=0), dict(samples_per_item=4, shadow_end=0.0), dict(samples_per_item=4, source_is_diffuse=2)):
        with pytest.raises(trt.TinyRTError) as e:
            sc.nee(np.zeros((2, 6), np.float32), table, **kw)
        assert e.value.code == trt._lib.ERR_INVALID_ARG
    with pytest.raises(trt.TinyRTError) as e:
        sc.nee(np.zeros((2, 6), np.float32), table[:0], 4)                  # an empty table
    assert e.value.code == trt._lib.ERR_INVALID_ARG
    p = trt.Scene._nee_params(7, source="cone", spread=0.25, shadow_end=0.5, source_is_diffuse=True, max_bounces=3, seed=9, first_stream=11,
                              sample_begin=1, sample_end=5, accumulate=True)
    g = p.gather
    assert (g.path.samples_per_ray, g.path.max_bounces, g.path.seed, g.path.first_stream, g.lobe, g.spread) == (7, 3, 9, 11, 2, 0.25)
    assert (g.path.sample_begin, g.path.sample_end, g.path.accumulate, p.shadow_end, p.source_is_diffuse) == (1, 5, 1, 0.5, 1)
    d = trt.Scene._nee_params(3)
    assert (np.float32(d.shadow_end), d.source_is_diffuse, d.gather.lobe, d.gather.path.sample_end) == (np.float32(0.999), 0, 1, 0)


def test_the_plan_symbol_checks_its_arguments(trt):
    sc = _scene(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_nee_launch_plan(None, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_nee_launch_plan(sc._h, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_nee_launch_plan(sc._h, 1, 0, C.byref(out)) == want
    assert trt.lib.trt_nee_launch_plan(sc._h, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.nee_plan(1, 304)["compute_units"] == 304


RAY_COUNTS = (1, 64, 257, 324, 100003, 2 ** 32 - 1)                          # test_radiance_abi.py's
# what plan_batch (stream_plan.h) derives from the kernel's launch bound: the resident workgroups and wave slots, and through them the runs
# of a batch too long for 256 items per wave
FROM_THE_BOUND = ("kernel_waves_per_simd", "workgroups_per_cu", "wave_slots")
FROM_THE_SLOTS = ("rays_per_wave", "waves", "workgroups")
# nee.hip kNeeKernels[pick][mis][source], the plain tables (profiles/nee_resource_usage.txt): (scene mode, walk, threads) -> launch bound
BOUNDS = {(1, 2, 256): 5, (1, 1, 256): 6, (1, 1, 768): 6, (1, 5, 512): 5, (0, 3, 256): 5, (0, 5, 256): 5}


def test_the_nee_plan_is_the_passes_plan_but_for_the_kernel_bound(trt):
    """Every (scene, options) of test_gpu_queries.PLAN_CASES at 256 compute units and every batch size test_radiance_abi.py walks: the
    plan's invariants, the listed kernel shape, and every field equal to trt_passes_launch_plan's but the bound and what the launch rule
    derives from it, and those obey the rule.  Every shape of the table is reached."""
    import test_gpu_queries as G
    import walk_ray_cases as W
    cus = 256
    r = trt.Renderer(4, 1, 8, False, (0.1, 0.1, 0.1))
    shapes, worlds, bounds = set(), {}, {}
    for name, options, shape in G.PLAN_CASES:
        if name not in worlds:
            worlds[name] = trt.world_from_description(W.scene(trt, name))
        world, cam = worlds[name]
        host_options = {k: v for k, v in options.items() if k != "on_device"}
        sc = world.get_bvh(**host_options) if host_options else world.get_bvh()
        streamed = r.launch_plan(cam, sc)
        for n in RAY_COUNTS:
            q, qa = sc.nee_plan(n, cus), sc.passes_plan(n, 3, cus)
            tag = (name, options, n, q, qa)
            _check_query_plan(q, n, cus, streamed, tag)
            assert G.plan_shape(q) == shape, tag
            assert set(q) == set(qa)
            assert 1 <= q["kernel_waves_per_simd"] <= 8
            same_bound = q["kernel_waves_per_simd"] == qa["kernel_waves_per_simd"]
            lengthened = q["rays_per_wave"] > 256 or qa["rays_per_wave"] > 256
            for k in q:
                if same_bound or not (k in FROM_THE_BOUND or (lengthened and k in FROM_THE_SLOTS)):
                    assert q[k] == qa[k], (k, tag)
            per_wave, waves = q["rays_per_wave"], q["waves"]
            assert (waves - 1) * per_wave < n <= waves * per_wave, tag
            assert q["workgroups"] == -(-waves // (q["threads_per_workgroup"] // 64)), tag
            shapes.add(shape[:3])
            bounds[shape[:3]] = q["kernel_waves_per_simd"]
    assert len(shapes) == 6, sorted(shapes)                                 # every entry of the tables
    assert bounds == BOUNDS, bounds
