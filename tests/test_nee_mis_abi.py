"""The weighted next-event entry points (tinyrt.h trt_nee_mis, trt_nee_mis_device, trt_nee_mis_launch_plan, trt_nee_mis_params_default) at
the C boundary, without a GPU: the symbols are declared, exported, bound and listed, the struct has the header's layout (ctypes, numpy,
gcc), the defaults land in a 0xCD-filled struct, misuse comes back as TRT_ERR_INVALID_ARG with a message before any device work - the
table rule of the host form included - an empty batch succeeds without a device, and the launch plan is the next-event queries' but for
the weighted kernels' launch bounds.  What the buffers hold is checked on the GPU (tests/test_gpu_nee_mis.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_nee_abi as A
from test_query_abi import _check_query_plan

ROOT = A.ROOT
NAMES = {"trt_nee_mis_params_default": (None, 1), "trt_nee_mis": (C.c_int, 9), "trt_nee_mis_device": (C.c_int, 10),
         "trt_nee_mis_launch_plan": (C.c_int, 4)}
# tinyrt.h trt_nee_mis_params as a numpy record (160 bytes)
MIS_DTYPE = np.dtype([("nee", A.NEE_DTYPE), ("heuristic", np.uint32), ("reserved", np.uint32, (7,))])
N = A.N
_invalid = A._invalid


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
    assert "trt_nee_mis_params," in later and "trt_mis_heuristic," in later
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    P = trt._lib.NeeMisParams
    assert C.sizeof(P) == 160
    assert (P.nee.offset, P.heuristic.offset, P.reserved.offset) == (0, 128, 132) and P.reserved.size == 28
    assert MIS_DTYPE.itemsize == 160 and [MIS_DTYPE.fields[n][1] for n in MIS_DTYPE.names] == [0, 128, 132]
    assert C.sizeof(trt._lib.NeeParams) == 128                             # unchanged
    assert (trt._lib.MIS_BALANCE, trt._lib.MIS_POWER) == (0, 1)
    assert re.search(r"enum\s+trt_mis_heuristic\s*\{\s*TRT_MIS_BALANCE\s*=\s*0\s*,\s*TRT_MIS_POWER\s*=\s*1\s*\}", header)
    # the signatures are the next-event queries' with the other parameter struct
    for name in ("trt_nee_mis", "trt_nee_mis_device"):
        mine, theirs = trt._lib.SIGNATURES[name][1], trt._lib.SIGNATURES[name.replace("_mis", "")][1]
        assert mine[5] is C.POINTER(P), name
        assert mine[:5] + mine[6:] == theirs[:5] + theirs[6:], name
    assert trt._lib.SIGNATURES["trt_nee_mis_launch_plan"][1] == trt._lib.SIGNATURES["trt_nee_launch_plan"][1]
    m = re.search(r"typedef struct \{([^}]*)\}\s*trt_nee_mis_params\s*;", header)
    assert m and re.findall(r"(\w+)\s+(\w+)(\[\d+\])?\s*;", m.group(1)) == [
        ("trt_nee_params", "nee", ""), ("uint32_t", "heuristic", ""), ("uint32_t", "reserved", "[7]")]


def test_the_layout_matches_the_c_compiler(trt, tmp_path):
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tinyrt.h"\nint main(void) { printf("%zu %zu %zu %zu %d %d\\n", '
                   'sizeof(trt_nee_mis_params), offsetof(trt_nee_mis_params, nee), offsetof(trt_nee_mis_params, heuristic), '
                   'offsetof(trt_nee_mis_params, reserved), (int)TRT_MIS_BALANCE, (int)TRT_MIS_POWER); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [160, 0, 128, 132, 0, 1]


def test_the_default_parameters(trt):
    p = trt._lib.NeeMisParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    trt.lib.trt_nee_mis_params_default(C.byref(p))
    want = trt._lib.NeeParams()
    trt.lib.trt_nee_params_default(C.byref(want))
    assert bytes(p.nee) == bytes(want) and p.heuristic == trt._lib.MIS_BALANCE and list(p.reserved) == [0] * 7
    rec = np.frombuffer(bytes(p), MIS_DTYPE)[0]
    assert rec["heuristic"] == 0 and rec["nee"]["shadow_end"] == np.float32(0.999) and rec["nee"]["gather"]["lobe"] == 1
    trt.lib.trt_nee_mis_params_default(None)                               # tolerated


def _params(trt, heuristic=0, **over):
    """test_nee_abi._params (K = 4, seed 5) inside a trt_nee_mis_params."""
    p = trt._lib.NeeMisParams()
    trt.lib.trt_nee_mis_params_default(C.byref(p))
    p.nee = A._params(trt, **over)
    p.heuristic = heuristic
    return p


def _call(trt, device, s, items, n, table, n_emitters, p, rad, m2):
    if device:
        return trt.lib.trt_nee_mis_device(s, items, n, table, n_emitters, p, rad, m2, None, None)
    return trt.lib.trt_nee_mis(s, items, n, table, n_emitters, p, rad, m2, None)


def _two_lamps(trt):
    """The Cornell box with a second, spherical lamp: two TRT_LIGHT geometries."""
    desc = trt.scenes.cornell(8, 8)
    desc = dict(desc, geometries=list(desc["geometries"]) + [("sphere", (50.0, 50.0, 50.0), 5.0, "light")])
    return trt.world_from_description(desc)[0].get_bvh()


@pytest.mark.parametrize("device", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work(trt, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)"""
    sc = A._scene(trt)
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
    # trt_nee's own errors on `nee`: one of each family (tests/test_nee_abi.py walks them all through trt_nee, which shares the check)
    _invalid(trt, call(sc._h, ip, N, _params(trt, samples_per_ray=0), rp, mp))
    _invalid(trt, call(sc._h, ip, N, _params(trt, sample_begin=3, sample_end=2), rp, mp))
    for k in range(6):
        for where in ("path", "gather", "nee"):
            q = _params(trt)
            (q.nee.gather.path if where == "path" else q.nee.gather if where == "gather" else q.nee).reserved[k] = 1
            _invalid(trt, call(sc._h, ip, N, q, rp, mp), "reserved")
    _invalid(trt, call(sc._h, ip, N, _params(trt, lobe=3), rp, mp), "source")
    _invalid(trt, call(sc._h, ip, N, _params(trt, lobe=trt._lib.PASSES_CONE, spread=-1.0), rp, mp), "spread")
    _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=None), "emitter")
    for e in (0, 2 ** 20 + 1):
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, e=e), "n_emitters")
    for end in (float("nan"), 0.0, 2.0):
        _invalid(trt, call(sc._h, ip, N, _params(trt, shadow_end=end), rp, mp), "shadow_end")
    _invalid(trt, call(sc._h, ip, N, _params(trt, source_is_diffuse=2), rp, mp), "source_is_diffuse")
    _invalid(trt, call(sc._h, ip, N, _params(trt, first_stream=2 ** 32 - N * 4 + 1), rp, mp), "2^32")
    # this struct's own
    for h in (2, 3, 2 ** 32 - 1):
        _invalid(trt, call(sc._h, ip, N, _params(trt, heuristic=h), rp, mp), "heuristic")
    for k in range(7):
        q = _params(trt)
        q.reserved[k] = 1
        _invalid(trt, call(sc._h, ip, N, q, rp, mp), "reserved")
    if not device:                                                          # the device form cannot read the table
        for kind in (2, 2 ** 32 - 1):
            bad = table.copy()
            bad["kind"][1] = kind
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=bad.ctypes.data), "kind")
        bad = table.copy()
        bad["reserved"][0, 1] = 1
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=bad.ctypes.data), "reserved")
        # the table rule: a light missing ...
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=table[1:].copy().ctypes.data, e=1), "lights")
        # ... a light twice ...
        twice = np.ascontiguousarray(np.concatenate([table, table[:1]]))
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=twice.ctypes.data, e=3), "lights")
        # ... a geometry word that is no light (geometry 3 of the box is its floor; and an index past the world)
        for g in (3, 1000):
            bad = table.copy()
            bad["geometry"][1] = g
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=bad.ctypes.data), "lights")
        bad = table.copy()
        bad["geometry"][0] = 3
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=bad.ctypes.data), "lights")
        # ... on a scene with two lamps, one of them alone, in either order both pass the rule
        two = _two_lamps(trt)
        both = two.emitters()
        assert len(both) == 2 and sorted(both["kind"]) == [0, 1]
        for one in (both[:1], both[1:]):
            _invalid(trt, call(two._h, ip, N, p, rp, mp, t=one.copy().ctypes.data, e=1), "lights")
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    if not device or want_ok != trt._lib.TRT_OK:                            # (the device form is given host pointers: never let it launch)
        for kw in (dict(), dict(heuristic=1), dict(max_bounces=0), dict(source_is_diffuse=1), dict(lobe=trt._lib.PASSES_RAYS),
                   dict(first_stream=2 ** 32 - N * 4)):
            assert call(sc._h, ip, N, _params(trt, **kw), rp, mp) == want_ok, kw
        assert call(sc._h, ip, N, p, rp, None) == want_ok                                          # moment2 is optional
        assert call(sc._h, ip, N, p, rp, mp, e=1) == want_ok                                       # the lamp alone
        swapped = np.ascontiguousarray(table[::-1])
        assert call(sc._h, ip, N, p, rp, mp, t=swapped.ctypes.data) == want_ok                     # any order
        if not device:
            two = _two_lamps(trt)
            both = np.ascontiguousarray(two.emitters()[::-1])
            assert call(two._h, ip, N, p, rp, mp, t=both.ctypes.data, e=2) == want_ok
        rad[:] = 7.0
        m2[:] = 7.0
    # an empty batch is checked too, but for the table, which it does not need
    _invalid(trt, call(None, None, 0, p, None, None))
    _invalid(trt, call(sc._h, None, 0, None, None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, heuristic=2), None, None))
    _invalid(trt, call(sc._h, None, 0, _params(trt, source_is_diffuse=2), None, None))
    q = _params(trt)
    q.reserved[6] = 1
    _invalid(trt, call(sc._h, None, 0, q, None, None))
    assert (rad == 7.0).all() and (m2 == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = A._scene(trt)
    rad = np.full((N, 3), 7.0, np.float32)
    p = _params(trt, heuristic=1, first_stream=2 ** 32 - 1, shadow_end=0.5, source_is_diffuse=1)
    assert _call(trt, device, sc._h, None, 0, None, 0, C.byref(p), None, None) == trt._lib.TRT_OK
    assert _call(trt, device, sc._h, None, 0, None, 7, C.byref(p), rad.ctypes.data, rad.ctypes.data) == trt._lib.TRT_OK
    assert (rad == 7.0).all()
    for mis in ("balance", "power"):
        got, m2, st = sc.nee(np.zeros((0, 6), np.float32), sc.emitters(), 4, moment2=True, mis=mis)
        assert got.shape == (0, 3) and m2.shape == (0, 3) and st["samples"] == 0 and st["rays"] == 0


def test_well_formed_calls_need_a_device(trt):
    """Without a GPU: TRT_ERR_NO_DEVICE - there is no CPU path.  With one: success."""
    sc = A._scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 0:3] = (50.0, 0.0, 50.0)
    items[:, 4] = 1.0
    rad = np.full((N, 3), 7.0, np.float32)
    table = sc.emitters()
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    p = _params(trt)
    assert trt.lib.trt_nee_mis(sc._h, items.ctypes.data, N, table.ctypes.data, len(table), C.byref(p), rad.ctypes.data, None, None) == want
    if want != trt._lib.TRT_OK:
        assert "no HIP device" in trt.lib.trt_last_error().decode()
        assert (rad == 7.0).all()
        assert trt.lib.trt_nee_mis_device(sc._h, items.ctypes.data, N, table.ctypes.data, len(table), C.byref(p), rad.ctypes.data, None, None,
                                          None) == want
        with pytest.raises(trt.TinyRTError) as e:
            sc.nee(items, table, 4, mis="balance")
        assert e.value.code == trt._lib.ERR_NO_DEVICE
    else:
        assert not (rad == 7.0).all()


def test_python_wrappers_check_their_arguments(trt):
    sc = A._scene(trt)
    table = sc.emitters()
    with pytest.raises(ValueError):
        sc.nee(np.zeros((2, 6), np.float32), table, 4, mis="maximum")
    with pytest.raises(ValueError):
        sc.nee_device(0, 0, 0, 0, 0, samples_per_item=4, mis=1)
    with pytest.raises(trt.TinyRTError) as e:
        sc.nee(np.zeros((2, 6), np.float32), trt.lights.table(trt.lights.sphere((50.0, 50.0, 50.0), 2.0, (1.0, 1.0, 1.0))), 4, mis="power")
    assert e.value.code == trt._lib.ERR_INVALID_ARG                        # the lamp is missing from the table
    p = trt.Scene._nee_params(7, source="cone", spread=0.25, shadow_end=0.5, source_is_diffuse=True, mis="power", max_bounces=3, seed=9)
    assert isinstance(p, trt._lib.NeeMisParams) and p.heuristic == 1 and list(p.reserved) == [0] * 7
    g = p.nee.gather
    assert (g.path.samples_per_ray, g.path.max_bounces, g.path.seed, g.lobe, g.spread, p.nee.shadow_end, p.nee.source_is_diffuse) == (7, 3, 9, 2, 0.25, 0.5, 1)
    assert trt.Scene._nee_params(3, mis="balance").heuristic == 0
    assert isinstance(trt.Scene._nee_params(3), trt._lib.NeeParams)        # mis=None: trt_nee's struct, as before


def test_the_plan_symbol_checks_its_arguments(trt):
    sc = A._scene(trt)
    out = trt._lib.QueryPlan()
    assert trt.lib.trt_nee_mis_launch_plan(None, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
    assert trt.lib.trt_nee_mis_launch_plan(sc._h, 1, 256, None) == trt._lib.ERR_INVALID_ARG
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    assert trt.lib.trt_nee_mis_launch_plan(sc._h, 1, 0, C.byref(out)) == want
    assert trt.lib.trt_nee_mis_launch_plan(sc._h, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.nee_plan(1, 304, mis="power")["compute_units"] == 304


# nee.hip kNeeKernels[pick][mis][source], the weighted tables (profiles/nee_mis_resource_usage.txt): (scene mode, walk, threads) -> launch bound
BOUNDS = {(1, 2, 256): 5, (1, 1, 256): 5, (1, 1, 768): 5, (1, 5, 512): 5, (0, 3, 256): 5, (0, 5, 256): 5}


def test_the_weighted_plan_is_the_nee_plan_but_for_the_kernel_bound(trt):
    """Every (scene, options) of test_gpu_queries.PLAN_CASES at 256 compute units and every batch size test_nee_abi.py walks: the plan's
    invariants, the listed kernel shape, and every field equal to trt_nee_launch_plan's but the bound and what the launch rule derives from
    it.  Every shape of the table is reached, and the heuristic does not enter."""
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
        for n in A.RAY_COUNTS:
            q, qa = sc.nee_plan(n, cus, mis="balance"), sc.nee_plan(n, cus)
            assert q == sc.nee_plan(n, cus, mis="power")
            tag = (name, options, n, q, qa)
            _check_query_plan(q, n, cus, streamed, tag)
            assert G.plan_shape(q) == shape, tag
            assert set(q) == set(qa)
            same_bound = q["kernel_waves_per_simd"] == qa["kernel_waves_per_simd"]
            lengthened = q["rays_per_wave"] > 256 or qa["rays_per_wave"] > 256
            for k in q:
                if same_bound or not (k in A.FROM_THE_BOUND or (lengthened and k in A.FROM_THE_SLOTS)):
                    assert q[k] == qa[k], (k, tag)
            per_wave, waves = q["rays_per_wave"], q["waves"]
            assert (waves - 1) * per_wave < n <= waves * per_wave, tag
            assert q["workgroups"] == -(-waves // (q["threads_per_workgroup"] // 64)), tag
            shapes.add(shape[:3])
            bounds[shape[:3]] = q["kernel_waves_per_simd"]
    assert len(shapes) == 6, sorted(shapes)                                 # every entry of the tables
    assert bounds == BOUNDS, bounds
