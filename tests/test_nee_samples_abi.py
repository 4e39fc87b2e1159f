"""The sample-parallel next-event entry points (tinyrt.h trt_nee_samples, trt_nee_samples_device, trt_nee_samples_launch_plan,
trt_nee_samples_params, trt_nee_samples_params_default) at the C boundary, without a GPU: the names are declared, exported, bound and
listed; the struct has its documented layout and defaults; every documented error comes back as TRT_ERR_INVALID_ARG in the documented
order before any device work, for the four (weighted, pick) combinations, each with its sibling's step list behind the entry point's own
checks (the walk is tests/test_direct_pick_abi.py's, the lists are the ones tests/test_nee_pick_abi.py walks for the siblings); an empty
batch succeeds without a device; the Python wrappers hand the library what they should (the recorder of
tests/test_emitter_query_dispatch.py); the launch plan of n items with a range of R samples is the sibling's plan of n * R items but for
the kernel's launch bound, which is the one profiles/nee_samples_resource_usage.txt reports.  What the buffers hold is checked on the GPU
(tests/test_gpu_nee_samples.py, tests/test_gpu_nee_samples_long.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_direct_pick_abi as DP
import test_emitter_query_dispatch as ED
import test_nee_abi as A
import test_nee_mis_abi as AM
from test_query_abi import _check_query_plan

ROOT = A.ROOT
NAMES = {"trt_nee_samples_params_default": (None, 1), "trt_nee_samples": (C.c_int, 10), "trt_nee_samples_device": (C.c_int, 11),
         "trt_nee_samples_launch_plan": (C.c_int, 7)}
N, K = A.N, 4
_invalid = A._invalid
MODES, WALKS = {"MODE_LDS": 1, "MODE_GLOBAL": 0}, {"WALK_FLAT": 2, "WALK_LDS_STACK": 1, "WALK_REGS": 5, "WALK_COMPACT": 3}
# nee.hip kNeeKernels (profiles/nee_resource_usage.txt, nee_mis_resource_usage.txt, nee_pick_resource_usage.txt): the siblings' bounds
SIBLING_BOUNDS = {False: {(1, 2, 256): 5, (1, 1, 256): 6, (1, 1, 768): 6, (1, 5, 512): 5, (0, 3, 256): 5, (0, 5, 256): 5},
                  True: {(1, 2, 256): 5, (1, 1, 256): 5, (1, 1, 768): 5, (1, 5, 512): 5, (0, 3, 256): 5, (0, 5, 256): 5}}


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
        assert re.search(r"\b" + name + r"\b", later), name + " is not listed under 'Later under 4'"
    assert "trt_nee_samples_params," in later
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    L = trt._lib
    P = L.NeeSamplesParams
    assert C.sizeof(P) == 192 and C.sizeof(L.NeeMisParams) == 160 and C.sizeof(L.NeeParams) == 128
    assert (P.query.offset, P.weighted.offset, P.total_power.offset, P.reserved.offset) == (0, 160, 164, 168)
    # the signatures are trt_nee_pick's with the params struct exchanged and the directions where the second moments stand; the plan
    # takes the range's length, weighted and pick behind n
    S = L.SIGNATURES
    for name, sibling in (("trt_nee_samples", "trt_nee_pick"), ("trt_nee_samples_device", "trt_nee_pick_device")):
        mine, theirs = S[name][1], S[sibling][1]
        assert mine[6] is C.POINTER(P) and mine[:6] + mine[7:] == theirs[:6] + theirs[7:], name
    plan, base = S["trt_nee_samples_launch_plan"][1], S["trt_nee_launch_plan"][1]
    assert plan == base[:2] + [C.c_uint32] * 3 + base[2:]
    for name in ("nee_samples", "nee_samples_device", "nee_samples_plan"):
        assert callable(getattr(trt.Scene, name))


def test_the_default_parameters(trt):
    p = trt._lib.NeeSamplesParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    trt.lib.trt_nee_samples_params_default(C.byref(p))
    want = trt._lib.NeeMisParams()
    trt.lib.trt_nee_mis_params_default(C.byref(want))
    assert bytes(p.query) == bytes(want)
    assert p.weighted == 0 and p.total_power == 0.0 and list(p.reserved) == [0] * 6
    assert p.query.nee.gather.path.accumulate == 0 and p.query.heuristic == trt._lib.MIS_BALANCE
    trt.lib.trt_nee_samples_params_default(None)                           # tolerated


def _params(trt, weighted=0, heuristic=0, total=0.0, **over):
    """test_nee_abi._params (K = 4, seed 5) inside a trt_nee_samples_params."""
    p = trt._lib.NeeSamplesParams()
    trt.lib.trt_nee_samples_params_default(C.byref(p))
    p.query = AM._params(trt, heuristic, **over)
    p.weighted, p.total_power = weighted, total
    return p


def _entry_call(trt, pick, device, c):
    """One call of trt_nee_samples[_device] with the arguments of `c` (test_direct_pick_abi's dict; `rad` are the colours, `m2` the
    directions; the total stands in the parameters)."""
    ptr = lambda a: None if a is None else a.ctypes.data
    if c["p"] is not None:
        c["p"].total_power = c["total"]
    args = [c["s"], ptr(c["items"]), c["n"], ptr(c["table"]), ptr(c["pick"]) if pick else None, c["E"], C.byref(c["p"]) if c["p"] is not None else None,
            ptr(c["rad"]), ptr(c["m2"])]
    if device:
        return trt.lib.trt_nee_samples_device(*args, None, None)
    return trt.lib.trt_nee_samples(*args, None)


def _fixture(trt, sc, weighted):
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    table = DP._table(trt, sc)
    pick, total = trt.lights.pick_table(table)
    assert len(table) == 2 and pick["q"][1] > 0.0
    return lambda: dict(s=sc._h, items=items, n=N, table=table, pick=pick, E=len(table), p=_params(trt, weighted=int(weighted)), total=float(total),
                        rad=np.full((N, K, 3), 7.0, np.float32), m2=np.full((N, K, 3), 7.0, np.float32))


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("pick", (False, True))
@pytest.mark.parametrize("mis", (False, True))
def test_every_error_is_reported_in_the_documented_order(trt, mis, pick, device):
    """The whole documented list of trt_nee_samples for (weighted, pick), walked pair by pair: one call breaks two adjacent rules, the
    earlier one's message comes back.  (Host pointers are handed to the device form too: every call returns before anything is
    dereferenced.)  The tail of the list is the sibling's step list, which test_nee_pick_abi walks behind the sibling's entry point."""
    sc = A._scene(trt)
    fresh = _fixture(trt, sc, mis)
    nee = lambda c: c["p"].query.nee

    def path(field, value):
        return lambda c: setattr(nee(c).gather.path, field, value)

    def word(of, k):
        return lambda c: of(c).reserved.__setitem__(k, 1)

    def cone_spread(c):
        nee(c).gather.lobe, nee(c).gather.spread = trt._lib.PASSES_CONE, -1.0

    def too_many_samples(c):                                                # n * K = 2^32 streams fit, n * R = 2^32 samples do not
        c["n"] = 2 ** 31
        nee(c).gather.path.samples_per_ray, nee(c).gather.path.sample_begin, nee(c).gather.path.sample_end = 2, 0, 0

    faults = [("null argument", DP._set("p", None)), ("null argument", DP._set("s", None)), ("null buffer", DP._set("items", None)),
              ("null buffer", DP._set("rad", None)), ("samples_per_ray must", path("samples_per_ray", 0)), ("sample range", path("sample_begin", 5)),
              ("reserved words must be zero", word(lambda c: nee(c).gather.path, 3)), ("2^32", path("first_stream", 2 ** 32 - N * K + 1)),
              ("source must", lambda c: setattr(nee(c).gather, "lobe", 3)), ("spread", cone_spread),
              ("reserved words must be zero", word(lambda c: nee(c).gather, 3)), ("null emitter table", DP._set("table", None)),
              ("n_emitters must", DP._set("E", 0)), ("shadow_end must", lambda c: setattr(nee(c), "shadow_end", float("nan"))),
              ("source_is_diffuse must", lambda c: setattr(nee(c), "source_is_diffuse", 2)), ("reserved words must be zero", word(nee, 3)),
              ("accumulate must be 0", path("accumulate", 1)), ("weighted must", lambda c: setattr(c["p"], "weighted", 2))]
    if mis:
        faults += [("heuristic must", lambda c: setattr(c["p"].query, "heuristic", 2)),
                   ("reserved words must be zero", word(lambda c: c["p"].query, 6))]
    faults += [("reserved words must be zero", word(lambda c: c["p"], 5)), ("2^32 - 1 samples", too_many_samples)]
    # the sibling's list, less its pointer check: a NULL `pick` is no error here, it selects the sibling without a table
    faults += [f for f in DP._ladder_faults(mis, pick, device, False, 2) if f[0] != "null argument"]
    # the spread is only read of a cone; a sample range past K = 4 cannot also be the whole range of K = 2; weighted = 2 is not the
    # weighted query, so the heuristic behind it is one pair this walk cannot form (it is formed below)
    DP._walk_adjacent_pairs(trt, faults, fresh, lambda c: _entry_call(trt, pick, device, c),
                            impossible={("source must", "spread"), ("weighted must", "heuristic must")})
    c = fresh()
    c["p"].weighted, c["p"].query.heuristic = 2, 2
    _invalid(trt, _entry_call(trt, pick, device, c), "weighted must")
    # accumulate is refused with trt_samples' message
    c = fresh()
    nee(c).gather.path.accumulate = 1
    _invalid(trt, _entry_call(trt, pick, device, c), "accumulate must be 0: a sample's record is written, never added to")
    for c in (fresh(), fresh()):
        assert (c["rad"] == 7.0).all() and (c["m2"] == 7.0).all()
    # well-formed calls: TRT_ERR_NO_DEVICE follows the argument checks (with a device the host form succeeds)
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    if not device or want_ok != trt._lib.TRT_OK:                            # (the device form is given host pointers: never let it launch)
        variants = [lambda c: None, path("max_bounces", 0), lambda c: setattr(nee(c), "source_is_diffuse", 1), lambda c: setattr(nee(c).gather, "lobe", 0),
                    DP._set("m2", None), path("sample_begin", 2)]
        if not mis:                                                         # what only the weighted sample reads is not checked without it
            variants += [lambda c: setattr(c["p"].query, "heuristic", 2), word(lambda c: c["p"].query, 6), DP._set("total", float("nan"))]
        if not (mis and pick):
            variants += [DP._set("total", -1.0)]
        for change in variants:
            c = fresh()
            change(c)
            assert _entry_call(trt, pick, device, c) == want_ok
            if want_ok != trt._lib.TRT_OK:
                assert "no HIP device" in trt.lib.trt_last_error().decode() and (c["rad"] == 7.0).all()
                assert c["m2"] is None or (c["m2"] == 7.0).all()


@pytest.mark.parametrize("device", (False, True))
def test_an_empty_batch_is_checked_succeeds_without_a_device_and_touches_nothing(trt, device):
    sc = A._scene(trt)
    cols = np.full((N, K, 3), 7.0, np.float32)
    call = trt.lib.trt_nee_samples_device if device else trt.lib.trt_nee_samples
    extra = (None, None) if device else (None,)
    for weighted in (0, 1):
        p = _params(trt, weighted=weighted, first_stream=2 ** 32 - 1)       # n * K == 0: any first stream passes
        for pick in (None, cols.ctypes.data):                               # the tables are not needed: null, or anything
            assert call(sc._h, None, 0, None, pick, 0, C.byref(p), None, None, *extra) == trt._lib.TRT_OK
            assert call(sc._h, None, 0, None, pick, 7, C.byref(p), cols.ctypes.data, cols.ctypes.data, *extra) == trt._lib.TRT_OK
        _invalid(trt, call(None, None, 0, None, None, 0, C.byref(p), None, None, *extra))
        _invalid(trt, call(sc._h, None, 0, None, None, 0, None, None, None, *extra))
        _invalid(trt, call(sc._h, None, 0, None, None, 0, C.byref(_params(trt, weighted=weighted, accumulate=1)), None, None, *extra), "accumulate")
        _invalid(trt, call(sc._h, None, 0, None, None, 0, C.byref(_params(trt, weighted=weighted, source_is_diffuse=2)), None, None, *extra))
        _invalid(trt, call(sc._h, None, 0, None, None, 0, C.byref(_params(trt, weighted=2)), None, None, *extra), "weighted")
    _invalid(trt, call(sc._h, None, 0, None, None, 0, C.byref(_params(trt, weighted=1, heuristic=2)), None, None, *extra), "heuristic")
    assert (cols == 7.0).all()
    table = sc.emitters()
    pick = trt.lights.pick_table(table)
    none = np.zeros((0, 6), np.float32)
    for mis, pk in ((None, None), ("balance", None), (None, pick[0]), (None, pick), ("power", pick)):
        got, dirs, st = sc.nee_samples(none, table, 4, mis=mis, pick=pk, directions=True)
        assert got.shape == (0, 4, 3) and dirs.shape == (0, 4, 3) and st["samples"] == 0 and st["rays"] == 0
    sc.nee_samples_device(0, 0, 0, 0, 0, samples_per_item=4)
    sc.nee_samples_device(0, 0, 0, 0, 0, samples_per_item=4, mis="power", pick=(0, 1.0))


def test_the_python_wrappers(trt, monkeypatch):
    """What nee_samples / nee_samples_device / nee_samples_plan hand the library, with the recorder of test_emitter_query_dispatch in the
    library's place: the symbol, where the pick pointer stands, weighted, the heuristic and total_power in the parameters."""
    rec = ED.Recorder(trt.lib)
    monkeypatch.setattr(trt.api, "lib", rec)
    sc = object.__new__(trt.api.Scene)
    sc._h = C.c_void_p(0x1234)
    try:
        table, records, total = ED._tables(trt)
        items = np.zeros((N, 6), np.float32)
        for mis in ED.MIS:
            for pick in (None, records, (records, total)):
                if mis is not None and pick is records:
                    with pytest.raises(ValueError, match="records, total"):
                        sc.nee_samples(items, table, K, mis=mis, pick=pick)
                    continue
                rec.calls.clear()
                cols, dirs, st = sc.nee_samples(items, table, K, mis=mis, pick=pick, source="cone", spread=0.5, sample_begin=1, sample_end=3, directions=True)
                (name, args), = rec.calls
                assert name == "trt_nee_samples" and len(args) == 10 and cols.shape == dirs.shape == (N, K, 3)
                assert args[0] is sc._h and args[1] == items.ctypes.data and args[2] == N and args[3] == table.ctypes.data and args[5] == len(table)
                assert (args[4] is None) == (pick is None)
                p = args[6]._obj
                assert type(p) is trt._lib.NeeSamplesParams and p.weighted == (mis is not None)
                assert p.query.heuristic == (trt._lib.MIS_POWER if mis == "power" else trt._lib.MIS_BALANCE)
                assert p.total_power == (total if isinstance(pick, tuple) else 0.0)
                g = p.query.nee.gather
                assert (g.path.samples_per_ray, g.path.sample_begin, g.path.sample_end, g.path.accumulate, g.lobe, g.spread) == (K, 1, 3, 0, 2, 0.5)
                assert args[7] == cols.ctypes.data and args[8] == dirs.ctypes.data
                rec.calls.clear()
                cols, dirs, st = sc.nee_samples(items, table, K, mis=mis, pick=pick)
                assert dirs is None and rec.calls[0][1][8] is None
        rec.calls.clear()
        sc.nee_samples_device(0x1000, N, 0x2000, 2, 0x3000, 0x4000, d_counters_ptr=0x6000, samples_per_item=K, mis="power", pick=(0x5000, 2.5))
        (name, args), = rec.calls
        assert name == "trt_nee_samples_device" and [ED._value(a) for a in args[1:6]] == [0x1000, N, 0x2000, 0x5000, 2]
        assert args[6]._obj.weighted == 1 and args[6]._obj.total_power == 2.5 and args[6]._obj.query.heuristic == trt._lib.MIS_POWER
        assert [ED._value(a) for a in args[7:]] == [0x3000, 0x4000, 0x6000, None]
        rec.calls.clear()
        sc.nee_samples_device(0x1000, N, 0x2000, 2, 0x3000, samples_per_item=K)
        args = rec.calls[0][1]
        assert ED._value(args[4]) is None and args[6]._obj.weighted == 0 and [ED._value(a) for a in args[7:]] == [0x3000, None, None, None]
        with pytest.raises(ValueError, match="records, total"):
            sc.nee_samples_device(0, 0, 0, 0, 0, samples_per_item=K, mis="balance", pick=0x5000)
        with pytest.raises(ValueError, match="mis must be"):
            sc.nee_samples(items, table, K, mis="optimal")
        with pytest.raises(ValueError, match="source must be"):
            sc.nee_samples(items, table, K, source="sphere")
        with pytest.raises(ValueError, match="PICK_DTYPE"):
            sc.nee_samples(items, table, K, pick=records[:1])
        with pytest.raises(TypeError):
            sc.nee_samples(items, table, K, accumulate=True)                # a record is written, never added to: the keyword is not offered
        with pytest.raises(AssertionError):
            sc.nee_samples(items, table, K, colors=np.zeros((N, K, 3), np.float64))
        for mis, pick, want in ((None, False, (0, 0)), ("balance", None, (1, 0)), (None, True, (0, 1)), ("power", (records, total), (1, 1))):
            rec.calls.clear()
            sc.nee_samples_plan(7, 5, mis=mis, pick=pick, compute_units=256)
            (name, args), = rec.calls
            assert name == "trt_nee_samples_launch_plan" and args[1:6] == (7, 5) + want + (256,)
    finally:
        sc._h = None


def test_the_plan_symbol_checks_its_arguments(trt):
    sc = A._scene(trt)
    out = trt._lib.QueryPlan()
    plan = trt.lib.trt_nee_samples_launch_plan
    for weighted in (0, 1):
        for pick in (0, 1):
            assert plan(None, 1, 1, weighted, pick, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
            assert plan(sc._h, 1, 1, weighted, pick, 256, None) == trt._lib.ERR_INVALID_ARG
            assert plan(sc._h, 2 ** 16, 2 ** 16, weighted, pick, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG      # n * R = 2^32
            assert "2^32 - 1" in trt.lib.trt_last_error().decode()
            assert plan(sc._h, 2 ** 16 + 1, 2 ** 16 - 1, weighted, pick, 256, C.byref(out)) == trt._lib.TRT_OK       # 2^32 - 1
            want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
            assert plan(sc._h, 1, 1, weighted, pick, 0, C.byref(out)) == want
            assert plan(sc._h, 1, 1, weighted, pick, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    assert sc.nee_samples_plan(1, 2, compute_units=304)["compute_units"] == 304
    assert sc.nee_samples_plan(7, None, compute_units=304) == sc.nee_samples_plan(7, 1, compute_units=304)
    assert sc.nee_samples_plan(0, 5, compute_units=256)["workgroups"] == 0 and sc.nee_samples_plan(5, 0, compute_units=256)["workgroups"] == 0


def bounds_of_the_profile():
    """{(weighted?, pick?, (scene mode, walk, threads)): launch bound} as profiles/nee_samples_resource_usage.txt reports the 24 kernels:
    the bound is the template's and the occupancy column, and no row has a VGPR spill or scratch."""
    rows = re.findall(r"^nee_samples_kernel<(\w+), (\w+), (\d+), (\d+), (plain|MIS), (uniform|PICK)>\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$",
                      open(os.path.join(ROOT, "profiles", "nee_samples_resource_usage.txt")).read(), flags=re.M)
    assert len(rows) == 24
    out = {}
    for mode, walk, threads, bound, mis, pick, vgpr, agpr, sgpr, s_spill, v_spill, scratch, occupancy, lds in rows:
        assert int(v_spill) == 0 and int(scratch) == 0 and int(occupancy) == int(bound), (mode, walk, threads, mis, pick)
        key = (mis == "MIS", pick == "PICK", (MODES[mode], WALKS[walk], int(threads)))
        assert key not in out
        out[key] = int(bound)
    assert len(out) == 24
    return out


def test_the_profile_lists_the_24_kernels_without_scratch_at_or_above_their_siblings():
    bounds = bounds_of_the_profile()
    for (mis, pick, shape), bound in bounds.items():
        assert bound >= SIBLING_BOUNDS[mis][shape], (mis, pick, shape)
        assert bound == bounds[(mis, False, shape)]                         # the PICK kernels keep the bound of the uniform ones


# (items, range length): n * R walks test_samples_abi.py's sizes, each as items of one sample and split n x R
WORK = ((1, 1), (64, 1), (1, 64), (257, 1), (36, 9), (100003, 1), (1, 100003), (324, 8), (1, 513), (64, 16384), (2 ** 32 - 1, 1), (1, 2 ** 32 - 1),
        (65537, 65535), (2 ** 20, 16))
FROM_THE_BOUND = ("kernel_waves_per_simd", "workgroups_per_cu", "wave_slots")
FROM_THE_SLOTS = ("rays_per_wave", "waves", "workgroups")


@pytest.mark.parametrize("pick", (False, True))
@pytest.mark.parametrize("mis", (None, "balance"))
def test_the_plan_is_the_siblings_plan_of_n_times_r_but_for_the_kernel_bound(trt, mis, pick):
    """Every (scene, options) of test_gpu_queries.PLAN_CASES at 256 compute units: the plan's invariants with n * R in the place of n, the
    listed kernel shape, every field equal to the sibling's trt_nee*_launch_plan(n * R) but the bound and what the launch rule derives
    from it; the bound is the profile's; and the runs lengthen exactly where n * R passes 256 x wave_slots."""
    import test_gpu_queries as G
    import walk_ray_cases as W
    cus = 256
    profile = bounds_of_the_profile()
    r = trt.Renderer(4, 1, 8, False, (0.1, 0.1, 0.1))
    shapes, worlds = set(), {}
    for name, options, shape in G.PLAN_CASES:
        if name not in worlds:
            worlds[name] = trt.world_from_description(W.scene(trt, name))
        world, cam = worlds[name]
        host_options = {k: v for k, v in options.items() if k != "on_device"}
        sc = world.get_bvh(**host_options) if host_options else world.get_bvh()
        streamed = r.launch_plan(cam, sc)
        for n, rl in WORK:
            work = n * rl
            q, qs = sc.nee_samples_plan(n, rl, mis=mis, pick=pick, compute_units=cus), sc.nee_plan(work, cus, mis=mis, pick=True if pick else None)
            tag = (name, options, n, rl, q, qs)
            _check_query_plan(q, work, cus, streamed, tag)
            assert q == sc.nee_samples_plan(rl, n, mis=mis, pick=pick, compute_units=cus), tag      # a function of n * R alone
            assert G.plan_shape(q) == shape, tag
            assert set(q) == set(qs)
            assert q["kernel_waves_per_simd"] == profile[(mis is not None, pick, shape[:3])], tag
            assert qs["kernel_waves_per_simd"] == SIBLING_BOUNDS[mis is not None][shape[:3]], tag
            same_bound = q["kernel_waves_per_simd"] == qs["kernel_waves_per_simd"]
            lengthened = q["rays_per_wave"] > 256 or qs["rays_per_wave"] > 256
            for k in q:
                if same_bound or not (k in FROM_THE_BOUND or (lengthened and k in FROM_THE_SLOTS)):
                    assert q[k] == qs[k], (k, tag)
            per_wave, waves = q["rays_per_wave"], q["waves"]
            assert waves * per_wave >= work and (waves - 1) * per_wave < work, tag
            assert q["workgroups"] == -(-waves // (q["threads_per_workgroup"] // 64)), tag
            assert (per_wave > 256) == (work > 256 * q["wave_slots"]), tag
            shapes.add(shape[:3])
        # the threshold itself, as items and as samples of one item
        edge = 256 * sc.nee_samples_plan(1, 1, mis=mis, pick=pick, compute_units=cus)["wave_slots"]
        for n, rl in ((edge, 1), (1, edge), (edge // 256, 256)):
            assert sc.nee_samples_plan(n, rl, mis=mis, pick=pick, compute_units=cus)["rays_per_wave"] == 256, (name, options, n, rl)
        for n, rl in ((edge + 1, 1), (1, edge + 1), (edge // 256 + 1, 256)):
            q = sc.nee_samples_plan(n, rl, mis=mis, pick=pick, compute_units=cus)
            assert q["rays_per_wave"] > 256 and q["rays_per_wave"] % 64 == 0 and q["waves"] <= q["wave_slots"], (name, options, n, rl, q)
    assert len(shapes) == 6, sorted(shapes)                                 # every entry of the table
