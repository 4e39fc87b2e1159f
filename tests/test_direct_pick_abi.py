"""The entry points of the direct-light queries that choose their emitter through an alias table (tinyrt.h trt_emitter_pick,
trt_emitter_pick_build, trt_direct_pick, trt_direct_pick_device, trt_direct_pick_launch_plan, trt_direct_mis_pick,
trt_direct_mis_pick_device, trt_direct_mis_pick_launch_plan) at the C boundary, without a GPU: the eight names are declared, exported,
bound and listed, the record has the header's layout (ctypes, numpy, gcc), every documented error comes back as TRT_ERR_INVALID_ARG in
its documented order before any device work, an empty batch succeeds without a device, TRT_ERR_NO_DEVICE follows the argument checks,
and the weighted host form rejects a caller-weighted table and a wrong total_power.  What the buffers hold is checked on the GPU
(tests/test_gpu_direct_pick.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_direct_abi as A
import test_direct_mis_abi as AM

ROOT = A.ROOT
FUNCTIONS = {"trt_emitter_pick_build": 5, "trt_direct_pick": 10, "trt_direct_pick_device": 11, "trt_direct_pick_launch_plan": 4,
             "trt_direct_mis_pick": 11, "trt_direct_mis_pick_device": 12, "trt_direct_mis_pick_launch_plan": 4}
N = A.N
_invalid = A._invalid


def test_the_eight_names_are_declared_exported_bound_and_listed(trt):
    text = open(os.path.join(ROOT, "include", "tinyrt.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(trt._lib.LIB_PATH)
    later = re.search(r"Later under 4[^/]*\*/", text, flags=re.S).group(0)
    for name, nargs in FUNCTIONS.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name + " is not declared in tinyrt.h"
        assert hasattr(raw, name), name + " is not exported"
        res, args = trt._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
        assert re.search(r"\b" + name + r"\b", later), name + " is not listed under 'Later under 4'"
    assert "trt_emitter_pick," in later
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    # the signatures are the direct-light queries' with the pick table behind the emitter table (and total_power behind the parameters)
    S = trt._lib.SIGNATURES
    for stem in ("trt_direct", "trt_direct_device"):
        base, pick = S[stem][1], S[stem.replace("trt_direct", "trt_direct_pick")][1]
        assert pick == base[:4] + [C.c_void_p] + base[4:], stem
        stem_mis = stem.replace("trt_direct", "trt_direct_mis")
        base, pick = S[stem_mis][1], S[stem_mis.replace("trt_direct_mis", "trt_direct_mis_pick")][1]
        assert pick == base[:4] + [C.c_void_p] + base[4:6] + [C.c_float] + base[6:], stem_mis
    assert S["trt_direct_pick_launch_plan"][1] == S["trt_direct_mis_pick_launch_plan"][1] == S["trt_direct_launch_plan"][1]
    m = re.search(r"typedef struct \{([^}]*)\}\s*trt_emitter_pick\s*;", header)
    assert m and re.findall(r"(\w+)\s+(\w+)\s*;", m.group(1)) == [("float", "q"), ("uint32_t", "alias"), ("float", "prob"), ("uint32_t", "reserved")]
    R = trt._lib.EmitterPick
    assert C.sizeof(R) == 16 and (R.q.offset, R.alias.offset, R.prob.offset, R.reserved.offset) == (0, 4, 8, 12)
    dt = trt.lights.PICK_DTYPE
    assert dt.itemsize == 16 and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12]


def test_the_layout_matches_the_c_compiler(trt, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tinyrt.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(trt_emitter_pick), offsetof(trt_emitter_pick, q), offsetof(trt_emitter_pick, alias), '
                   'offsetof(trt_emitter_pick, prob), offsetof(trt_emitter_pick, reserved)); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [16, 0, 4, 8, 12]


def _table(trt, sc):
    return trt.lights.table(sc.emitters(), trt.lights.sphere((50.0, 50.0, 50.0), 2.0, (1.0, 1.0, 1.0)))


def test_the_builder_checks_its_arguments_in_order_and_needs_no_device(trt):
    sc = A._scene(trt)
    table = _table(trt, sc)
    E = len(table)
    out = np.full(E, 7, trt.lights.PICK_DTYPE)
    total = C.c_float(-1.0)
    build = trt.lib.trt_emitter_pick_build
    tp, op = table.ctypes.data, out.ctypes.data
    nan_w = np.array([1.0, np.nan], np.float32)
    _invalid(trt, build(None, 0, nan_w.ctypes.data, op, C.byref(total)), "null")            # the pointers come first
    _invalid(trt, build(tp, 0, nan_w.ctypes.data, None, C.byref(total)), "null")
    for e in (0, 2 ** 20 + 1):
        _invalid(trt, build(tp, e, nan_w.ctypes.data, op, C.byref(total)), "n_emitters")  # then the size, before a weight is read
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-45):
        w = np.array([0.0, bad], np.float32)                                                # a total of 0 besides: the weight comes first
        _invalid(trt, build(tp, E, w.ctypes.data, op, C.byref(total)), "negative or not finite")
    w = np.zeros(E, np.float32)
    _invalid(trt, build(tp, E, w.ctypes.data, op, C.byref(total)), "total")
    w = np.full(E, 3e38, np.float32)
    _invalid(trt, build(tp, E, w.ctypes.data, op, C.byref(total)), "total")               # the f32 total overflows
    black = table.copy()
    black["color"] = 0.0
    _invalid(trt, build(black.ctypes.data, E, None, op, C.byref(total)), "total")
    nan = table.copy()
    nan["area"][1] = np.nan
    _invalid(trt, build(nan.ctypes.data, E, None, op, C.byref(total)), "negative or not finite")
    assert out.tobytes() == np.full(E, 7, trt.lights.PICK_DTYPE).tobytes() and total.value == -1.0      # nothing was written
    assert build(tp, E, None, op, None) == trt._lib.TRT_OK                                 # total is optional
    again = np.zeros(E, trt.lights.PICK_DTYPE)
    assert build(tp, E, None, again.ctypes.data, C.byref(total)) == trt._lib.TRT_OK and total.value > 0
    assert again.tobytes() == out.tobytes() and (out["reserved"] == 0).all() and (out["alias"] < E).all()
    with pytest.raises(ValueError):
        trt.lights.pick_table(table, np.ones(E + 1, np.float32))
    with pytest.raises(ValueError):
        trt.lights.pick_table(np.zeros(3, np.float32))


def _call(trt, mis, device, s, items, n, table, pick, n_emitters, p, total, rad, m2):
    lib = trt.lib
    if mis:
        if device:
            return lib.trt_direct_mis_pick_device(s, items, n, table, pick, n_emitters, p, total, rad, m2, None, None)
        return lib.trt_direct_mis_pick(s, items, n, table, pick, n_emitters, p, total, rad, m2, None)
    if device:
        return lib.trt_direct_pick_device(s, items, n, table, pick, n_emitters, p, rad, m2, None, None)
    return lib.trt_direct_pick(s, items, n, table, pick, n_emitters, p, rad, m2, None)


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("mis", (False, True))
def test_misuse_is_invalid_arg_before_any_device_work_in_the_documented_order(trt, mis, device):
    """(Host pointers are handed to the device form too: every one of these calls must return before anything is dereferenced.)  The
    order is shown by calls that break two rules at once: the earlier rule's message comes back."""
    sc = A._scene(trt)
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    rad = np.full((N, 3), 7.0, np.float32)
    m2 = np.full((N, 3), 7.0, np.float32)
    table = _table(trt, sc)
    E = len(table)
    pick, total = trt.lights.pick_table(table)
    ip, rp, mp, tp, kp = items.ctypes.data, rad.ctypes.data, m2.ctypes.data, table.ctypes.data, pick.ctypes.data
    params = (lambda **kw: AM._params(trt, **kw)) if mis else (lambda **kw: A._params(trt, **kw))
    p = params()

    def call(s, r, n, q, a, b, t=tp, k=kp, e=E, tot=total):
        return _call(trt, mis, device, s, r, n, t, k, e, C.byref(q) if q is not None else None, C.c_float(tot), a, b)

    # trt_direct's own, one of each family, each with a NULL pick besides: trt_direct's rule is reported
    _invalid(trt, call(None, ip, N, p, rp, mp, k=None))
    _invalid(trt, call(sc._h, ip, N, None, rp, mp, k=None))
    _invalid(trt, call(sc._h, None, N, p, rp, mp, k=None))
    _invalid(trt, call(sc._h, ip, N, p, None, mp, k=None))
    _invalid(trt, call(sc._h, ip, N, params(samples_per_ray=0), rp, mp, k=None))
    _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=None, k=None), "emitter")
    for e in (0, 2 ** 20 + 1):
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, e=e, k=None), "n_emitters")
    _invalid(trt, call(sc._h, ip, N, params(shadow_end=float("nan")), rp, mp, k=None), "shadow_end")
    q = params()
    (q.direct if mis else q).reserved[3] = 1
    _invalid(trt, call(sc._h, ip, N, q, rp, mp, k=None), "reserved")
    if mis:
        _invalid(trt, call(sc._h, ip, N, params(heuristic=2), rp, mp, k=None), "heuristic")
    # then the pick pointer, in both forms
    _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=None), "null")
    if not device:                                                          # the device form cannot read either table
        bad_kind = table.copy()
        bad_kind["kind"][1] = 2
        bad_q = pick.copy()
        bad_q["q"][0] = 2.0
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=bad_kind.ctypes.data, k=bad_q.ctypes.data), "kind")          # the emitter records first
        if mis:                                                             # then the table rule of the emitters
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=table[1:].copy().ctypes.data, k=bad_q.ctypes.data, e=1), "lights")
        # then each pick record in table order: q, alias, prob, reserved
        for word, field, values in (("q must", "q", (np.nan, -1e-9, 1.0000001, np.inf)), ("alias", "alias", (E, 0xFFFFFFFF)),
                                    ("prob must", "prob", (np.nan, -1e-9, 1.0000001)), ("reserved", "reserved", (1,))):
            for v in values:
                for at in range(E):
                    bad = pick.copy()
                    bad[field][at] = v
                    _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=bad.ctypes.data), word)
        both = pick.copy()
        both["q"][1], both["alias"][0] = 2.0, E                             # record 0's alias is reported before record 1's q
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=both.ctypes.data), "alias")
        both = pick.copy()
        both["reserved"][0], both["prob"][0] = 1, 2.0                       # within a record: prob before reserved
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=both.ctypes.data), "prob must")
        # then an emitter that can be chosen with prob 0: as a slot's own (q > 0) and as an alias (of a slot with q < 1)
        assert pick["q"][1] < 1.0 and pick["alias"][1] == 0 and pick["q"][0] == 1.0
        zero = pick.copy()
        zero["prob"][1] = 0.0
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=zero.ctypes.data), "prob 0")
        zero = pick.copy()
        zero["prob"][0] = 0.0
        zero["q"][0] = 0.0                                                  # slot 0 never keeps emitter 0, but slot 1 sends to it
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=zero.ctypes.data), "prob 0")
        zero["reserved"][1] = 1
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=zero.ctypes.data), "reserved")        # the records' own rules come first
        if mis:
            # the weighted form: total_power, then prob bit for bit - a caller-weighted table and a wrong total are rejected
            for tot in (0.0, -1.0, np.nan, np.inf):
                _invalid(trt, call(sc._h, ip, N, p, rp, mp, tot=tot), "total_power")
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, tot=total * np.float32(1.001)), "power / total_power")
            weighted, wtotal = trt.lights.pick_table(table, np.array([1.0, 1.0], np.float32))
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=weighted.ctypes.data, tot=wtotal), "power / total_power")
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=weighted.ctypes.data, tot=total), "power / total_power")
            off = pick.copy()
            off["prob"][1] = np.nextafter(off["prob"][1], np.float32(1.0))
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=off.ctypes.data), "power / total_power")
    # well-formed calls: TRT_ERR_NO_DEVICE follows the argument checks (with a device the host form succeeds)
    want_ok = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE
    if not device or want_ok != trt._lib.TRT_OK:                            # (the device form is given host pointers: never let it launch)
        assert call(sc._h, ip, N, p, rp, mp) == want_ok
        assert call(sc._h, ip, N, p, rp, None) == want_ok
        if want_ok != trt._lib.TRT_OK:
            assert "no HIP device" in trt.lib.trt_last_error().decode() and (rad == 7.0).all()
        if not mis:                                                         # any weights will do for the plain query
            weighted, _ = trt.lights.pick_table(table, np.array([1.0, 0.0], np.float32))
            assert weighted["q"][1] == 0.0 and weighted["prob"][1] == 0.0
            assert call(sc._h, ip, N, p, rp, mp, k=weighted.ctypes.data) == want_ok
        rad[:] = 7.0
        m2[:] = 7.0
    # an empty batch is checked too, but for the tables, which it does not need; it succeeds without a device and touches nothing
    _invalid(trt, call(None, None, 0, p, None, None))
    _invalid(trt, call(sc._h, None, 0, None, None, None))
    _invalid(trt, call(sc._h, None, 0, params(shadow_end=float("nan")), None, None))
    assert call(sc._h, None, 0, p, None, None, t=None, k=None, e=0, tot=0.0) == trt._lib.TRT_OK
    assert call(sc._h, None, 0, p, rp, mp, t=None, k=None, e=7, tot=np.nan) == trt._lib.TRT_OK
    assert (rad == 7.0).all() and (m2 == 7.0).all()


def test_the_python_keyword(trt):
    sc = A._scene(trt)
    table = sc.emitters()
    pick, total = trt.lights.pick_table(table)
    none = np.zeros((0, 6), np.float32)
    for mis in (None, "balance", "power"):
        got, m2, st = sc.direct(none, table, 4, moment2=True, mis=mis, pick=(pick, total))
        assert got.shape == (0, 3) and m2.shape == (0, 3) and st["samples"] == 0 and st["rays"] == 0
    sc.direct(none, table, 4, pick=pick)                                    # the records alone will do without mis
    with pytest.raises(ValueError):
        sc.direct(none, table, 4, mis="balance", pick=pick)                 # ... but the weighted query needs the total
    with pytest.raises(ValueError):
        sc.direct(none, table, 4, pick=pick[:0])
    with pytest.raises(ValueError):
        sc.direct(none, table, 4, pick=np.zeros(1, np.float32))
    with pytest.raises(ValueError):
        sc.direct_device(0, 0, 0, 0, 0, samples_per_item=4, mis="power", pick=1234)
    sc.direct_device(0, 0, 0, 0, 0, samples_per_item=4, pick=0)             # n == 0: nothing is touched
    sc.direct_device(0, 0, 0, 0, 0, samples_per_item=4, mis="power", pick=(0, 1.0))


def test_the_plan_symbols(trt):
    """The PICK plans check their arguments, and every field is the plan's of the query without the table: the same shapes and bounds."""
    import test_gpu_queries as G
    import walk_ray_cases as W
    sc = A._scene(trt)
    out = trt._lib.QueryPlan()
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    for fn in (trt.lib.trt_direct_pick_launch_plan, trt.lib.trt_direct_mis_pick_launch_plan):
        assert fn(None, 1, 256, C.byref(out)) == trt._lib.ERR_INVALID_ARG
        assert fn(sc._h, 1, 256, None) == trt._lib.ERR_INVALID_ARG
        assert fn(sc._h, 1, 0, C.byref(out)) == want
        assert fn(sc._h, 1, 256, C.byref(out)) == trt._lib.TRT_OK and out.compute_units == 256
    shapes, worlds = set(), {}
    for name, options, shape in G.PLAN_CASES:
        if name not in worlds:
            worlds[name] = trt.world_from_description(W.scene(trt, name))[0]
        host_options = {k: v for k, v in options.items() if k != "on_device"}
        s = worlds[name].get_bvh(**host_options) if host_options else worlds[name].get_bvh()
        for n in (1, 257, 100000):
            for mis in (None, "balance", "power"):
                q = s.direct_plan(n, 256, mis=mis, pick=True)
                assert q == s.direct_plan(n, 256, mis=mis), (name, options, n, mis)
                assert G.plan_shape(q) == shape
        shapes.add(shape[:3])
    assert len(shapes) == 6


# ---- the order of the checks, pair by pair: one call breaks two adjacent rules of the documented list, the earlier one is reported ----
def _entry_call(trt, family, mis, pick, device, c):
    """One call of trt_<family>[_mis][_pick][_device] with the arguments of `c` (a dict; tables are numpy arrays or None)."""
    fn = getattr(trt.lib, "trt_" + family + ("_mis" if mis else "") + ("_pick" if pick else "") + ("_device" if device else ""))
    ptr = lambda a: None if a is None else a.ctypes.data
    args = [c["s"], ptr(c["items"]), c["n"], ptr(c["table"])] + ([ptr(c["pick"])] if pick else []) + [c["E"], C.byref(c["p"]) if c["p"] is not None else None]
    args += ([C.c_float(c["total"])] if mis and pick else []) + [ptr(c["rad"]), ptr(c["m2"])] + ([None, None] if device else [None])
    return fn(*args)


def _set(key, value):
    return lambda c: c.__setitem__(key, value)


def _record(which, field, at, value):
    """Breaks one word of one record of the emitter table or of the pick table (the caller's copy)."""
    def fault(c):
        c[which] = c[which].copy()
        c[which][field][at] = value
    return fault


def _ladder_faults(mis, pick, device, table_rule_first, E):
    """What follows the family's own parameter checks, in tinyrt.h's order: the pick pointer (both forms), then - host form only - the
    emitter records, the pick records and the weighted queries' table rule (trt_direct_mis_pick: before the pick records;
    trt_nee_mis_pick: behind them), total_power and prob."""
    out = [("null argument", _set("pick", None))] if pick else []
    if device:
        return out
    out += [("emitter kind", _record("table", "kind", 0, 2)), ("reserved words of an emitter", _record("table", "reserved", (0, 0), 1))]
    rule = [("lights", _record("table", "geometry", 0, 3))] if mis else []          # geometry 3 of the box is its floor: no light
    records = [("q must", _record("pick", "q", 0, 2.0)), ("alias must", _record("pick", "alias", 0, E)), ("prob must", _record("pick", "prob", 0, 2.0)),
               ("reserved words must be zero", _record("pick", "reserved", 0, 1)), ("prob 0", _record("pick", "prob", 1, 0.0))] if pick else []
    out += rule + records if table_rule_first else records + rule
    if mis and pick:
        def off_by_an_ulp(c):
            c["pick"] = c["pick"].copy()
            c["pick"]["prob"][1] = np.nextafter(c["pick"]["prob"][1], np.float32(1.0))
        out += [("total_power must", _set("total", float("nan"))), ("power / total_power", off_by_an_ulp)]
    return out


def _walk_adjacent_pairs(trt, faults, fresh, call, impossible=()):
    """Every fault alone is reported under its own words; every two neighbours together under the earlier one's."""
    for k, (word, fault) in enumerate(faults):
        c = fresh()
        fault(c)
        _invalid(trt, call(c), word)
        if k + 1 < len(faults) and (word, faults[k + 1][0]) not in impossible:
            faults[k + 1][1](c)
            _invalid(trt, call(c), word)


def _pair_fixture(trt, sc, params):
    items = np.zeros((N, 6), np.float32)
    items[:, 4] = 1.0
    table = _table(trt, sc)
    pick, total = trt.lights.pick_table(table)
    assert len(table) == 2 and pick["q"][1] > 0.0
    return lambda: dict(s=sc._h, items=items, n=N, table=table, pick=pick, E=len(table), p=params(), total=float(total), rad=np.full((N, 3), 7.0, np.float32),
                        m2=np.full((N, 3), 7.0, np.float32))


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("pick", (False, True))
@pytest.mark.parametrize("mis", (False, True))
def test_adjacent_checks_are_reported_in_the_documented_order(trt, mis, pick, device):
    """trt_direct, trt_direct_mis, trt_direct_pick, trt_direct_mis_pick and their device forms: the whole documented list of each, walked
    pair by pair.  Among them: a table that breaks the table rule and holds a bad pick record gives trt_direct_mis_pick the table-rule
    message (trt_nee_mis_pick reports the record: tests/test_nee_pick_abi.py)."""
    sc = A._scene(trt)
    fresh = _pair_fixture(trt, sc, (lambda: AM._params(trt)) if mis else (lambda: A._params(trt)))
    own = (lambda c: c["p"].direct) if mis else (lambda c: c["p"])

    def path(field, value):
        return lambda c: setattr(own(c).path, field, value)

    def word(of, k):
        return lambda c: of(c).reserved.__setitem__(k, 1)

    faults = [("null argument", _set("p", None)), ("null argument", _set("s", None)), ("null buffer", _set("items", None)), ("null buffer", _set("rad", None)),
              ("samples_per_ray must", path("samples_per_ray", 0)), ("sample range", path("sample_begin", 5)),
              ("reserved words must be zero", word(lambda c: own(c).path, 3)), ("2^32", path("first_stream", 2 ** 32 - N * 4 + 1)),
              ("null emitter table", _set("table", None)), ("n_emitters must", _set("E", 0)),
              ("shadow_end must", lambda c: setattr(own(c), "shadow_end", float("nan"))), ("reserved words must be zero", word(own, 6))]
    if mis:
        faults += [("heuristic must", lambda c: setattr(c["p"], "heuristic", 2)), ("reserved words must be zero", word(lambda c: c["p"], 6))]
    faults += _ladder_faults(mis, pick, device, True, 2)
    _walk_adjacent_pairs(trt, faults, fresh, lambda c: _entry_call(trt, "direct", mis, pick, device, c))
