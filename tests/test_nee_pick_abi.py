"""The entry points of the next-event queries that choose their emitter through an alias table (tinyrt.h trt_nee_pick, trt_nee_pick_device,
trt_nee_pick_launch_plan, trt_nee_mis_pick, trt_nee_mis_pick_device, trt_nee_mis_pick_launch_plan) at the C boundary, without a GPU: the six
names are declared, exported, bound and listed, their signatures are their siblings' plus the pick pointer (and total_power), every
documented error comes back as TRT_ERR_INVALID_ARG in its documented order before any device work, an empty batch succeeds without a
device, TRT_ERR_NO_DEVICE follows the argument checks, and the weighted host form rejects a caller-weighted table and a wrong total_power.
What the buffers hold is checked on the GPU (tests/test_gpu_nee_pick.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_nee_abi as A
import test_nee_mis_abi as AM

ROOT = A.ROOT
FUNCTIONS = {"trt_nee_pick": 10, "trt_nee_pick_device": 11, "trt_nee_pick_launch_plan": 4, "trt_nee_mis_pick": 11, "trt_nee_mis_pick_device": 12,
             "trt_nee_mis_pick_launch_plan": 4}
N = A.N
_invalid = A._invalid


def test_the_six_names_are_declared_exported_bound_and_listed(trt):
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
    assert trt.lib.trt_abi_version() == 4                                  # new symbols only: the ABI version stays
    # the signatures are the next-event queries' with the pick table behind the emitter table (and total_power behind the parameters),
    # which is where trt_direct_pick / trt_direct_mis_pick have them
    S = trt._lib.SIGNATURES
    for stem in ("trt_nee", "trt_nee_device"):
        base, pick = S[stem][1], S[stem.replace("trt_nee", "trt_nee_pick")][1]
        assert pick == base[:4] + [C.c_void_p] + base[4:], stem
        stem_mis = stem.replace("trt_nee", "trt_nee_mis")
        base, pick = S[stem_mis][1], S[stem_mis.replace("trt_nee_mis", "trt_nee_mis_pick")][1]
        assert pick == base[:4] + [C.c_void_p] + base[4:6] + [C.c_float] + base[6:], stem_mis
        for a, b in ((stem.replace("trt_nee", "trt_nee_pick"), stem.replace("trt_nee", "trt_direct_pick")),
                     (stem.replace("trt_nee", "trt_nee_mis_pick"), stem.replace("trt_nee", "trt_direct_mis_pick"))):
            assert [t for t in S[a][1] if not hasattr(t, "contents")] == [t for t in S[b][1] if not hasattr(t, "contents")], (a, b)
    assert S["trt_nee_pick_launch_plan"][1] == S["trt_nee_mis_pick_launch_plan"][1] == S["trt_nee_launch_plan"][1]
    # the header no longer says that the next-event queries have no PICK form
    assert "the next-event queries are unchanged and still choose uniformly" not in text


def _table(trt, sc):
    return trt.lights.table(sc.emitters(), trt.lights.sphere((50.0, 50.0, 50.0), 2.0, (1.0, 1.0, 1.0)))


def _call(trt, mis, device, s, items, n, table, pick, n_emitters, p, total, rad, m2):
    lib = trt.lib
    if mis:
        if device:
            return lib.trt_nee_mis_pick_device(s, items, n, table, pick, n_emitters, p, total, rad, m2, None, None)
        return lib.trt_nee_mis_pick(s, items, n, table, pick, n_emitters, p, total, rad, m2, None)
    if device:
        return lib.trt_nee_pick_device(s, items, n, table, pick, n_emitters, p, rad, m2, None, None)
    return lib.trt_nee_pick(s, items, n, table, pick, n_emitters, p, rad, m2, None)


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
    assert E == 2
    pick, total = trt.lights.pick_table(table)
    ip, rp, mp, tp, kp = items.ctypes.data, rad.ctypes.data, m2.ctypes.data, table.ctypes.data, pick.ctypes.data
    params = (lambda **kw: AM._params(trt, **kw)) if mis else (lambda **kw: A._params(trt, **kw))
    inner = (lambda q: q.nee) if mis else (lambda q: q)
    p = params()

    def call(s, r, n, q, a, b, t=tp, k=kp, e=E, tot=total):
        return _call(trt, mis, device, s, r, n, t, k, e, C.byref(q) if q is not None else None, C.c_float(tot), a, b)

    # trt_nee's / trt_nee_mis' own, one of each family, each with a NULL pick besides: the sibling's rule is reported
    _invalid(trt, call(None, ip, N, p, rp, mp, k=None))
    _invalid(trt, call(sc._h, ip, N, None, rp, mp, k=None))
    _invalid(trt, call(sc._h, None, N, p, rp, mp, k=None))
    _invalid(trt, call(sc._h, ip, N, p, None, mp, k=None))
    _invalid(trt, call(sc._h, ip, N, params(samples_per_ray=0), rp, mp, k=None))
    _invalid(trt, call(sc._h, ip, N, params(sample_begin=3, sample_end=2), rp, mp, k=None))
    _invalid(trt, call(sc._h, ip, N, params(lobe=3), rp, mp, k=None), "source")
    _invalid(trt, call(sc._h, ip, N, params(lobe=trt._lib.PASSES_CONE, spread=-1.0), rp, mp, k=None), "spread")
    _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=None, k=None), "emitter")
    for e in (0, 2 ** 20 + 1):
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, e=e, k=None), "n_emitters")
    for end in (float("nan"), 0.0, 2.0):
        _invalid(trt, call(sc._h, ip, N, params(shadow_end=end), rp, mp, k=None), "shadow_end")
    _invalid(trt, call(sc._h, ip, N, params(source_is_diffuse=2), rp, mp, k=None), "source_is_diffuse")
    for where in ("path", "gather", "nee"):
        q = params()
        n_ = inner(q)
        (n_.gather.path if where == "path" else n_.gather if where == "gather" else n_).reserved[3] = 1
        _invalid(trt, call(sc._h, ip, N, q, rp, mp, k=None), "reserved")
    if mis:
        _invalid(trt, call(sc._h, ip, N, params(heuristic=2), rp, mp, k=None), "heuristic")
        q = params()
        q.reserved[6] = 1
        _invalid(trt, call(sc._h, ip, N, q, rp, mp, k=None), "reserved")
    # the table's size comes before the source_is_diffuse word, as in trt_nee
    _invalid(trt, call(sc._h, ip, N, params(source_is_diffuse=2), rp, mp, e=0, k=None), "n_emitters")
    # then the pick pointer, in both forms
    _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=None), "null")
    if not device:                                                          # the device form cannot read either table
        bad_kind = table.copy()
        bad_kind["kind"][1] = 2
        bad_q = pick.copy()
        bad_q["q"][0] = 2.0
        _invalid(trt, call(sc._h, ip, N, p, rp, mp, t=bad_kind.ctypes.data, k=bad_q.ctypes.data), "kind")          # the emitter records first
        # then each pick record in table order: q, alias, prob, reserved - ahead of the weighted form's table rule
        lamp_missing = dict(t=table[1:].copy().ctypes.data, e=1)
        for word, field, values in (("q must", "q", (np.nan, -1e-9, 1.0000001, np.inf)), ("alias", "alias", (E, 0xFFFFFFFF)),
                                    ("prob must", "prob", (np.nan, -1e-9, 1.0000001)), ("reserved", "reserved", (1,))):
            for v in values:
                for at in range(E):
                    bad = pick.copy()
                    bad[field][at] = v
                    _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=bad.ctypes.data), word)
                bad = pick[:1].copy()
                bad[field][0] = v
                _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=bad.ctypes.data, **lamp_missing), word)
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
            # the weighted form: trt_nee_mis' table rule, then total_power, then prob bit for bit
            one = pick[:1].copy()
            one["prob"][0] = 1.0
            _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=one.ctypes.data, tot=np.nan, **lamp_missing), "lights")
            for tot in (0.0, -1.0, np.nan, np.inf):
                off = pick.copy()
                off["prob"][1] = np.nextafter(off["prob"][1], np.float32(1.0))
                _invalid(trt, call(sc._h, ip, N, p, rp, mp, k=off.ctypes.data, tot=tot), "total_power")
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
        for kw in (dict(), dict(max_bounces=0), dict(source_is_diffuse=1), dict(lobe=trt._lib.PASSES_RAYS)):
            assert call(sc._h, ip, N, params(**kw), rp, mp) == want_ok, kw
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
    _invalid(trt, call(sc._h, None, 0, params(source_is_diffuse=2), None, None))
    assert call(sc._h, None, 0, p, None, None, t=None, k=None, e=0, tot=0.0) == trt._lib.TRT_OK
    assert call(sc._h, None, 0, p, rp, mp, t=None, k=None, e=7, tot=np.nan) == trt._lib.TRT_OK
    assert (rad == 7.0).all() and (m2 == 7.0).all()


def test_the_python_keyword(trt):
    sc = A._scene(trt)
    table = sc.emitters()
    pick, total = trt.lights.pick_table(table)
    none = np.zeros((0, 6), np.float32)
    for mis in (None, "balance", "power"):
        got, m2, st = sc.nee(none, table, 4, moment2=True, mis=mis, pick=(pick, total))
        assert got.shape == (0, 3) and m2.shape == (0, 3) and st["samples"] == 0 and st["rays"] == 0
    sc.nee(none, table, 4, pick=pick)                                       # the records alone will do without mis
    with pytest.raises(ValueError):
        sc.nee(none, table, 4, mis="balance", pick=pick)                    # ... but the weighted query needs the total
    with pytest.raises(ValueError):
        sc.nee(none, table, 4, pick=pick[:0])
    with pytest.raises(ValueError):
        sc.nee(none, table, 4, pick=np.zeros(1, np.float32))
    with pytest.raises(ValueError):
        sc.nee_device(0, 0, 0, 0, 0, samples_per_item=4, mis="power", pick=1234)
    sc.nee_device(0, 0, 0, 0, 0, samples_per_item=4, pick=0)                # n == 0: nothing is touched
    sc.nee_device(0, 0, 0, 0, 0, samples_per_item=4, mis="power", pick=(0, 1.0))
    sc.nee_device(0, 0, 0, 0, 0, samples_per_item=4)                        # pick=None: the calls of before
    sc.nee_device(0, 0, 0, 0, 0, samples_per_item=4, mis="balance")


def test_the_plan_symbols(trt):
    """The PICK plans check their arguments, and every field is the plan's of the query without the table: the same shapes and bounds
    (profiles/nee_pick_resource_usage.txt)."""
    import test_gpu_queries as G
    import walk_ray_cases as W
    sc = A._scene(trt)
    out = trt._lib.QueryPlan()
    want = trt._lib.TRT_OK if trt.lib.trt_device_count() > 0 else trt._lib.ERR_NO_DEVICE      # compute_units = 0 asks the current device
    for fn in (trt.lib.trt_nee_pick_launch_plan, trt.lib.trt_nee_mis_pick_launch_plan):
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
                q = s.nee_plan(n, 256, mis=mis, pick=True)
                assert q == s.nee_plan(n, 256, mis=mis), (name, options, n, mis)
                assert G.plan_shape(q) == shape
        shapes.add(shape[:3])
    assert len(shapes) == 6


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("pick", (False, True))
@pytest.mark.parametrize("mis", (False, True))
def test_adjacent_checks_are_reported_in_the_documented_order(trt, mis, pick, device):
    """trt_nee, trt_nee_mis, trt_nee_pick, trt_nee_mis_pick and their device forms: the whole documented list of each, walked pair by
    pair (tests/test_direct_pick_abi.py has the walk).  Among them: a table that breaks the table rule and holds a bad pick record gives
    trt_nee_mis_pick the pick-record message, where trt_direct_mis_pick reports the table rule."""
    import test_direct_pick_abi as DP
    sc = A._scene(trt)
    fresh = DP._pair_fixture(trt, sc, (lambda: AM._params(trt)) if mis else (lambda: A._params(trt)))
    own = (lambda c: c["p"].nee) if mis else (lambda c: c["p"])

    def path(field, value):
        return lambda c: setattr(own(c).gather.path, field, value)

    def word(of, k):
        return lambda c: of(c).reserved.__setitem__(k, 1)

    def cone_spread(c):
        own(c).gather.lobe, own(c).gather.spread = trt._lib.PASSES_CONE, -1.0

    faults = [("null argument", DP._set("p", None)), ("null argument", DP._set("s", None)), ("null buffer", DP._set("items", None)),
              ("null buffer", DP._set("rad", None)), ("samples_per_ray must", path("samples_per_ray", 0)), ("sample range", path("sample_begin", 5)),
              ("reserved words must be zero", word(lambda c: own(c).gather.path, 3)), ("2^32", path("first_stream", 2 ** 32 - N * 4 + 1)),
              ("source must", lambda c: setattr(own(c).gather, "lobe", 3)), ("spread", cone_spread),
              ("reserved words must be zero", word(lambda c: own(c).gather, 3)), ("null emitter table", DP._set("table", None)),
              ("n_emitters must", DP._set("E", 0)), ("shadow_end must", lambda c: setattr(own(c), "shadow_end", float("nan"))),
              ("source_is_diffuse must", lambda c: setattr(own(c), "source_is_diffuse", 2)), ("reserved words must be zero", word(own, 3))]
    if mis:
        faults += [("heuristic must", lambda c: setattr(c["p"], "heuristic", 2)), ("reserved words must be zero", word(lambda c: c["p"], 6))]
    faults += DP._ladder_faults(mis, pick, device, False, 2)
    # the spread is only read of a cone: a source that is none cannot also have a bad spread
    DP._walk_adjacent_pairs(trt, faults, fresh, lambda c: DP._entry_call(trt, "nee", mis, pick, device, c), impossible={("source must", "spread")})
