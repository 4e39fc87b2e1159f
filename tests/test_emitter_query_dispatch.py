"""How api.py hands the eight emitter-table queries (direct / nee x plain / mis x uniform / pick) to the C ABI, without a GPU and without
the library doing anything: `lib` is replaced by a recorder that answers TRT_OK, and every public form - direct, direct_device,
direct_plan, nee, nee_device, nee_plan - is called over mis in {None, "balance", "power"} x pick in {None, records, (records, total)}.
Checked per call: the symbol, the number of arguments, the parameter struct's type and heuristic, where the pick pointer and total_power
stand, and that n == 0 and an absent moment2 pass null pointers.  Then the ValueErrors the wrappers raise themselves."""
import ctypes as C

import numpy as np
import pytest

N_ITEMS, N_EMITTERS = 3, 2
MIS = (None, "balance", "power")


class Recorder:
    """Stands where api.py's `lib` stands: the *_params_default functions are the library's own, every other symbol is noted and succeeds."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith("_params_default"):
            return getattr(self.real, name)

        def symbol(*args):
            self.calls.append((name, args))
            return 0
        return symbol


@pytest.fixture
def scene(trt, monkeypatch):
    rec = Recorder(trt.lib)
    monkeypatch.setattr(trt.api, "lib", rec)
    sc = object.__new__(trt.api.Scene)
    sc._h = C.c_void_p(0x1234)                                              # never handed to the library
    yield sc, rec
    sc._h = None


def _tables(trt):
    table = trt.lights.table(trt.lights.sphere((0.0, 5.0, 0.0), 1.0, (1.0, 1.0, 1.0)), trt.lights.sphere((5.0, 5.0, 0.0), 2.0, (2.0, 1.0, 1.0)))
    assert len(table) == N_EMITTERS
    records, total = trt.lights.pick_table(table)
    return table, records, total


def _params_of(trt, family, arg, mis):
    """The struct behind the byref argument: its type says which query, its heuristic which weighting."""
    p = arg._obj
    plain, weighted = {"direct": (trt._lib.DirectParams, trt._lib.DirectMisParams), "nee": (trt._lib.NeeParams, trt._lib.NeeMisParams)}[family]
    if mis is None:
        assert type(p) is plain
    else:
        assert type(p) is weighted and p.heuristic == {"balance": trt._lib.MIS_BALANCE, "power": trt._lib.MIS_POWER}[mis]
    return p


def _symbol(family, mis, pick, suffix=""):
    return "trt_" + family + ("_mis" if mis is not None else "") + ("_pick" if pick is not None else "") + suffix


def _value(a):
    return a.value if hasattr(a, "value") else a


@pytest.mark.parametrize("pick_form", ("none", "records", "pair"))
@pytest.mark.parametrize("mis", MIS)
@pytest.mark.parametrize("family", ("direct", "nee"))
def test_the_host_form(trt, scene, family, mis, pick_form):
    sc, rec = scene
    table, records, total = _tables(trt)
    pick = {"none": None, "records": records, "pair": (records, total)}[pick_form]
    items = np.zeros((N_ITEMS, 6), np.float32)
    query = getattr(sc, family)
    if mis is not None and pick_form == "records":
        with pytest.raises(ValueError, match="records, total"):
            query(items, table, 4, mis=mis, pick=pick)
        assert rec.calls == []
        return
    for n, want_m2 in ((N_ITEMS, True), (N_ITEMS, None), (0, True)):
        rec.calls.clear()
        rad, m2, st = query(items[:n], table, 4, mis=mis, pick=pick, moment2=want_m2)
        assert rad.shape == (n, 3) and (m2 is None if want_m2 is None else m2.shape == (n, 3)) and st == trt._lib.Stats().as_dict()
        (name, args), = rec.calls
        assert name == _symbol(family, mis, pick)
        assert len(args) == 9 + (pick is not None) + (pick is not None and mis is not None)
        assert args[0] is sc._h and args[2] == n and args[3] == table.ctypes.data
        assert (args[1] is None) == (n == 0)                                # the items
        at = 4
        if pick is not None:
            assert isinstance(args[4], int) and args[4] != 0 and args[4] != table.ctypes.data      # the pick pointer stands behind the table
            at = 5
        assert args[at] == N_EMITTERS
        _params_of(trt, family, args[at + 1], mis)
        at += 2
        if pick is not None and mis is not None:
            assert isinstance(args[at], C.c_float) and args[at].value == total                     # total_power stands behind the parameters
            at += 1
        assert (args[at] is None) == (n == 0) and (n == 0 or args[at] == rad.ctypes.data)
        assert args[at + 1] == (m2.ctypes.data if want_m2 and n else None)
        assert isinstance(args[at + 2]._obj, trt._lib.Stats)
    # an empty table and an empty pick table are null pointers too
    rec.calls.clear()
    none = None if pick is None else (records[:0], total) if pick_form == "pair" else records[:0]
    query(items[:0], table[:0], 4, mis=mis, pick=none)
    (name, args), = rec.calls
    assert args[3] is None and (pick is None or args[4] is None) and args[5 if pick is not None else 4] == 0


@pytest.mark.parametrize("pick_form", ("none", "pointer", "pair"))
@pytest.mark.parametrize("mis", MIS)
@pytest.mark.parametrize("family", ("direct", "nee"))
def test_the_device_form(trt, scene, family, mis, pick_form):
    sc, rec = scene
    pick = {"none": None, "pointer": 0x5000, "pair": (0x5000, 2.5)}[pick_form]
    query = getattr(sc, family + "_device")
    if mis is not None and pick_form == "pointer":
        with pytest.raises(ValueError, match="records, total"):
            query(0x1000, N_ITEMS, 0x2000, N_EMITTERS, 0x3000, samples_per_item=4, mis=mis, pick=pick)
        assert rec.calls == []
        return
    assert query(0x1000, N_ITEMS, 0x2000, N_EMITTERS, 0x3000, d_counters_ptr=0x6000, samples_per_item=4, mis=mis, pick=pick) is None
    (name, args), = rec.calls
    assert name == _symbol(family, mis, pick, "_device")
    assert len(args) == 10 + (pick is not None) + (pick is not None and mis is not None)
    assert args[0] is sc._h and _value(args[1]) == 0x1000 and args[2] == N_ITEMS and _value(args[3]) == 0x2000
    at = 4
    if pick is not None:
        assert _value(args[4]) == 0x5000
        at = 5
    assert args[at] == N_EMITTERS
    _params_of(trt, family, args[at + 1], mis)
    at += 2
    if pick is not None and mis is not None:
        assert isinstance(args[at], C.c_float) and args[at].value == 2.5
        at += 1
    assert [_value(a) for a in args[at:]] == [0x3000, None, 0x6000, None]  # radiance, no moment2, counters, the default stream


@pytest.mark.parametrize("pick", (None, True))
@pytest.mark.parametrize("mis", MIS)
@pytest.mark.parametrize("family", ("direct", "nee"))
def test_the_plan_form(trt, scene, family, mis, pick):
    sc, rec = scene
    plan = getattr(sc, family + "_plan")(257, 256, mis=mis, pick=pick)
    (name, args), = rec.calls
    assert name == _symbol(family, mis, pick, "_launch_plan")
    assert len(args) == 4 and args[0] is sc._h and args[1:3] == (257, 256) and isinstance(args[3]._obj, trt._lib.QueryPlan)
    assert plan == trt._lib.QueryPlan().as_dict()


@pytest.mark.parametrize("family", ("direct", "nee"))
def test_what_the_wrappers_refuse_themselves(trt, scene, family):
    sc, rec = scene
    table, records, total = _tables(trt)
    items = np.zeros((N_ITEMS, 6), np.float32)
    query, device, plan = getattr(sc, family), getattr(sc, family + "_device"), getattr(sc, family + "_plan")
    with pytest.raises(ValueError, match="mis must be"):
        query(items, table, 4, mis="optimal")
    with pytest.raises(ValueError, match="mis must be"):
        device(0, 0, 0, 0, 0, samples_per_item=4, mis="optimal")
    with pytest.raises(ValueError, match="records, total"):
        query(items, table, 4, mis="power", pick=records)
    with pytest.raises(ValueError, match="records, total"):
        device(0, 0, 0, 0, 0, samples_per_item=4, mis="balance", pick=0x5000)
    for bad in (records[:1], np.zeros(N_EMITTERS, np.float32), np.zeros((N_EMITTERS, 1), trt.lights.PICK_DTYPE)):
        with pytest.raises(ValueError, match="PICK_DTYPE"):
            query(items, table, 4, pick=bad)
        with pytest.raises(ValueError, match="PICK_DTYPE"):
            query(items, table, 4, mis="balance", pick=(bad, total))
    with pytest.raises(ValueError, match="EMITTER_DTYPE"):
        query(items, np.zeros(N_EMITTERS, np.float32), 4)
    with pytest.raises(ValueError, match="rays must be"):
        query(items[:, :5], table, 4)
    if family == "nee":
        with pytest.raises(ValueError, match="source must be"):
            query(items, table, 4, source="lobe")
        with pytest.raises(ValueError, match="source must be"):
            device(0, 0, 0, 0, 0, samples_per_item=4, source="lobe")
    with pytest.raises(AssertionError):
        query(items, table, 4, radiance=np.zeros((N_ITEMS, 3), np.float64))
    with pytest.raises(AssertionError):
        query(items, table, 4, moment2=np.zeros((N_ITEMS + 1, 3), np.float32))
    assert rec.calls == []
    plan(1)                                                                # the plans take anything for mis and pick but None
    assert rec.calls[0][0] == "trt_" + family + "_launch_plan"
