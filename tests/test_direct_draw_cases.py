"""The inputs of the draw-level test of the emitter draw (tests/direct_draw_cases.py, run on the GPU by tests/test_gpu_direct_draws.py and
tests/test_gpu_direct_draw_entry.py) checked on the CPU: the recorded edge streams are what the oracle's generator says they are, the
case list and its tables are deterministic, every class has its minimum count and its defining property under the oracle, the pick
clamp is dead code for every E, a second float32 restatement equals the oracle bit for bit on every case, direct_cases.samples and
nee_cases.draw agree with the expectation where they overlap, NaN words occur only where they are listed, and the list tells the
restatement from sixteen altered copies of it by a class other than `generic` (two more are equivalent; run with -s for the table).
tests/README_direct_draws.md holds the measured counts and the table.
"""
import collections

import numpy as np
import pytest

import direct_cases as DC
import direct_draw_cases as D
import nee_cases as NC
import shade_cases as S

F = np.float32
MIN_COUNTS = {"generic": 2 * 11 * D.GENERIC_PER_CELL, "pick_rounded": 100, "pick_top": 36, "u_zero": 128, "cs_zero": 300, "cs_sign": 160, "on_the_light": 300,
              "far": 144, "wgt_edge": 12, "cl_zero": 84, "degenerate": 40, "tmax_edge": 18}


@pytest.fixture(scope="module")
def lst(orc):
    """(cases, tables, expectation uint32 [n, 13], non-finite rows, traces of the expectation)."""
    cases, tabs = D.case_list(orc)
    traces = []
    exp = np.zeros((len(cases), D.OUT_WORDS), np.uint32)
    for i, c in enumerate(cases):
        tr = {}
        exp[i] = D.expect_case(orc, tabs, c, tr)
        traces.append(tr)
    exp2, nonfinite = D.expectations(orc, tabs, cases)
    assert np.array_equal(exp, exp2)
    exp.setflags(write=False)
    return cases, tabs, exp, nonfinite, traces


def of_class(lst, cls):
    cases, _, exp, _, traces = lst
    sel = [(c, e, tr) for c, e, tr in zip(cases, exp, traces) if c["cls"] == cls]
    assert sel, cls
    return sel


def fl(words):
    return np.asarray(words, np.uint32).view(F)


def test_recorded_edge_streams_are_zero_draws_under_the_oracle(orc):
    streams = D.edge_streams()
    for pos, name in enumerate(("u1_zero", "u2_zero", "u3_zero", "u4_zero")):
        assert len(streams[name]) >= 4 and len(set(streams[name])) == len(streams[name])
        for j in streams[name]:
            draws = D.stream_draws(orc, j, 1, 4)
            assert S.bits(draws[pos])[0] == 0, (name, j, draws)                # exactly +0.0
            assert all(d != 0 for d in draws[:pos]), (name, j, draws)
    assert streams["u4_zero"][0] == 1248906                                    # the first of a 2^27 scan (golden/make_direct_edge_streams.py)
    # the vectorised generator of the scans is the oracle's, for every sample word the list uses
    j = np.array([0, 1, 1248906, 0xFFFFFFFF], np.uint32)
    for word in D.WORDS:
        k = D.first_draw_k(j, word)
        for jj, kk in zip(j, k):
            assert F(int(kk) / float(1 << 23)) == D.stream_draws(orc, int(jj), word, 1)[0]


def test_the_pick_clamp_is_dead_code_for_every_table_size():
    """u0 <= 1 - 2^-23 and rounding is monotone: u0 * float(E) <= f32((1 - 2^-23) * E) < E, so uint32(u0 * float(E)) <= E - 1."""
    E = np.arange(1, (1 << 20) + 1, dtype=np.int64)
    fE = E.astype(F)
    assert np.array_equal(fE.astype(np.int64), E)                              # every E is a float
    top = F(1.0 - 2.0 ** -23) * fE
    assert top.dtype == F and (top < fE).all() and (top.astype(np.int64) == E - 1).all()


def test_the_list_and_its_tables_are_deterministic_and_every_class_has_its_count(lst, orc):
    cases, tabs, exp, _, traces = lst
    count = collections.Counter(c["cls"] for c in cases)
    print(f"\n{len(cases)} cases, {len(tabs)} tables:", dict(count))
    print("per form:", dict(collections.Counter(c["form"] for c in cases)), "quads / spheres:", dict(collections.Counter(tr["quad"] for tr in traces)),
          "live / dead:", dict(collections.Counter(tr["live"] for tr in traces)))
    assert set(count) == set(MIN_COUNTS)
    for cls, n in MIN_COUNTS.items():
        assert count[cls] >= n, (cls, count[cls], n)
    again, tabs2 = D.case_list(orc)
    assert len(again) == len(cases) and len(tabs2) == len(tabs)
    for a, b in zip(cases, again):
        assert np.array_equal(D.case_words(a), D.case_words(b)) and a["cls"] == b["cls"]
    for a, b in zip(tabs, tabs2):
        assert a["E"] == b["E"] and a["records"].tobytes() == b["records"].tobytes()
    order, tasks = D.wave_lists(len(cases))
    n = len(cases)
    assert sorted(order[:n]) == list(range(n)) and sorted(order[n:]) == list(range(n))
    assert tasks[:, 1].sum() == len(order) and set(D.LIST_LENGTHS) <= set(int(x) for x in tasks[1:, 1]) and int(tasks[0, 1]) == n
    # the first wave holds quads and spheres, live and dead samples and both forms side by side
    assert len({(traces[i]["quad"], traces[i]["live"], cases[i]["form"]) for i in order[:64]}) == 8


def test_tables(lst):
    _, tabs, _, _, _ = lst
    main = {t["E"]: t for t in tabs if t["name"] == "E%d" % t["E"]}
    assert tuple(sorted(main)) == tuple(sorted(D.MAIN_E)) == (1, 2, 3, 5, 64, 1000, 1000003, (1 << 20) - 1, 1 << 20)
    for t in tabs:
        r = t["records"]
        assert 1 <= len(r) <= D.MAX_PERIOD and len(r) <= t["E"] <= (1 << 20) and r.dtype == DC.EMITTER_DTYPE
    for E, t in main.items():
        r = t["records"]
        assert len({x.tobytes() for x in r["color"]}) == len(r) and len({x.tobytes() for x in r["a"]}) == len(r)
        if E >= 5:
            assert (r["kind"] == 1).any() and (r["kind"] == 0).any()
    assert [int(k) for k in main[3]["records"]["kind"]] == [2, 0x3F800000, 0xFFFFFFFF]
    assert (main[5]["records"]["area"] < 0).sum() == 1 and (main[64]["records"]["area"] == 0).sum() == 1
    # the large tables repeat a period of many records: neighbouring picks are different records
    for E in (1000, 1000003, (1 << 20) - 1, 1 << 20):
        assert len(main[E]["records"]) >= 37


def test_generic_cells(lst):
    sel = of_class(lst, "generic")
    _, tabs, _, _, _ = lst
    cells = collections.Counter((tabs[c["t"]]["name"], c["form"]) for c, _, _ in sel)
    assert len(cells) == 22 and set(cells.values()) == {D.GENERIC_PER_CELL}
    assert {tabs[c["t"]]["E"] for c, _, _ in sel} >= set(D.MAIN_E)
    assert {c["word"] for c, _, _ in sel} == set(D.WORDS) and {float(c["shadow_end"]) for c, _, _ in sel} == {float(s) for s in D.SHADOW_ENDS}
    for name, form in cells:
        rows = [c for c, _, _ in sel if tabs[c["t"]]["name"] == name and c["form"] == form]
        assert sum(np.isnan(c["x"][0]) for c in rows) >= 1 and sum((c["n"] == 0).all() for c in rows) >= 1
        assert sum(np.isinf(c["n"][0]) for c in rows) >= 1 and sum(abs(float(np.linalg.norm(c["n"].astype(np.float64))) - 1e-9) < 1e-12 for c in rows) >= 1
        assert [c["j"] for c in rows] == list(range(rows[0]["j"], rows[0]["j"] + len(rows)))
    live = sum(tr["live"] for _, _, tr in sel)
    assert 0.2 * len(sel) < live < 0.8 * len(sel)


def test_pick_classes(lst):
    _, tabs, _, _, _ = lst
    per_E = collections.Counter()
    for c, e, tr in of_class(lst, "pick_rounded"):
        E = tabs[c["t"]]["E"]
        exact = (int(round(float(tr["u0"]) * (1 << 23))) * E) >> 23
        assert tr["pick"] != exact and exact == c["exact"] and abs(tr["pick"] - exact) == 1 and tr["pick"] < E
        # a wrong pick is another record: colour and position differ
        a, b = D.record_of(tabs[c["t"]], tr["pick"]), D.record_of(tabs[c["t"]], exact)
        assert a["color"].tobytes() != b["color"].tobytes() and a["a"].tobytes() != b["a"].tobytes()
        per_E[E] += 1
    print("\npick_rounded per E:", dict(per_E))
    assert set(per_E) == set(D.ROUNDED_E) and per_E[1000003] >= 40 and per_E[(1 << 20) - 1] >= 40 and per_E[1000] >= 8
    seen = set()
    for c, e, tr in of_class(lst, "pick_top"):
        E = tabs[c["t"]]["E"]
        assert tr["pick"] == c["want"] and c["want"] in (0, E - 1)
        assert (tr["u0"] == 0) == (c["want"] == 0 and E > 1) or E == 1
        seen.add((E, c["want"]))
    assert seen == {(E, w) for E in D.MAIN_E for w in (0, E - 1)}
    top = max(float(tr["u0"]) for _, _, tr in of_class(lst, "pick_top"))
    assert top >= 1.0 - 2.0 ** -21                                             # the largest u0 of the scan: E - 1 for every E <= 2^20


def test_zero_draw_class(lst, orc):
    sel = of_class(lst, "u_zero")
    seen = collections.Counter()
    for c, e, tr in sel:
        pos = ("u1_zero", "u2_zero", "u3_zero", "u4_zero").index(c["zero"])
        draws = D.stream_draws(orc, c["j"], c["word"], 4)
        assert draws[pos] == 0 and np.isfinite(c["x"]).all() and np.isfinite(c["n"]).all()
        seen[(c["zero"], tr["quad"])] += 1
        if c["zero"] == "u1_zero":
            assert tr["pick"] == 0
        if c["zero"] == "u4_zero" and not tr["quad"]:                          # the sphere's u3: nl = 0/0, dead by NaN
            assert np.isnan(tr["nl"]).all() and not tr["live"] and np.isnan(fl(e[3:10])).all() and not np.isnan(fl(e[0:3])).any()
        elif c["zero"] != "u4_zero":
            assert np.isfinite(tr["y"]).all() and np.isfinite(fl(e[0:10])).all()
    print("\nu_zero (draw, quad):", dict(seen))
    assert len(seen) == 8 and min(seen.values()) >= 8


def test_cosine_classes(lst):
    for c, e, tr in of_class(lst, "cs_zero"):
        assert S.bits(tr["cs"])[0] == 0 and not tr["live"] and tr["d2"] > 0 and np.isfinite(tr["wgt"]) and e[10] == 0
    signs = collections.Counter()
    for c, e, tr in of_class(lst, "cs_sign"):
        if c.get("negative_zero"):
            assert S.bits(tr["cs"])[0] == 0x80000000 and not tr["live"]
            signs["-0"] += 1
        else:
            assert tr["cs"] != 0 and abs(tr["cs"]) < D.MIN_NORMAL and tr["live"] == bool(tr["cs"] > 0)
            signs[int(np.sign(tr["cs"]))] += 1
    print("\ncs_sign:", dict(signs))
    assert signs["-0"] >= 20 and signs[1] >= 60 and signs[-1] >= 60


def test_on_the_light_and_far_classes(lst):
    kinds = collections.Counter()
    sides = collections.Counter()
    for c, e, tr in of_class(lst, "on_the_light"):
        w, d2 = tr["w"], tr["d2"]
        with np.errstate(all="ignore"):
            dd = d2 * d2
        if c.get("exact"):
            assert (w == 0).all() and d2 == 0 and np.isnan(fl(e[3:6])).all() and S.bits(fl(e[9]))[0] == 0 and not tr["live"]
            kinds["x = y"] += 1
        elif d2 == 0:
            assert (w != 0).any() and not tr["live"]
            kinds["d2 = 0, w != 0"] += 1
        elif d2 < D.MIN_NORMAL:
            assert dd == 0 and not np.isfinite(tr["wgt"]) and not tr["live"]
            kinds["d2 subnormal"] += 1
        else:
            kinds["d2 ordinary"] += 1
        if (w != 0).any():
            sides[bool(np.abs(w[w != 0]).min() < D.LO)] += 1
    print("\non_the_light:", dict(kinds), "smallest non-zero component below 2^-39:", dict(sides))
    assert kinds["x = y"] >= 18 and kinds["d2 = 0, w != 0"] >= 12 and kinds["d2 subnormal"] >= 12 and kinds["d2 ordinary"] >= 200
    assert sides[True] >= 30 and sides[False] >= 30
    ends = collections.Counter()
    for c, e, tr in of_class(lst, "far"):
        with np.errstate(all="ignore"):
            assert np.isinf(tr["d2"] * tr["d2"]) and (S.bits(tr["wgt"])[0] == 0 or (np.isnan(tr["wgt"]) and np.isinf(tr["cs"] * tr["cl"])))
        assert np.isinf(tr["d2"]) == (c["log2"] == 65) and np.isinf(tr["t_max"]) == (c["log2"] == 65) and tr["cs"] > 0
        assert tr["live"] == bool(tr["wgt"] == 0)
        ends[(c["log2"], tr["live"])] += 1
    print("far (log2 |w|, live):", dict(ends))
    assert all(ends[(e, True)] >= 12 for e in (40, 63, 65)) and ends[(65, False)] >= 12 and ends[(40, False)] == ends[(63, False)] == 0


def test_weight_edges(lst):
    _, tabs, _, _, _ = lst
    seen = {}
    for c, e, tr in of_class(lst, "wgt_edge"):
        seen[(c["j"], c["edge"], c["side"], c["form"])] = (tabs[c["t"]]["records"]["area"][0], tr["wgt"], tr["live"])
    edges = {(j, edge) for j, edge, _, _ in seen}
    assert {edge for _, edge in edges} == {"inf", "normal", "nonzero"}
    for j, edge in edges:
        (a0, w0, l0), (a1, w1, l1) = seen[(j, edge, "below", "item")], seen[(j, edge, "above", "item")]
        assert S.bits(a1)[0] == S.bits(a0)[0] + 1                              # neighbouring floats
        if edge == "inf":
            assert np.isfinite(w0) and l0 and np.isinf(w1) and not l1
        elif edge == "normal":
            assert 0 < w0 < D.MIN_NORMAL <= w1 and l0 and l1
        else:
            assert S.bits(w0)[0] == 0 and w1 > 0 and l0 and l1
        print(f"\nwgt_edge {edge} (stream {j}): area {a0!r} -> weight {w0!r}, area {a1!r} -> weight {w1!r}")


def test_cl_zero_degenerate_and_tmax_classes(lst):
    _, tabs, _, _, _ = lst
    kinds = collections.Counter()
    for c, e, tr in of_class(lst, "cl_zero"):
        d = S.dot(tr["nl"], tr["w"])
        if c["height"] == 0:
            assert S.bits(tr["cl"])[0] == 0 and S.bits(tr["wgt"])[0] == 0 and tr["live"] and e[10] == 1
            assert sorted(int(x) for x in e[6:9]) == [0, 0x80000000, 0x80000000]          # colour (-1, 2, -0.5) times +0
            kinds["zero"] += 1
        else:
            assert d != 0 and abs(d) < D.MIN_NORMAL and np.sign(d) == -np.sign(c["height"]) and tr["live"]
            kinds[int(np.sign(d))] += 1
    assert kinds["zero"] >= 12 and kinds[1] >= 30 and kinds[-1] >= 30
    picked = collections.Counter(c["record"] for c, _, tr in of_class(lst, "degenerate") if tr["pick"] == c["record"])
    assert set(picked) == set(range(10)) and min(picked.values()) >= 4
    seen = {}
    for c, e, tr in of_class(lst, "tmax_edge"):
        want = {-1: S.nextf(D.T_MIN, -1), 0: D.T_MIN, 1: S.nextf(D.T_MIN, 1)}[c["side"]]
        assert S.bits(tr["t_max"])[0] == S.bits(want)[0] == e[9] and bool(tr["t_max"] > D.T_MIN) == (c["side"] == 1) and tr["live"]
        seen[(float(c["shadow_end"]), c["side"])] = True
    assert len(seen) == 9


def test_every_non_generic_case_is_there_in_both_forms(lst):
    cases, _, exp, _, _ = lst
    rest = [(c, e) for c, e in zip(cases, exp) if c["cls"] != "generic"]
    assert len(rest) % 2 == 0
    for (a, ea), (b, eb) in zip(rest[0::2], rest[1::2]):
        assert (a["form"], b["form"]) == D.FORMS and np.array_equal(D.case_words(a)[1:], D.case_words(b)[1:]) and np.array_equal(ea, eb)


def test_nan_words_only_where_listed(lst):
    cases, _, exp, nonfinite, _ = lst
    rows = collections.Counter()
    for c, e, nf in zip(cases, exp, nonfinite):
        if np.isnan(fl(e[0:10])).any():
            rows[c["cls"]] += 1
            assert D.nan_words_allowed(c, nf), c
            # a NaN in the surfel, the draw or the record's geometry fails one of the three rules; one in the colour alone reaches c only
            assert e[10] == 0 or (nf and not np.isnan(fl(e[0:6])).any() and not np.isnan(fl(e[9]))), c
    words = {cls: int(np.isnan(fl(exp[[i for i, c in enumerate(cases) if c["cls"] == cls]][:, 0:10])).sum()) for cls in rows}
    print(f"\nrows with NaN words per class: {dict(rows)}; NaN words per class: {words}; {int(nonfinite.sum())} rows with a non-finite surfel or record")
    assert rows["u_zero"] >= 8 and rows["on_the_light"] >= 18 and rows["generic"] >= 40


def test_second_restatement_equals_the_oracle_bit_for_bit(lst, orc):
    cases, tabs, exp, nonfinite, _ = lst
    got = np.stack([D.restate_case(orc, tabs, c) for c in cases])
    bad, by_class = D.differing_words(got, exp, nonfinite)
    print(f"\nrestatement == oracle on {len(cases)} cases; {int(by_class.sum())} NaN words passed by class")
    rows = np.flatnonzero(bad.any(axis=1))
    assert len(rows) == 0, [(int(r), cases[r]["cls"], got[r], exp[r]) for r in rows[:5]]


def test_the_two_restatements_of_the_queries_agree_with_it(lst, orc):
    """nee_cases.draw (any sample word) and direct_cases.samples (word 1): the modules the entry-point tests take their reference from."""
    cases, tabs, exp, _, traces = lst
    n_direct = 0
    for i, (c, e, tr) in enumerate(zip(cases, exp, traces)):
        if c["form"] != "item" and c["cls"] != "generic":
            continue                                                           # the second form of a pair holds the same values
        table = D.Periodic(tabs[c["t"]])
        live, walked, occ, col = NC.draw(orc, None, c["x"], c["n"], table, D.SEED, c["j"], c["word"], c["shadow_end"], occlusion=False)
        assert live == bool(e[10]) and walked == (live and bool(tr["t_max"] > D.T_MIN)) and not occ
        same = S.bits(col) == e[6:9]
        assert (same | (np.isnan(col) & np.isnan(fl(e[6:9])))).all(), (i, c["cls"])
        if c["word"] == 1:
            smp = DC.samples(orc, None, np.concatenate([c["x"], c["n"]])[None, :], table, k=1, seed=D.SEED, first_stream=c["j"], shadow_end=c["shadow_end"],
                             occlusion=False)
            assert smp["e"][0, 0] == tr["pick"] and bool(smp["live"][0, 0]) == live and bool(smp["walked"][0, 0]) == walked
            assert S.bits(smp["t_max"][0, 0])[0] == e[9] or (np.isnan(smp["t_max"][0, 0]) and np.isnan(tr["t_max"]))
            ray = S.bits(smp["rays"][0, 0])
            assert ((ray == e[0:6]) | (np.isnan(smp["rays"][0, 0]) & np.isnan(fl(e[0:6])))).all()
            if live:
                assert np.array_equal(S.bits(smp["c"][0, 0]), e[6:9])
            else:
                assert (smp["c"][0, 0] == 0).all()
            n_direct += 1
    assert n_direct >= 1500                                                    # a third of the generic rows and every non-generic pair


def test_the_case_list_kills_the_mutants(lst, orc):
    cases, tabs, _, _, _ = lst
    base = np.stack([D.restate_case(orc, tabs, c) for c in cases])
    for mut in range(1, D.N_MUTANTS + 1):
        killers = [i for i, c in enumerate(cases) if not np.array_equal(D.restate_case(orc, tabs, c, mut), base[i])]
        classes = collections.Counter(cases[i]["cls"] for i in killers)
        print(f"\nmutant {mut:2d} ({D.MUTANT_NAMES[mut]}): killed by {len(killers)} cases; classes {dict(classes)}")
        if mut in D.EQUIVALENT_MUTANTS:
            assert not killers, (mut, D.MUTANT_NAMES[mut])                     # proved equivalent in direct_draw_cases' text; 2: the test above
        else:
            assert set(classes) - {"generic"}, (mut, D.MUTANT_NAMES[mut])
    # mutant 4's proof on the list's own rows: wherever d2 is 0 the weight is not finite
    _, _, _, _, traces = lst
    zero = [tr for tr in traces if tr["d2"] == 0]
    assert len(zero) >= 30 and not any(np.isfinite(tr["wgt"]) for tr in zero)


# ------------------------------------------------------------------------------------------------------------------
# the batches of tests/test_gpu_direct_draw_entry.py: what the GPU test compares with is there and is not vacuous
# ------------------------------------------------------------------------------------------------------------------
EDGE = (D.ENTRY_N - 1, D.ENTRY_SAMPLE)
EDGE_STATE = dict(cs_zero=(False, False), on_the_light=(False, False), wgt_max=(True, False), wgt_inf=(False, False), cl_zero=(True, True), u4_zero=(False, False),
                  pick_rounded=(True, True), tmax_below=(True, False), tmax_at=(True, False), tmax_above=(True, True))          # (live, walked)


@pytest.fixture(scope="module")
def cornell(trt, orc):
    import draw_cases as DR
    import passes_cases as PS
    import walk_ray_cases as W
    desc = W.scene(trt, "cornell")
    ow, _ = orc.world_from_description(desc)
    return dict(desc=desc, ow=ow, bg=PS.background_of(desc), items=DR.entry_items(orc, ow, desc))


def test_entry_scenes_cover_both_kernel_forms():
    import test_gpu_queries as G
    assert [G.DEFAULT_SHAPES[n] for n in D.ENTRY_SCENES] == [(G.LDS, G.LOCK_STEP, 256, 0), (G.GLOBAL, G.NODES16, 256, 0)]


def test_direct_entry_batches_put_item_64_on_the_edge(orc, cornell, lst):
    cases, tabs, _, _, _ = lst
    batches = D.direct_entry_batches(orc)
    assert set(batches) == set(EDGE_STATE)
    refs = {}
    for name, b in batches.items():
        assert b["first_stream"] + EDGE[0] * D.ENTRY_K + EDGE[1] == b["j"] and b["table"]["E"] <= 1000 or b["device_only"]
        items = D.direct_entry_items(cornell["items"], b)
        ref = refs[name] = D.direct_entry_reference(orc, cornell["ow"], items, b)
        tr = {}
        exp = D.expect(orc, b["table"], b["j"], 1, b["shadow_end"], items[EDGE[0], 0:3], items[EDGE[0], 3:6], tr)
        ray = ref["rays"][EDGE]
        assert ((S.bits(ray) == exp[0:6]) | np.isnan(ray)).all() and ref["e"][EDGE] == tr["pick"]
        assert (bool(ref["live"][EDGE]), bool(ref["walked"][EDGE])) == EDGE_STATE[name] == (tr["live"], tr["live"] and bool(tr["t_max"] > D.T_MIN)), name
        assert not ref["occ"][EDGE], name
        assert np.isfinite(ref["rays"][:EDGE[0]]).all() and len({r.tobytes() for r in ref["S"]}) >= 20, name
        if not name.startswith("tmax"):                                       # the batch IS a case of the list
            assert any(c["j"] == b["j"] and c["word"] == 1 and tabs[c["t"]]["name"] == b["table"]["name"]
                       and np.array_equal(np.concatenate([c["x"], c["n"]]), b["surfel"]) for c in cases), name
    tr = {}
    b = batches["pick_rounded"]
    D.expect(orc, b["table"], b["j"], 1, b["shadow_end"], b["surfel"][0:3], b["surfel"][3:6], tr)
    assert b["table"]["E"] == 1000003 and tr["pick"] != (int(round(float(tr["u0"]) * (1 << 23))) * 1000003) >> 23 and len(b["table"]["records"]) == 61
    assert refs["wgt_max"]["wgt"][EDGE] == np.finfo(F).max and np.isinf(refs["wgt_inf"]["wgt"][EDGE])
    assert S.bits(refs["cs_zero"]["wgt"][EDGE])[0] == 0 and refs["on_the_light"]["t_max"][EDGE] == 0 and np.isnan(refs["u4_zero"]["t_max"][EDGE])
    assert S.bits(refs["cl_zero"]["wgt"][EDGE])[0] == 0 and (refs["cl_zero"]["c"][EDGE] == 0).all()
    # t_max one float either side of 0.001: the same table, stream and the other 259 samples; one walk more above, the term added in all three
    t = [int(S.bits(refs[s]["t_max"][EDGE])[0]) for s in D.TMAX_SIDES]
    assert t[0] + 1 == t[1] == int(S.bits(D.T_MIN)[0]) == t[2] - 1
    walks = [refs[s]["n_walks"] for s in D.TMAX_SIDES]
    assert walks[0] == walks[1] == walks[2] - 1
    assert list(refs["tmax_at"]["e"][EDGE[0]]) == [1, 0, 1, 1]                 # only sample 1 of item 64 picks the record at the origin
    for s in D.TMAX_SIDES:
        assert (refs[s]["c"][EDGE] != 0).all() and np.array_equal(refs[s]["S"][:EDGE[0]], refs["tmax_at"]["S"][:EDGE[0]])


def test_nee_entry_tables_are_built_around_the_first_lambertian_vertex(orc, cornell, monkeypatch):
    c = cornell
    st = D.nee_entry_setup(orc, c["ow"], c["desc"], c["items"])
    assert st["first_stream"] + EDGE[0] * D.ENTRY_K + EDGE[1] == st["j"] and st["d"] == 0
    assert st["t_max"]["tmax_below"] < D.T_MIN < st["t_max"]["tmax_above"] and set(st["tables"]) >= {"light_on_vertex", "sphere_on_vertex", "tmax_below", "tmax_above"}
    # the vertex is where nee_cases.nee_path makes its first draw of that sample
    calls = []
    real = NC.draw

    def spy(orc_, ow, x, nrm, table, seed, stream, word, *a, **kw):
        calls.append((stream, word, np.array(x, F), np.array(nrm, F)))
        return real(orc_, ow, x, nrm, table, seed, stream, word, *a, **kw)

    monkeypatch.setattr(NC, "draw", spy)
    refs = {tn: D.nee_entry_reference(orc, c["ow"], c["desc"], c["items"], st, table, c["bg"], False) for tn, table in st["tables"].items()}
    first = [k for k in calls if k[0] == st["j"]][0]
    assert first[1] == 2 and np.array_equal(first[2], st["x"]) and np.array_equal(first[3], st["n"])
    below, above = refs["tmax_below"], refs["tmax_above"]
    assert above["n_rays"] == below["n_rays"] + 1 and above["walks"][EDGE] == below["walks"][EDGE] + 1 and above["lit"][EDGE] == below["lit"][EDGE] >= 1
    for tn in ("light_on_vertex", "sphere_on_vertex"):
        assert refs[tn]["lit"][EDGE] == below["lit"][EDGE] - 1
    print(f"\nnext-event batch on cornell: first_stream {st['first_stream']}, vertex {st['x']}, normal {st['n']}; t_max {st['t_max']}; "
          f"rays below / above 0.001: {below['n_rays']} / {above['n_rays']}")
