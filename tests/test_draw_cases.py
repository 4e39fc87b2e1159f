"""The inputs of the draw-level test (tests/draw_cases.py, run on the GPU by tests/test_gpu_draws.py) checked on the CPU: the recorded
edge streams are what the oracle's generator says they are, the case list is deterministic, every class has its minimum count and its
defining property under the oracle, NaN words occur only where they are listed, a second float32 restatement of the two draws equals
the oracle bit for bit on every case, and the list tells that restatement from ten altered copies of it (run with -s for the table).
tests/README_draws.md holds the measured counts and the table.
"""
import collections

import numpy as np
import pytest

import draw_cases as D
import shade_cases as S

F = np.float32
MIN_COUNTS = {"generic": 4 * D.GENERIC_PER_KIND, "cos_near_zero_taken": 40, "cos_near_zero_not_taken": 40, "cos_u_zero": 24, "cone_u_zero": 72,
              "sphere_u_zero": 24, "hemi_u_zero": 24, "cone_zero_sum": 24, "cone_tiny_sum": 200, "hemi_dot_zero": 96, "hemi_dot_subnormal": 64,
              "probe_renormalised": 40, "probe_not_renormalised": 40}


@pytest.fixture(scope="module")
def lst(orc):
    """(cases, expectation uint32 [n, 8], traces of the unmutated restatement)."""
    cases = D.case_list(orc)
    exp = D.expectations(orc, cases)
    exp.setflags(write=False)
    traces = []
    for c in cases:
        tr = {}
        D.restate(orc, c, 0, tr)
        traces.append(tr)
    return cases, exp, traces


def of_class(lst, cls):
    cases, exp, traces = lst
    sel = [(c, e, tr) for c, e, tr in zip(cases, exp, traces) if c["cls"] == cls]
    assert sel, cls
    return sel


def fl(words):
    return np.asarray(words, np.uint32).view(F)


def test_recorded_edge_streams_are_zero_draws_under_the_oracle(orc):
    streams = D.edge_streams()
    for pos, name in enumerate(("u1_zero", "u2_zero", "u3_zero")):
        assert len(streams[name]) >= 4 and len(set(streams[name])) == len(streams[name])
        for j in streams[name]:
            draws = D.stream_draws(orc, j)
            assert S.bits(draws[pos])[0] == 0, (name, j, draws)                # exactly +0.0
            assert all(d != 0 for k, d in enumerate(draws) if k != pos), (name, j, draws)
    # the generator's own scan and this file agree on the first entries (the examples of a 2^27 scan)
    assert streams["u1_zero"][0] == 1339711 and streams["u2_zero"][0] == 4364899 and streams["u3_zero"][0] == 7768312
    # the device's seed key is the oracle's seeding: rng_seed(key, j, 1) restated on the host gives orc_rng_seed's state
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_draw_edge_streams", os.path.join(os.path.dirname(__file__), "golden", "make_draw_edge_streams.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    j = np.array([0, 1, 1339711, 0xFFFFFFFF], np.uint32)
    with np.errstate(over="ignore"):
        s0, s1 = gen.rng_seed(D.SEED, j, 1)
        assert int(gen.mix32(np.array([(D.SEED + 0x9E3779B9) & 0xFFFFFFFF], np.uint32))[0]) == D.seed_key()
    for k, jj in enumerate(j):
        st = D.stream_state(orc, int(jj))
        assert (int(s0[k]), int(s1[k])) == (st[0], st[1])


def test_the_list_is_deterministic_and_every_class_has_its_count(lst, orc):
    cases, exp, _ = lst
    count = collections.Counter(c["cls"] for c in cases)
    print(f"\n{len(cases)} cases:", dict(count))
    print("per kind:", dict(collections.Counter(c["kind"] for c in cases)))
    assert set(count) == set(MIN_COUNTS)
    for cls, n in MIN_COUNTS.items():
        assert count[cls] >= n, (cls, count[cls], n)
    again = D.case_list(orc)
    assert len(again) == len(cases)
    for a, b in zip(cases, again):
        assert np.array_equal(D.case_words(a), D.case_words(b)) and a["cls"] == b["cls"]
    order, tasks = D.wave_lists(len(cases))
    n = len(cases)
    assert sorted(order[:n]) == list(range(n)) and sorted(order[n:]) == list(range(n))
    assert tasks[:, 1].sum() == len(order) and set(D.LIST_LENGTHS) <= set(int(x) for x in tasks[1:, 1]) and int(tasks[0, 1]) == n
    assert len({cases[i]["kind"] for i in order[:64]}) == 4                              # the first wave mixes the four kinds
    # one expectation per case by the batched route == the single-case route
    g = np.random.default_rng(3)
    for i in g.choice(n, 200, replace=False):
        assert np.array_equal(exp[i, 0:6], S.bits(D.oracle_ray(orc, cases[i])))


def test_generic_cells(lst):
    sel = of_class(lst, "generic")
    for kind in D.KINDS:
        rows = [c for c, _, _ in sel if c["kind"] == kind]
        assert len(rows) == D.GENERIC_PER_KIND
        lengths = np.array([np.linalg.norm(c["item"][3:6].astype(np.float64)) for c in rows if np.isfinite(c["item"]).all()])
        for scale in (0.25, 1.0, 3.0):
            assert (np.abs(lengths - scale) < 1e-6).sum() > 1200
        assert sum(np.isnan(c["item"][0]) for c in rows) == 4 and sum((c["item"][3:6] == 0).all() for c in rows) == 4
        assert sum(np.isinf(c["item"][3]) for c in rows) == 4 and sum(abs(lengths - 1e-9) < 1e-12) == 4
        assert len({c["j"] for c in rows}) == len(rows)
    assert sorted({float(c["spread"]) for c, _, _ in sel if c["kind"] == "cone"}) == sorted(float(F(s)) for s in D.CONE_SPREADS)


def test_cosine_near_zero_classes(lst, orc):
    taken, not_taken = of_class(lst, "cos_near_zero_taken"), of_class(lst, "cos_near_zero_not_taken")
    for c, e, tr in taken:
        assert tr["near_zero"] and np.array_equal(e[3:6], S.bits(D.oracle_normalized(orc, c["item"][3:6]))), c
        if c["k"] == 0:                                                                      # axis == -u exactly: the sum is (0, 0, 0)
            assert np.array_equal(S.bits(-c["item"][3:6]), S.bits(tr["unit"])) and (tr["sum"] == 0).all()
    assert sum(c["k"] == 0 for c, _, _ in taken) >= 8
    for c, e, tr in not_taken:
        assert not tr["near_zero"] and not np.array_equal(e[3:6], S.bits(D.oracle_normalized(orc, c["item"][3:6]))), c
        assert abs(c["k"]) == c["edge"] and F(1e-7) <= np.abs(tr["sum"]).max() < F(1.2e-7)   # the very next float sum: < one ulp of 0.5 past eps
    # the largest taken nudge sits next to it: for every (stream, component, sign) both sides are in the list
    edges = {(c["j"], c["nudged"], np.sign(c["k"])) for c, _, _ in not_taken}
    inner = {(c["j"], c["nudged"], np.sign(c["k"])) for c, _, _ in taken if c["k"] != 0 and abs(c["k"]) == c["edge"] - 1}
    assert len(edges) == 48 and inner <= edges and len(inner) >= 40                          # (an edge of 1 has no taken nudge)
    # eps 1e-8 and 1e-6 are told apart: taken sums at or above 1e-8, refused sums below 1e-6
    assert sum(np.abs(tr["sum"]).max() >= F(1e-8) for _, _, tr in taken) >= 40
    # components in different binades: the edge is another number of floats in each
    binades = {int(np.floor(np.log2(abs(float(c["item"][3 + c["nudged"]]))))) for c, _, _ in not_taken}
    print(f"\nnear_zero edges: binades {sorted(binades)}, edge nudges {sorted({c['edge'] for c, _, _ in not_taken})}")
    assert len(binades) >= 3 and len({c["edge"] for c, _, _ in not_taken}) >= 3


def test_zero_draw_classes(lst, orc):
    for cls in ("cos_u_zero", "cone_u_zero", "sphere_u_zero", "hemi_u_zero"):
        sel = of_class(lst, cls)
        assert {c["zero"] for c, _, _ in sel} == {"u1_zero", "u2_zero", "u3_zero"}
        for c, e, tr in sel:
            v = tr["in_sphere"]
            assert np.isfinite(c["item"]).all() and not np.isnan(fl(e[0:3])).any()
            if c["zero"] == "u3_zero":
                assert (v == 0).all()
                if cls == "cone_u_zero":                                                     # the axis exactly
                    assert np.array_equal(e[3:6], S.bits(D.oracle_normalized(orc, c["item"][3:6])))
                else:                                                                        # 0 / 0: a NaN ray from a finite item
                    assert np.isnan(fl(e[3:6])).all()
            else:
                assert (v == 0).any() and (v != 0).any() and np.isfinite(fl(e[3:6])).all()   # zero components: normalized()'s plain path
                assert v[1] == 0 and (c["zero"] == "u1_zero" or v[0] == 0)
                if cls in ("sphere_u_zero", "hemi_u_zero"):
                    assert (fl(e[3:6]) == 0).any()


def test_cone_sum_classes(lst):
    sel = of_class(lst, "cone_zero_sum")
    assert {float(c["spread"]) for c, _, _ in sel} >= {0.0, 1.0}
    for c, e, tr in sel:
        assert (tr["sum"] == 0).all() and np.isnan(fl(e[3:6])).all() and not np.isnan(fl(e[0:3])).any()
    sel = of_class(lst, "cone_tiny_sum")
    assert {float(c["spread"]) for c, _, _ in sel} >= {0.0, 1.0}
    below = above = 0
    for c, e, tr in sel:
        s = np.abs(tr["sum"])
        assert (s != 0).any() and s.max() < F(1e-6)
        if s.min() < D.LO:
            below += 1                                                                       # a component below 2^-39: the plain path
        else:
            above += 1
            assert np.isfinite(fl(e[3:6])).all() and abs(float(np.linalg.norm(fl(e[3:6]).astype(np.float64))) - 1.0) < 1e-6
    print(f"\ncone_tiny_sum: {below} sums with a component below 2^-39, {above} with none")
    assert below >= 100 and above >= 30
    mins = {float(np.abs(tr["sum"]).min()) for _, _, tr in sel}
    assert float(D.LO) in mins and float(S.nextf(D.LO, -1)) in mins                          # the switch's own two floats


def test_hemisphere_dot_classes(lst, orc):
    for c, e, tr in of_class(lst, "hemi_dot_zero"):
        axis = c["item"][3:6]
        d = D.oracle_dot(orc, tr["unit"], axis)
        assert d == 0 and tr["dot"] == 0 and np.isfinite(axis).all() and (axis != 0).sum() == 2 and tr["flipped"]
        assert np.array_equal(e[3:6], S.bits(D.oracle_normalized(orc, -tr["unit"])))
    signs = collections.Counter()
    for c, e, tr in of_class(lst, "hemi_dot_subnormal"):
        d = D.oracle_dot(orc, tr["unit"], c["item"][3:6])
        assert d != 0 and abs(d) < D.MIN_NORMAL and S.bits(d)[0] == S.bits(tr["dot"])[0]
        assert tr["flipped"] == bool(d < 0)
        assert np.array_equal(e[3:6], S.bits(D.oracle_normalized(orc, -tr["unit"] if d < 0 else tr["unit"])))
        signs[(int(np.sign(d)), bool((np.abs(c["item"][3:5]) >= D.MIN_NORMAL).all()))] += 1
    print("\nhemi_dot_subnormal (sign of the dot, axis x and y normal numbers):", dict(signs))
    assert len(signs) == 4 and min(signs.values()) >= 8


def test_probe_renormalisation_classes(lst):
    for cls, same in (("probe_renormalised", False), ("probe_not_renormalised", True)):
        sel = of_class(lst, cls)
        assert {c["kind"] for c, _, _ in sel} == {"sphere", "hemisphere"}
        for c, e, tr in sel:
            assert np.array_equal(S.bits(np.abs(fl(e[3:6]))), S.bits(np.abs(tr["unit"]))) == same


def test_nan_words_only_where_listed(lst):
    cases, exp, _ = lst
    n_rows = 0
    for c, e in zip(cases, exp):
        if np.isnan(fl(e[0:6])).any():
            n_rows += 1
            assert D.nan_words_allowed(c), c
    nonfinite = np.array([not np.isfinite(c["item"]).all() for c in cases])
    class_words = int(np.isnan(fl(exp[nonfinite][:, 0:6])).sum())
    print(f"\n{n_rows} rows with NaN words; {int(nonfinite.sum())} rows with a non-finite item hold {class_words} NaN words (compared by class on the GPU, "
          f"twice each); {int(np.isnan(fl(exp[~nonfinite][:, 0:6])).sum())} NaN words in rows with finite items (compared by bits)")
    assert class_words > 0 and n_rows > int(nonfinite.sum()) // 2


def test_second_restatement_equals_the_oracle_bit_for_bit(lst, orc):
    cases, exp, _ = lst
    nonfinite = np.array([not np.isfinite(c["item"]).all() for c in cases])
    got = np.stack([D.restate(orc, c) for c in cases])
    bad, by_class = D.differing_words(got, exp, nonfinite)
    print(f"\nrestatement == oracle on {len(cases)} cases; {int(by_class.sum())} NaN words compared by class")
    rows = np.flatnonzero(bad.any(axis=1))
    assert len(rows) == 0, [(int(r), cases[r]["cls"], cases[r]["kind"], got[r], exp[r]) for r in rows[:5]]


def test_the_case_list_kills_the_mutants(lst, orc):
    cases, exp, _ = lst
    base = np.stack([D.restate(orc, c) for c in cases])
    for mut in range(1, D.N_MUTANTS + 1):
        killers = [i for i, c in enumerate(cases) if not np.array_equal(D.restate(orc, c, mut), base[i])]
        classes = collections.Counter(cases[i]["cls"] for i in killers)
        print(f"\nmutant {mut:2d} ({D.MUTANT_NAMES[mut]}): killed by {len(killers)} cases; classes {dict(classes)}")
        assert set(classes) - {"generic"}, (mut, D.MUTANT_NAMES[mut])


# ------------------------------------------------------------------------------------------------------------------
# the batches of tests/test_gpu_draw_entry.py: what the GPU test compares with is there and is not vacuous
# ------------------------------------------------------------------------------------------------------------------
def test_entry_scenes_cover_both_kernel_forms_and_every_walk_kind():
    import test_gpu_queries as G
    assert [G.DEFAULT_SHAPES[n] for n in D.ENTRY_SCENES] == [(G.LDS, G.LOCK_STEP, 256, 0), (G.GLOBAL, G.NODES16, 256, 0)]
    assert [G.DEFAULT_SHAPES[n][1] for n in D.AT_HIT_SCENES] == [G.LOCK_STEP, G.LDS_TREE, G.NODES16, G.REGISTER_SLOTS]
    assert D.TOP_FIRST_STREAM == 2 ** 32 - 520 and D.TOP_FIRST_STREAM + (D.ENTRY_N - 1) * D.TOP_K + D.TOP_K - 1 == 2 ** 32 - 1


@pytest.fixture(scope="module")
def cornell(trt, orc):
    import passes_cases as PS
    import walk_ray_cases as W
    desc = W.scene(trt, "cornell")
    ow, _ = orc.world_from_description(desc)
    return dict(desc=desc, ow=ow, bg=PS.background_of(desc), items=D.entry_items(orc, ow, desc))


def test_entry_batches_put_item_64_on_the_edge(trt, orc, cornell, lst):
    import gather_cases as GC
    import passes_cases as PS
    c, n, s = cornell, D.ENTRY_N, D.ENTRY_SAMPLE
    batches = D.entry_batches(orc)
    assert set(batches) == {"u1_zero", "u2_zero", "u3_zero", "cos_near_zero_taken", "cone_zero_sum", "cone_tiny_sum", "hemi_dot_zero", "hemi_dot_subnormal"}
    seen = set()
    for name, b in batches.items():
        items = D.entry_batch_items(c["items"], b)
        assert b["first_stream"] + (n - 1) * D.ENTRY_K + s == b["j"]
        for kind in b["kinds"]:
            ref = D.entry_reference(orc, c["ow"], c["desc"], trt.sh.basis, items, kind, D.ENTRY_K, PS.MAX_BOUNCES, c["bg"], b["first_stream"])
            edge = ref["rays"][n - 1, s]
            case = dict(kind=kind, spread=F(GC.SPREAD), item=items[n - 1], j=b["j"])
            assert np.array_equal(S.bits(edge), S.bits(D.oracle_ray(orc, case)))
            others = np.delete(ref["rays"].reshape(-1, 6), (n - 1) * D.ENTRY_K + s, axis=0)
            assert np.isfinite(others).all() and np.isfinite(edge[0:3]).all()
            tr = {}
            D.restate(orc, case, 0, tr)
            axis = items[n - 1, 3:6]
            if name == "u3_zero":
                assert (tr["in_sphere"] == 0).all() and np.isnan(edge[3:6]).all() == (kind != "cone")
            elif name in ("u1_zero", "u2_zero"):
                assert (tr["in_sphere"] == 0).any() and np.isfinite(edge).all()
            elif name == "cos_near_zero_taken":
                assert tr["near_zero"] and np.array_equal(S.bits(edge[3:6]), S.bits(D.oracle_normalized(orc, axis)))
            elif name == "cone_zero_sum":
                assert (tr["sum"] == 0).all() and np.isnan(edge[3:6]).all()
            elif name == "cone_tiny_sum":
                assert (tr["sum"] == 0).sum() == 2 and np.isfinite(edge).all()
            elif name == "hemi_dot_zero":
                assert tr["dot"] == 0 and tr["flipped"] and (axis != 0).any()
            else:
                assert 0 < tr["dot"] < D.MIN_NORMAL and not tr["flipped"]
            if np.isnan(edge).any():
                # traced and counted like any ray: one world.hit call, a miss at depth 0 that carries the background
                assert ref["ends"][n - 1, s] == PS.SKY and ref["depths"][n - 1, s] == 0
                assert np.array_equal(ref["cols"][n - 1, s], np.array(c["bg"], F))
                seen.add((name, kind))
            # the batch is no constant: the fold has many distinct rows
            rows = ref["SH"] if "SH" in ref else ref["S"]
            assert len({r.tobytes() for r in rows}) >= 20, (name, kind)
    assert seen == {("u3_zero", "cosine"), ("u3_zero", "sphere"), ("u3_zero", "hemisphere"), ("cone_zero_sum", "cone")}


def test_oracle_paths_at_any_stream_is_the_oracles_batch_sampler(trt, orc, cornell):
    """entry_reference's paths (passes_cases.oracle_paths) against radiance_cases.oracle_samples (orc.sample_batch), where that can go."""
    import passes_cases as PS
    import radiance_cases as R
    c = cornell
    ref = D.entry_reference(orc, c["ow"], c["desc"], trt.sh.basis, c["items"], "cosine", D.ENTRY_K, PS.MAX_BOUNCES, c["bg"], 1000)
    cols, n_rays = R.oracle_samples(orc, c["ow"], ref["rays"].reshape(-1, 6), 1, PS.MAX_BOUNCES, c["bg"], D.SEED, 1000)
    assert np.array_equal(S.bits(cols.reshape(ref["cols"].shape)), S.bits(ref["cols"])) and n_rays == ref["n_rays"]


@pytest.mark.parametrize("name", D.AT_HIT_SCENES)
def test_ambient_at_a_hit_distance_changes_the_chosen_item(trt, orc, name):
    import walk_ray_cases as W
    desc = W.scene(trt, name)
    ow, _ = orc.world_from_description(desc)
    items = D.entry_items(orc, ow, desc)
    rays, chosen, t_star, calls = D.at_hit_reference(orc, ow, items)
    assert np.array_equal(S.bits(rays[chosen, 0, 3:6]), S.bits(D.oracle_normalized(orc, items[chosen, 3:6])))
    assert [bool(o[chosen, 0]) for _, o, _, _ in calls] == [False, False, True]               # [0.001, max_distance) excludes t* itself
    assert [float(V[chosen]) for _, _, V, _ in calls] == [1.0, 1.0, 0.0]
    assert calls[0][0] < calls[1][0] == float(t_star) < calls[2][0]
    n_occ = [int(o.sum()) for _, o, _, _ in calls]
    print(f"\n{name}: item {chosen}, t* = {float(t_star)!r}; occluded items at the three distances: {n_occ}")
    assert 0 < n_occ[2] < D.ENTRY_N
