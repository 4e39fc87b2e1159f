"""The restatement of the alias-table next-event queries (tests/nee_pick_cases.py) without a GPU: it is nee_cases' / nee_mis_cases'
restatement where the table says nothing new, every deliberately wrong variant of it is told apart by a named class of cases, the two
weights of one light point sum to 1, it is unbiased against the restated trt_nee_mis with the uniform choice, and it does what the
feature is for - less variance where powers differ.

Classes (the Cornell box's 324 items of nee_cases, B = 5, its table of three - the lamp, a virtual quad, a virtual sphere - and the same box
with the lamp recoloured so that its luminance depends on the parenthesisation):
  edge_of_q        one vertex draw with q[k] set to its own u1: the alias is taken; `u1 <= q` keeps the slot
  alias_taken      vertex draws that took an alias whose prob is not the slot's
  later_vertices   paths that draw at a second or later vertex: the table is used there too
  shadow_weight    lit shadow samples of the lamp in the weighted query: wl comes from the PICK weight
  weighted_hits    the lamp reached after a diffuse scatter at hit >= 2: ph has the bits of the table's prob
Mutants (nee_pick_cases.MUTANTS) and the class that kills each are listed in KILLED_BY."""
import ctypes as C

import numpy as np
import pytest

import direct_cases as D
import direct_pick_cases as DP
import nee_cases as N
import nee_mis_cases as NM
import nee_pick_cases as NP

f32 = np.float32
KILLED_BY = {"hit_uses_E": "weighted_hits", "luminance_parens": "weighted_hits", "prob_of_slot": "alias_taken", "u1_le_q": "edge_of_q",
             "pick_first_vertex_only": "later_vertices", "uniform_wl": "shadow_weight"}
LAMP_COLOUR = (12.5, 9.3, 12.0)


@pytest.fixture(scope="module")
def box(trt, orc):
    """The Cornell box of nee_cases with the lamp recoloured; items and first rays are the scene fixture's (they do not read a colour)."""
    sc = NP.scene(trt, orc, "cornell")
    mats = [(n, k, LAMP_COLOUR if n == "light" else c, f) for n, k, c, f in sc["desc"]["materials"]]
    desc = dict(sc["desc"], materials=mats)
    ow, _ = orc.world_from_description(desc)
    table = D.table_of(orc, desc)
    pick, total = DP.build(table)
    assert len(table) == 3 and table["geometry"][0] != D.NO_GEOMETRY and (table["geometry"][1:] == D.NO_GEOMETRY).all()
    assert DP.luminance(table["color"][0]) != DP.luminance(table["color"][0], "luminance_parens")
    return dict(desc=desc, ow=ow, table=table, pick=pick, total=total, bg=sc["bg"], rays={s: sc[s]["rays"] for s in NP.SOURCES})


def run(orc, box, source="cosine", pick=None, **kw):
    if kw.get("heuristic") is not None:
        kw.setdefault("total_power", box["total"])
    return NP.pick_paths(orc, box["ow"], box["desc"], box["rays"][source], box["table"], box["pick"] if pick is None else pick,
                         background=box["bg"], **kw)


def test_every_mutant_has_a_class():
    assert set(KILLED_BY) == set(NP.MUTANTS)


def test_with_the_uniform_draw_at_every_vertex_the_restatement_is_nee_cases(trt, orc):
    """The loop written out anew is nee_path's and mis_path's: with every vertex drawn uniformly (draw's uniform=True, the step the
    first-vertex mutant takes at later vertices) the plain form is nee_cases' bytes; and nee_cases.draw is draw(uniform=True)."""
    sc = NP.scene(trt, orc, "cornell")
    want = N.reference(trt, orc, "cornell", "cosine")
    mats = N.P.material_table(orc, sc["ow"], sc["desc"])
    rays = sc["cosine"]["rays"]
    checked = 0
    for i in range(0, 324, 9):
        for s in range(NP.K):
            stream = NP.FIRST_STREAM + i * NP.K + s
            a = N.nee_path(orc, sc["ow"], mats, rays[i, s], NP.MAX_BOUNCES, sc["bg"], NP.SEED, stream, sc["nee_table"])
            assert a["color"].tobytes() == want["cols"][i, s].tobytes()
            x, nrm = rays[i, s, 0:3], rays[i, s, 3:6]
            live, walked, occ, c = N.draw(orc, sc["ow"], x, nrm, sc["nee_table"], NP.SEED, stream, 2)
            b = NP.draw(orc, sc["ow"], x, nrm, sc["nee_table"], sc["nee_pick"], NP.SEED, stream, 2, uniform=True)
            assert (live, walked, occ) == (b["live"], b["walked"], b["occ"])
            e = min(int(_u(orc, stream, 2)[0] * f32(3.0)), 2)
            assert b["e"] == e and not b["took_alias"]
            with np.errstate(all="ignore"):
                assert (sc["nee_table"]["color"][e] * b["wgt"]).astype(np.float32).tobytes() == c.tobytes()
            checked += live
    assert checked >= 50


def _u(orc, stream, word, n=2):
    rng = (C.c_uint32 * 2)()
    orc.lib.orc_rng_seed(NP.SEED, stream & 0xFFFFFFFF, word, C.byref(rng))
    return [f32(orc.lib.orc_rng_random(C.byref(rng))) for _ in range(n)]


def test_the_draw_is_direct_pick_cases_at_word_1(trt, orc, box):
    """nee_pick_cases.draw on stream word 1 about an item is direct_pick_cases.samples' sample: e, the alias, liveness, occlusion, the
    weight's bits."""
    sc = NP.scene(trt, orc, "cornell")
    items = sc["cosine"]["items"]
    only = list(range(0, 324, 5))
    want = DP.samples(orc, box["ow"], items, box["table"], box["pick"], only=only)
    lit = 0
    for i in only:
        for s in range(NP.K):
            got = NP.draw(orc, box["ow"], items[i, 0:3], items[i, 3:6], box["table"], box["pick"], NP.SEED, NP.FIRST_STREAM + i * NP.K + s, 1)
            assert (got["e"], got["took_alias"], got["live"], got["walked"], got["occ"]) == \
                (want["e"][i, s], want["took_alias"][i, s], want["live"][i, s], want["walked"][i, s], want["occ"][i, s]), (i, s)
            assert np.array([got["wgt"]], np.float32).tobytes() == want["wgt"][i, s].tobytes()
            lit += bool(got["live"] and not got["occ"])
    assert lit >= 100


def test_edge_of_q(orc, box):
    """A path whose first vertex draws on stream word 2: q[k] set to that draw's own u1 takes the alias, the next float up keeps the slot;
    `u1 <= q` keeps both."""
    right = run(orc, box)
    tried = 0
    for i, s in zip(*np.nonzero(right["lit"] > 0)):
        u0, u1 = _u(orc, NP.FIRST_STREAM + i * NP.K + s, 2)
        k = min(int(u0 * f32(3.0)), 2)
        at, above = box["pick"].copy(), box["pick"].copy()
        at["q"][k], above["q"][k] = u1, np.nextafter(u1, f32(2.0))
        at["alias"][k] = above["alias"][k] = (k + 1) % 3
        a = run(orc, box, pick=at, only=[i])
        b = run(orc, box, pick=above, only=[i])
        wrong = run(orc, box, pick=at, only=[i], mutant="u1_le_q")
        if a["hits"][i, s] < 2 or a["cols"][i, s].tobytes() == b["cols"][i, s].tobytes():
            continue                                                        # the first vertex was not this path's word-2 draw, or both ends are dark
        assert wrong["cols"][i].tobytes() == b["cols"][i].tobytes() != a["cols"][i].tobytes(), (i, s)
        assert wrong["alias_taken"][i, s] == b["alias_taken"][i, s] and a["alias_taken"][i, s] >= 1
        tried += 1
        if tried == 3:
            break
    assert tried == 3


def test_alias_taken_and_later_vertices(orc, box):
    right = run(orc, box)
    draws = right["walks"].sum()
    print("alias-taken draws", int(right["alias_taken"].sum()), "shadow walks", int(draws), "lit", int(right["lit"].sum()))
    assert right["alias_taken"].sum() >= 1500 and right["lit"].sum() >= 1500
    # the lamp's slot keeps itself: an alias is taken from a virtual emitter's slot, to another prob
    took = box["pick"]["q"] < 1
    assert took.any() and (box["pick"]["prob"][box["pick"]["alias"][took]] != box["pick"]["prob"][took]).all()
    wrong = run(orc, box, mutant="prob_of_slot")
    assert N.differing(right["cols"], wrong["cols"]) >= 100
    # later vertices: samples with two or more shadow walks drew at a later vertex too
    later = int((right["walks"] >= 2).sum())
    assert later >= 300, later
    wrong = run(orc, box, mutant="pick_first_vertex_only")
    assert N.differing(right["cols"], wrong["cols"]) >= 100
    assert wrong["alias_taken"].sum() < right["alias_taken"].sum()


@pytest.mark.parametrize("heuristic", sorted(NP.HEURISTICS))
def test_shadow_weight_and_weighted_hits(orc, box, heuristic):
    """wl is taken from the PICK weight; every weighted hit recomputes ph with the bits of the table's prob for the lamp, float(E) in the
    hit weight and another parenthesisation of the luminance are told apart, and the two weights of one light point sum to 1."""
    h = NP.HEURISTICS[heuristic]
    hits = 0
    for source in NP.SOURCES:
        right = run(orc, box, source, heuristic=h)
        plain = run(orc, box, source)
        n_w = int(right["weighted"].sum())
        hits += n_w
        assert len(right["ph"]) == n_w
        assert (right["ph"][:, 0] == box["table"]["geometry"][0]).all()
        assert (right["ph"][:, 1] == box["pick"]["prob"][:1].view(np.uint32)[0]).all()
        # the walks, hits and draws are the plain PICK query's
        for name in ("hits", "walks", "lit", "hidden", "skipped", "alias_taken", "first_hidden"):
            assert right[name].tobytes() == plain[name].tobytes(), name
        if source == "cosine":
            assert n_w >= 10 and right["lit"].sum() >= 1500
            wrong = run(orc, box, source, heuristic=h, mutant="uniform_wl")
            assert N.differing(right["cols"], wrong["cols"]) >= 100
            for mutant in ("hit_uses_E", "luminance_parens"):
                wrong = run(orc, box, source, heuristic=h, mutant=mutant)
                changed = np.nonzero((right["cols"] != wrong["cols"]).any(axis=2))
                assert len(changed[0]) >= 1 and (right["weighted"][changed] >= 1).all(), mutant
        # wl(g) + wb(g) = 1 up to the two roundings: the shadow sample of the same point has wgt = g since prob has ph's bits
        g = right["ph"][:, 2].astype(np.uint32).view(np.float32)
        with np.errstate(all="ignore"):
            qg = NP.q(g, h)
            ok = np.isfinite(qg)
            wl, wb = f32(1.0) / (f32(1.0) + qg[ok]), qg[ok] / (f32(1.0) + qg[ok])
        assert (np.abs((wl.astype(np.float64) + wb.astype(np.float64)) - 1.0) <= 2.0 ** -23).all()
    print(heuristic, "weighted hits over the three sources", hits)
    assert hits >= 30


def test_a_weighted_hits_g_is_the_shadow_samples_weight(orc, box):
    """The point of ph's bits: for the lamp, area / prob[e] in the draw and area / ph at the hit are the same f32."""
    area = box["table"]["area"][0]
    ph = (DP.luminance(box["table"]["color"][0]) * area) / box["total"]
    assert np.array([ph], np.float32).tobytes() == box["pick"]["prob"][:1].tobytes()
    assert (area / ph).tobytes() == (area / box["pick"]["prob"][0]).tobytes()


def test_with_virtual_emitters_only_mis_pick_is_pick(trt, orc):
    """random_spheres holds no light: its table is the two virtual emitters, wl = 1 and no hit is weighted (tests/test_gpu_nee_mis.py's
    identity 3)."""
    sc = NP.scene(trt, orc, "random_spheres")
    assert len(sc["nee_table"]) == 2 and (sc["nee_table"]["geometry"] == D.NO_GEOMETRY).all()
    for source in NP.SOURCES:
        plain = NP.reference(trt, orc, "random_spheres", source)
        assert plain["lit"].sum() >= 100 and plain["alias_taken"].sum() >= 100
        for h in sorted(NP.HEURISTICS.values()):
            got = NP.reference(trt, orc, "random_spheres", source, heuristic=h)
            assert got["cols"].tobytes() == plain["cols"].tobytes() and got["weighted"].sum() == 0
            assert got["n_rays"] == plain["n_rays"]


def test_with_one_bounce_no_vertex_draws(trt, orc):
    sc = NP.scene(trt, orc, "cornell")
    for source in NP.SOURCES:
        got = NP.pick_paths(orc, sc["ow"], sc["desc"], sc[source]["rays"], sc["nee_table"], sc["nee_pick"], max_bounces=1, background=sc["bg"],
                            only=range(0, 324, 4))
        want = N.nee_paths(orc, sc["ow"], sc["desc"], sc[source]["rays"], sc["nee_table"], max_bounces=1, background=sc["bg"], only=range(0, 324, 4))
        assert got["cols"].tobytes() == want["cols"].tobytes() and got["walks"].sum() == 0 and got["alias_taken"].sum() == 0


def _pooled_z(a, ka, g, kg):
    """tests/test_direct_mis_cases.py's pooling: z = (mean_a - mean_g) / sqrt(sum_i(var_a,i / K_a + var_g,i / K_g)) * n."""
    return (a.mean() - g.mean()) / np.sqrt((a.var(axis=1, ddof=1) / ka + g.var(axis=1, ddof=1) / kg).sum()) * len(a)


# Measured with the fixtures below (tests/README_nee_pick.md): the uniform choice's mean per-surfel sample variance (restated trt_nee) over
# the PICK query's (restated trt_nee_pick), same surfels, same streams for the paths, same K.  The test asserts half of it.
MEASURED_GAIN = 5.60


def test_unbiased_and_the_point_of_the_feature(trt, orc):
    """The many-light room (the lamp at y = 99 and 60 dim sphere lights), 40 floor surfels, cosine source, B = 4, source_is_diffuse = 1:
    the indirect half of a bake, where the vertex draws are all the light there is.  The restated trt_nee_pick and trt_nee_mis_pick (both
    heuristics) at K = 512 against the restated trt_nee_mis (BALANCE, uniform choice: bounded samples) at K = 2 x 2048 on streams of its
    own: pooled |z| <= 4, the project's bound.  First the reference alone: its two halves, disjoint stream sets, against each other under
    the same bound.  Then the point: at the same K = 512 the PICK query's mean per-surfel sample variance against the uniform choice's."""
    k, kh, B = 512, 2048, 4
    desc, ow, items, table = DP.many_light_room(trt, orc)
    pick, total = DP.build(table)
    n = len(items)
    common = dict(max_bounces=B, source_is_diffuse=True)
    own = NP.FIRST_STREAM + n * k + 7
    halves = []
    for first in (own, own + n * kh + 11):
        rays = NP.first_rays(orc, items, kh, first_stream=first)
        ref = NM.mis_paths(orc, ow, desc, rays, table, first_stream=first, heuristic=NM.BALANCE, **common)
        halves.append(ref["cols"][:, :, 0].astype(np.float64))
    z_ref = _pooled_z(halves[0], kh, halves[1], kh)
    print("reference alone: means", halves[0].mean(), halves[1].mean(), "z", z_ref)
    assert abs(z_ref) <= 4.0, z_ref
    g, kg = np.concatenate(halves, axis=1), 2 * kh
    rays = NP.first_rays(orc, items, k)
    runs = {"pick": NP.pick_paths(orc, ow, desc, rays, table, pick, **common)}
    for name, h in sorted(NP.HEURISTICS.items()):
        runs["mis_pick, " + name] = NP.pick_paths(orc, ow, desc, rays, table, pick, total_power=total, heuristic=h, **common)
    assert runs["pick"]["alias_taken"].sum() >= 10000 and runs["mis_pick, balance"]["weighted"].sum() >= 100
    uniform = N.nee_paths(orc, ow, desc, rays, table, **common)["cols"][:, :, 0].astype(np.float64)
    var_uniform = uniform.var(axis=1, ddof=1).mean()
    out = {}
    for what, r in runs.items():
        a = r["cols"][:, :, 0].astype(np.float64)
        out[what] = (a.mean(), a.var(axis=1, ddof=1).mean(), _pooled_z(a, k, g, kg))
        print(what, "mean", out[what][0], "variance", out[what][1], "| uniform mis K=%d mean" % kg, g.mean(), "| z", out[what][2])
    gain = var_uniform / out["pick"][1]
    print("uniform K=512 mean", uniform.mean(), "variance", var_uniform, "| gain of pick", gain, "| of mis_pick balance",
          var_uniform / out["mis_pick, balance"][1])
    for what, (mean_a, _, z) in out.items():
        assert mean_a > 0.01 and g.mean() > 0.01
        assert abs(z) <= 4.0, (what, mean_a, g.mean(), z)
    assert out["pick"][1] < var_uniform                                     # never less than "lower than uniform"
    assert MEASURED_GAIN is not None and gain >= MEASURED_GAIN / 2.0, (gain, MEASURED_GAIN)
