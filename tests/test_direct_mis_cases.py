"""The reference of the weighted direct-light query tests (tests/direct_mis_cases.py) is pinned to direct_cases' restatement, keeps the
contract's identities, is not vacuous, loses the tail that trt_direct has beside a lamp, and is unbiased against the reference's own light
transport: conditions on the oracle's answers alone, no GPU.  The measured figures are in tests/README_direct_mis.md."""
import numpy as np
import pytest

import direct_cases as D
import direct_mis_cases as M
import gather_cases as GC
import passes_cases as P

# lobe light hits, of which counted in full, items with one, shadow terms with a weight, virtual shadow terms (tests/README_direct_mis.md)
COUNTS = {"cornell": (4, 0, 4, 675, 1195), "prims33": (225, 62, 105, 456, 224), "prims600": (82, 41, 56, 11, 5),
          "random_spheres_lit": (77, 13, 51, 247, 39), "grid3000_lit": (126, 38, 73, 86, 10)}


def counts_of(sc, ref):
    virtual = sc["table"]["geometry"][ref["e"]] == D.NO_GEOMETRY
    return (int(ref["has_b"].sum()), int(ref["full"].sum()), int(ref["has_b"].any(axis=1).sum()), int((ref["has_l"] & ~virtual).sum()),
            int((ref["has_l"] & virtual).sum()))


@pytest.mark.parametrize("name", M.SCENES)
def test_with_the_weights_forced_off_the_restatement_is_direct_cases(trt, orc, name):
    """plain=True: wl = 1 and no lobe term - trt_direct's contract byte for byte, sample by sample and folded."""
    sc = M.scene(trt, orc, name)
    want = D.reference(orc, sc["ow"], sc["items"], sc["table"])
    got = M.reference(trt, orc, name, plain=True)
    assert got["c"].tobytes() == want["c"].tobytes() and got["S"].tobytes() == want["S"].tobytes() and got["M"].tobytes() == want["M"].tobytes()
    assert got["n_walks"] == want["n_walks"] and not got["has_b"].any() and (got["wl"] == 1).all()


@pytest.mark.parametrize("heuristic", sorted(M.HEURISTICS))
def test_identity_1_with_virtual_emitters_only_the_result_is_direct_cases(trt, orc, heuristic):
    """The stock random_spheres scene holds no TRT_LIGHT geometry and its table is the two virtual emitters: wl = 1 and no lobe ray
    finds a light, so radiance and moment2 are trt_direct's bytes."""
    import walk_ray_cases as W
    desc = W.scene(trt, "random_spheres")
    ow, _ = orc.world_from_description(desc)
    items, _ = GC.items_of(orc, ow, desc)
    table = D.table_of(orc, desc)
    assert len(table) == 2 and (table["geometry"] == D.NO_GEOMETRY).all()
    want = D.reference(orc, ow, items, table)
    assert int((want["live"] & ~want["occ"]).sum()) >= 300
    got = M.finish(M.samples(orc, ow, desc, items, table, heuristic=M.HEURISTICS[heuristic]), M.K)
    assert got["S"].tobytes() == want["S"].tobytes() and got["M"].tobytes() == want["M"].tobytes()
    assert not got["has_b"].any() and (got["geo"] >= 0).sum() >= 300       # the lobe rays do hit the scene


@pytest.mark.parametrize("name", M.SCENES)
def test_identities_2_and_3_the_counters(trt, orc, name):
    """samples are trt_direct's; rays are trt_direct's walks plus the world.hit calls of a gather at max_bounces = 1 over the same items
    and K (one per sample, cpu.rs:48)."""
    sc = M.scene(trt, orc, name)
    want = D.reference(orc, sc["ow"], sc["items"], sc["table"])
    _, _, gather_hits = GC.oracle_gather(orc, sc["ow"], sc["items"], "cosine", M.K, 1, (0.0, 0.0, 0.0), M.SEED, M.FIRST_STREAM)
    for h in (M.BALANCE, M.POWER):
        got = M.reference(trt, orc, name, heuristic=h)
        assert got["n_samples"] == M.N_ITEMS * M.K == want["live"].size
        assert (got["walked"] == want["walked"]).all()
        assert got["n_rays"] == want["n_walks"] + gather_hits, (name, h, got["n_rays"], want["n_walks"], gather_hits)


@pytest.mark.parametrize("name", M.SCENES)
def test_the_reference_is_not_vacuous(trt, orc, name):
    """The counted terms of every fixture, and on every kernel shape's fixture a lobe hit with wb < 1 and a shadow term with wl < 1."""
    sc = M.scene(trt, orc, name)
    ref = M.reference(trt, orc, name)
    got = counts_of(sc, ref)
    print(name, "lobe light hits %d, in full %d, items %d, weighted shadow terms %d, virtual %d" % got, "| both terms in one sample",
          int((ref["has_l"] & ref["has_b"]).sum()), "| items that differ from trt_direct's", M.differing(ref["S"], M.reference(trt, orc, name, plain=True)["S"]))
    assert got == COUNTS[name], (name, got)
    assert (ref["has_b"] & (ref["wb"] < 1)).any() and (ref["has_l"] & (ref["wl"] < 1)).any()
    assert (ref["has_l"] & ref["has_b"]).any()                              # T_l + T_b is folded as one sample somewhere
    assert (ref["full"] <= ref["has_b"]).all() and (ref["wb"][ref["full"]] == 1).all()
    power = M.reference(trt, orc, name, heuristic=M.POWER)
    assert M.differing(power["S"], ref["S"]) >= 1


def test_a_quad_light_and_a_sphere_light_are_both_weighted(trt, orc):
    kinds = set()
    for name in ("cornell", "prims33"):
        sc, ref = M.scene(trt, orc, name), M.reference(trt, orc, name)
        weighted = ref["has_b"] & ~ref["full"]
        kinds |= set(sc["desc"]["geometries"][int(g)][0] for g in ref["geo"][weighted])
    assert kinds == {"quad", "sphere"}


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_of_the_restatement_changes_the_answer(trt, orc, mutant):
    """Each on a named scene: cornell (one quad lamp, two virtual emitters) for the weights, prims33 (several lights of different areas,
    non-unit axes) for the area, the hit's t and the cosine."""
    where = {"first_area": "prims33", "t_once": "prims33", "csh_hit_normal": "prims33", "no_wb": "prims33"}.get(mutant, "cornell")
    right = M.reference(trt, orc, where)
    wrong = M.reference(trt, orc, where, mutant=mutant)
    changed = M.differing(wrong["S"], right["S"]) if mutant != "two_samples" else M.differing(wrong["M"], right["M"])
    print(mutant, "on", where, "changes", changed, "items")
    assert changed >= 1, (mutant, where)


def _lowered_sets(trt, orc):
    desc, ow, items, table = M.lowered_cornell(trt, orc)
    return desc, ow, table, {"ceiling": items[:20], "floor": M.floor_texels(trt, desc)}


def test_the_tail_is_gone_beside_the_lamp(trt, orc):
    """The 20 ceiling surfels one unit above the lowered lamp, K = 512, the scene's own table, red channel.  A BALANCE sample is at most
    2 x the largest colour channel = 30 (up to rounding: 1 + 1e-6): each of its two terms is at most the colour.  trt_direct's
    restatement on the same streams has a sample above that bound, and its mean per-surfel sample variance is more than ten times
    BALANCE's (tenfold: trt_direct's figure is carried by a few samples).  The streams are fixed: deterministic."""
    k = 512
    desc, ow, table, sets = _lowered_sets(trt, orc)
    items = sets["ceiling"]
    assert table["color"].max() == 15.0 and len(table) == 1
    base = D.samples(orc, ow, items, table, k=k)
    plain = base["c"].astype(np.float64)
    mis = M.samples(orc, ow, desc, items, table, k=k, base=base)
    c = mis["c"].astype(np.float64)
    bound = 30.0 * (1 + 1e-6)
    var_mis, var_plain = c[:, :, 0].var(axis=1, ddof=1).mean(), plain[:, :, 0].var(axis=1, ddof=1).mean()
    print("trt_direct_mis mean", c[:, :, 0].mean(), "variance", var_mis, "largest", c.max(), "| trt_direct mean", plain[:, :, 0].mean(), "variance",
          var_plain, "largest", plain.max(), "| share of lobe rays on the lamp", mis["has_b"].mean())
    assert plain.max() > bound, plain.max()
    assert c.max() <= bound, c.max()
    assert var_mis < var_plain / 10.0, (var_mis, var_plain)
    assert 0.2 < mis["has_b"].mean() < 0.4


def _pooled_z(a, ka, g, kg):
    """tests/test_nee_cases.py's pooling: z = (mean_a - mean_g) / sqrt(sum_i(var_a,i / K_a + var_g,i / K_g)) * n."""
    return (a.mean() - g.mean()) / np.sqrt((a.var(axis=1, ddof=1) / ka + g.var(axis=1, ddof=1) / kg).sum()) * len(a)


def test_the_contract_is_unbiased_against_the_references_transport(trt, orc):
    """The lowered box: the 20 ceiling surfels and 20 floor texels, both heuristics, K = 512, against the oracle's gather at
    max_bounces = 1 (black background) on streams of its own, K = 4096; pooled |z| <= 4, the project's bound."""
    k, kg = 512, 4096
    desc, ow, table, sets = _lowered_sets(trt, orc)
    out = {}
    for which, items in sets.items():
        own = M.FIRST_STREAM + len(items) * k + 7
        _, g, _ = GC.oracle_gather(orc, ow, items, "cosine", kg, 1, (0.0, 0.0, 0.0), M.SEED, own)
        g = g[:, :, 0].astype(np.float64)
        base = D.samples(orc, ow, items, table, k=k)
        for name, h in sorted(M.HEURISTICS.items()):
            a = M.samples(orc, ow, desc, items, table, heuristic=h, k=k, base=base)["c"][:, :, 0].astype(np.float64)
            out[which + ", " + name] = (a.mean(), g.mean(), a.var(axis=1, ddof=1).mean(), g.var(axis=1, ddof=1).mean(), _pooled_z(a, k, g, kg))
    for what, (mean_a, mean_g, var_a, var_g, z) in out.items():
        print(what, "mean", mean_a, "variance", var_a, "| gather mean", mean_g, "variance", var_g, "| z", z)
    for what, (mean_a, mean_g, _, _, z) in out.items():
        assert mean_a > 0.05 and mean_g > 0.05
        assert abs(z) <= 4.0, (what, mean_a, mean_g, z)
