"""The reference of the next-event query tests (tests/nee_cases.py) is pinned to the oracle, is not vacuous, and the contract it restates is
unbiased against the reference's own light transport: conditions on the oracle's answers alone, no GPU.  The measured figures are in
tests/README_nee.md."""
import numpy as np
import pytest

import direct_cases as D
import gather_cases as GC
import nee_cases as N
import passes_cases as P
import radiance_cases as R

# scene -> least (samples with an unoccluded next-event term, samples with a hidden light hit or None, samples whose next event
# remain == 0 ruled out, items that differ from the plain gather), cosine source: each at no more than half the measured value
# (tests/README_nee.md).  Hidden hits need a scene with lights: cornell and prims33.
BOUNDS = {"cornell": (500, 7, 300, 130), "prims33": (19, 8, 7, 19), "random_spheres": (300, None, 100, 110), "grid3000": (220, None, 150, 80)}


def _plain(trt, orc, name, source):
    return P.reference(trt, orc, name)[source]


@pytest.mark.parametrize("source", N.SOURCES)
@pytest.mark.parametrize("name", ("cornell", "prims33"))
def test_without_next_event_and_hiding_the_restatement_is_the_oracles_loop(trt, orc, name, source):
    """Byte for byte orc.sample_batch's colours (through radiance_cases.oracle_samples, one sample per drawn ray), and its world.hit calls."""
    sc = N.scene(trt, orc, name)
    rays = sc[source]["rays"]
    got = N.nee_paths(orc, sc["ow"], sc["desc"], rays, sc["nee_table"], background=sc["bg"], next_event=False, hide=False)
    flat = np.ascontiguousarray(rays.reshape(-1, 6))
    want, hits = R.oracle_samples(orc, sc["ow"], flat, 1, N.MAX_BOUNCES, sc["bg"], N.SEED, N.FIRST_STREAM)
    N.assert_same_bits(got["cols"].reshape(-1, 3), want.reshape(-1, 3), (name, source))
    assert int(got["hits"].sum()) == hits and got["walks"].sum() == 0 and got["lit"].sum() == 0 and got["hidden"].sum() == 0
    # and passes_cases.oracle_path's, which the passes tests pin the same way
    N.assert_same_bits(got["cols"].reshape(-1, 3), sc[source]["cols"].reshape(-1, 3), (name, source, "passes_cases"))


def test_the_draw_is_direct_cases_draw_at_word_1(trt, orc):
    sc = N.scene(trt, orc, "prims33")
    items, table = sc["cosine"]["items"], sc["nee_table"]
    only = list(range(0, N.N_ITEMS, 7)) + list(range(N.N_ITEMS - 4, N.N_ITEMS))
    want = D.samples(orc, sc["ow"], items, table, only=only)
    for i in only:
        for s in range(N.K):
            live, walked, occ, c = N.draw(orc, sc["ow"], items[i, 0:3], items[i, 3:6], table, N.SEED, N.FIRST_STREAM + i * N.K + s, 1)
            assert (live, walked, occ) == (want["live"][i, s], want["walked"][i, s], want["occ"][i, s]), (i, s)
            if live and not occ:
                N.assert_same_bits(c.reshape(1, 3), want["c"][i, s].reshape(1, 3), (i, s))


@pytest.mark.parametrize("source", N.SOURCES)
def test_with_one_bounce_the_result_is_the_plain_querys(trt, orc, source):
    """B == 1: no next event, nothing hidden (source_is_diffuse == 0)."""
    for name in ("cornell", "prims33"):
        sc = N.scene(trt, orc, name)
        rays = sc[source]["rays"]
        got = N.nee_paths(orc, sc["ow"], sc["desc"], rays, sc["nee_table"], max_bounces=1, background=sc["bg"])
        want, _, _, hits = P.oracle_paths(orc, sc["ow"], sc["desc"], rays, 1, sc["bg"], N.SEED, N.FIRST_STREAM)
        N.assert_same_bits(got["cols"].reshape(-1, 3), want.reshape(-1, 3), (name, source))
        assert got["walks"].sum() == 0 and got["hidden"].sum() == 0 and int(got["hits"].sum()) == hits
        assert got["skipped"].sum() > 0                                     # Lambertian vertices were there: remain == 0 ruled them out


def test_without_a_lambertian_material_the_result_is_the_gathers(trt, orc):
    """prims33 with every Lambertian turned into a metal of fuzz 1: any B."""
    sc = N.scene(trt, orc, "prims33")
    desc = sc["desc"]
    mats = [(n, 1 if k == GC.ORC_LAMBERTIAN else k, a, 1.0 if k == GC.ORC_LAMBERTIAN else p) for n, k, a, p in desc["materials"]]
    assert any(k == GC.ORC_LAMBERTIAN for _, k, _, _ in desc["materials"])
    changed = dict(desc, materials=mats)
    ow, _ = orc.world_from_description(changed)
    rays = sc["cosine"]["rays"]
    got = N.nee_paths(orc, ow, changed, rays, sc["nee_table"], background=sc["bg"])
    want, _, _, hits = P.oracle_paths(orc, ow, changed, rays, N.MAX_BOUNCES, sc["bg"], N.SEED, N.FIRST_STREAM)
    N.assert_same_bits(got["cols"].reshape(-1, 3), want.reshape(-1, 3), "no lambertian")
    assert got["walks"].sum() == 0 and got["hidden"].sum() == 0 and got["skipped"].sum() == 0 and int(got["hits"].sum()) == hits


@pytest.mark.parametrize("name", list(BOUNDS))
def test_the_reference_is_not_vacuous(trt, orc, name):
    ref = N.reference(trt, orc, name, "cosine")
    plain = _plain(trt, orc, name, "cosine")
    lit = int((ref["lit"] > 0).sum())
    hidden = int((ref["hidden"] > 0).sum())
    skipped = int((ref["skipped"] > 0).sum())
    differ = N.differing(ref["S"], R.fold(plain["cols"], N.K)[0])
    print(name, "lit samples", lit, "hidden", hidden, "skipped", skipped, "items that differ from the gather", differ, "hits", int(ref["hits"].sum()),
          "walks", int(ref["walks"].sum()))
    lit_min, hidden_min, skipped_min, differ_min = BOUNDS[name]
    assert lit >= lit_min > 0, (name, lit)
    if hidden_min is not None:
        assert hidden >= hidden_min > 0, (name, hidden)
    else:
        assert hidden == 0
    assert skipped >= skipped_min > 0, (name, skipped)
    assert differ >= differ_min > 0, (name, differ)
    assert int(ref["hits"].sum()) == plain["n_rays"]                        # the path is the gather's: the same world.hit calls
    assert 0 < ref["walks"].sum() and (ref["lit"] <= ref["walks"] + (ref["lit"] > 0)).all()


# (scene, mutant) -> the bounce budget at which the mutant is asserted where the fixtures' B = 5 cannot show it.  Next event at the last
# vertex needs a path whose LAST vertex is Lambertian and sees an emitter.  prims33 is dense: at B = 5 its 972 items x 8 samples hold 20
# such vertices over the three sources, the mutant walks 13 shadow rays from them and every one is occluded (measured; printed below), so
# no item changes.  At B = 2 the last vertex is the second one, in the open, and the mutant changes dozens of items.
SHORT_BUDGET = {("prims33", "nee_at_last"): 2}


@pytest.mark.parametrize("mutant", N.MUTANTS)
def test_every_mutant_of_the_restatement_changes_the_answer(trt, orc, mutant):
    """On cornell and on prims33, which holds both metals and lights (the mutant that lets a metal hit keep after_diffuse can show only
    there: the box holds no metal).  Counted over the three sources of a scene, at the fixtures' B = 5 but for SHORT_BUDGET."""
    for name in ("cornell", "prims33"):
        if mutant == "metal_keeps_diffuse" and name == "cornell":
            continue
        sc = N.scene(trt, orc, name)
        changed, short = {}, {}
        for source in N.SOURCES:
            kw = dict(background=sc["bg"])
            ref = N.reference(trt, orc, name, source)
            wrong = N.nee_paths(orc, sc["ow"], sc["desc"], sc[source]["rays"], sc["nee_table"], mutant=mutant, **kw)
            changed[source] = N.differing(wrong["cols"], ref["cols"])
            if (name, mutant) in SHORT_BUDGET:
                kw["max_bounces"] = SHORT_BUDGET[name, mutant]
                right = N.nee_paths(orc, sc["ow"], sc["desc"], sc[source]["rays"], sc["nee_table"], **kw)
                wrong = N.nee_paths(orc, sc["ow"], sc["desc"], sc[source]["rays"], sc["nee_table"], mutant=mutant, **kw)
                short[source] = N.differing(wrong["cols"], right["cols"])
        print(name, mutant, "changes", changed, "at the short budget", short)
        if (name, mutant) in SHORT_BUDGET:
            assert sum(short.values()) >= 1, (name, mutant, short)
        else:
            assert sum(changed.values()) >= 1, (name, mutant, changed)


def test_prims33_holds_metals_and_lights(trt, orc):
    kinds = {k for _, k, _, _ in N.scene(trt, orc, "prims33")["desc"]["materials"]}
    assert N.ORC_METAL in kinds and N.ORC_LIGHT in kinds and N.ORC_LAMBERTIAN in kinds


def test_the_contract_is_unbiased_against_the_references_transport(trt, orc):
    """Cornell with the lamp lowered to y = 99, 40 unit surfels, cosine source, B = 4.  Pooled as tests/test_direct_cases.py pools:
    z = (mean_a - mean_g) / sqrt(sum_i(var_a,i / K_a + var_g,i / K_g)) * 40, |z| <= 4, for a = the next-event restatement and for
    a = direct + next event with source_is_diffuse = 1, both against orc.sample_batch over the same first-ray rule."""
    desc, ow, items, table = N.lowered_cornell(trt, orc)
    B, KN, KG = 4, 512, 8192
    black = (0.0, 0.0, 0.0)
    rays = GC.first_rays(orc, items, "cosine", KN, N.SPREAD, N.SEED, N.FIRST_STREAM)
    nee = N.nee_paths(orc, ow, desc, rays, table, max_bounces=B, background=black)["cols"][:, :, 0].astype(np.float64)
    ind = N.nee_paths(orc, ow, desc, rays, table, max_bounces=B, background=black, source_is_diffuse=True)["cols"][:, :, 0].astype(np.float64)
    direct = D.samples(orc, ow, items, table, k=KN)["c"][:, :, 0].astype(np.float64)
    _, g, _ = GC.oracle_gather(orc, ow, items, "cosine", KG, B, black, N.SEED, N.FIRST_STREAM)
    g = g[:, :, 0].astype(np.float64)
    mean_g = g.mean()
    var_g = g.var(axis=1, ddof=1) / KG
    out = {}
    for what, a in (("nee", nee), ("direct + nee(source_is_diffuse)", direct + ind)):
        mean_a = a.mean()
        z = (mean_a - mean_g) / np.sqrt((a.var(axis=1, ddof=1) / KN + var_g).sum()) * len(items)
        ratio_a = np.sqrt(a.var(axis=1, ddof=1)).mean() / mean_a
        out[what] = (mean_a, z)
        print(what, "mean", mean_a, "gather mean", mean_g, "z", z, "sd/mean", ratio_a, "gather", np.sqrt(g.var(axis=1, ddof=1)).mean() / mean_g)
    for what, (mean_a, z) in out.items():
        assert mean_a > 0.05 and mean_g > 0.05
        assert abs(z) <= 4.0, (what, mean_a, mean_g, z)
