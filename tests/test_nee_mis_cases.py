"""The reference of the weighted next-event query tests (tests/nee_mis_cases.py) is pinned to nee_cases' restatement, keeps the contract's
identities, is not vacuous, loses the tail that trt_nee has beside a lamp, and is unbiased against the reference's own light transport:
conditions on the oracle's answers alone, no GPU.  The measured figures are in tests/README_nee_mis.md."""
import numpy as np
import pytest

import direct_cases as D
import gather_cases as GC
import nee_cases as N
import nee_mis_cases as M
import passes_cases as P

# scenes whose fixtures hold hidden light hits (tests/test_nee_cases.py BOUNDS)
LIT_SCENES = ("cornell", "prims33")


@pytest.mark.parametrize("source", M.SOURCES)
@pytest.mark.parametrize("name", LIT_SCENES)
def test_with_the_weights_forced_off_the_restatement_is_nee_cases(trt, orc, name, source):
    """wb = 0, wl = 1: trt_nee's contract byte for byte, and every count nee_cases keeps."""
    want = N.reference(trt, orc, name, source)
    got = M.reference(trt, orc, name, source, plain=True)
    M.assert_same_bits(got["cols"].reshape(-1, 3), want["cols"].reshape(-1, 3), (name, source))
    for what in N.COUNTS:
        assert (got[what] == want[what]).all(), (name, source, what)
    assert got["weighted"].sum() == 0


@pytest.mark.parametrize("heuristic", sorted(M.HEURISTICS))
@pytest.mark.parametrize("source", M.SOURCES)
def test_identity_1_with_one_bounce_the_result_is_the_plain_querys(trt, orc, source, heuristic):
    for name in LIT_SCENES:
        sc = M.scene(trt, orc, name)
        rays = sc[source]["rays"]
        got = M.mis_paths(orc, sc["ow"], sc["desc"], rays, sc["nee_table"], max_bounces=1, background=sc["bg"], heuristic=M.HEURISTICS[heuristic])
        want, _, _, hits = P.oracle_paths(orc, sc["ow"], sc["desc"], rays, 1, sc["bg"], M.SEED, M.FIRST_STREAM)
        M.assert_same_bits(got["cols"].reshape(-1, 3), want.reshape(-1, 3), (name, source))
        assert got["walks"].sum() == 0 and got["hidden"].sum() == 0 and got["weighted"].sum() == 0 and int(got["hits"].sum()) == hits


def test_identity_2_without_a_lambertian_material_the_result_is_the_gathers(trt, orc):
    """prims33 with every Lambertian turned into a metal of fuzz 1: any B, both heuristics."""
    sc = M.scene(trt, orc, "prims33")
    desc = sc["desc"]
    mats = [(n, 1 if k == GC.ORC_LAMBERTIAN else k, a, 1.0 if k == GC.ORC_LAMBERTIAN else p) for n, k, a, p in desc["materials"]]
    changed = dict(desc, materials=mats)
    ow, _ = orc.world_from_description(changed)
    rays = sc["cosine"]["rays"]
    want, _, _, hits = P.oracle_paths(orc, ow, changed, rays, M.MAX_BOUNCES, sc["bg"], M.SEED, M.FIRST_STREAM)
    for h in (M.BALANCE, M.POWER):
        got = M.mis_paths(orc, ow, changed, rays, sc["nee_table"], background=sc["bg"], heuristic=h)
        M.assert_same_bits(got["cols"].reshape(-1, 3), want.reshape(-1, 3), "no lambertian")
        assert got["walks"].sum() == 0 and got["weighted"].sum() == 0 and int(got["hits"].sum()) == hits


def test_identity_3_with_virtual_emitters_only_the_result_is_nee_cases(trt, orc):
    """random_spheres has no TRT_LIGHT geometry; its table is the two virtual emitters: wl = 1, nothing to weight."""
    sc = M.scene(trt, orc, "random_spheres")
    table = sc["nee_table"]
    assert len(table) == 2 and (table["geometry"] == D.NO_GEOMETRY).all()
    want = N.reference(trt, orc, "random_spheres", "cosine")
    assert int((want["lit"] > 0).sum()) >= 300
    for h in (M.BALANCE, M.POWER):
        got = M.reference(trt, orc, "random_spheres", "cosine", heuristic=h)
        M.assert_same_bits(got["cols"].reshape(-1, 3), want["cols"].reshape(-1, 3), h)
        assert got["weighted"].sum() == 0 and got["hidden"].sum() == 0


@pytest.mark.parametrize("source", M.SOURCES)
@pytest.mark.parametrize("name", LIT_SCENES)
def test_identity_4_the_walks_and_hits_are_nee_cases(trt, orc, name, source):
    want = N.reference(trt, orc, name, source)
    for h in (M.BALANCE, M.POWER):
        got = M.reference(trt, orc, name, source, heuristic=h)
        assert (got["hits"] == want["hits"]).all() and (got["walks"] == want["walks"]).all(), (name, source, h)
        assert got["n_rays"] == want["n_rays"] and got["n_samples"] == want["n_samples"]


def sphere_lamp_room(trt, orc):
    """A closed room of grey Lambertian quads with a sphere lamp in its middle, and 16 floor surfels: the cosine source reaches the lamp
    after a diffuse scatter off a wall."""
    mats = [("grey", N.ORC_LAMBERTIAN, (0.7, 0.7, 0.7), 0.0), ("lamp", N.ORC_LIGHT, (6.0, 5.0, 4.0), 0.0)]
    s = 10.0
    geos = [("quad", (0.0, 0.0, 0.0), (s, 0.0, 0.0), (0.0, 0.0, s), "grey"), ("quad", (0.0, s, 0.0), (s, 0.0, 0.0), (0.0, 0.0, s), "grey"),
            ("quad", (0.0, 0.0, 0.0), (0.0, s, 0.0), (0.0, 0.0, s), "grey"), ("quad", (s, 0.0, 0.0), (0.0, s, 0.0), (0.0, 0.0, s), "grey"),
            ("quad", (0.0, 0.0, 0.0), (s, 0.0, 0.0), (0.0, s, 0.0), "grey"), ("quad", (0.0, 0.0, s), (s, 0.0, 0.0), (0.0, s, 0.0), "grey"),
            ("sphere", (5.0, 5.0, 5.0), 1.5, "lamp")]
    base = M.scene(trt, orc, "cornell")["desc"]
    desc = dict(base, materials=mats, geometries=geos)
    ow, _ = orc.world_from_description(desc)
    items = np.array([[1.0 + 2.5 * (i % 4), 0.0, 1.0 + 2.5 * (i // 4), 0.0, 1.0, 0.0] for i in range(16)], np.float32)
    return desc, ow, items, D.emitters_of(orc, desc)


def test_the_reference_is_not_vacuous(trt, orc):
    """weighted >= 1 on every fixture scene with hidden hits; a weighted hit on a quad light and on a sphere light; the table of the
    fixtures makes the wl = 1 rule run beside the weighted one."""
    kinds = set()
    for name in LIT_SCENES:
        ref = M.reference(trt, orc, name, "cosine")
        plain = N.reference(trt, orc, name, "cosine")
        weighted = int(ref["weighted"].sum())
        differ = M.differing(ref["S"], plain["S"])
        print(name, "weighted hits", weighted, "first_hidden", int(ref["first_hidden"].sum()), "hidden", int(ref["hidden"].sum()), "lit samples",
              int((ref["lit"] > 0).sum()), "items that differ from trt_nee's", differ)
        assert weighted >= 1 and differ >= 1, (name, weighted, differ)
        assert (ref["weighted"] + ref["first_hidden"] == ref["hidden"]).all()
        table = M.scene(trt, orc, name)["nee_table"]
        lights = table[table["geometry"] != D.NO_GEOMETRY]
        kinds |= set(int(k) for k in lights["kind"])
        assert (table["geometry"] == D.NO_GEOMETRY).sum() == 2
    desc, ow, items, table = sphere_lamp_room(trt, orc)
    assert len(table) == 1 and table["kind"][0] == 0
    rays = GC.first_rays(orc, items, "cosine", M.K, M.SPREAD, M.SEED, M.FIRST_STREAM)
    room = M.mis_paths(orc, ow, desc, rays, table)
    print("sphere lamp room: weighted hits", int(room["weighted"].sum()), "lit", int(room["lit"].sum()))
    assert room["weighted"].sum() >= 1                                      # a sphere light reached after a diffuse scatter
    cornell = M.scene(trt, orc, "cornell")["nee_table"]
    assert cornell["kind"][0] == 1 and cornell["geometry"][0] != D.NO_GEOMETRY                             # and the box's lamp is a quad


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_of_the_restatement_changes_the_answer(trt, orc, mutant):
    """Each on a named scene: cornell (one quad lamp, two virtual emitters) for the weights themselves, prims33 (several lights of
    different areas) for the area, the sphere lamp's room with source_is_diffuse for the first hit."""
    where = {"first_area": "prims33", "first_hit_weighted": "room"}.get(mutant, "cornell")
    if where == "room":
        desc, ow, items, table = sphere_lamp_room(trt, orc)
        rays = GC.first_rays(orc, items, "cosine", M.K, M.SPREAD, M.SEED, M.FIRST_STREAM)
        right = M.mis_paths(orc, ow, desc, rays, table, source_is_diffuse=True)
        wrong = M.mis_paths(orc, ow, desc, rays, table, source_is_diffuse=True, mutant=mutant)
        assert right["first_hidden"].sum() >= 1
        changed = M.differing(wrong["cols"], right["cols"])
    else:
        sc = M.scene(trt, orc, where)
        changed = 0
        for source in M.SOURCES:
            right = M.reference(trt, orc, where, source)
            wrong = M.mis_paths(orc, sc["ow"], sc["desc"], sc[source]["rays"], sc["nee_table"], background=sc["bg"], mutant=mutant)
            changed += M.differing(wrong["cols"], right["cols"])
    print(mutant, "on", where, "changes", changed, "items")
    assert changed >= 1, (mutant, where)


def _lowered(trt, orc, k, first_stream=M.FIRST_STREAM):
    desc, ow, items, table = M.lowered_cornell(trt, orc)
    rays = GC.first_rays(orc, items, "cosine", k, M.SPREAD, M.SEED, first_stream)
    return desc, ow, items, table, rays


def test_the_tail_is_gone_on_the_lowered_cornell_box(trt, orc):
    """40 floor surfels, cosine source, B = 4, source_is_diffuse = 1, K = 2048, the scene's own table, BALANCE.  Every sample is within
    the derived bound B x the largest colour channel = 4 x 15 (up to rounding: 1 + 1e-6); trt_nee's restatement on the same streams has
    a sample above it (measured: 837.8); the mean per-texel sample variance is below a tenth of trt_nee's (measured: 0.0902 against
    10.88 - the tenfold margin because trt_nee's figure is carried by a few samples).  The streams are fixed: deterministic."""
    B, k = 4, 2048
    desc, ow, items, table, rays = _lowered(trt, orc, k)
    assert table["color"].max() == 15.0
    kw = dict(max_bounces=B, background=(0.0, 0.0, 0.0), source_is_diffuse=True)
    mis = M.mis_paths(orc, ow, desc, rays, table, heuristic=M.BALANCE, **kw)["cols"].astype(np.float64)
    nee = N.nee_paths(orc, ow, desc, rays, table, **kw)["cols"].astype(np.float64)
    bound = 4 * 15 * (1 + 1e-6)
    var_mis, var_nee = mis[:, :, 0].var(axis=1, ddof=1).mean(), nee[:, :, 0].var(axis=1, ddof=1).mean()
    print("trt_nee_mis mean", mis[:, :, 0].mean(), "variance", var_mis, "largest", mis.max(), "| trt_nee mean", nee[:, :, 0].mean(), "variance", var_nee,
          "largest", nee.max())
    assert mis.max() <= bound, mis.max()
    assert nee.max() > bound, nee.max()
    assert var_mis < var_nee / 10.0, (var_mis, var_nee)


def _pooled_z(a, ka, g, kg):
    """tests/test_nee_cases.py's pooling: z = (mean_a - mean_g) / sqrt(sum_i(var_a,i / K_a + var_g,i / K_g)) * n."""
    return (a.mean() - g.mean()) / np.sqrt((a.var(axis=1, ddof=1) / ka + g.var(axis=1, ddof=1) / kg).sum()) * len(a)


def test_the_contract_is_unbiased_against_the_references_transport(trt, orc):
    """The lowered box, 40 surfels, cosine source, B = 4, |z| <= 4 (the project's bound).  Both heuristics with source_is_diffuse = 1
    against the plain restated path with the first hit's emission dropped (passes_cases.oracle_paths: a path that ends on a light
    at hit 1 carries that emission alone and counts 0, every other path added nothing at hit 1), K = 2048 against 8192 on streams of
    its own; BALANCE with source_is_diffuse = 0 against oracle_gather, K = 2048 against 4096."""
    B, KM, KP, KG = 4, 2048, 8192, 4096
    black = (0.0, 0.0, 0.0)
    desc, ow, items, table, rays = _lowered(trt, orc, KM)
    # plain paths, first hit's emission dropped: the reference's loop minus what it adds at hit 1 (colour is linear in the emissions)
    own = 1000 + 40 * KM + 7
    rays_p = GC.first_rays(orc, items, "cosine", KP, M.SPREAD, M.SEED, own)
    cols, kinds, depths, _ = P.oracle_paths(orc, ow, desc, rays_p, B, black, M.SEED, own)
    first_is_light = (kinds == P.LIGHT) & (depths == 0)                     # the path ended on the lamp at hit 1: its colour is that emission alone
    plain = np.where(first_is_light, 0.0, cols[:, :, 0].astype(np.float64))
    assert first_is_light.any() and plain.mean() > 0.05
    out = {}
    for name, h in sorted(M.HEURISTICS.items()):
        a = M.mis_paths(orc, ow, desc, rays, table, max_bounces=B, background=black, source_is_diffuse=True, heuristic=h)["cols"][:, :, 0].astype(np.float64)
        out[name + ", indirect"] = (a.mean(), plain.mean(), _pooled_z(a, KM, plain, KP))
    _, g, _ = GC.oracle_gather(orc, ow, items, "cosine", KG, B, black, M.SEED, own)
    g = g[:, :, 0].astype(np.float64)
    a = M.mis_paths(orc, ow, desc, rays, table, max_bounces=B, background=black, heuristic=M.BALANCE)["cols"][:, :, 0].astype(np.float64)
    out["balance, first hit seen"] = (a.mean(), g.mean(), _pooled_z(a, KM, g, KG))
    for what, (mean_a, mean_b, z) in out.items():
        print(what, "mean", mean_a, "against", mean_b, "z", z)
    for what, (mean_a, mean_b, z) in out.items():
        assert mean_a > 0.05 and mean_b > 0.05
        assert abs(z) <= 4.0, (what, mean_a, mean_b, z)
