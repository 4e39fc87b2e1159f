"""The reference of the direct-light query tests (tests/direct_cases.py) is not vacuous, and the contract it restates is unbiased against
the reference's own light transport: conditions on the oracle's answers alone, no GPU.

Per scene, 324 items x 8 samples against the scene's own emitters plus the two virtual ones.  Measured with the CPU oracle when this file
was written (E, occluded share of the live samples, lit samples, items with both a lit and an occluded sample, dead samples):
  cornell 3 / 0.195 / 1870 / 170 / 268     prims33 10 / 0.572 / 680 / 222 / 1004     grid3000 2 / 0.069 / 2164 / 42 / 267
  random_spheres 2 / 0.106 / 1708 / 47 / 682     mixed400 lit 15     prims600 lit 16
mixed400 and prims600 are dense: almost everything there is shadowed.  The bounds asserted below lie under those figures.  Every mutant of
the restatement changes between 195 and 320 of the 324 items on cornell and prims33; shadow_end = 0.5 changes 254 items on prims33.

Unbiasedness, on the Cornell box with the lamp lowered to y = 99 (the stock lamp is coplanar with the ceiling, both y = 100: the
reference's own paths see it only where rounding lets the lamp win the tie, the shadow ray sees it fully - a property of that scene, not
of the query): the mean over 40 unit surfels of the direct-light estimate at K = 512 against the oracle's gather with one bounce and a
black background at K = 8192.  Measured: 0.12644 against 0.12515, pooled z = 0.54."""
import numpy as np
import pytest

import direct_cases as D
import gather_cases as GC
import walk_ray_cases as W

# scene -> (least occluded share of the live samples or None, least lit samples, least partly shadowed items or None)
BOUNDS = {"cornell": (0.05, 400, 10), "prims33": (None, 400, 10), "grid3000": (0.05, 400, 10), "random_spheres": (None, 400, 10),
          "mixed400": (None, 5, None), "prims600": (None, 5, None)}
TABLE_SIZES = {"cornell": 3, "prims33": 10, "grid3000": 2, "random_spheres": 2}


@pytest.fixture(scope="module")
def reference(trt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            desc = W.scene(trt, name)
            ow, _ = orc.world_from_description(desc)
            items, unit = GC.items_of(orc, ow, desc)
            table = D.table_of(orc, desc)
            cache[name] = dict(ow=ow, items=items, unit=unit, table=table, ref=D.freeze(D.reference(orc, ow, items, table)))
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(BOUNDS))
def test_the_reference_is_not_vacuous(reference, name):
    c = reference(name)
    r, table = c["ref"], c["table"]
    share_min, lit_min, partly_min = BOUNDS[name]
    live, occ = r["live"], r["occ"]
    lit = live & ~occ
    share = (occ & live).sum() / live.sum()
    partly = int((lit.any(axis=1) & (occ & live).any(axis=1)).sum())
    kinds = np.bincount(table["kind"][r["e"]].reshape(-1), minlength=2)
    print(name, "E", len(table), "occluded share", share, "lit", int(lit.sum()), "partly", partly, "dead", int((~live).sum()), "kinds", kinds,
          "walks", r["n_walks"])
    if name in TABLE_SIZES:
        assert len(table) == TABLE_SIZES[name]
    if share_min is not None:
        assert share >= share_min, (name, share)
    assert int(lit.sum()) >= lit_min, (name, int(lit.sum()))
    if partly_min is not None:
        assert partly >= partly_min, (name, partly)
    assert kinds[0] > 0 and kinds[1] > 0, (name, kinds)                      # both emitter kinds are chosen
    assert (~live).any(), name                                               # dead samples exist
    assert not (occ & ~r["walked"]).any() and not (r["walked"] & ~live).any()
    assert (r["c"][~lit] == 0).all() and (r["c"][lit] >= 0).all() and (r["c"][lit].sum(axis=-1) > 0).any()
    assert 0 < r["n_walks"] <= live.sum()
    assert D.differing(r["S"], np.zeros_like(r["S"])) >= min(lit_min // 8, 50)


def test_the_shadow_end_matters(reference, orc):
    c = reference("prims33")
    half = D.reference(orc, c["ow"], c["items"], c["table"], shadow_end=0.5)
    n = D.differing(half["S"], c["ref"]["S"])
    print("prims33: items that shadow_end = 0.5 changes", n)
    assert n >= 10
    assert not (half["occ"] & ~c["ref"]["occ"]).any()                        # a shorter segment never adds a hit


@pytest.mark.parametrize("mutant", D.MUTANTS)
def test_every_mutant_of_the_restatement_changes_the_answer(reference, orc, mutant):
    for name in ("cornell", "prims33"):
        c = reference(name)
        wrong = D.reference(orc, c["ow"], c["items"], c["table"], mutant=mutant)
        n = D.differing(wrong["S"], c["ref"]["S"])
        print(name, mutant, "changes", n, "items")
        assert n >= 1, (name, mutant)


def test_the_fold_is_the_contracts():
    """A sample that adds nothing leaves the sums as they are where they are +0 or positive; ranges continue."""
    smp = dict(c=np.array([[[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [0.5, 0.0, 0.25], [0.0, 0.0, 0.0]]], np.float32))
    S, M = D.fold(smp, 4)
    assert S.tolist() == [[0.375, 0.5, 0.8125]] and M.tolist() == [[0.3125, 1.0, 2.265625]]
    S2, M2 = D.fold(smp, 4, 0, 1)
    S2, M2 = D.fold(smp, 4, 1, 4, S2, M2)
    assert S2.tobytes() == S.tobytes() and M2.tobytes() == M.tobytes()


def test_the_contract_is_unbiased_against_the_references_transport(trt, orc):
    """Pooled over the items: many items never reach the lamp in the gather's 8192 samples, so their sample variance there is 0 and a
    per-item z means nothing.  z = (mean_d - mean_g) / sqrt(sum_i(var_d,i / 512 + var_g,i / 8192)) * 40: the standard error of the mean
    of the 40 item means.  |z| <= 4."""
    desc = W.scene(trt, "cornell")
    geos = list(desc["geometries"])
    kind, corner, u, v, mat = geos[2]
    assert mat == "light" and corner[1] == 100.0
    geos[2] = (kind, (corner[0], 99.0, corner[2]), u, v, mat)
    lowered = dict(desc, geometries=geos)
    ow, _ = orc.world_from_description(lowered)
    items, unit = GC.items_of(orc, ow, lowered)
    items = np.ascontiguousarray(items[np.flatnonzero(unit)[:40]])
    assert len(items) == 40
    table = D.emitters_of(orc, lowered)
    assert len(table) == 1 and table["a"][0, 1] == 99.0
    KD, KG = 512, 8192
    d = D.samples(orc, ow, items, table, k=KD)["c"][:, :, 0].astype(np.float64)
    _, g, _ = GC.oracle_gather(orc, ow, items, "cosine", KG, 1, (0.0, 0.0, 0.0), D.SEED, D.FIRST_STREAM)
    g = g[:, :, 0].astype(np.float64)
    mean_d, mean_g = d.mean(), g.mean()
    var = (d.var(axis=1, ddof=1) / KD + g.var(axis=1, ddof=1) / KG).sum()
    z = (mean_d - mean_g) / np.sqrt(var) * len(items)
    ratio_d = np.sqrt(d.var(axis=1, ddof=1)).mean() / mean_d
    ratio_g = np.sqrt(g.var(axis=1, ddof=1)).mean() / mean_g
    print("direct mean", mean_d, "gather mean", mean_g, "z", z, "sd/mean direct", ratio_d, "gather", ratio_g)
    assert mean_d > 0.05 and mean_g > 0.05
    assert abs(z) <= 4.0, (mean_d, mean_g, z)
