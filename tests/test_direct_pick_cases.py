"""The restatement of the alias-table direct-light queries (tests/direct_pick_cases.py) without a GPU: it is what tinyrt.h states at the
edges of the new steps 2 and 5 and of the new hit weight, every deliberately wrong variant of it is told apart by a named class of
cases, it is unbiased against the restated trt_direct, and it does what the feature is for - less variance where powers differ.

Classes (the Cornell box's 324 items of direct_cases, its table of three - the lamp, a virtual quad, a virtual sphere):
  edge_of_q       u1 one float either side of q[k]: q = u1 takes the alias, q = the next float keeps the slot
  q_0_1_nan       q = 0 and NaN always take the alias, q = 1 never
  alias_clamped   alias >= E reads record E - 1
  prob_edges      prob = 0 and a prob that overflows area / p are dead samples; a subnormal prob that does not overflow is a live one
  alias_taken     samples that took an alias with another prob than the slot's
  table_of_one    E = 1: every draw ends on record 0, and one draw more than trt_direct is taken
  f32_slot        E = 65521: slots where uint32(u0 * float(E)) in f32 is not the exact floor
  light_hits      trt_direct_mis_pick's lobe hits on lights: ph has the bits of the table's prob
Mutants (direct_pick_cases.MUTANTS) and the class that kills each are listed in KILLED_BY."""
import numpy as np
import pytest

import direct_cases as D
import direct_mis_cases as M
import direct_pick_cases as P

f32 = np.float32
KILLED_BY = {"u1_le_q": "edge_of_q", "alias_unclamped": "alias_clamped", "area_times_inv_p": "prob_edges", "prob_of_slot": "alias_taken",
             "u1_first": "alias_taken", "hit_uses_E": "light_hits", "luminance_parens": "light_hits"}
ITEMS = list(range(0, 324, 3))                                              # every third item of the batch: 108 surfels, K = 8


@pytest.fixture(scope="module")
def box(trt, orc):
    sc = M.scene(trt, orc, "cornell")
    pick, total = P.build(sc["table"])
    assert len(sc["table"]) == 3
    return dict(sc, pick=pick, total=total)


def run(orc, box, pick, mutant=None, only=ITEMS, table=None, **kw):
    return P.samples(orc, box["ow"], box["items"], box["table"] if table is None else table, pick, mutant=mutant, only=only, **kw)


def first_two(orc, n, k=P.K):
    """u0, u1 [n, k] of the batch's streams."""
    out = np.zeros((2, n, k), np.float32)
    for i in range(n):
        for s in range(k):
            out[:, i, s] = P.draws(orc, P.SEED, P.FIRST_STREAM + i * k + s)
    return out


def differ(a, b, keys=("e", "live", "c", "wgt")):
    return any(a[k].tobytes() != b[k].tobytes() for k in keys)


def test_every_mutant_has_a_class():
    assert set(KILLED_BY) == set(P.MUTANTS)


def test_edge_of_q(orc, box):
    """One sample: q[k] set to its own u1 takes the alias (u1 < q is false), q[k] one float above keeps the slot; `u1 <= q` keeps both."""
    i, s = ITEMS[5], 2
    u0, u1 = P.draws(orc, P.SEED, P.FIRST_STREAM + i * P.K + s)
    k = min(int(u0 * f32(3.0)), 2)
    at, above = box["pick"].copy(), box["pick"].copy()
    at["q"][k], above["q"][k] = u1, np.nextafter(u1, f32(2.0))
    at["alias"][k] = above["alias"][k] = (k + 1) % 3
    a = P.samples(orc, box["ow"], box["items"], box["table"], at, only=[i])
    b = P.samples(orc, box["ow"], box["items"], box["table"], above, only=[i])
    assert a["slot"][i, s] == b["slot"][i, s] == k
    assert a["took_alias"][i, s] and a["e"][i, s] == (k + 1) % 3
    assert not b["took_alias"][i, s] and b["e"][i, s] == k
    wrong = P.samples(orc, box["ow"], box["items"], box["table"], at, only=[i], mutant="u1_le_q")
    assert not wrong["took_alias"][i, s] and differ(a, wrong)


def test_q_0_1_nan(orc, box):
    for q, takes in ((0.0, True), (np.nan, True), (1.0, False)):
        pick = box["pick"].copy()
        pick["q"] = q
        pick["alias"] = [1, 2, 0]
        got = run(orc, box, pick)
        assert (got["took_alias"][ITEMS] == takes).all(), q
        want_e = np.array([1, 2, 0])[got["slot"][ITEMS]] if takes else got["slot"][ITEMS]
        assert (got["e"][ITEMS] == want_e).all() and len(np.unique(got["slot"][ITEMS])) == 3


def test_alias_clamped(orc, box):
    pick = box["pick"].copy()
    pick["q"] = 0.0
    for alias in (3, 4, 2 ** 31, 0xFFFFFFFF):
        pick["alias"] = alias
        got = run(orc, box, pick)
        assert (got["e"][ITEMS] == 2).all() and got["live"][ITEMS].any()
        wrong = run(orc, box, pick, mutant="alias_unclamped")
        assert (wrong["e"][ITEMS] == -1).all() and differ(got, wrong)


def test_prob_edges(orc, box):
    """prob = 0: area / 0 = inf, the weight is inf or NaN, the sample dead.  prob = 1e-37 under the lamp's area of 600: area / p
    overflows, dead.  prob = 1e-39, a subnormal, under the area 0.1257 of a sphere of radius 0.1: area / p = 1.26e38 is finite and the
    sample lives with the weight the division gives - area * (1 / p) overflows in 1 / p and kills it."""
    good = run(orc, box, box["pick"])
    assert good["live"][ITEMS].mean() > 0.5
    for p in (0.0, 1e-37):
        pick = box["pick"].copy()
        pick["prob"][0] = p
        got = run(orc, box, pick)
        lamp = got["e"][ITEMS] == 0
        assert lamp.sum() > 100 and not got["live"][ITEMS][lamp].any() and (got["c"][ITEMS][lamp] == 0).all()
        assert got["live"][ITEMS][~lamp].tobytes() == good["live"][ITEMS][~lamp].tobytes()
    table = box["table"].copy()
    table[2:] = D.sphere_record((50.0, 50.0, 50.0), 0.1, (1e-30, 1e-30, 1e-30))
    pick = box["pick"].copy()
    pick["prob"][2] = 1e-39
    pick["q"], pick["alias"] = 0.0, 2                                       # every sample goes to the small sphere
    assert 0 < pick["prob"][2] < np.finfo(np.float32).tiny
    got = run(orc, box, pick, table=table)
    assert (got["e"][ITEMS] == 2).all() and got["live"][ITEMS].mean() > 0.3
    assert np.isfinite(got["wgt"][ITEMS]).all() and got["wgt"][ITEMS].max() > 1e30
    wrong = run(orc, box, pick, table=table, mutant="area_times_inv_p")
    assert not wrong["live"][ITEMS].any() and differ(got, wrong)


def test_alias_taken(orc, box):
    """The power table of the box: the lamp's slot keeps itself, the two virtual emitters' slots mostly send to it.  prob is the chosen
    emitter's, not the slot's; u1 is the second draw, not the first."""
    got = run(orc, box, box["pick"])
    took = got["took_alias"][ITEMS]
    assert 0.3 < took.mean() < 0.8
    e, slot = got["e"][ITEMS], got["slot"][ITEMS]
    assert (box["pick"]["prob"][e[took]] != box["pick"]["prob"][slot[took]]).all()
    u0, u1 = first_two(orc, 324)
    assert (slot == np.minimum((u0[ITEMS] * f32(3.0)).astype(np.int64), 2)).all()
    assert (took == ~(u1[ITEMS] < box["pick"]["q"][slot])).all()
    for mutant in ("prob_of_slot", "u1_first"):
        assert differ(got, run(orc, box, box["pick"], mutant=mutant)), mutant
    # the frequencies are the table's prob (108 x 8 samples: a coarse check that the structure and prob speak of the same thing)
    freq = np.bincount(e.ravel(), minlength=3) / e.size
    assert np.abs(freq - box["pick"]["prob"]).max() < 0.05, (freq, box["pick"]["prob"])


def test_table_of_one(orc, box):
    own = box["table"][:1]
    pick, total = P.build(own)
    assert pick["q"][0] == 1.0 and pick["alias"][0] == 0 and pick["prob"][0] == 1.0
    got = run(orc, box, pick, table=own)
    uniform = D.samples(orc, box["ow"], box["items"], own, only=ITEMS)
    assert (got["e"][ITEMS] == 0).all() and not got["took_alias"][ITEMS].any()
    assert got["live"][ITEMS].any() and got["rays"][ITEMS].tobytes() != uniform["rays"][ITEMS].tobytes()      # one draw more was taken


def test_f32_slot(trt, orc, box):
    """E = 65521: u0 * float(E) rounds up to the next integer in f32 for about one stream in 2^9; the slot is the f32 product's."""
    E = 65521
    table = np.ascontiguousarray(box["table"][np.arange(E) % 3])
    pick, _ = P.build(table)
    found = []
    for stream in range(20000):
        u0 = P.draws(orc, P.SEED, P.FIRST_STREAM + stream, 1)[0]
        if int(u0 * f32(E)) != int(float(u0) * E):
            found.append((stream, int(u0 * f32(E)), int(float(u0) * E)))
            if len(found) == 3:
                break
    assert len(found) == 3, found
    items = box["items"][:1]
    for stream, slot32, exact in found:
        got = P.samples(orc, box["ow"], items, table, pick, k=1, first_stream=P.FIRST_STREAM + stream)
        assert got["slot"][0, 0] == slot32 == exact + 1


@pytest.fixture(scope="module")
def lowered(trt, orc):
    """direct_mis_cases' lowered box: 20 ceiling surfels one unit above the lamp, where about 30 % of the lobe rays hit it, and 40 floor
    surfels; the lamp recoloured so that the luminance depends on its parenthesisation."""
    desc, _, items, _ = M.lowered_cornell(trt, orc)
    mats = [(n, k, (12.5, 9.3, 12.0) if n == "light" else c, f) for n, k, c, f in desc["materials"]]
    desc = dict(desc, materials=mats)
    ow, _ = orc.world_from_description(desc)
    table = np.ascontiguousarray(np.concatenate([D.emitters_of(orc, desc), D.virtual_emitters(orc)]))
    pick, total = P.build(table)
    return dict(desc=desc, ow=ow, items=items, table=table, pick=pick, total=total)


@pytest.mark.parametrize("heuristic", sorted(P.HEURISTICS))
def test_light_hits(orc, lowered, heuristic):
    """Every lobe hit on the lamp recomputes ph with the bits of the table's prob for the lamp; float(E) in the hit weight and another
    parenthesisation of the luminance are told apart; with BALANCE a sample stays within twice the largest colour channel."""
    L = lowered
    h = P.HEURISTICS[heuristic]
    args = (orc, L["ow"], L["desc"], L["items"], L["table"], L["pick"], L["total"])
    base = P.samples(orc, L["ow"], L["items"], L["table"], L["pick"])
    got = P.mis_samples(*args, heuristic=h, base=base)
    hits = got["has_b"]
    assert hits[:20].mean() > 0.2 and (hits & ~got["full"]).sum() > 30
    assert (got["ph_bits"][hits] == L["pick"]["prob"][:1].view(np.uint32)[0]).all()
    assert P.luminance(L["table"]["color"][0]) != P.luminance(L["table"]["color"][0], "luminance_parens")
    for mutant in P.HIT_MUTANTS:
        wrong = P.mis_samples(*args, heuristic=h, base=base, mutant=mutant)
        assert differ(got, wrong, ("wb", "c")), mutant
    assert (got["has_l"] & hits).sum() >= 5                                 # both terms in one sample
    if heuristic == "balance":
        own = got["e"] == 0                                                 # (a virtual emitter's shadow term counts in full)
        assert got["c"][own].max() <= 2.0 * 12.5 * (1 + 1e-6)


def _pooled_z(a, ka, g, kg):
    """tests/test_direct_mis_cases.py's pooling: z = (mean_a - mean_g) / sqrt(sum_i(var_a,i / K_a + var_g,i / K_g)) * n."""
    return (a.mean() - g.mean()) / np.sqrt((a.var(axis=1, ddof=1) / ka + g.var(axis=1, ddof=1) / kg).sum()) * len(a)


# Measured with the fixtures below (tests/README_direct_pick.md): the uniform choice's mean per-surfel sample variance over the PICK
# query's, same surfels, same K.  The test asserts half of it.
MEASURED_GAIN = 127.7


def test_unbiased_and_the_point_of_the_feature(trt, orc):
    """The many-light room (the lamp at y = 99 and 60 dim sphere lights), 40 floor surfels.  The restated trt_direct_pick and
    trt_direct_mis_pick (both heuristics) at K = 512 against the restated trt_direct at K = 8192 on streams of its own: pooled
    |z| <= 4, the project's bound.  Then the point: at the same K = 512 the PICK query's mean per-surfel sample variance against the
    uniform choice's."""
    k, kg = 512, 8192
    desc, ow, items, table = P.many_light_room(trt, orc)
    pick, total = P.build(table)
    g = D.samples(orc, ow, items, table, k=kg, first_stream=P.FIRST_STREAM + len(items) * k + 7)["c"][:, :, 0].astype(np.float64)
    base = P.samples(orc, ow, items, table, pick, k=k)
    runs = {"pick": base["c"][:, :, 0].astype(np.float64)}
    for name, h in sorted(P.HEURISTICS.items()):
        runs["mis_pick, " + name] = P.mis_samples(orc, ow, desc, items, table, pick, total, heuristic=h, k=k, base=base)["c"][:, :, 0].astype(np.float64)
    uniform = D.samples(orc, ow, items, table, k=k)["c"][:, :, 0].astype(np.float64)
    var_uniform = uniform.var(axis=1, ddof=1).mean()
    out = {}
    for what, a in runs.items():
        out[what] = (a.mean(), a.var(axis=1, ddof=1).mean(), _pooled_z(a, k, g, kg))
        print(what, "mean", out[what][0], "variance", out[what][1], "| uniform K=8192 mean", g.mean(), "| z", out[what][2])
    gain = var_uniform / out["pick"][1]
    print("uniform K=512 mean", uniform.mean(), "variance", var_uniform, "| gain of pick", gain, "| of mis_pick balance",
          var_uniform / out["mis_pick, balance"][1])
    for what, (mean_a, _, z) in out.items():
        assert mean_a > 0.05 and g.mean() > 0.05
        assert abs(z) <= 4.0, (what, mean_a, g.mean(), z)
    assert out["pick"][1] < var_uniform                                     # never less than "lower than uniform"
    assert gain >= MEASURED_GAIN / 2.0, (gain, MEASURED_GAIN)
