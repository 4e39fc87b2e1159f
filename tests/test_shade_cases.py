"""The inputs of the shade-level test (tests/shade_cases.py, run on the GPU by tests/test_gpu_shade.py) checked on the CPU: the case
list is deterministic, every class has its defining property under the oracle, a second float32 restatement of HitRecord::new +
Material::scatter equals orc_sphere_hit / orc_quad_hit + orc_material_scatter bit for bit on every case, and the list tells that
restatement from twelve altered copies of it (run with -s for the killing cases).

Measured (seed 1): 1436 cases on `zoo` and as many on `hot`, 1024 of them generic; the restatement differs from the oracle on 0;
ri * sinv == 1.0 exactly is reached for all four (index, face) pairs that can reflect totally.
Killing cases on `zoo` (mutant: number of cases, classes; `hot` has the same rays):
   1 near_zero eps 1e-8: 3 (lam_tiny_sum)
   2 near_zero branch removed: 6 (lam_zero_sum, lam_tiny_sum)
   3 no clamp in the scatter's cosine: 8 (dielectric_scaled_dir)
   4 no clamp in refract: 11 (dielectric_cos_above_one)
   5 >= in the total-reflection test: 13 (dielectric_tir_straddle 10, and one case each of dielectric_grazing, front_face_sphere and front_face_quad whose
     product lands on 1.0)
   6 >= in reflectance-versus-draw: 6 (dielectric_draw_edge 2 - the 1/32 cases -, dielectric_scaled_dir 4)
   7 a draw consumed on total reflection: 57 (generic 26, dielectric_tir_straddle 14, ...)
   8 front_face with <=: 6 (front_face_sphere: the exact tangents)
   9 index not inverted on the front face: 151 (generic 100, ...)
  10 x^5 as (x2 * x2) * x: NOT DISTINGUISHED - the same product, IEEE multiplication commutes; 0 of 4 194 304 random x differ
  11 no fabs in refract: 13 (dielectric_scaled_dir 12, dielectric_tir_straddle 1)
  12 dot with fused multiply-adds: 274 (generic 179, extreme_quad 16, extreme_quad_grazing 12, ...)
Mutant 3 is killed only by the directions of length 0.9 .. 1.2 that Ray::new makes of vectors with a subnormal squared length: for a
direction that is unit to within rounding the clamp moves cosv by an ulp, sinv = sqrt(1 - cosv^2) is 0 instead of NaN and both fail
`ri * sinv > 1`, and (1 - cosv)^5 ~ -1e-35 vanishes against r0 (or, for r0 = 0, is no more above a draw than +0 is).
"""
import collections

import numpy as np
import pytest

import shade_cases as S

F = np.float32


@pytest.fixture(scope="module")
def lists(orc):
    """scene name -> (Scene, cases, traces of the unmutated restatement)."""
    out = {}
    for name in S.scene_names():
        sc = S.Scene(name)
        cases = S.case_list(orc, sc)
        traces = []
        for c in cases:
            tr = {}
            if c["geo"] >= 0:
                S.restate(orc, sc, c, 0, tr)
            traces.append(tr)
        out[name] = (sc, cases, traces)
    return out


def of_class(lists, name, cls):
    sc, cases, traces = lists[name]
    sel = [(c, tr) for c, tr in zip(cases, traces) if c["cls"] == cls]
    assert sel, (name, cls)
    return sc, sel


def test_the_list_is_deterministic_and_every_class_is_there(lists, orc):
    expected = {"generic", "generic_big_inside", "lam_zero_sum", "lam_tiny_sum", "lam_not_near_zero", "lam_u3_zero", "lam_domain_edge", "metal_incidence",
                "metal_tiny_dir", "metal_below_surface", "dielectric_tir_straddle", "dielectric_cos_above_one", "dielectric_scaled_dir",
                "dielectric_draw_edge", "dielectric_grazing", "front_face_sphere", "front_face_quad", "front_face_far", "extreme_quad",
                "extreme_quad_grazing", "light", "miss"}
    for name, (sc, cases, _) in lists.items():
        assert sc.n == 32 and sc.lazy == (name == "zoo")
        count = collections.Counter(c["cls"] for c in cases)
        print(f"\n{name}: {len(cases)} cases:", dict(count))
        assert set(count) == expected
        again = S.case_list(orc, S.Scene(name))
        assert len(again) == len(cases)
        for a, b in zip(cases, again):
            assert np.array_equal(S.case_words(sc, a), S.case_words(sc, b)) and a["cls"] == b["cls"]
        order, tasks = S.wave_lists(len(cases))
        assert sorted(order[:len(cases)]) == list(range(len(cases))) and sorted(order[len(cases):]) == list(range(len(cases)))
        assert tasks[:, 1].sum() == len(order) and set(S.LIST_LENGTHS) <= set(int(x) for x in tasks[:, 1]) and int(tasks[0, 1]) == len(cases)
        # the first wave of the whole-list shuffle holds several material kinds
        assert len({S.kind_of_case(sc, cases[i]) for i in order[:64]}) >= 4
    vc = S.vector_cases()
    assert np.array_equal(S.bits(vc), S.bits(S.vector_cases())) and len(vc) > 8000


def test_generic_cells_are_full(lists):
    for name in lists:
        sc, sel = of_class(lists, name, "generic")
        cells = collections.Counter((S.kind_of_case(sc, c), int(sc.kind[c["geo"]]), c["front"]) for c, _ in sel)
        assert len(cells) == 16 and set(cells.values()) == {S.GENERIC_PER_CELL}
        assert {c["remain"] for c, _ in sel} == {1, 2}
        used = {sc.geo_mat[c["geo"]] for c, _ in sel}
        assert used == set(range(len(S.MATERIALS)))                         # every fuzz, every index
        for m in range(len(S.MATERIALS)):
            if sc.mats[m][0] == S.DIELECTRIC:
                assert {c["front"] for c, _ in sel if sc.geo_mat[c["geo"]] == m} == {True, False}
        lazy = sum(c["lazy_ok"] for c, _ in sel)
        assert (lazy > len(sel) // 2) if name == "zoo" else lazy == 0
        if name == "hot":
            assert any(np.isinf(c["atten"]).any() for c, _ in sel)


def test_lambertian_classes(lists, orc):
    for name in lists:
        sc, sel = of_class(lists, name, "lam_zero_sum")
        for c, tr in sel:
            assert tr["near_zero"] and (tr["sum"] == 0).all() and tuple(tr["normal"]) == (0.0, 0.0, -1.0)
            e = S.expectation(orc, sc, c)
            assert np.array_equal(e[3:6], S.bits([-0.0, -0.0, -1.0]))                        # (-0, -0, -1), not NaN
        sc, sel = of_class(lists, name, "lam_tiny_sum")
        for c, tr in sel:
            assert tr["near_zero"] and (tr["sum"] != 0).any() and (np.abs(tr["sum"]) < F(1e-7)).all()
            assert (np.abs(tr["sum"]) >= F(1e-8)).any()                                       # an eps of 1e-8 would not take the branch
        sc, sel = of_class(lists, name, "lam_not_near_zero")
        for c, tr in sel:
            big = np.sort(np.abs(tr["sum"]))
            assert not tr["near_zero"] and F(1e-7) <= big[2] < F(2e-6)
        # the nearest sum that does not take the branch stays pinned: within 2 ulp of a component ~1 (2.4e-7) of zero
        assert min(float(np.abs(tr["sum"]).max()) for _, tr in sel) <= 2.4e-7
        sc, sel = of_class(lists, name, "lam_u3_zero")
        for c, tr in sel:
            assert (tr["in_sphere"] == 0).all()
            e = S.expectation(orc, sc, c)
            assert np.isnan(e[3:6].view(F)).all() and not np.isnan(e[0:3].view(F)).any()
        sc, sel = of_class(lists, name, "lam_domain_edge")
        mins = sorted(float(np.abs(tr["dir"]).min()) for _, tr in sel)
        assert mins[0] == float(S.nextf(S.LO, -1)) and mins[-1] == float(S.LO)              # plain path; short path with its smallest operand
        for _, tr in sel:
            assert (tr["dir"] != 0).all() and not tr["near_zero"] and float(np.abs(tr["dir"]).max()) == 2.0


def test_metal_classes(lists):
    for name in lists:
        sc, sel = of_class(lists, name, "metal_incidence")
        assert {sc.geo_mat[c["geo"]] for c, _ in sel} == {m for m in range(len(S.MATERIALS)) if sc.mats[m][0] == S.METAL}
        assert sorted({float(sc.material(c["geo"])[2]) for c, _ in sel}) == [0.0, float(F(0.3)), 1.0]     # -0.5 and 1.5 clamped
        with np.errstate(all="ignore"):
            cosines = [abs(float(S.dot(c["d"], tr["normal"]))) for c, tr in sel]
        assert min(cosines) < 0.01 and max(cosines) > 0.999999
        sc, sel = of_class(lists, name, "metal_below_surface")
        for c, tr in sel:
            assert float(S.dot(tr["dir"], tr["normal"])) < 0.0
        sc, sel = of_class(lists, name, "metal_tiny_dir")
        mins = [float(np.abs(tr["dir"]).min()) for _, tr in sel]
        for (c, tr), m in zip(sel, mins):
            assert float(sc.material(c["geo"])[2]) == 1.0 and (tr["dir"] != 0).all() and float(np.abs(tr["dir"]).max()) < 5e-7
        assert min(mins) < float(S.LO) and float(S.LO) in mins and max(mins) > float(S.LO)


STRADDLE_FLOATS = {"die09": (1, 1), "die15": (2, 1), "die067": (2, 1), "die24": (3, 6)}


def nearest_products(ri, span=20000):
    """(smallest ri * sqrt(1 - c * c) above 1.0, largest below 1.0) over the floats c around sqrt(1 - 1 / ri^2) - the product falls
    monotonically in c, so floats further away give nothing nearer."""
    one = F(1.0)
    with np.errstate(all="ignore"):
        c0 = F(np.sqrt(1.0 - 1.0 / float(ri) ** 2))
        c = (int(S.bits(c0)[0]) + np.arange(-span, span + 1)).astype(np.uint32).view(F)
        prod = F(ri) * np.sqrt(one - c * c)
    assert prod[0] > S.nextf(one, 8) and prod[-1] < S.nextf(one, -8) and (np.diff(prod) <= 0).all()
    return prod[prod > one].min(), prod[prod < one].max()


def test_dielectric_classes(lists, orc):
    for name in lists:
        one = F(1.0)
        sc, sel = of_class(lists, name, "dielectric_tir_straddle")
        seen = collections.defaultdict(set)
        for c, tr in sel:
            key = (sc.desc["materials"][sc.geo_mat[c["geo"]]][0], tr["front"])
            side = 1 if tr["prod"] > one else (0 if tr["prod"] == one else -1)
            # floats above 1.0 (2^-23 each) / below (2^-24 each) per index: one ulp wherever the arithmetic allows it - sinv is a function of
            # the float cosv alone, so the products are a fixed set per ri, and the scan below shows these are its members next to 1.0
            up, down = STRADDLE_FLOATS[key[0]]
            assert S.nextf(one, -down) <= tr["prod"] <= S.nextf(one, up) and tr["tir"] == (side == 1), (key, tr["prod"])
            above, below = nearest_products(tr["ri"])
            assert tr["prod"] == (above if side == 1 else one if side == 0 else below), (key, tr["prod"], above, below)
            seen[key].add(side)
            e = S.expectation(orc, sc, c)
            if tr["tir"]:
                assert (int(e[13]), int(e[14])) == c["rng"]                                  # no draw on total reflection
            else:
                assert (int(e[13]), int(e[14])) == S.rng_step(*c["rng"])[1]
        print(f"\n{name}: total-reflection straddles (material, front face) -> sides of 1.0 reached:", dict(seen))
        assert set(seen) == set(S.TIR_FACES)
        for key, sides in seen.items():
            assert {1, -1} <= sides, key
        assert all(0 in s for s in seen.values())                                             # ri * sinv == 1.0 exactly: found for every pair
        n_tir = 0
        for c, tr in zip(lists[name][1], lists[name][2]):
            if tr.get("tir"):
                n_tir += 1
                e = S.expectation(orc, sc, c)
                assert (int(e[13]), int(e[14])) == c["rng"], c["cls"]
        assert n_tir >= 50
        sc, sel = of_class(lists, name, "dielectric_cos_above_one")
        for c, tr in sel:
            assert tr["cos_raw"] > one and tr["cos_raw"] <= S.nextf(one, 4)
        assert {int(sc.kind[c["geo"]]) for c, _ in sel} == {0, 1}
        sc, sel = of_class(lists, name, "dielectric_scaled_dir")
        lengths = [float(np.linalg.norm(c["d"].astype(np.float64))) for c, _ in sel]
        assert min(lengths) < 0.99 and max(lengths) > 1.05 and all(0.85 < x < 1.25 for x in lengths)
        for c, _ in sel:                                                                      # a direction Ray::new can return
            tiny = c["d"].astype(np.float64) * 2.0 ** -74
            assert any(np.array_equal(S.bits(S._vec(orc.lib.orc_ray_new(orc.Vec3(), orc.Vec3(*[float(F(x * k)) for x in tiny])).direction)), S.bits(c["d"]))
                       for k in np.linspace(0.6, 1.7, 221))
        assert any(tr["cos_raw"] > F(1.01) for _, tr in sel) and any("refract_k" in tr and tr["refract_k"] < 0 for _, tr in sel)
        sc, sel = of_class(lists, name, "dielectric_draw_edge")
        sides = collections.Counter()
        for c, tr in sel:
            step = F(2.0 ** -23)
            assert not tr["tir"] and abs(float(tr["u"]) - float(tr["reflectance"])) <= float(step)
            sides[int(np.sign(float(tr["u"]) - float(tr["reflectance"])))] += 1
            if tr["u"] == tr["reflectance"]:
                assert tr["reflectance"] == F(1.0 / 32.0) and not tr["do_reflect"]            # strict: equal refracts
        assert sides[0] == 2 and sides[-1] >= 10 and sides[1] >= 10
        sc, sel = of_class(lists, name, "dielectric_grazing")
        assert sum(float(tr["reflectance"]) > 0.9 for _, tr in sel if not tr["tir"]) >= 3
        assert {sc.geo_mat[c["geo"]] for c, _ in sel} == {m for m in range(len(S.MATERIALS)) if sc.mats[m][0] == S.DIELECTRIC}


def test_front_face_light_and_miss_classes(lists, orc):
    for name in lists:
        sc, sel = of_class(lists, name, "front_face_sphere")
        dots = np.array([float(tr["front_dot"]) for _, tr in sel])
        r = np.array([abs(float(sc.b[c["geo"], 0])) for c, _ in sel])
        # within a few ulp of the operands (|d| = 1, |p - c| = r: an ulp of their product is 1.2e-7 r)
        assert (np.abs(dots) <= 4e-7 * r).all() and (dots < 0).sum() >= 4 and (dots > 0).sum() >= 4 and (dots == 0).sum() >= 2
        for c, tr in sel:
            assert tr["front"] == (tr["front_dot"] < 0) == c["front"]
        sc, sel = of_class(lists, name, "front_face_quad")
        dots = np.array([float(tr["front_dot"]) / float(np.linalg.norm(sc.quad_n[c["geo"]].astype(np.float64))) for c, tr in sel])
        assert (np.abs(dots) <= 2e-6).all() and (dots < 0).sum() >= 4 and (dots > 0).sum() >= 4
        for gi, kind in ((S.GEO["tiny"], S.METAL), (S.GEO["huge"], S.LAMBERTIAN)):           # |n| ~ 1e-12 and ~ 1e12
            sc, sel = of_class(lists, name, "extreme_quad")
            sel = [(c, tr) for c, tr in sel if c["geo"] == gi]
            nl = float(np.linalg.norm(sc.quad_n[gi].astype(np.float64)))
            assert (nl < 2e-12 if gi == S.GEO["tiny"] else nl > 1e12) and S.kind_of_case(sc, sel[0][0]) == kind
            assert sum(c["front"] for c, _ in sel) >= 4 and sum(not c["front"] for c, _ in sel) >= 4
            for c, tr in sel:
                e = S.expectation(orc, sc, c)
                assert np.isfinite(e[0:6].view(F)).all() and tr["front"] == c["front"]      # a finite scattered ray: the normal reaches the output
                assert abs(float(np.linalg.norm(e[3:6].view(F).astype(np.float64))) - 1.0) < 1e-6
        sc, sel = of_class(lists, name, "extreme_quad_grazing")
        nl = float(np.linalg.norm(sc.quad_n[S.GEO["huge"]].astype(np.float64)))
        dots = np.array([float(tr["front_dot"]) / nl for _, tr in sel])
        assert all(c["geo"] == S.GEO["huge"] for c, _ in sel) and (np.abs(dots) <= 2e-6).all() and (dots < 0).sum() >= 3 and (dots > 0).sum() >= 3
        for c, _ in sel:
            assert np.isfinite(S.expectation(orc, sc, c)[0:6].view(F)).all()
        sc, sel = of_class(lists, name, "front_face_far")
        assert all(9e5 < float(c["t"]) < 1.1e6 for c, _ in sel) and len(sel) >= 4
        sc, sel = of_class(lists, name, "light")
        assert len(sel) >= 4
        for c, _ in sel:
            e = S.expectation(orc, sc, c)
            assert np.array_equal(e[0:3], S.bits(c["o"])) and np.array_equal(e[3:6], S.bits(c["d"])) and np.array_equal(e[9:12], S.bits(c["atten"]))
            assert (int(e[12]), int(e[13]), int(e[14]), int(e[15])) == (c["remain"], c["rng"][0], c["rng"][1], 1)
        sc, sel = of_class(lists, name, "miss")
        assert len({tuple(S.bits(c["bg"])) for c, _ in sel}) >= 4 and len({tuple(S.bits(c["atten"])) for c, _ in sel}) >= 4
        if name == "hot":                                                                     # inf * 0 = NaN in the carried colour
            allc = lists[name][1]
            assert any(np.isnan(S.expectation(orc, sc, c)[6:9].view(F)).any() for c in allc if np.isinf(c["atten"]).any())


def test_second_restatement_equals_the_oracle_bit_for_bit(lists, orc):
    for name, (sc, cases, _) in lists.items():
        n = 0
        for i, c in enumerate(cases):
            if c["geo"] < 0:
                continue
            a, b = S.restate(orc, sc, c), S.oracle_scatter(orc, sc, c)
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), (name, i, c["cls"], a, b)
            n += 1
        print(f"\n{name}: restatement == oracle on {n} cases")


def power_five_search(n=1 << 22):
    g = np.random.default_rng([S.SEED, 10])
    x = g.uniform(-0.25, 2.0, n).astype(F)
    x2 = x * x
    return int((S.bits((x2 * x2) * x) != S.bits(x * (x2 * x2))).sum()), n


def test_the_case_list_kills_the_mutants(lists, orc):
    not_distinguished = {}
    for name, (sc, cases, _) in lists.items():
        base = [S.restate(orc, sc, c) if c["geo"] >= 0 else None for c in cases]
        for mut in range(1, S.N_MUTANTS + 1):
            killers = []
            for i, c in enumerate(cases):
                if base[i] is None:
                    continue
                m = S.restate(orc, sc, c, mut)
                if not np.array_equal(m, base[i]):
                    killers.append(i)
            classes = collections.Counter(cases[i]["cls"] for i in killers)
            if killers:
                print(f"\n{name}: mutant {mut:2d} ({S.MUTANT_NAMES[mut]}): killed by {len(killers)} cases, first: case {killers[0]} "
                      f"({cases[killers[0]]['cls']}, geometry {cases[killers[0]]['geo']}); classes {dict(classes)}")
            else:
                not_distinguished.setdefault(mut, []).append(name)
                print(f"\n{name}: mutant {mut:2d} ({S.MUTANT_NAMES[mut]}): NOT DISTINGUISHED by {len(cases)} cases")
    diff, n = power_five_search()
    print(f"\nmutant 10: (x2 * x2) * x against x * (x2 * x2) on {n} random x: {diff} differ")
    assert set(not_distinguished) <= {10, 11}, not_distinguished
    if 10 in not_distinguished:
        assert diff == 0 and n >= 10 ** 6 and "\n  10  " in S.__doc__
    if 11 in not_distinguished:
        assert "\n  11  " in S.__doc__


def test_info_expectation_of_shade_hit_info(lists, orc):
    """What tests/test_gpu_shade.py expects of shade_hit_info: the record of expectation() plus (kind, normal).  The normal is the
    oracle's hit-record normal and has the bits of the restatement's; hide_light moves nothing but the colour words of a light, to
    colour + attenuation * 0; a miss reports SHADE_KIND_MISS and leaves the normal alone."""
    for name, (sc, cases, traces) in lists.items():
        seen, hidden = S.info_expectations(orc, sc, cases, False), S.info_expectations(orc, sc, cases, True)
        assert seen.shape == (len(cases), 20) and np.array_equal(seen[:, :16], S.expectations(orc, sc, cases))
        kinds = np.array([S.kind_of_case(sc, c) for c in cases])
        assert np.array_equal(seen[kinds >= 0, 16], kinds[kinds >= 0].astype(np.uint32)) and (seen[kinds < 0, 16:] == [S.SHADE_KIND_MISS] + [S.INFO_UNSET] * 3).all()
        for i in np.flatnonzero(kinds >= 0):
            assert np.array_equal(seen[i, 17:20], S.bits(traces[i]["normal"])), (name, i, cases[i]["cls"])
        differs = (seen != hidden).any(axis=1)
        assert not differs[kinds != S.LIGHT].any() and differs[kinds == S.LIGHT].any()
        assert np.array_equal(np.delete(seen, [6, 7, 8], axis=1), np.delete(hidden, [6, 7, 8], axis=1))
        with np.errstate(all="ignore"):
            for i in np.flatnonzero(kinds == S.LIGHT):
                assert np.array_equal(hidden[i, 6:9], S.bits(cases[i]["color"] + cases[i]["atten"] * np.zeros(3, F)))
