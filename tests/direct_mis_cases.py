"""What tests/test_direct_mis_cases.py, tests/test_direct_mis_abi.py, tests/test_gpu_direct_mis.py and tests/test_gpu_direct_mis_long.py share,
none of it touching a GPU: the restatement of a weighted direct-light query (tinyrt.h trt_direct_mis) with the CPU oracle's pieces.

The shadow sample is direct_cases.samples itself, by import: its e, live, occ, wgt and c on stream (seed, j, 1).  On top of it stands
wl = 1 / (1 + q(wgt)) (1 for a virtual emitter) and the lobe part: the reference's own Lambertian scatter (orc_material_scatter on a hit
record whose point and normal are the surfel's, as gather_cases.first_rays draws a cosine ray) on stream (seed, j, 0xFFFFFFFF), the oracle's
World.hit_index over [0.001, inf), the material table of passes_cases.material_table, the area of nee_mis_cases.area_of, and the contract's
arithmetic in numpy float32 scalars with orc_vec3_dot for the dot products.  plain=True forces wl = 1 and no lobe term: trt_direct's
contract, which tests/test_direct_mis_cases.py pins byte for byte to direct_cases.

Fixtures are direct_cases' own: 324 items, K = 8, seed 5, first_stream 1000, the table of direct_cases.table_of.  One scene per kernel
shape (passes_cases.CASES); random_spheres and grid3000 hold no light, so their descriptions are varied - the description only: every
fourth sphere gets a TRT_LIGHT material - and the tests assert by Scene.direct_plan(n, mis=...) that the kernel shape is still the one
meant."""
import ctypes as C

import numpy as np

import direct_cases as D
import gather_cases as GC
import nee_cases as N
import nee_mis_cases as NM
import passes_cases as P
import radiance_cases as R

f32 = np.float32
K, SEED, FIRST_STREAM = D.K, D.SEED, D.FIRST_STREAM
N_ITEMS = D.N_ITEMS
SHADOW_END = D.SHADOW_END
BALANCE, POWER = NM.BALANCE, NM.POWER
HEURISTICS = NM.HEURISTICS
LOBE_WORD = 0xFFFFFFFF                                                      # the stream word of the lobe ray
ORC_LAMBERTIAN, ORC_LIGHT = 0, 3                                            # rt_oracle.h
# (case, the scene of walk_ray_cases.scene it is made from, scene options): one per kernel shape of direct.hip kDirectKernels[pick][mis], the weighted tables
CASES = (("cornell", "cornell", {}), ("prims33", "prims33", {}), ("random_spheres_lit", "random_spheres", {}), ("prims600", "prims600", {}),
         ("grid3000_lit", "grid3000", {}), ("grid3000_lit", "grid3000", dict(compact_nodes=0)))
SCENES = ("cornell", "prims33", "random_spheres_lit", "prims600", "grid3000_lit")
LAMP = ("direct_mis_lamp", ORC_LIGHT, (5.0, 4.0, 3.0), 0.0)                 # the material the varied descriptions add
# deliberately wrong restatements: wl dropped; wb dropped (the lobe hit counts in full); a virtual emitter weighted like a real one; the
# first table record's area in place of the hit's; t in place of t * t; the heuristics swapped; the lobe ray drawn on stream 1; csh from
# the hit's normal instead of the item's axis; T_l and T_b folded as two samples
MUTANTS = ("no_wl", "no_wb", "virtual_weighted", "first_area", "t_once", "swapped", "lobe_stream_1", "csh_hit_normal", "two_samples")

_vec, _arr = D._vec, D._arr
q = NM.q


def with_lights(desc):
    """The description with one material more, a light, on every fourth sphere (insertion index % 4 == 1): nothing moves."""
    geos = [(g[:-1] + (LAMP[0],)) if g[0] == "sphere" and i % 4 == 1 else g for i, g in enumerate(desc["geometries"])]
    assert sum(g[-1] == LAMP[0] for g in geos) >= 2
    return dict(desc, materials=list(desc["materials"]) + [LAMP], geometries=geos)


def lobe_ray(orc, point, axis, seed, stream, word=LOBE_WORD):
    """trt_gather's TRT_LOBE_COSINE draw about (point, axis) on RNG stream (seed, stream, word): the reference's Lambertian scatter."""
    rng = (C.c_uint32 * 2)()
    ray_in, ray, att, rec = orc.Ray(), orc.Ray(), orc.Vec3(), orc.HitRecord()
    orc.lib.orc_rng_seed(seed, stream & 0xFFFFFFFF, word, C.byref(rng))
    rec.point, rec.normal = point, axis
    ok = orc.lib.orc_material_scatter(ORC_LAMBERTIAN, orc.Vec3(1.0, 1.0, 1.0), 0.0, C.byref(ray_in), C.byref(rec), C.byref(rng), C.byref(ray), C.byref(att))
    assert ok
    return ray


def samples(orc, ow, desc, items, table, heuristic=BALANCE, k=K, seed=SEED, first_stream=FIRST_STREAM, shadow_end=SHADOW_END, plain=False,
            mutant=None, only=None, item_index=None, base=None):
    """The contract of tinyrt.h trt_direct_mis, sample by sample.  dict of arrays over [n, k]: direct_cases.samples' own (e, live, walked,
    occ, wgt, rays, t_max; `base`, where given, is that dict computed before with the same arguments) with has_l, tl [n, k, 3] and wl for
    the shadow term, lobe_rays [n, k, 6], geo (the insertion index the lobe ray hit, -1 on a miss), has_b, full (a light hit counted in
    full: csh <= 0 or q(g) not finite), wb and tb [n, k, 3] for the lobe term, and c [n, k, 3], what the sample folds (0 where it adds
    nothing).  plain=True: wl = 1 and no lobe term.  `mutant`: one of MUTANTS ("two_samples" changes fold() only)."""
    assert mutant is None or mutant in MUTANTS
    if mutant == "swapped":
        heuristic = POWER if heuristic == BALANCE else BALANCE
    if base is None:
        base = D.samples(orc, ow, items, table, k=k, seed=seed, first_stream=first_stream, shadow_end=shadow_end, only=only, item_index=item_index)
    n, E = len(items), f32(len(table))
    lib = orc.lib
    mats = P.material_table(orc, ow, desc)
    out = dict(base)
    out.update(has_l=np.zeros((n, k), bool), tl=np.zeros((n, k, 3), np.float32), wl=np.ones((n, k), np.float32),
               lobe_rays=np.zeros((n, k, 6), np.float32), geo=np.full((n, k), -1, np.int64), has_b=np.zeros((n, k), bool),
               full=np.zeros((n, k), bool), wb=np.zeros((n, k), np.float32), tb=np.zeros((n, k, 3), np.float32),
               c=np.zeros((n, k, 3), np.float32))
    with np.errstate(all="ignore"):
        for i in (range(n) if only is None else only):
            point, axis = _vec(orc, items[i, 0:3]), _vec(orc, items[i, 3:6])
            item = i if item_index is None else int(item_index[i])
            for s in range(k):
                stream = first_stream + item * k + s
                # ---- step 1: the shadow sample of direct_cases, weighted ----
                has_l = bool(base["live"][i, s] and not base["occ"][i, s])
                if has_l:
                    rec = table[base["e"][i, s]]
                    wgt = f32(base["wgt"][i, s])
                    tl = (rec["color"] * wgt).astype(np.float32)
                    assert tl.tobytes() == base["c"][i, s].tobytes()
                    virtual = rec["geometry"] == D.NO_GEOMETRY and mutant != "virtual_weighted"
                    if not (plain or virtual or mutant == "no_wl"):
                        wl = f32(1.0) / (f32(1.0) + q(wgt, heuristic))
                        assert wl.dtype == np.float32
                        tl = tl * wl
                        out["wl"][i, s] = wl
                    out["has_l"][i, s], out["tl"][i, s] = True, tl
                if plain:
                    out["c"][i, s] = out["tl"][i, s]
                    continue
                # ---- step 2: the lobe sample ----
                ray = lobe_ray(orc, point, axis, seed, stream, 1 if mutant == "lobe_stream_1" else LOBE_WORD)
                out["lobe_rays"][i, s] = np.frombuffer(bytes(ray), np.float32)
                hit, geometry = ow.hit_index(ray, D.T_MIN, float("inf"))
                if hit is not None:
                    out["geo"][i, s] = geometry
                    mkind, emission, _ = mats[hit.material]
                    if mkind == ORC_LIGHT:
                        t = f32(hit.t)
                        csh = f32(lib.orc_vec3_dot(hit.normal if mutant == "csh_hit_normal" else axis, ray.direction))
                        clh = np.abs(f32(lib.orc_vec3_dot(hit.normal, ray.direction)))
                        area = NM.area_of(table, geometry, mutant)
                        g = ((csh * clh) / (t if mutant == "t_once" else t * t)) * ((area * E) * D.INV_PI)
                        assert g.dtype == np.float32
                        qg = q(g, heuristic)
                        weighted = bool(csh > 0 and np.isfinite(qg))
                        wb = qg / (f32(1.0) + qg) if weighted and mutant != "no_wb" else f32(1.0)
                        assert wb.dtype == np.float32
                        out["has_b"][i, s], out["full"][i, s], out["wb"][i, s] = True, not weighted, wb
                        out["tb"][i, s] = _arr(emission) * wb
                # ---- step 3: what the sample folds ----
                if out["has_l"][i, s] and out["has_b"][i, s]:
                    out["c"][i, s] = out["tl"][i, s] + out["tb"][i, s]
                elif out["has_b"][i, s]:
                    out["c"][i, s] = out["tb"][i, s]
                else:
                    out["c"][i, s] = out["tl"][i, s]
    out["mutant"] = mutant
    return out


def fold(smp, k, begin=0, end=None, s=None, m=None):
    """radiance_cases.fold over what the samples fold: (radiance [n, 3], moment2 [n, 3]).  Every term is >= +0 (a live sample has
    cs > 0, a weight is in [0, 1], the fixtures' colours are positive), so a sample that adds nothing may add +0.  The mutant
    "two_samples" folds T_l and T_b one after the other."""
    if smp.get("mutant") != "two_samples":
        return R.fold(smp["c"], k, begin, end, s, m)
    both = np.stack([smp["tl"], smp["tb"]], axis=2).reshape(smp["tl"].shape[0], -1, 3)
    end = smp["tl"].shape[1] if end is None else end
    inv = f32(1.0) / f32(k)
    S = np.zeros((both.shape[0], 3), np.float32) if s is None else s.copy()
    M = np.zeros((both.shape[0], 3), np.float32) if m is None else m.copy()
    with np.errstate(all="ignore"):
        for j in range(2 * begin, 2 * end):
            S = S + both[:, j, :] * inv
            M = M + (both[:, j, :] * both[:, j, :]) * inv
    return S, M


def finish(smp, k):
    """The fold under S, M and the counters' expectations: n_samples, n_walks (trt_direct's rays) and n_rays = n_walks + one lobe ray per
    sample (trt_gather's world.hit calls at max_bounces = 1); frozen."""
    smp["S"], smp["M"] = fold(smp, k)
    smp["n_samples"] = smp["c"].shape[0] * smp["c"].shape[1]
    smp["n_walks"] = int(smp["walked"].sum())
    smp["n_rays"] = smp["n_walks"] + (0 if smp["c"].shape[1] == 0 else smp["n_samples"])
    return D.freeze(smp)


_SCENES, _REFERENCE = {}, {}


def scene(trt, orc, name):
    """case name -> description, oracle world, the 324 items, the table (direct_cases.table_of) and direct_cases.samples of them; computed
    once per process and never changed."""
    import walk_ray_cases as W
    if name not in _SCENES:
        stock = {c: b for c, b, _ in CASES}[name]
        desc = W.scene(trt, stock)
        if name != stock:
            desc = with_lights(desc)
        ow, _ = orc.world_from_description(desc)
        items, _ = GC.items_of(orc, ow, desc)
        table = D.table_of(orc, desc)
        for a in (items, table):
            a.setflags(write=False)
        _SCENES[name] = dict(desc=desc, ow=ow, items=items, table=table, base=D.freeze(D.samples(orc, ow, items, table)))
    return _SCENES[name]


def reference(trt, orc, name, **kw):
    """The restatement of trt_direct_mis over the 324 items of a case with the fixtures above; kw: samples' heuristic, plain, mutant."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _REFERENCE:
        sc = scene(trt, orc, name)
        _REFERENCE[key] = finish(samples(orc, sc["ow"], sc["desc"], sc["items"], sc["table"], base=sc["base"], **kw), K)
    return _REFERENCE[key]


def ceiling_surfels():
    """The 20 surfels of the lowered box's ceiling above its lamp: y = 100, axis down, x in 30 .. 70 step 10, z in 35 .. 65 step 10."""
    return np.array([[x, 100.0, z, 0.0, -1.0, 0.0] for x in range(30, 71, 10) for z in range(35, 66, 10)], np.float32)


def lowered_cornell(trt, orc):
    """(description, oracle world, items, the scene's own table) of the Cornell box with the lamp lowered to y = 99 (nee_cases.
    lowered_cornell): the 20 ceiling surfels, one unit above the lamp, then nee_cases' 40 floor surfels."""
    desc, ow, floor, table = N.lowered_cornell(trt, orc)
    items = np.ascontiguousarray(np.concatenate([ceiling_surfels(), floor]))
    assert items.shape == (60, 6) and (items[:20, 1] == 100.0).all()
    return desc, ow, items, table


def floor_texels(trt, desc):
    """The 20 floor surfels of the statistical tests: bake.quad_texels over the floor quad of the box, 5 x 4, the axis up."""
    kind, corner, u, v, _ = desc["geometries"][3]
    assert kind == "quad" and corner[1] == 0.0
    items = trt.bake.quad_texels(corner, u, v, 5, 4, flip=True)
    assert len(items) == 20 and (items[:, 3:6] == np.array([0.0, 1.0, 0.0], np.float32)).all()
    return items


differing = D.differing
assert_same_bits = R.assert_same_bits
