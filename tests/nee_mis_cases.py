"""What tests/test_nee_mis_cases.py, tests/test_nee_mis_abi.py, tests/test_gpu_nee_mis.py and tests/test_gpu_nee_mis_long.py share, none of it
touching a GPU: the restatement of a weighted next-event query (tinyrt.h trt_nee_mis) with the CPU oracle's pieces.

mis_path is nee_cases.nee_path's loop - the same streams, World hits, orc_material_scatter, colour arithmetic through orc_vec3_binop and
the draw of nee_cases.draw - with the contract's two changes: a live, unoccluded shadow sample is scaled by wl = 1 / (1 + q(wgt)) (1 for a
virtual emitter), and a light the path reaches after a diffuse scatter at hit >= 2 adds emission * wb, wb = q(g) / (1 + q(g)), where
nee_path adds nothing.  The hit's geometry is World.hit_index's insertion index, its area the table record's with that `geometry` word.
wgt comes out of nee_cases.draw itself: drawn against a copy of the table whose colours are 1, c = 1 * wgt is wgt, bit for bit.  With
wb = 0 and wl = 1 forced (plain=True) the loop is nee_path's, which tests/test_nee_mis_cases.py pins byte for byte.

Fixtures are nee_cases' own: 324 items, K = 8, seed 5, first_stream 1000, B = 5, the table of direct_cases.table_of (the scene's emitters, a
virtual quad, a virtual sphere: the wl = 1 rule runs), scenes and kernel shapes of passes_cases.CASES."""
import ctypes as C

import numpy as np

import direct_cases as D
import nee_cases as N
import passes_cases as P
import radiance_cases as R

f32 = np.float32
K, SEED, FIRST_STREAM, MAX_BOUNCES = N.K, N.SEED, N.FIRST_STREAM, N.MAX_BOUNCES
N_ITEMS = N.N_ITEMS
SOURCES = N.SOURCES
SPREAD = N.SPREAD
CASES, SCENES = N.CASES, N.SCENES
SHADOW_END = N.SHADOW_END
BALANCE, POWER = 0, 1                                                         # tinyrt.h enum trt_mis_heuristic
HEURISTICS = {"balance": BALANCE, "power": POWER}
# deliberately wrong restatements: wb dropped (pure hiding); wl dropped; a virtual emitter weighted like a real one; the first table
# record's area in place of the hit's; csh from the outward normal; the heuristics swapped; the first hit weighted instead of hidden under
# source_is_diffuse; t in place of t * t
MUTANTS = ("no_wb", "no_wl", "virtual_weighted", "first_area", "csh_outward", "swapped", "first_hit_weighted", "t_once")
COUNTS = N.COUNTS + ("weighted", "first_hidden")

_vec, _arr = N._vec, N._arr


def q(x, heuristic):
    return x * x if heuristic == POWER else x


def unit_colours(table):
    """The table with every colour 1: nee_cases.draw's c against it is wgt itself."""
    t = table.copy()
    t["color"] = 1.0
    return t


def area_of(table, geometry, mutant=None):
    """The area of the table record whose `geometry` word is the hit's insertion index (the table rule: there is exactly one)."""
    if mutant == "first_area":
        return f32(table["area"][0])
    rows = np.nonzero(table["geometry"] == np.uint32(geometry))[0]
    assert len(rows) == 1, ("the table rule", geometry)
    return f32(table["area"][rows[0]])


def mis_path(orc, ow, mat_table, ray6, max_bounces, background, seed, stream, emitters, units, heuristic=BALANCE, shadow_end=SHADOW_END,
             source_is_diffuse=False, plain=False, mutant=None):
    """One sample of tinyrt.h trt_nee_mis on streams (seed, stream, 0) and (seed, stream, 2 + d).  `units`: unit_colours(emitters).
    dict: color float32 [3] and nee_cases.nee_path's counts, plus weighted (light hits at hit >= 2 that got a wb) and first_hidden (light
    hits at hit 1 hidden in full).  plain=True forces wb = 0 and wl = 1: trt_nee's contract."""
    assert mutant is None or mutant in MUTANTS
    if mutant == "swapped":
        heuristic = POWER if heuristic == BALANCE else BALANCE
    lib = orc.lib
    rng = (C.c_uint32 * 2)()
    lib.orc_rng_seed(seed, stream & 0xFFFFFFFF, 0, C.byref(rng))
    ray = orc.Ray(_vec(orc, ray6[0:3]), _vec(orc, ray6[3:6]))               # cpu.rs:42: the ray as given
    remain = max_bounces
    color, atten = orc.Vec3(0.0, 0.0, 0.0), orc.Vec3(1.0, 1.0, 1.0)
    bg = _vec(orc, background)
    zero = orc.Vec3(0.0, 0.0, 0.0)
    out = dict.fromkeys(COUNTS, 0)
    after_diffuse = bool(source_is_diffuse)
    new_ray, attenuation = orc.Ray(), orc.Vec3()
    E = f32(len(emitters))
    csh = f32(0.0)
    hit_no = 0
    with np.errstate(all="ignore"):
        while remain > 0:                                                   # cpu.rs:47
            rec, geometry = ow.hit_index(ray, 0.001, float("inf"))          # cpu.rs:48
            out["hits"] += 1
            hit_no += 1
            if rec is None:
                color = lib.orc_vec3_binop(0, color, lib.orc_vec3_binop(2, atten, bg))                    # cpu.rs:59: never hidden
                break
            mkind, albedo, param = mat_table[rec.material]
            emission = albedo if mkind == N.ORC_LIGHT else zero             # cpu.rs:49
            hidden = mkind == N.ORC_LIGHT and after_diffuse
            if hidden:
                emission = zero                                             # step 3: the two strategies share this light
                out["hidden"] += 1
            color = lib.orc_vec3_binop(0, color, lib.orc_vec3_binop(2, atten, emission))                  # cpu.rs:50
            if hidden and hit_no == 1 and mutant != "first_hit_weighted":
                out["first_hidden"] += 1                                    # hidden in full: trt_direct has no weights
            elif hidden and not plain and mutant != "no_wb":
                t = f32(rec.t)
                clh = np.abs(f32(lib.orc_vec3_dot(rec.normal, ray.direction)))
                area = area_of(emitters, geometry, mutant)
                g = ((csh * clh) / (t if mutant == "t_once" else t * t)) * ((area * E) * D.INV_PI)
                assert g.dtype == np.float32
                qg = q(g, heuristic)
                wb = qg / (f32(1.0) + qg) if bool(csh > 0 and np.isfinite(qg)) else f32(1.0)
                assert wb.dtype == np.float32
                weighted = _vec(orc, _arr(albedo) * wb)
                color = lib.orc_vec3_binop(0, color, lib.orc_vec3_binop(2, atten, weighted))
                out["weighted"] += 1
            if not lib.orc_material_scatter(mkind, albedo, param, C.byref(ray), C.byref(rec), C.byref(rng), C.byref(new_ray), C.byref(attenuation)):
                assert mkind == N.ORC_LIGHT                                 # cpu.rs:55-57: only Light::scatter returns None
                break
            atten = lib.orc_vec3_binop(2, atten, attenuation)               # cpu.rs:52
            d = max_bounces - remain                                        # scatters made before this vertex
            ray = orc.Ray(new_ray.origin, new_ray.direction)                # cpu.rs:53
            remain -= 1                                                     # cpu.rs:54
            after_diffuse = mkind == N.ORC_LAMBERTIAN                       # step 4
            if mkind == N.ORC_LAMBERTIAN:
                nrm = _arr(rec.normal)
                facing = rec.normal
                if mutant == "csh_outward" and not rec.front_face:
                    facing = _vec(orc, -nrm)
                csh = f32(lib.orc_vec3_dot(facing, ray.direction))
                if remain == 0:                                             # step 5
                    out["skipped"] += 1
                    continue
                x = _arr(ray.origin)
                live, walked, occ, w3 = N.draw(orc, ow, x, nrm, units, seed, stream, 2 + d, shadow_end)
                out["walks"] += int(walked)
                if live and not occ:
                    u0 = _first_draw(lib, seed, stream, 2 + d)
                    e = min(int(u0 * E), len(emitters) - 1)
                    rec_e = emitters[e]
                    wgt = f32(w3[0])
                    c = (rec_e["color"] * wgt).astype(np.float32)
                    virtual = rec_e["geometry"] == D.NO_GEOMETRY and mutant != "virtual_weighted"
                    if not (plain or mutant == "no_wl" or virtual):
                        wl = f32(1.0) / (f32(1.0) + q(wgt, heuristic))
                        assert wl.dtype == np.float32
                        c = c * wl
                    color = lib.orc_vec3_binop(0, color, lib.orc_vec3_binop(2, atten, _vec(orc, c)))
                    out["lit"] += 1
    out["color"] = np.frombuffer(bytes(color), np.float32).copy()
    return out


def _first_draw(lib, seed, stream, word):
    """u0 of trt_direct's step 2 on stream (seed, stream, word): which record nee_cases.draw chose."""
    rng = (C.c_uint32 * 2)()
    lib.orc_rng_seed(seed, stream & 0xFFFFFFFF, word, C.byref(rng))
    return f32(lib.orc_rng_random(C.byref(rng)))


def mis_paths(orc, ow, desc, rays, emitters, max_bounces=MAX_BOUNCES, background=(0.0, 0.0, 0.0), seed=SEED, first_stream=FIRST_STREAM, only=None,
              item_index=None, **kw):
    """nee_cases.nee_paths for mis_path: cols float32 [n, k, 3] and int32 [n, k] arrays of COUNTS.  kw: mis_path's heuristic, shadow_end,
    source_is_diffuse, plain, mutant."""
    n, k = rays.shape[:2]
    mat_table = P.material_table(orc, ow, desc)
    units = unit_colours(emitters)
    out = dict(cols=np.zeros((n, k, 3), np.float32))
    for name in COUNTS:
        out[name] = np.zeros((n, k), np.int32)
    for i in (range(n) if only is None else only):
        item = i if item_index is None else int(item_index[i])
        for s in range(k):
            r = mis_path(orc, ow, mat_table, rays[i, s], max_bounces, background, seed, first_stream + item * k + s, emitters, units, **kw)
            out["cols"][i, s] = r["color"]
            for name in COUNTS:
                out[name][i, s] = r[name]
    return out


finish = N.finish
scene = N.scene
_REFERENCE = {}


def reference(trt, orc, name, source, **kw):
    """The restatement of trt_nee_mis over the 324 items of (scene, source) with nee_cases' fixtures and table; kw as mis_paths'.  Computed
    once per process and never changed."""
    key = (name, source, tuple(sorted(kw.items())))
    if key not in _REFERENCE:
        sc = scene(trt, orc, name)
        _REFERENCE[key] = finish(mis_paths(orc, sc["ow"], sc["desc"], sc[source]["rays"], sc["nee_table"], background=sc["bg"], **kw), K)
    return _REFERENCE[key]


lowered_cornell = N.lowered_cornell
differing = N.differing
assert_same_bits = R.assert_same_bits
