"""What tests/test_nee_pick_cases.py, tests/test_nee_pick_abi.py, tests/test_gpu_nee_pick.py and tests/test_gpu_nee_pick_long.py share, none of
it touching a GPU: the restatement of the next-event queries that choose their emitter through an alias table (tinyrt.h trt_nee_pick,
trt_nee_mis_pick) with the CPU oracle's pieces.

pick_path is nee_cases.nee_path's / nee_mis_cases.mis_path's loop - the same streams, World hits, orc_material_scatter and colour arithmetic
through orc_vec3_binop - written out anew with the vertex draw replaced: `draw` below is nee_cases.draw with steps 2 and 5 of trt_direct_pick
(u0, the slot, u1, the clamped alias, area / prob) over the oracle's draws on stream (seed, j, 2 + d), as direct_pick_cases.samples restates
them for stream word 1.  With mis the shadow sample is scaled by wl = 1 / (1 + q(wgt)) (1 for a virtual emitter) and a light reached after a
diffuse scatter at hit >= 2 adds emission * wb with ph = power / total_power in the builder's operations (direct_pick_cases.luminance) in the
place of 1 / E.  The product is never called.

Fixtures are nee_cases' own: 324 items, K = 8, seed 5, first_stream 1000, B = 5, the table of direct_cases.table_of (the scene's emitters, a
virtual quad, a virtual sphere: E >= 2 with unequal powers), its power table from direct_pick_cases.build, which tests/test_gpu_nee_pick.py
pins against lights.pick_table byte for byte."""
import ctypes as C

import numpy as np

import direct_cases as D
import direct_pick_cases as DP
import nee_cases as N
import nee_mis_cases as NM
import passes_cases as P
import radiance_cases as R

f32 = np.float32
K, SEED, FIRST_STREAM, MAX_BOUNCES = N.K, N.SEED, N.FIRST_STREAM, N.MAX_BOUNCES
N_ITEMS = N.N_ITEMS
SOURCES = N.SOURCES
SPREAD = N.SPREAD
CASES, SCENES = N.CASES, N.SCENES
SHADOW_END = N.SHADOW_END
BALANCE, POWER = NM.BALANCE, NM.POWER
HEURISTICS = NM.HEURISTICS
PICK_DTYPE = DP.PICK_DTYPE
# deliberately wrong restatements: the weighted hit still scales by float(E); prob of the slot in place of the chosen emitter's; u1 <= q;
# only the first vertex of a path draws through the table, later ones uniformly; wl from the uniform weight; the luminance summed in
# another parenthesisation
MUTANTS = ("hit_uses_E", "prob_of_slot", "u1_le_q", "pick_first_vertex_only", "uniform_wl", "luminance_parens")
COUNTS = NM.COUNTS + ("alias_taken",)

_vec, _arr = N._vec, N._arr
q = NM.q


def draw(orc, ow, x, nrm, table, pick, seed, stream, word, shadow_end=SHADOW_END, mutant=None, uniform=False):
    """Steps 2-7 of tinyrt.h trt_direct_pick for the surfel (x, nrm) (float32 [3] each) on RNG stream (seed, stream, word): dict(live,
    walked, occ, wgt f32, e, took_alias, wgt_uniform f32 = the weight trt_direct's step 5 would give the same point).  uniform=True: no u1 is
    drawn and the slot is the emitter, with trt_direct's scale (nee_cases.draw's sample)."""
    lib = orc.lib
    rng = (C.c_uint32 * 2)()
    E = len(table)
    fE = f32(E)
    x, nrm = np.asarray(x, np.float32), np.asarray(nrm, np.float32)
    with np.errstate(all="ignore"):
        lib.orc_rng_seed(seed, stream & 0xFFFFFFFF, word, C.byref(rng))
        # ---- step 2 ----
        u0 = f32(lib.orc_rng_random(C.byref(rng)))
        slot = min(int(u0 * fE), E - 1)
        e, took = slot, False
        if not uniform:
            u1 = f32(lib.orc_rng_random(C.byref(rng)))
            qk = f32(pick["q"][slot])
            keep = bool(u1 <= qk) if mutant == "u1_le_q" else bool(u1 < qk)   # a NaN q: False
            e = slot if keep else min(int(pick["alias"][slot]), E - 1)
            took = not keep
        rec = table[e]
        if rec["kind"] == 1:
            a = f32(lib.orc_rng_random(C.byref(rng)))
            b = f32(lib.orc_rng_random(C.byref(rng)))
            y = (rec["a"] + rec["b"] * a) + rec["c"] * b
            nl = rec["normal"]
        else:
            nl = _arr(lib.orc_random_unit_vector(C.byref(rng)))
            y = rec["a"] + nl * rec["b"][0]
        assert y.dtype == np.float32
        w = y - x
        wv, nv = _vec(orc, w), _vec(orc, nrm)
        d2 = f32(lib.orc_vec3_dot(wv, wv))
        cs = f32(lib.orc_vec3_dot(nv, wv))
        cl = np.abs(f32(lib.orc_vec3_dot(_vec(orc, nl), wv)))
        geom = (cs * cl) / (d2 * d2)
        # ---- step 5 ----
        wgt_uniform = geom * ((rec["area"] * fE) * D.INV_PI)
        if uniform:
            wgt = wgt_uniform
        else:
            p = f32(pick["prob"][slot if mutant == "prob_of_slot" else e])
            wgt = geom * ((rec["area"] / p) * D.INV_PI)
        assert wgt.dtype == np.float32
        live = bool(cs > 0 and d2 > 0 and np.isfinite(wgt))
        ray = lib.orc_ray_new(_vec(orc, x), wv)
        t_max = np.sqrt(d2) * f32(shadow_end)
        walked = live and bool(t_max > f32(D.T_MIN))
        occ = False
        if walked:
            occ = ow.hit(ray, D.T_MIN, float(t_max))[0] is not None
    return dict(live=live, walked=walked, occ=occ, wgt=wgt, e=e, took_alias=took, wgt_uniform=wgt_uniform)


def pick_path(orc, ow, mat_table, ray6, max_bounces, background, seed, stream, emitters, pick, total_power=None, heuristic=None,
              shadow_end=SHADOW_END, source_is_diffuse=False, mutant=None, ph_out=None):
    """One sample of tinyrt.h trt_nee_pick (heuristic None) or trt_nee_mis_pick (BALANCE / POWER, with total_power) on streams (seed,
    stream, 0) and (seed, stream, 2 + d).  dict: color float32 [3] and COUNTS.  ph_out: a list that takes (geometry, ph as uint32, g as uint32) of
    every weighted hit."""
    assert mutant is None or mutant in MUTANTS
    mis = heuristic is not None
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
    total = f32(total_power) if mis else None
    csh = f32(0.0)
    hit_no = 0
    first_vertex = True
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
                emission = zero                                             # trt_nee's step 3
                out["hidden"] += 1
            color = lib.orc_vec3_binop(0, color, lib.orc_vec3_binop(2, atten, emission))                  # cpu.rs:50
            if hidden and hit_no == 1:
                out["first_hidden"] += 1                                    # hidden in full, weighted or not
            elif hidden and mis:
                t = f32(rec.t)
                clh = np.abs(f32(lib.orc_vec3_dot(rec.normal, ray.direction)))
                area = NM.area_of(emitters, geometry)
                em = _arr(albedo)
                ph = (DP.luminance(em, mutant) * area) / total              # the builder's operations: power / total
                g = ((csh * clh) / (t * t)) * ((area * E if mutant == "hit_uses_E" else area / ph) * D.INV_PI)
                assert g.dtype == np.float32
                qg = q(g, heuristic)
                wb = qg / (f32(1.0) + qg) if bool(csh > 0 and np.isfinite(qg)) else f32(1.0)
                assert wb.dtype == np.float32
                color = lib.orc_vec3_binop(0, color, lib.orc_vec3_binop(2, atten, _vec(orc, em * wb)))
                out["weighted"] += 1
                if ph_out is not None:
                    ph_out.append((int(geometry), int(np.array([ph], np.float32).view(np.uint32)[0]), int(np.array([g], np.float32).view(np.uint32)[0])))
            if not lib.orc_material_scatter(mkind, albedo, param, C.byref(ray), C.byref(rec), C.byref(rng), C.byref(new_ray), C.byref(attenuation)):
                assert mkind == N.ORC_LIGHT                                 # cpu.rs:55-57: only Light::scatter returns None
                break
            atten = lib.orc_vec3_binop(2, atten, attenuation)               # cpu.rs:52
            d = max_bounces - remain                                        # scatters made before this vertex
            ray = orc.Ray(new_ray.origin, new_ray.direction)                # cpu.rs:53
            remain -= 1                                                     # cpu.rs:54
            after_diffuse = mkind == N.ORC_LAMBERTIAN                       # trt_nee's step 4
            if mkind == N.ORC_LAMBERTIAN:
                nrm = _arr(rec.normal)
                csh = f32(lib.orc_vec3_dot(rec.normal, ray.direction))
                if remain == 0:                                             # trt_nee's step 5: the last vertex draws nothing
                    out["skipped"] += 1
                    continue
                uniform = mutant == "pick_first_vertex_only" and not first_vertex
                first_vertex = False
                smp = draw(orc, ow, _arr(ray.origin), nrm, emitters, pick, seed, stream, 2 + d, shadow_end, mutant, uniform)
                out["walks"] += int(smp["walked"])
                out["alias_taken"] += int(smp["took_alias"])
                if smp["live"] and not smp["occ"]:
                    rec_e = emitters[smp["e"]]
                    c = (rec_e["color"] * smp["wgt"]).astype(np.float32)
                    if mis and rec_e["geometry"] != D.NO_GEOMETRY:
                        wl = f32(1.0) / (f32(1.0) + q(smp["wgt_uniform"] if mutant == "uniform_wl" else smp["wgt"], heuristic))
                        assert wl.dtype == np.float32
                        c = c * wl
                    color = lib.orc_vec3_binop(0, color, lib.orc_vec3_binop(2, atten, _vec(orc, c)))
                    out["lit"] += 1
    out["color"] = np.frombuffer(bytes(color), np.float32).copy()
    return out


def pick_paths(orc, ow, desc, rays, emitters, pick, max_bounces=MAX_BOUNCES, background=(0.0, 0.0, 0.0), seed=SEED, first_stream=FIRST_STREAM,
               only=None, item_index=None, **kw):
    """nee_cases.nee_paths for pick_path: cols float32 [n, k, 3], int32 [n, k] arrays of COUNTS and ph, the list of (geometry, ph bits, g bits) of
    every weighted hit.  kw: pick_path's total_power, heuristic, shadow_end, source_is_diffuse, mutant."""
    n, k = rays.shape[:2]
    mat_table = P.material_table(orc, ow, desc)
    out = dict(cols=np.zeros((n, k, 3), np.float32))
    for name in COUNTS:
        out[name] = np.zeros((n, k), np.int32)
    ph = []
    for i in (range(n) if only is None else only):
        item = i if item_index is None else int(item_index[i])
        for s in range(k):
            r = pick_path(orc, ow, mat_table, rays[i, s], max_bounces, background, seed, first_stream + item * k + s, emitters, pick, ph_out=ph, **kw)
            out["cols"][i, s] = r["color"]
            for name in COUNTS:
                out[name][i, s] = r[name]
    out["ph"] = np.array(ph, np.int64).reshape(-1, 3)
    return out


finish = N.finish
_REFERENCE = {}


def scene(trt, orc, name):
    """nee_cases.scene's entry plus the power table of its emitter table: nee_pick (records) and nee_total."""
    ref = N.scene(trt, orc, name)
    if "nee_pick" not in ref:
        pick, total = DP.build(ref["nee_table"])
        pick.setflags(write=False)
        ref["nee_pick"], ref["nee_total"] = pick, total
    return ref


def reference(trt, orc, name, source, pick=None, **kw):
    """The restatement of trt_nee_pick (no heuristic) or trt_nee_mis_pick over the 324 items of (scene, source) with nee_cases' fixtures
    and the scene's power table, or `pick` (records used as given; the total stays the power table's); kw as pick_paths'.  Computed once
    per process and never changed."""
    key = (name, source, None if pick is None else pick.tobytes(), tuple(sorted(kw.items())))
    if key not in _REFERENCE:
        sc = scene(trt, orc, name)
        if kw.get("heuristic") is not None:
            kw = dict(kw, total_power=sc["nee_total"])
        _REFERENCE[key] = finish(pick_paths(orc, sc["ow"], sc["desc"], sc[source]["rays"], sc["nee_table"], sc["nee_pick"] if pick is None else pick,
                                            background=sc["bg"], **kw), K)
    return _REFERENCE[key]


def first_rays(orc, items, k, seed=SEED, first_stream=FIRST_STREAM):
    """The cosine source's first rays [n, k, 6] of surfels, as gather_cases draws them (stream (seed, j, 1))."""
    import gather_cases as GC
    return GC.first_rays(orc, items, "cosine", k, SPREAD, seed, first_stream)


differing = N.differing
assert_same_bits = R.assert_same_bits
