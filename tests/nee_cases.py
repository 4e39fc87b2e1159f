"""What tests/test_nee_cases.py, tests/test_nee_abi.py, tests/test_gpu_nee.py and tests/test_gpu_nee_long.py share, none of it touching a GPU:
the restatement of a next-event query (tinyrt.h trt_nee) with the CPU oracle's pieces.

nee_path is passes_cases.oracle_path - CpuSampler::single_point_sampling (cpu.rs:39-65) line by line: orc_rng_seed for stream (seed, j, 0),
World.hit over [0.001, inf), orc_material_scatter, the colour arithmetic through orc_vec3_binop - with steps 3-5 of the contract: the
hidden emission, the after_diffuse flag, and at a Lambertian vertex that leaves bounce budget the draw of direct_cases.samples (restated
here as `draw`, with the stream word as a parameter and the surfel as two vectors; tests/test_nee_cases.py pins it to direct_cases.samples
at word 1) with occlusion by ow.hit(ray, 0.001, t_max).  With next event and hiding switched off it is the oracle's own loop, which
tests/test_nee_cases.py pins byte for byte against orc.sample_batch.

Items and first rays are passes_cases.items_of / first_rays (324 items: a full run of 256 and a ragged 68), K = 8, seed 5, first_stream
1000, B = 5; the table is direct_cases.table_of (the scene's own emitters, a virtual quad, a virtual sphere); scenes and kernel shapes are
passes_cases.CASES."""
import ctypes as C

import numpy as np

import direct_cases as D
import passes_cases as P
import radiance_cases as R

f32 = np.float32
K, SEED, FIRST_STREAM, MAX_BOUNCES = P.K, P.SEED, P.FIRST_STREAM, P.MAX_BOUNCES
N_ITEMS = P.N_ITEMS
SOURCES = P.SOURCES
SPREAD = P.SPREAD
CASES, SCENES = P.CASES, P.SCENES
SHADOW_END = D.SHADOW_END
ORC_LAMBERTIAN, ORC_METAL, ORC_LIGHT = 0, 1, 3                                # rt_oracle.h
# deliberately wrong restatements: the hidden-light rule dropped; next event also at the last vertex (remain == 0); stream word 1 instead
# of 2 + d; the outward normal instead of the facing one; atten from before the albedo; after_diffuse not cleared by a metal hit
MUTANTS = ("no_hide", "nee_at_last", "word1", "outward_normal", "atten_before", "metal_keeps_diffuse")


def _vec(orc, a):
    return orc.Vec3(float(a[0]), float(a[1]), float(a[2]))


def _arr(v):
    return np.array([v.x, v.y, v.z], np.float32)


def draw(orc, ow, x, nrm, table, seed, stream, word, shadow_end=SHADOW_END, occlusion=True):
    """Steps 2-7 of tinyrt.h trt_direct for the surfel (x, nrm) (float32 [3] each) on RNG stream (seed, stream, word): (live, walked,
    occluded, c float32 [3] = colour * wgt).  direct_cases.samples' arithmetic, operator by operator."""
    lib = orc.lib
    rng = (C.c_uint32 * 2)()
    E = len(table)
    fE = f32(E)
    x, nrm = np.asarray(x, np.float32), np.asarray(nrm, np.float32)
    with np.errstate(all="ignore"):
        lib.orc_rng_seed(seed, stream & 0xFFFFFFFF, word, C.byref(rng))
        u0 = f32(lib.orc_rng_random(C.byref(rng)))
        e = min(int(u0 * fE), E - 1)
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
        scale = (rec["area"] * fE) * D.INV_PI
        wgt = ((cs * cl) / (d2 * d2)) * scale
        assert wgt.dtype == np.float32
        live = bool(cs > 0 and d2 > 0 and np.isfinite(wgt))
        ray = lib.orc_ray_new(_vec(orc, x), wv)
        t_max = np.sqrt(d2) * f32(shadow_end)
        walked = live and bool(t_max > f32(D.T_MIN))
        occ = False
        if walked and occlusion:
            occ = ow.hit(ray, D.T_MIN, float(t_max))[0] is not None
        c = (rec["color"] * wgt).astype(np.float32)
    return live, walked, occ, c


def nee_path(orc, ow, mat_table, ray6, max_bounces, background, seed, stream, emitters, shadow_end=SHADOW_END, source_is_diffuse=False,
             next_event=True, hide=True, mutant=None):
    """One sample of tinyrt.h trt_nee on streams (seed, stream, 0) and (seed, stream, 2 + d).  dict: color float32 [3], hits (world.hit
    calls, cpu.rs:48), walks (shadow walks made), lit (next-event terms added), hidden (light hits whose emission was hidden), skipped
    (Lambertian vertices whose next event remain == 0 ruled out)."""
    assert mutant is None or mutant in MUTANTS
    lib = orc.lib
    rng = (C.c_uint32 * 2)()
    lib.orc_rng_seed(seed, stream & 0xFFFFFFFF, 0, C.byref(rng))
    ray = orc.Ray(_vec(orc, ray6[0:3]), _vec(orc, ray6[3:6]))               # cpu.rs:42: the ray as given
    remain = max_bounces
    color, atten = orc.Vec3(0.0, 0.0, 0.0), orc.Vec3(1.0, 1.0, 1.0)
    bg = _vec(orc, background)
    zero = orc.Vec3(0.0, 0.0, 0.0)
    out = dict(hits=0, walks=0, lit=0, hidden=0, skipped=0)
    after_diffuse = bool(source_is_diffuse)
    new_ray, attenuation = orc.Ray(), orc.Vec3()
    while remain > 0:                                                       # cpu.rs:47
        rec, _ = ow.hit(ray, 0.001, float("inf"))                           # cpu.rs:48
        out["hits"] += 1
        if rec is None:
            color = lib.orc_vec3_binop(0, color, lib.orc_vec3_binop(2, atten, bg))                        # cpu.rs:59: never hidden
            break
        mkind, albedo, param = mat_table[rec.material]
        emission = albedo if mkind == ORC_LIGHT else zero                   # cpu.rs:49
        if mkind == ORC_LIGHT and after_diffuse and hide and mutant != "no_hide":
            emission = zero                                                 # step 3: a shadow ray has stood for this light
            out["hidden"] += 1
        color = lib.orc_vec3_binop(0, color, lib.orc_vec3_binop(2, atten, emission))                      # cpu.rs:50
        if not lib.orc_material_scatter(mkind, albedo, param, C.byref(ray), C.byref(rec), C.byref(rng), C.byref(new_ray), C.byref(attenuation)):
            assert mkind == ORC_LIGHT                                       # cpu.rs:55-57: only Light::scatter returns None
            break
        before = atten
        atten = lib.orc_vec3_binop(2, atten, attenuation)                   # cpu.rs:52
        d = max_bounces - remain                                            # scatters made before this vertex
        ray = orc.Ray(new_ray.origin, new_ray.direction)                    # cpu.rs:53
        remain -= 1                                                         # cpu.rs:54
        if mutant == "metal_keeps_diffuse" and mkind == ORC_METAL:
            pass
        else:
            after_diffuse = mkind == ORC_LAMBERTIAN                         # step 4
        if mkind == ORC_LAMBERTIAN and next_event:                          # step 5
            if remain == 0 and mutant != "nee_at_last":
                out["skipped"] += 1
                continue
            nrm = _arr(rec.normal)
            if mutant == "outward_normal" and not rec.front_face:
                nrm = -nrm
            live, walked, occ, c = draw(orc, ow, _arr(ray.origin), nrm, emitters, seed, stream, 1 if mutant == "word1" else 2 + d, shadow_end)
            out["walks"] += int(walked)
            if live and not occ:
                term = lib.orc_vec3_binop(2, before if mutant == "atten_before" else atten, _vec(orc, c))
                color = lib.orc_vec3_binop(0, color, term)
                out["lit"] += 1
    out["color"] = np.frombuffer(bytes(color), np.float32).copy()
    return out


COUNTS = ("hits", "walks", "lit", "hidden", "skipped")


def nee_paths(orc, ow, desc, rays, emitters, max_bounces=MAX_BOUNCES, background=(0.0, 0.0, 0.0), seed=SEED, first_stream=FIRST_STREAM, only=None,
              item_index=None, **kw):
    """rays float32 [n, k, 6]: sample s of item i runs on stream first_stream + i * k + s (row r is item item_index[r] of a longer batch
    where given).  dict: cols float32 [n, k, 3] and int32 [n, k] arrays hits, walks, lit, hidden, skipped.  `only`: the item indices to
    trace (the others stay 0).  kw: nee_path's shadow_end, source_is_diffuse, next_event, hide, mutant."""
    n, k = rays.shape[:2]
    mat_table = P.material_table(orc, ow, desc)
    out = dict(cols=np.zeros((n, k, 3), np.float32))
    for name in COUNTS:
        out[name] = np.zeros((n, k), np.int32)
    for i in (range(n) if only is None else only):
        item = i if item_index is None else int(item_index[i])
        for s in range(k):
            r = nee_path(orc, ow, mat_table, rays[i, s], max_bounces, background, seed, first_stream + item * k + s, emitters, **kw)
            out["cols"][i, s] = r["color"]
            for name in COUNTS:
                out[name][i, s] = r[name]
    return out


def finish(ref, k):
    """The fold (radiance_cases.fold: trt_radiance's) under S, M and the counters' expectations under n_samples, n_rays; frozen."""
    ref["S"], ref["M"] = R.fold(ref["cols"], k)
    ref["n_rays"] = int(ref["hits"].sum()) + int(ref["walks"].sum())
    ref["n_samples"] = ref["cols"].shape[0] * ref["cols"].shape[1]
    return D.freeze(ref)


_REFERENCE = {}


def scene(trt, orc, name):
    """name -> passes_cases.reference's entry (description, oracle world, background, per source items and first rays) plus the table."""
    ref = P.reference(trt, orc, name)
    if "nee_table" not in ref:
        table = D.table_of(orc, ref["desc"])
        table.setflags(write=False)
        ref["nee_table"] = table
    return ref


def reference(trt, orc, name, source, **kw):
    """The restatement of trt_nee over the 324 items of (scene, source) with the fixtures above and the table of direct_cases.table_of;
    kw as nee_paths'.  Computed once per process and never changed."""
    key = (name, source, tuple(sorted(kw.items())))
    if key not in _REFERENCE:
        sc = scene(trt, orc, name)
        _REFERENCE[key] = finish(nee_paths(orc, sc["ow"], sc["desc"], sc[source]["rays"], sc["nee_table"], background=sc["bg"], **kw), K)
    return _REFERENCE[key]


def lowered_cornell(trt, orc):
    """(description, oracle world, 40 unit floor surfels, the scene's own table) of the Cornell box with the lamp lowered to y = 99: the
    stock lamp is coplanar with the ceiling (tinyrt.h trt_direct, limit 4).  The surfels are the first 40 a bake of the floor has: the
    texel centres of bake.quad_texels over the floor quad, 8 x 5, the axis up.  (The 324 items of the other tests hold 11 unit floor
    surfels only; their ceiling surfels lie one unit from the lowered lamp, where single next-event samples weigh a thousand times the
    mean and no K a test can afford settles a z.)"""
    import walk_ray_cases as W
    desc = W.scene(trt, "cornell")
    geos = list(desc["geometries"])
    kind, corner, u, v, mat = geos[2]
    assert mat == "light" and corner[1] == 100.0
    geos[2] = (kind, (corner[0], 99.0, corner[2]), u, v, mat)
    lowered = dict(desc, geometries=geos)
    ow, _ = orc.world_from_description(lowered)
    kind, corner, u, v, _ = geos[3]
    assert kind == "quad" and corner[1] == 0.0
    items = trt.bake.quad_texels(corner, u, v, 8, 5, flip=True)
    table = D.emitters_of(orc, lowered)
    assert len(items) == 40 and (items[:, 1] == 0.0).all() and (items[:, 3:6] == np.array([0.0, 1.0, 0.0], np.float32)).all()
    assert len(table) == 1 and table["a"][0, 1] == 99.0
    return lowered, ow, items, table


differing = D.differing
assert_same_bits = R.assert_same_bits
