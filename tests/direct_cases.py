"""What tests/test_direct_abi.py, tests/test_direct_cases.py, tests/test_gpu_direct.py and tests/test_gpu_direct_long.py share, none of it
touching a GPU: the restatement of a direct-light query (tinyrt.h trt_direct) with the CPU oracle's pieces.

The draws are the oracle's (orc_rng_seed on stream (seed, j, 1), orc_rng_random, orc_random_unit_vector), the arithmetic is numpy float32
scalars - one IEEE operation per operator - with orc_vec3_dot for the dot products and orc_ray_new for the two normalisations, occlusion
is the oracle's World.hit over [0.001, t_max) (ow.hit), and the fold is radiance_cases.fold over colours that are 0 where a sample adds
nothing: every sum of the tests starts at +0 or at a sum of non-negative terms, to which adding +0 changes no bit.

Items are gather_cases.items_of: 324 surfels, one full run of 256 and a ragged one of 68, with the NaN, zero, inf and 1e-9 items.  K = 8,
seed 5, first_stream 1000.  The table of a scene is its own emitters (emitters_of: the restatement of trt_scene_emitters from the scene's
description) followed by two virtual ones, a quad above the scenes and a small sphere inside them."""
import ctypes as C

import numpy as np

import gather_cases as GC
import radiance_cases as R

f32 = np.float32
K, SEED, FIRST_STREAM = GC.K, GC.SEED, GC.FIRST_STREAM
N_ITEMS = GC.N_ITEMS
SHADOW_END = f32(0.999)
T_MIN = 0.001
INV_PI = f32(0.318309886)
FOUR_PI = f32(12.566371)
LIGHT = 3                                                                   # tinyrt.h TRT_LIGHT
NO_GEOMETRY = 0xFFFFFFFF
# tinyrt.h trt_emitter (80 bytes)
EMITTER_DTYPE = np.dtype([("kind", np.uint32), ("geometry", np.uint32), ("a", np.float32, (3,)), ("b", np.float32, (3,)), ("c", np.float32, (3,)),
                          ("normal", np.float32, (3,)), ("color", np.float32, (3,)), ("area", np.float32), ("reserved", np.uint32, (2,))])
assert EMITTER_DTYPE.itemsize == 80
VIRTUAL_QUAD = dict(corner=(-20.0, 60.0, -20.0), u=(40.0, 0.0, 0.0), v=(0.0, 0.0, 40.0), color=(4.0, 3.0, 2.0))
VIRTUAL_SPHERE = dict(centre=(5.0, 8.0, -5.0), radius=2.0, color=(9.0, 9.0, 12.0))
MUTANTS = ("no_abs_cl", "no_E", "swap_ab", "word0", "d2_once")


def _vec(orc, a):
    return orc.Vec3(float(a[0]), float(a[1]), float(a[2]))


def _arr(v):
    return np.array([v.x, v.y, v.z], np.float32)


def quad_record(orc, corner, u, v, color, geometry=NO_GEOMETRY):
    """trt_emitter_init_quad restated: cross and length in float32 scalars, the unit normal as orc_ray_new makes it."""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        cross = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], np.float32)
        area = np.sqrt((cross[0] * cross[0] + cross[1] * cross[1]) + cross[2] * cross[2])
    normal = _arr(orc.lib.orc_ray_new(orc.Vec3(0.0, 0.0, 0.0), _vec(orc, cross)).direction)
    e = np.zeros(1, EMITTER_DTYPE)
    e["kind"], e["geometry"], e["a"], e["b"], e["c"], e["normal"], e["color"], e["area"] = 1, geometry, np.asarray(corner, np.float32), u, v, normal, \
        np.asarray(color, np.float32), area
    assert area.dtype == np.float32
    return e


def sphere_record(centre, radius, color, geometry=NO_GEOMETRY):
    """trt_emitter_init_sphere restated."""
    r = f32(radius)
    e = np.zeros(1, EMITTER_DTYPE)
    with np.errstate(all="ignore"):
        area = FOUR_PI * (r * r)
    e["kind"], e["geometry"], e["a"], e["b"], e["color"], e["area"] = 0, geometry, np.asarray(centre, np.float32), (r, 0.0, 0.0), \
        np.asarray(color, np.float32), area
    assert area.dtype == np.float32
    return e


def emitters_of(orc, desc):
    """trt_scene_emitters restated from the description: the geometries whose material is a light, in insertion order."""
    mats = {name: (kind, albedo) for name, kind, albedo, _ in desc["materials"]}
    out = [np.zeros(0, EMITTER_DTYPE)]
    for g, geo in enumerate(desc["geometries"]):
        kind, color = mats[geo[-1]]
        if kind != LIGHT:
            continue
        if geo[0] == "quad":
            out.append(quad_record(orc, geo[1], geo[2], geo[3], color, g))
        else:
            out.append(sphere_record(geo[1], geo[2], color, g))
    return np.concatenate(out)


def virtual_emitters(orc):
    return np.concatenate([quad_record(orc, **VIRTUAL_QUAD), sphere_record(**VIRTUAL_SPHERE)])


def table_of(orc, desc):
    """The table of the tests: the scene's own emitters, then the virtual quad, then the virtual sphere."""
    return np.ascontiguousarray(np.concatenate([emitters_of(orc, desc), virtual_emitters(orc)]))


def samples(orc, ow, items, table, k=K, seed=SEED, first_stream=FIRST_STREAM, shadow_end=SHADOW_END, mutant=None, only=None, occlusion=True,
            item_index=None):
    """The contract of tinyrt.h trt_direct, sample by sample.  dict of arrays over [n, k]: e (emitter chosen), live, walked (live and
    t_max > 0.001), occ (the oracle's World.hit over [0.001, t_max); False where not walked), rays [n, k, 6], t_max, and c [n, k, 3] -
    colour * wgt where the sample is live and unoccluded, 0 where it adds nothing.  `only`: the item indices to work on (the others stay
    0).  `item_index`: row r of `items` is item item_index[r] of a longer batch (its streams are first_stream + item_index[r] * k + s).
    `mutant`: one of MUTANTS, a deliberately wrong restatement.  occlusion=False leaves occ False and c as if nothing occluded."""
    assert mutant is None or mutant in MUTANTS
    n, E = len(items), len(table)
    shadow_end = f32(shadow_end)
    out = dict(e=np.zeros((n, k), np.int64), live=np.zeros((n, k), bool), walked=np.zeros((n, k), bool), occ=np.zeros((n, k), bool),
               rays=np.zeros((n, k, 6), np.float32), t_max=np.zeros((n, k), np.float32), c=np.zeros((n, k, 3), np.float32),
               wgt=np.zeros((n, k), np.float32))
    rng = (C.c_uint32 * 2)()
    lib = orc.lib
    fE = f32(E)
    with np.errstate(all="ignore"):
        for i in (range(n) if only is None else only):
            x, nrm = _vec(orc, items[i, 0:3]), _vec(orc, items[i, 3:6])
            item = i if item_index is None else int(item_index[i])
            for s in range(k):
                lib.orc_rng_seed(seed, (first_stream + item * k + s) & 0xFFFFFFFF, 0 if mutant == "word0" else 1, C.byref(rng))
                u0 = f32(lib.orc_rng_random(C.byref(rng)))
                e = min(int(u0 * fE), E - 1)
                rec = table[e]
                if rec["kind"] == 1:
                    a = f32(lib.orc_rng_random(C.byref(rng)))
                    b = f32(lib.orc_rng_random(C.byref(rng)))
                    if mutant == "swap_ab":
                        a, b = b, a
                    y = (rec["a"] + rec["b"] * a) + rec["c"] * b
                    nl = rec["normal"]
                else:
                    nl = _arr(lib.orc_random_unit_vector(C.byref(rng)))
                    y = rec["a"] + nl * rec["b"][0]
                assert y.dtype == np.float32
                w = y - items[i, 0:3]
                wv = _vec(orc, w)
                d2 = f32(lib.orc_vec3_dot(wv, wv))
                cs = f32(lib.orc_vec3_dot(nrm, wv))
                cl = f32(lib.orc_vec3_dot(_vec(orc, nl), wv))
                if mutant != "no_abs_cl":
                    cl = np.abs(cl)
                scale = (rec["area"] if mutant == "no_E" else rec["area"] * fE) * INV_PI
                geom = (cs * cl) / (d2 if mutant == "d2_once" else d2 * d2)
                wgt = geom * scale
                assert wgt.dtype == np.float32
                live = bool(cs > 0 and d2 > 0 and np.isfinite(wgt))
                ray = lib.orc_ray_new(x, wv)
                t_max = np.sqrt(d2) * shadow_end
                walked = live and bool(t_max > f32(T_MIN))
                occ = False
                if walked and occlusion:
                    occ = ow.hit(ray, T_MIN, float(t_max))[0] is not None
                out["e"][i, s], out["live"][i, s], out["walked"][i, s], out["occ"][i, s] = e, live, walked, occ
                out["rays"][i, s] = np.frombuffer(bytes(ray), np.float32)
                out["t_max"][i, s] = t_max
                out["wgt"][i, s] = wgt
                if live and not occ:
                    out["c"][i, s] = rec["color"] * wgt
    return out


def fold(smp, k, begin=0, end=None, s=None, m=None):
    """radiance_cases.fold over the samples' colours: (radiance [n, 3], moment2 [n, 3])."""
    return R.fold(smp["c"], k, begin, end, s, m)


def reference(orc, ow, items, table, **kw):
    """samples() with its fold under S, M and the walk count under n_walks."""
    smp = samples(orc, ow, items, table, **kw)
    smp["S"], smp["M"] = fold(smp, kw.get("k", K))
    smp["n_walks"] = int(smp["walked"].sum())
    return smp


def freeze(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def differing(a, b):
    """Items whose bits differ."""
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum())


assert_same_bits = R.assert_same_bits
