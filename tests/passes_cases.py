"""What tests/test_passes_cases.py, tests/test_gpu_passes.py and tests/test_gpu_passes_long.py share, none of it touching a GPU: the oracle's
restatement of one sample's path WITH its class (tinyrt.h trt_passes) and the fold in numpy float32.

oracle_paths restates CpuSampler::single_point_sampling (cpu.rs:39-65) line by line from the oracle's pieces - orc_rng_seed for stream
(seed, j, 0), World.hit over [0.001, inf), orc_material_scatter with the scene description's material table, the colour arithmetic through
orc_vec3_binop, so every product and sum is the oracle's f32 - and says which line ended the path: `break` after Light::scatter returned
None (LIGHT), the miss branch (SKY) or the loop condition (SPENT), after how many scatters, and how often world.hit was called.
tests/test_passes_cases.py pins it to the oracle's own loop (orc.sample_batch): the colours byte for byte, the calls by their count.

First rays: gather_cases.first_rays (cosine, cone), radiance_cases.rays_of (rays)."""
import ctypes as C

import numpy as np

import gather_cases as GC
import radiance_cases as R

f32 = np.float32
K, SEED, FIRST_STREAM = R.K, R.SEED, R.FIRST_STREAM
MAX_BOUNCES = 5
N_ITEMS = GC.N_ITEMS
SOURCES = ("rays", "cosine", "cone")
SPREAD = GC.SPREAD
LIGHT, SKY, SPENT = 0, 1, 2
ORC_METAL, ORC_LIGHT = 1, 3                                                 # rt_oracle.h
BINS = (1, 2, 3, 4)


def _vec(orc, a):
    return orc.Vec3(float(a[0]), float(a[1]), float(a[2]))


def material_table(orc, ow, desc):
    """World material index -> (kind, albedo Vec3, param): what World::add_material stored (Metal::new clamps its fuzz, metal.rs:12-14)."""
    table = {}
    for name, kind, albedo, param in desc["materials"]:
        p = float(f32(param))
        if kind == ORC_METAL:
            p = min(max(p, 0.0), 1.0)
        table[ow.get_material(name)] = (int(kind), orc.Vec3(*albedo), p)
    return table


def oracle_path(orc, ow, table, ray6, max_bounces, background, seed, stream):
    """cpu.rs:39-65 for one sample on RNG stream (seed, stream, 0): (colour float32 [3], kind, scatters before the end, world.hit calls)."""
    rng = (C.c_uint32 * 2)()
    orc.lib.orc_rng_seed(seed, stream & 0xFFFFFFFF, 0, C.byref(rng))
    ray = orc.Ray(_vec(orc, ray6[0:3]), _vec(orc, ray6[3:6]))               # cpu.rs:42: the ray as given
    remain = max_bounces
    color, atten = orc.Vec3(0.0, 0.0, 0.0), orc.Vec3(1.0, 1.0, 1.0)
    bg = _vec(orc, background)
    zero = orc.Vec3(0.0, 0.0, 0.0)
    kind, hits = SPENT, 0
    new_ray, attenuation = orc.Ray(), orc.Vec3()
    while remain > 0:                                                       # cpu.rs:47
        rec, _ = ow.hit(ray, 0.001, float("inf"))                           # cpu.rs:48
        hits += 1
        if rec is not None:
            mkind, albedo, param = table[rec.material]
            emission = albedo if mkind == ORC_LIGHT else zero               # cpu.rs:49
            color = orc.lib.orc_vec3_binop(0, color, orc.lib.orc_vec3_binop(2, atten, emission))          # cpu.rs:50
            if orc.lib.orc_material_scatter(mkind, albedo, param, C.byref(ray), C.byref(rec), C.byref(rng), C.byref(new_ray), C.byref(attenuation)):
                atten = orc.lib.orc_vec3_binop(2, atten, attenuation)       # cpu.rs:52
                ray = orc.Ray(new_ray.origin, new_ray.direction)            # cpu.rs:53
                remain -= 1                                                 # cpu.rs:54
            else:
                kind = LIGHT                                                # cpu.rs:55-57: only Light::scatter returns None
                assert mkind == ORC_LIGHT
                break
        else:
            color = orc.lib.orc_vec3_binop(0, color, orc.lib.orc_vec3_binop(2, atten, bg))                # cpu.rs:59
            kind = SKY
            break
    return np.frombuffer(bytes(color), np.float32).copy(), kind, max_bounces - remain, hits


def oracle_paths(orc, ow, desc, rays, max_bounces, background, seed, first_stream, only=None):
    """rays float32 [n, k, 6]: sample s of item i runs on stream first_stream + i * k + s.  (colours float32 [n, k, 3], kinds int8 [n, k],
    depths int32 [n, k], world.hit calls of all of them).  `only`: the item indices to trace (the others stay 0)."""
    n, k = rays.shape[:2]
    table = material_table(orc, ow, desc)
    cols, kinds, depths = np.zeros((n, k, 3), np.float32), np.zeros((n, k), np.int8), np.zeros((n, k), np.int32)
    hits = 0
    for i in (range(n) if only is None else only):
        for s in range(k):
            cols[i, s], kinds[i, s], depths[i, s], h = oracle_path(orc, ow, table, rays[i, s], max_bounces, background, seed, first_stream + i * k + s)
            hits += h
    return cols, kinds, depths, hits


def first_rays(orc, desc, items, source, k=K, seed=SEED, first_stream=FIRST_STREAM, only=None):
    """float32 [n, k, 6]: the first ray of sample s of item i - the item itself for "rays", gather_cases.first_rays for the lobes."""
    assert source in SOURCES
    if source == "rays":
        return np.ascontiguousarray(np.repeat(items[:, None, :], k, axis=1))
    return GC.first_rays(orc, items, source, k, SPREAD, seed, first_stream, only)


def slots_of(kinds, depths, bins):
    """int32 [n, k]: the slot of every sample - min(d, B - 1) for LIGHT, B + min(d, B - 1) for SKY, -1 for SPENT."""
    b = np.minimum(depths, bins - 1)
    return np.where(kinds == LIGHT, b, np.where(kinds == SKY, bins + b, -1)).astype(np.int32)


def fold(cols, kinds, depths, k, bins, begin=0, end=None, passes=None, spent=None):
    """tinyrt.h trt_passes: passes[i][slot].ch = passes[i][slot].ch + c.ch * inv_K, spent[i] = spent[i] + inv_K (SPENT) over samples
    [begin, end) in order, from (passes, spent) or from 0, all float32.  A sample changes its own slot only: the others are not added 0
    to, they are left."""
    n = cols.shape[0]
    end = cols.shape[1] if end is None else end
    inv = f32(1.0) / f32(k)
    P = np.zeros((n, 2 * bins, 3), np.float32) if passes is None else passes.copy()
    S = np.zeros(n, np.float32) if spent is None else spent.copy()
    slots = slots_of(kinds, depths, bins)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        for s in range(begin, end):
            t = cols[:, s, :] * inv
            live = slots[:, s] >= 0
            r, sl = rows[live], slots[live, s]
            P[r, sl] = P[r, sl] + t[live]                                   # one row per item: no index repeats
            S = np.where(live, S, S + inv)
    assert P.dtype == np.float32 and S.dtype == np.float32
    return P, S


def fold_one_item(cols, kinds, depths, k, bins):
    """The same fold for one item written out scalar by scalar (cols [k, 3], kinds [k], depths [k])."""
    inv = f32(1.0) / f32(k)
    P = [[f32(0.0)] * 3 for _ in range(2 * bins)]
    S = f32(0.0)
    for s in range(len(cols)):
        if kinds[s] == SPENT:
            S = f32(S + inv)
            continue
        b = min(int(depths[s]), bins - 1)
        slot = b if kinds[s] == LIGHT else bins + b
        for ch in range(3):
            P[slot][ch] = f32(P[slot][ch] + f32(f32(cols[s, ch]) * inv))
    return np.array(P, np.float32), S


def items_of(orc, ow, desc, source):
    """The 324 items of a scene: radiance_cases.rays_of for "rays", gather_cases.items_of for the lobes."""
    return R.rays_of(desc) if source == "rays" else GC.items_of(orc, ow, desc)[0]


# One scene per kernel shape of passes.hip (test_gpu_queries.DEFAULT_SHAPES and, for the register-slot walk from global memory, its
# OTHER_WALKS entry): (scene, scene options).  tests/test_gpu_passes.py asserts the shape of each.
CASES = (("cornell", {}), ("prims33", {}), ("random_spheres", {}), ("prims600", {}), ("grid3000", {}), ("grid3000", dict(compact_nodes=0)))
SCENES = ("cornell", "prims33", "random_spheres", "prims600", "grid3000")
# cornell's own background is black: its SKY slots would hold sums of zeros
BACKGROUND_IF_BLACK = (0.25, 0.5, 1.0)
_REFERENCE = {}


def background_of(desc):
    bg = tuple(float(c) for c in desc["background"])
    return bg if any(bg) else BACKGROUND_IF_BLACK


def reference(trt, orc, name):
    """name -> description, oracle world, background and, per source: items [324, 6], first rays [n, K, 6], colours, kinds, depths and the
    oracle's world.hit calls at max_bounces = 5.  Computed once per process and never changed."""
    import walk_ray_cases as W
    if name not in _REFERENCE:
        desc = W.scene(trt, name)
        ow, _ = orc.world_from_description(desc)
        bg = background_of(desc)
        ref = dict(desc=desc, ow=ow, bg=bg)
        for source in SOURCES:
            items = items_of(orc, ow, desc, source)
            rays = first_rays(orc, desc, items, source)
            cols, kinds, depths, hits = oracle_paths(orc, ow, desc, rays, MAX_BOUNCES, bg, SEED, FIRST_STREAM)
            for a in (items, rays, cols, kinds, depths):
                a.setflags(write=False)
            ref[source] = dict(items=items, rays=rays, cols=cols, kinds=kinds, depths=depths, n_rays=hits)
        _REFERENCE[name] = ref
    return _REFERENCE[name]
