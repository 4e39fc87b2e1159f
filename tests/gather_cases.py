"""What tests/test_gpu_gather.py shares, none of it touching a GPU: the surfels of a scene, the oracle's restatement of the first ray of
every sample (tinyrt.h trt_gather: the draw has RNG stream (seed, j, 1) of its own) and, through tests/radiance_cases.py, of the path that
follows on stream (seed, j, 0) and of the fold.

The cosine lobe is the reference's own function: orc_material_scatter(LAMBERTIAN) on a hit record whose point and normal are the surfel's.
The cone lobe is Metal::scatter's line with the axis in the place of the reflected direction, from the oracle's pieces:
orc_ray_new(point, axis + spread * orc_random_in_unit_sphere(rng))."""
import ctypes as C

import numpy as np

import radiance_cases as R

f32 = np.float32
K, MAX_BOUNCES, SEED, FIRST_STREAM = R.K, R.MAX_BOUNCES, R.SEED, R.FIRST_STREAM
N_ITEMS = R.N_RAYS
SPREAD = 0.5
LOBES = ("cosine", "cone")
ORC_LAMBERTIAN = 0                                                          # rt_oracle.h
AXIS_SCALES = (1.0, 0.25, 3.0)                                              # item k: the axis times AXIS_SCALES[k % 3], in f32


def _vec(orc, a):
    return orc.Vec3(float(a[0]), float(a[1]), float(a[2]))


def items_of(orc, ow, desc):
    """(items float32 [324, 6], unit bool [324]).  For each of radiance_cases.rays_of(desc): where the oracle's World.hit finds a hit, the
    surfel (hit point, hit normal); where it misses, the ray itself - a probe in free space.  The axis of every third item is scaled by
    0.25 and of the next by 3.  The last four are, at the camera position: a NaN point, a zero axis, an axis with an inf component, and an
    ordinary item whose axis has length 1e-9 (so that only the draw decides near_zero).  `unit`: the item is a surfel with its unit normal
    as the axis."""
    rays = R.rays_of(desc)
    items = rays.copy()
    unit = np.zeros(len(rays), bool)
    for k, r in enumerate(rays[:-4]):
        rec, _ = ow.hit(orc.Ray(_vec(orc, r[0:3]), _vec(orc, r[3:6])))
        if rec is not None:
            items[k, 0:3] = rec.point.tolist()
            items[k, 3:6] = rec.normal.tolist()
            unit[k] = k % 3 == 0
    items[:-4, 3:6] *= np.array(AXIS_SCALES, np.float32)[np.arange(len(items) - 4) % 3][:, None]
    pos = np.array(desc["camera"]["position"], np.float32)
    items[-4:, 0:3] = pos
    items[-4, 0] = np.nan
    items[-4, 3:6] = (0.0, 0.0, 1.0)
    items[-3, 3:6] = (0.0, 0.0, 0.0)
    items[-2, 3:6] = (np.inf, 0.0, 1.0)
    items[-1, 3:6] = (0.0, 1e-9, 0.0)
    assert items.dtype == np.float32 and items.shape == (N_ITEMS, 6)
    return np.ascontiguousarray(items), unit


def first_rays(orc, items, lobe, k=K, spread=SPREAD, seed=SEED, first_stream=FIRST_STREAM, only=None):
    """float32 [n, k, 6]: the first ray of sample s of item i, drawn from RNG stream (seed, first_stream + i * k + s, 1).  `only`: the item
    indices to draw for (the others stay 0)."""
    n = len(items)
    out = np.zeros((n, k, 6), np.float32)
    rng = (C.c_uint32 * 2)()
    ray_in, ray, att, rec = orc.Ray(), orc.Ray(), orc.Vec3(), orc.HitRecord()
    for i in (range(n) if only is None else only):
        point, axis = _vec(orc, items[i, 0:3]), _vec(orc, items[i, 3:6])
        for s in range(k):
            orc.lib.orc_rng_seed(seed, (first_stream + i * k + s) & 0xFFFFFFFF, 1, C.byref(rng))
            if lobe == "cosine":
                rec.point, rec.normal = point, axis
                ok = orc.lib.orc_material_scatter(ORC_LAMBERTIAN, orc.Vec3(1.0, 1.0, 1.0), 0.0, C.byref(ray_in), C.byref(rec), C.byref(rng), C.byref(ray),
                                                  C.byref(att))
                assert ok
            else:
                v = orc.lib.orc_random_in_unit_sphere(C.byref(rng))
                ray = orc.lib.orc_ray_new(point, orc.lib.orc_vec3_binop(0, axis, orc.lib.orc_vec3_scale(0, v, spread)))
            out[i, s] = np.frombuffer(bytes(ray), np.float32)
    return out


def oracle_gather(orc, ow, items, lobe, k, max_bounces, background, seed, first_stream, spread=SPREAD):
    """(first rays [n, k, 6], colours [n, k, 3], the oracle's world.hit calls): the n * k drawn rays go through
    radiance_cases.oracle_samples with one sample each, so that ray i * k + s has stream first_stream + i * k + s."""
    rays = first_rays(orc, items, lobe, k, spread, seed, first_stream)
    cols, n_rays = R.oracle_samples(orc, ow, rays.reshape(-1, 6), 1, max_bounces, background, seed, first_stream)
    return rays, cols.reshape(len(items), k, 3), n_rays
