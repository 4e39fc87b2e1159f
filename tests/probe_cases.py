"""What tests/test_probe_cases.py, tests/test_gpu_probe.py and tests/test_gpu_probe_long.py share, none of it touching a GPU: the items of
a scene (gather_cases.items_of), the oracle's restatement of the first ray of every sample (tinyrt.h trt_probe: the draw has RNG stream
(seed, j, 1) of its own), of the path that follows on stream (seed, j, 0) (radiance_cases.oracle_samples over the n * K drawn rays with
one sample each) and the fold in numpy float32.

The draw is the reference's own functions: orc_random_unit_vector (Vec3::new_random_unit_vector), for the hemisphere orc_vec3_dot and a
negation (Vec3::new_random_on_hemisphere), then orc_ray_new, which normalises again - the direction the fold sees is the ray's, not the
unit vector's.  The basis is passed in (the product's restatement, tiny-raytracer_amd/sh.py basis; tests/test_probe_cases.py checks it
against a quadrature)."""
import ctypes as C

import numpy as np

import gather_cases as GC
import radiance_cases as R

f32 = np.float32
K, MAX_BOUNCES, SEED, FIRST_STREAM = R.K, R.MAX_BOUNCES, R.SEED, R.FIRST_STREAM
N_ITEMS = GC.N_ITEMS
DOMAINS = ("sphere", "hemisphere")
BANDS = 3
COEFFS = BANDS * BANDS
items_of = GC.items_of

# The furnace: inside one light of colour E every path ends at its first hit with colour E, whatever the direction.
FURNACE_E = (1.0, 2.0, 0.5)
FURNACE_K, FURNACE_DEPTH = 4096, 2
FURNACE_ITEMS = np.array([[0, 0, 0, 0, 0, 1], [3, 0, 0, 0, 0, -1], [0, -4, 2, 0, 1, 0], [1, 1, 1, 1, 0, 0]], np.float32)
FURNACE_AXIS_K = (2, 2, 1, 3)                                               # the band-1 coefficient along each item's axis: z, z, y, x
FURNACE_AXIS_SIGN = (1.0, -1.0, 1.0, 1.0)


def furnace_description(light_kind):
    """One light sphere of radius 10 about the origin, background 0 (`light_kind`: the package's LIGHT constant)."""
    cam = dict(focus_distance=1.0, defocus_angle=0.0, position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vertical_fov=40.0,
               width=8, height=8)
    return dict(name="furnace", materials=[("E", light_kind, FURNACE_E, 0.0)], geometries=[("sphere", (0.0, 0.0, 0.0), 10.0, "E")], camera=cam,
                background=(0.0, 0.0, 0.0))


def _vec(orc, a):
    return orc.Vec3(float(a[0]), float(a[1]), float(a[2]))


def first_rays(orc, items, domain, k=K, seed=SEED, first_stream=FIRST_STREAM, only=None):
    """(rays float32 [n, k, 6], units float32 [n, k, 3], flipped bool [n, k]): the first ray of sample s of item i, drawn from RNG stream
    (seed, first_stream + i * k + s, 1); the unit vector orc_random_unit_vector returned for it, and whether the hemisphere rule negated
    it.  `only`: the item indices to draw for (the others stay 0)."""
    assert domain in DOMAINS
    n = len(items)
    rays, units, flipped = np.zeros((n, k, 6), np.float32), np.zeros((n, k, 3), np.float32), np.zeros((n, k), bool)
    rng = (C.c_uint32 * 2)()
    for i in (range(n) if only is None else only):
        point, axis = _vec(orc, items[i, 0:3]), _vec(orc, items[i, 3:6])
        for s in range(k):
            orc.lib.orc_rng_seed(seed, (first_stream + i * k + s) & 0xFFFFFFFF, 1, C.byref(rng))
            u = orc.lib.orc_random_unit_vector(C.byref(rng))
            units[i, s] = np.frombuffer(bytes(u), np.float32)
            direction = u
            if domain == "hemisphere" and not (orc.lib.orc_vec3_dot(u, axis) > 0.0):        # a zero or NaN dot flips
                direction = orc.Vec3(-u.x, -u.y, -u.z)
                flipped[i, s] = True
            rays[i, s] = np.frombuffer(bytes(orc.lib.orc_ray_new(point, direction)), np.float32)
    return rays, units, flipped


def oracle_probe(orc, ow, items, domain, k, max_bounces, background, seed, first_stream):
    """(first rays [n, k, 6], colours [n, k, 3], the oracle's world.hit calls, units, flipped): the n * k drawn rays go through
    radiance_cases.oracle_samples with one sample each, so that ray i * k + s has stream first_stream + i * k + s."""
    rays, units, flipped = first_rays(orc, items, domain, k, seed, first_stream)
    cols, n_rays = R.oracle_samples(orc, ow, rays.reshape(-1, 6), 1, max_bounces, background, seed, first_stream)
    return rays, cols.reshape(len(items), k, 3), n_rays, units, flipped


def fold(basis, rays, cols, k, bands=BANDS, begin=0, end=None, sh=None):
    """tinyrt.h trt_probe: t = b_k * inv_K; sh[k].ch = sh[k].ch + c.ch * t over samples [begin, end) in order, from `sh` or from 0, all
    float32; b = basis(the ray's stored direction, bands).  A sample whose ray has a NaN component adds nothing."""
    end = cols.shape[1] if end is None else end
    inv = f32(1.0) / f32(k)
    S = np.zeros((cols.shape[0], bands * bands, 3), np.float32) if sh is None else sh.copy()
    with np.errstate(all="ignore"):
        for s in range(begin, end):
            t = basis(rays[:, s, 3:6], bands) * inv                         # [n, C]
            assert t.dtype == np.float32
            added = S + cols[:, s, None, :] * t[:, :, None]
            folds = ~np.isnan(rays[:, s, :]).any(axis=1)
            S = np.where(folds[:, None, None], added, S)
    assert S.dtype == np.float32
    return S


_FURNACE = {}


def furnace_reference(orc, light_kind, basis):
    """description, and per domain the first rays [4, K, 6], colours, ray count and fold of the furnace case; computed once, never changed."""
    if not _FURNACE:
        desc = furnace_description(light_kind)
        ow, _ = orc.world_from_description(desc)
        _FURNACE["desc"] = desc
        for domain in DOMAINS:
            rays, cols, n_rays, _, _ = oracle_probe(orc, ow, FURNACE_ITEMS, domain, FURNACE_K, FURNACE_DEPTH, desc["background"], SEED, FIRST_STREAM)
            S = fold(basis, rays, cols, FURNACE_K)
            for a in (rays, cols, S):
                a.setflags(write=False)
            _FURNACE[domain] = dict(rays=rays, cols=cols, n_rays=n_rays, S=S)
    return _FURNACE


def fold_one_item(basis_row, rays, cols, k):
    """The same fold for one item written out scalar by scalar (rays [k, 6], cols [k, 3]; basis_row(x, y, z) -> the nine f32 values)."""
    inv = f32(1.0) / f32(k)
    S = [[f32(0.0)] * 3 for _ in range(COEFFS)]
    for s in range(len(rays)):
        if any(np.isnan(v) for v in rays[s]):
            continue
        b = basis_row(f32(rays[s, 3]), f32(rays[s, 4]), f32(rays[s, 5]))
        for c in range(COEFFS):
            t = f32(b[c] * inv)
            for ch in range(3):
                S[c][ch] = f32(S[c][ch] + f32(f32(cols[s, ch]) * t))
    return np.array(S, np.float32)
