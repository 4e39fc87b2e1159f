"""Scenes, chosen rays and wave lists of the ray-level walk test (tests/test_walk_ray_cases.py on the CPU, tests/test_gpu_walk_rays.py on
the GPU).  Everything is seeded numpy, computed in float64 and rounded ONCE to float32; a ray is used as given (never normalised again).

Ray classes, per scene, from the root box [lo, hi] of the oracle's BVH (non-finite bounds replaced by +-10), ext = hi - lo, and its
leaf boxes:
  generic                 origin uniform in lo - ext/4 .. hi + ext/4, aimed at a uniform point inside the root box (every other ray: at a
                          point of a random primitive - a root box blown up by one far-away sphere is nearly empty)
  axis_parallel           one non-zero component (+-1; the zeros also as -0), starting half an extent outside, through a leaf box
  on_plane_axis_parallel  one origin coordinate exactly a leaf-box plane, direction along another axis (0 * inf in aabb.rs:45-46); every
                          other ray runs in the plane midway between the leaf's two planes instead (a ray inside a face plane of a
                          primitive's own box cannot hit that primitive: in a sparse scene the class would hit next to nothing)
  at_corners              generic origins aimed exactly at a corner of a random leaf box
  far_sliver              (spheres of radius < 5) from L = 300 / 1000 away, passing delta = 5e-4 / 2e-3 above the top face of the sphere's
                          box: the reference's f32 Sphere::hit has false positives there that only the sphere's LEAF BOX keeps out.
                          L and delta are for a sphere of radius 0.2 and scale with the radius (f32 arithmetic is scale-free: the
                          scene shrunk by 1e-3 gets the same rays, shrunk); heading towards the middle of the scene, +-45 degrees
  near_axis_parallel      one component +-1, the other two from {2^-59, 2^-60, 2^-61, 1e-30, 1e-39, -2^-60, -1e-39}: both sides of the
                          fused loop's |1/d| <= 2^60 border, 1/d overflowing to inf
  scaled_dir              generic directions (all aimed at primitives) times 1e-18, 1e-6, 1e6, 1e18 (the last two mostly miss: t < t_min)
  origin_limit            (scenes with 16-byte nodes) |o| on one axis exactly the fused loop's origin limit, one ulp either side, 1e38, inf
  surface                 origins exactly on a primitive (quad corner / edge / interior, sphere pole, sphere centre), directions along the
                          surface, along quad edges and straight out (the t_min edge); rays at coincident twin spheres and at quad interiors
                          (coplanar overlapping quads: the first in left-first order wins)
  special                 every NaN subset of origin and direction, the zero direction, infinite components (1/d = 0)
"""
import struct

import numpy as np

SEED = 1
PER_CLASS = 192                  # rays per class and scene in the GPU test's lists
WAVE_LIST = 192                  # rays per wave list: three refills of a wave, so parked stragglers resume beside fresh rays
SMALL = [2.0 ** -59, 2.0 ** -60, 2.0 ** -61, 1e-30, 1e-39, -(2.0 ** -60), -1e-39]
SLIVER_DELTAS = (5e-4, 2e-3)
SLIVER_LS = (300.0, 1000.0)


# ------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------
def scene_names():
    return ["cornell", "box_stacks", "thin_sheets", "signed_zero_planes", "one_primitive", "prims32", "prims33", "random_spheres",
            "mixed400", "grid3000", "mixed2600", "grid3000_far_sphere", "grid3000_tiny", "degenerate", "nonfinite"]


def scene(trt, name):
    """The description (tiny-raytracer_amd.scenes format) of one of scene_names(), or of prims600 (the ray queries' tests only)."""
    import test_gpu_flat_reuse as fr
    from test_gpu_fuzz import random_scene
    if name == "cornell":
        return trt.scenes.cornell(8, 8)
    if name in ("box_stacks", "thin_sheets", "signed_zero_planes"):
        return getattr(fr, name)(trt)
    if name == "one_primitive":
        desc = random_scene(1, n_prims=1)
        return dict(desc, geometries=[("sphere", (0.3, -0.2, 0.5), 6.0, desc["materials"][0][0])])
    if name == "prims32":                                                   # the last scene of the lock-step leaf list
        return random_scene(21, n_prims=32)
    if name == "prims33":                                                   # the first tree
        return random_scene(22, n_prims=33)
    if name == "random_spheres":
        return trt.scenes.random_spheres(8, 8)
    if name == "mixed400":
        return random_scene(1100, n_prims=400)
    if name == "prims600":                                                  # an LDS copy of 59 680 B: planned as LDS tree / 512 lanes (queries: register slots)
        return random_scene(1100, n_prims=600)
    if name == "mixed2600":
        return random_scene(11, n_prims=2600)
    if name == "degenerate":
        return random_scene(7, n_prims=12, degenerate=True)
    if name == "nonfinite":
        return random_scene(9, n_prims=10, nonfinite=True)
    desc = trt.scenes.sphere_grid(3000, 8, 8)                               # walked from global memory: 16-byte nodes
    geos = list(desc["geometries"])
    if name == "grid3000_far_sphere":                                       # (the cases of test_fused_slab_walk_in_and_out_of_its_domain)
        geos.append(("sphere", (1.0e5, 50.0, -3.0e4), 10.0, desc["materials"][3][0]))
    elif name == "grid3000_tiny":
        k = 1.0e-3
        geos = [(g[0], tuple(c * k for c in g[1]), g[2] * k, g[3]) for g in geos]
    else:
        assert name == "grid3000", name
    return dict(desc, geometries=geos, name=name)


def f32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, np.float64).astype(np.float32)


def geometry_arrays(desc):
    """(kind[n] 0 sphere / 1 quad, a[n,3], b[n,3], c[n,3]) float32 as the worlds store them (scene.h Geometry)."""
    n = len(desc["geometries"])
    kind = np.zeros(n, np.uint32)
    a, b, c = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    for i, g in enumerate(desc["geometries"]):
        if g[0] == "sphere":
            a[i], b[i, 0] = f32(g[1]), np.float32(g[2])
        else:
            kind[i] = 1
            a[i], b[i], c[i] = f32(g[1]), f32(g[2]), f32(g[3])
    return kind, a, b, c


def write_scene_file(path, desc, cull_prune=0.5, flat_walk=-1, compact_nodes=-1):
    """The harness's scene file (tests/native/walk_rays.hip): materials, geometries, scene options."""
    names = [m[0] for m in desc["materials"]]
    kind, a, b, c = geometry_arrays(desc)
    with open(path, "wb") as f:
        f.write(struct.pack("<IIIfii", 0x31535257, len(names), len(kind), cull_prune, flat_walk, compact_nodes))
        for _, k, albedo, param in desc["materials"]:
            f.write(struct.pack("<Iffff", int(k), *[float(x) for x in albedo], float(param)))
        mat = np.array([names.index(g[-1]) for g in desc["geometries"]], np.uint32)
        rec = np.zeros((len(kind), 11), np.uint32)
        rec[:, 0], rec[:, 1] = kind, mat
        rec[:, 2:5], rec[:, 5:8], rec[:, 8:11] = a.view(np.uint32), b.view(np.uint32), c.view(np.uint32)
        f.write(rec.tobytes())


def write_ray_file(path, rays, tasks):
    with open(path, "wb") as f:
        f.write(struct.pack("<III", 0x31525257, len(rays), len(tasks)))
        f.write(np.ascontiguousarray(rays, np.float32).tobytes())
        f.write(np.ascontiguousarray(tasks, np.uint32).tobytes())


def prim_to_geometry(desc, prim):
    """rt_path.h prim_best (kind bit | index within kind; 0xFFFFFFFF = none) -> geometry insertion index (-1 = none)."""
    kind = geometry_arrays(desc)[0]
    of_sphere, of_quad = np.flatnonzero(kind == 0), np.flatnonzero(kind == 1)
    prim = np.asarray(prim, np.uint32)
    out = np.full(len(prim), -1, np.int64)
    none = prim == 0xFFFFFFFF
    quad = ~none & ((prim & 0x40000000) != 0)
    sph = ~none & ~quad
    idx = (prim & 0x3FFFFFFF).astype(np.int64)
    assert (idx[quad] < len(of_quad)).all() and (idx[sph] < len(of_sphere)).all(), "primitive reference out of range"
    out[quad] = of_quad[idx[quad]]
    out[sph] = of_sphere[idx[sph]]
    return out


def predict_flags(rays, all_finite, limit=None):
    """rt_path.h trav_begin's `fast` for each ray: the scene is all finite, 1/d and o are finite; with `limit` (the fused loop's domain:
    SceneLayout::compact_origin_limit) also |o| <= limit per axis and |1/d| <= 2^60."""
    r = np.asarray(rays, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (np.float32(1.0) / r[:, 3:]).astype(np.float32)
    fast = np.isfinite(inv).all(axis=1) & np.isfinite(r[:, :3]).all(axis=1) & bool(all_finite)
    if limit is not None:
        lim = np.asarray(limit, np.float32)
        fast &= (np.abs(r[:, :3]) <= lim).all(axis=1) & (np.abs(inv) <= np.float32(2.0 ** 60)).all(axis=1)
    return fast


def origin_limit(cull_root):
    """scene_common.h compact_eps_rule's limit for an all-finite scene: 4 B per axis, B the culling root's largest |coordinate|."""
    root = np.asarray(cull_root, np.float32)
    return (np.float32(4.0) * np.maximum(np.abs(root[:3]), np.abs(root[3:]))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# rays
# ------------------------------------------------------------------------------------------------------------------
def _unit(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return v / n


class RayMaker:
    def __init__(self, desc, bbox, prim, seed=SEED, limit=None):
        """bbox, prim: World.bvh_dump() of the oracle; limit: the fused loop's origin limit (scenes with 16-byte nodes), else None."""
        self.desc = desc
        self.kind, self.a, self.b, self.c = (x.astype(np.float64) if x.dtype == np.float32 else x for x in geometry_arrays(desc))
        root = bbox[0].astype(np.float64)
        self.lo = np.where(np.isfinite(root[:3]), root[:3], -10.0)
        self.hi = np.where(np.isfinite(root[3:]), root[3:], 10.0)
        self.ext = self.hi - self.lo
        leaves = bbox[prim >= 0].astype(np.float64)
        leaves = leaves[np.isfinite(leaves).all(axis=1)]
        self.leaves = leaves if len(leaves) else np.concatenate([self.lo, self.hi])[None, :]
        self.limit = None if limit is None else np.asarray(limit, np.float32)
        self.seed = seed

    def rng(self, salt):
        return np.random.default_rng([self.seed, salt, len(self.kind)])

    # -- building blocks
    def _origins(self, g, n):
        return g.uniform(self.lo - self.ext / 4.0, self.hi + self.ext / 4.0, (n, 3))

    def _leaf_points(self, g, n):
        b = self.leaves[g.integers(0, len(self.leaves), n)]
        return b[:, :3] + g.uniform(0.0, 1.0, (n, 3)) * (b[:, 3:] - b[:, :3])

    def _outside_start(self, pts, axis, sign):
        """pts with coordinate `axis` moved half an extent outside the root box, on the side a ray along sign * axis comes from."""
        o = pts.copy()
        rows = np.arange(len(o))
        o[rows, axis] = np.where(sign > 0, self.lo[axis] - self.ext[axis] / 2.0, self.hi[axis] + self.ext[axis] / 2.0)
        return o

    def _prim_points(self, g, n):
        """A point of a random primitive each: inside the sphere, inside the quad."""
        ok = np.flatnonzero(np.isfinite(self.a).all(axis=1) & np.isfinite(self.b).all(axis=1) & np.isfinite(self.c).all(axis=1))
        p = ok[g.integers(0, len(ok), n)]
        s, t = g.uniform(0.1, 0.9, n)[:, None], g.uniform(0.1, 0.9, n)[:, None]
        on_quad = self.a[p] + s * self.b[p] + t * self.c[p]
        in_sphere = self.a[p] + 0.5 * self.b[p, :1] * _unit(g.normal(size=(n, 3)))
        return np.where((self.kind[p] == 1)[:, None], on_quad, in_sphere)

    def generic(self, n, salt=1, at_prims=0.5):
        g = self.rng(salt)
        o = self._origins(g, n)
        target = np.where((g.random(n) < at_prims)[:, None], self._prim_points(g, n), g.uniform(self.lo, self.hi, (n, 3)))
        return np.concatenate([o, _unit(target - o)], axis=1)

    def axis_parallel(self, n):
        g = self.rng(2)
        axis, sign = g.integers(0, 3, n), g.choice([-1.0, 1.0], n)
        d = np.where(g.random((n, 3)) < 0.5, 0.0, -0.0)
        d[np.arange(n), axis] = sign
        return np.concatenate([self._outside_start(self._leaf_points(g, n), axis, sign), d], axis=1)

    def on_plane_axis_parallel(self, n):
        g = self.rng(3)
        b = self.leaves[g.integers(0, len(self.leaves), n)]
        plane_axis = g.integers(0, 3, n)
        axis = (plane_axis + g.integers(1, 3, n)) % 3                      # the direction's axis: another one
        sign = g.choice([-1.0, 1.0], n)
        pts = b[:, :3] + g.uniform(0.0, 1.0, (n, 3)) * (b[:, 3:] - b[:, :3])
        rows = np.arange(n)
        pts[rows, plane_axis] = np.where(g.random(n) < 0.5, b[rows, plane_axis], b[rows, 3 + plane_axis])      # exactly a box plane
        mid = (b[rows, plane_axis] + b[rows, 3 + plane_axis]) / 2.0
        pts[rows, plane_axis] = np.where(rows % 2 == 1, mid, pts[rows, plane_axis])
        d = np.zeros((n, 3))
        d[rows, axis] = sign
        return np.concatenate([self._outside_start(pts, axis, sign), d], axis=1)

    def at_corners(self, n):
        g = self.rng(4)
        o = self._origins(g, n)
        b = self.leaves[g.integers(0, len(self.leaves), n)]
        pick = g.integers(0, 2, (n, 3))
        corner = np.where(pick == 0, b[:, :3], b[:, 3:])
        return np.concatenate([o, _unit(corner - o)], axis=1)

    def sliver_spheres(self):
        return np.flatnonzero((self.kind == 0) & (self.b[:, 0] > 0.0) & (self.b[:, 0] < 5.0) & np.isfinite(self.a).all(axis=1))

    def far_sliver(self, n, Ls=SLIVER_LS):
        """Returns (rays, sphere geometry index per ray, L per ray), or None if the scene has no such sphere."""
        cand = self.sliver_spheres()
        if len(cand) == 0:
            return None
        g = self.rng(5)
        s = cand[g.integers(0, len(cand), n)]
        c, r = self.a[s], self.b[s, 0]
        # heading: towards the middle of the scene's primitives, +-45 degrees, so that the ray goes on over the scene behind the sphere
        ok = np.isfinite(self.a).all(axis=1)
        to_mid = np.median(self.a[ok], axis=0) - c
        ang = np.arctan2(to_mid[:, 2], to_mid[:, 0]) + g.uniform(-np.pi / 4.0, np.pi / 4.0, n)
        h = np.stack([np.cos(ang), np.zeros(n), np.sin(ang)], axis=1)
        delta = g.choice(SLIVER_DELTAS, n)
        L = g.choice(Ls, n)
        up = np.array([0.0, 1.0, 0.0])
        k = r / 0.2                                                        # the scale of the class: radius 0.2 is what L and delta were chosen on
        p = c + (r + delta * k)[:, None] * up + h * (r / 2.0)[:, None]
        o = p - (L * k)[:, None] * h + (L * k / 1000.0)[:, None] * up
        return np.concatenate([o, p - o], axis=1), s, L

    def near_axis_parallel(self, n):
        g = self.rng(6)
        axis, sign = g.integers(0, 3, n), g.choice([-1.0, 1.0], n)
        d = g.choice(SMALL, (n, 3))
        d[np.arange(n), axis] = sign
        return np.concatenate([self._outside_start(self._leaf_points(g, n), axis, sign), d], axis=1)

    def scaled_dir(self, n):
        r = self.generic(n, salt=7, at_prims=1.0)
        r[:, 3:] *= np.resize([1e-18, 1e-6, 1e6, 1e18], n)[:, None]
        return r

    def origin_limit(self, n):
        if self.limit is None:
            return None
        g = self.rng(8)
        axis, sign = g.integers(0, 3, n), g.choice([-1.0, 1.0], n)
        lim = self.limit[axis]
        values = np.stack([lim, np.nextafter(lim, np.float32(0.0)), np.nextafter(lim, np.float32(np.inf)),
                           np.full(n, np.float32(1e38)), np.full(n, np.float32(np.inf))], axis=1).astype(np.float64)
        o = g.uniform(self.lo, self.hi, (n, 3))
        o[np.arange(n), axis] = sign * values[np.arange(n), np.arange(n) % 5]
        target = self._leaf_points(g, n)
        with np.errstate(invalid="ignore", over="ignore"):
            d = target - o
            norm = np.linalg.norm(d, axis=1, keepdims=True)
            d = np.where(np.isfinite(norm), d / norm, d)                   # (an infinite origin: the direction as the subtraction gives it)
        return np.concatenate([o, d], axis=1)

    def surface(self, n):
        g = self.rng(9)
        rays = []
        finite = np.isfinite(self.a).all(axis=1) & np.isfinite(self.b).all(axis=1) & np.isfinite(self.c).all(axis=1)
        quads, spheres = np.flatnonzero((self.kind == 1) & finite), np.flatnonzero((self.kind == 0) & finite)
        per = max(1, n // 20)
        for q in (quads[g.integers(0, len(quads), per)] if len(quads) else []):
            Q, u, v = self.a[q], self.b[q], self.c[q]
            nrm = np.cross(u, v)
            nrm = nrm / np.linalg.norm(nrm) if np.linalg.norm(nrm) > 0 else np.array([0.0, 1.0, 0.0])
            for o in (Q, Q + u / 2.0, Q + 0.3 * u + 0.6 * v):
                for d in (u, v, nrm, -nrm):
                    rays.append(np.concatenate([o, d]))
            for o in self._origins(g, 8):                                  # at the interior point from outside (coplanar overlapping quads tie there)
                rays.append(np.concatenate([o, Q + 0.3 * u + 0.6 * v - o]))
        for s in (spheres[g.integers(0, len(spheres), per)] if len(spheres) else []):
            c, r = self.a[s], self.b[s, 0]
            pole = c + np.array([0.0, r, 0.0])
            for d in ([1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.6, 0.8, 0.0]):
                rays.append(np.concatenate([pole, d]))
            for d in _unit(g.normal(size=(3, 3))):
                rays.append(np.concatenate([c, d]))
        rays = np.array(rays)
        ties = self.tie_rays()[0]                                          # never cut
        keep = max(0, n - len(ties))
        rays = rays[g.permutation(len(rays))[:keep]] if len(rays) > keep else rays
        return np.concatenate([rays, ties]) if len(ties) else rays

    def tie_rays(self):
        """Rays at primitives that coincide - twin spheres (same centre and radius), twin quads (same corner and edges, +0 and -0 alike):
        both give the same t, and the first in left-first order must win.  (rays [k, 6], geometry indices of the group per ray)."""
        g = self.rng(11)
        rays, groups = [], []
        finite = np.isfinite(self.a).all(axis=1) & np.isfinite(self.b).all(axis=1) & np.isfinite(self.c).all(axis=1)
        key = np.concatenate([self.kind[:, None].astype(np.float64), self.a, self.b, self.c], axis=1) + 0.0      # (-0 + 0 = +0)
        idx = np.flatnonzero(finite & ((self.kind == 1) | (self.b[:, 0] > 0.0)))
        if len(idx) == 0:
            return np.zeros((0, 6)), []
        uniq, inverse, count = np.unique(key[idx], axis=0, return_inverse=True, return_counts=True)
        inverse = np.asarray(inverse).reshape(-1)
        for u in np.flatnonzero(count > 1)[:4]:
            members = idx[inverse == u]
            m = members[0]
            target = self.a[m] + 0.3 * self.b[m] + 0.6 * self.c[m] if self.kind[m] == 1 else self.a[m]
            for o in self._origins(g, 8):
                rays.append(np.concatenate([o, _unit(target - o)]))
                groups.append(tuple(int(x) for x in members))
        return (np.array(rays) if rays else np.zeros((0, 6))), groups

    def special(self):
        base = self.generic(1, salt=10)[0]
        o0, d0 = base[:3], base[3:]
        nan, inf = np.nan, np.inf
        rays = [np.concatenate([o0, d0])]
        for k in range(1, 8):
            rays.append(np.concatenate([o0, [nan if k >> a & 1 else d0[a] for a in range(3)]]))
        for k in range(1, 8):
            rays.append(np.concatenate([[nan if k >> a & 1 else o0[a] for a in range(3)], d0]))
        rays.append(np.full(6, nan))
        rays.append(np.concatenate([o0, [-nan, 0.0, 1.0]]))
        for d in ([0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [inf, 0.0, 0.0], [inf, d0[1], d0[2]], [-inf, inf, d0[2]], [inf, inf, inf], [d0[0], -inf, d0[2]]):
            rays.append(np.concatenate([o0, d]))
        return np.array(rays)

    def classes(self, n=PER_CLASS):
        """{class name: float32 [k, 6]} in a fixed order; classes the scene does not have are left out."""
        out = {"generic": self.generic(n), "axis_parallel": self.axis_parallel(n), "on_plane_axis_parallel": self.on_plane_axis_parallel(n),
               "at_corners": self.at_corners(n)}
        fs = self.far_sliver(n)
        if fs is not None:
            out["far_sliver"] = fs[0]
        out["near_axis_parallel"] = self.near_axis_parallel(n)
        out["scaled_dir"] = self.scaled_dir(n)
        ol = self.origin_limit(n)
        if ol is not None:
            out["origin_limit"] = ol
        out["surface"] = self.surface(n)
        out["special"] = self.special()
        return {k: f32(v) for k, v in out.items()}


def wave_lists(classes, seed=SEED):
    """The ray array the harness gets and its wave lists.  Every ray of every class appears (a) in a list of its own class, (b) in a
    shuffle of all classes and (c) in a second shuffle of half of them cut into shorter, ragged lists - no multiple of 64; into every
    list of (b) and (c) a NaN ray, another `special` ray and an axis-parallel (exact-path) ray are dealt after every 30 rays, in turn
    and with repetition, so that every wave mixes fast, exact-path and NaN rays all the way through its list; and (d) one ray of each
    class fills a whole wave, 64 copies.
    Returns (rays float32 [m, 6], tasks uint32 [k, 2] = (begin, count), label per ray: 'a:generic', 'b', 'c', 'd:generic')."""
    g = np.random.default_rng([seed, 77])
    rays, tasks, labels = [], [], []
    pos = 0

    def add(block, chunk, label):
        nonlocal pos
        for b in range(0, len(block), chunk):
            part = block[b:b + chunk]
            rays.append(part)
            tasks.append((pos, len(part)))
            labels.extend([label] * len(part))
            pos += len(part)

    for name, r in classes.items():
        add(r, WAVE_LIST, "a:" + name)
    special = classes["special"]
    with_nan = np.isnan(special).any(axis=1)
    deal = [special[with_nan], special[~with_nan], classes["axis_parallel"]]
    dealt = [0, 0, 0]

    def add_mixed(block, chunk, label):
        for b in range(0, len(block), chunk):
            part = block[b:b + chunk]
            pieces = []
            for s0 in range(0, len(part), 30):
                pieces.append(part[s0:s0 + 30])
                for k in range(3):
                    pieces.append(deal[k][dealt[k] % len(deal[k])][None, :])
                    dealt[k] += 1
            add(np.concatenate(pieces), 1 << 30, label)

    everything = np.concatenate(list(classes.values()))
    add_mixed(everything[g.permutation(len(everything))], WAVE_LIST, "b")
    add_mixed(everything[g.permutation(len(everything))[:len(everything) // 2 | 1]], 100, "c")
    for name, r in classes.items():
        add(np.repeat(r[len(r) // 2][None, :], 64, axis=0), 64, "d:" + name)
    return np.concatenate(rays).astype(np.float32), np.array(tasks, np.uint32), labels


def oracle_answers(ow, rays):
    """(hit bool[n], t float32[n] (inf on a miss), geometry index int32[n] (-1 on a miss)) of the oracle's BVH closest hit in 0.001..inf."""
    return ow.hit_index_batch(rays, 0.001, float("inf"))
