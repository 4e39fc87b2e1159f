"""Axis-exact quads (tiny-raytracer_amd/csrc/axis_quads.h) without a GPU.

(a) The scene-level switch, compiled with g++ and driven on packed quad records: on for Cornell, for stacked boxes and for planes at
    +-0; off for a rotated quad, a NaN / inf component, a sheared parallelogram, more than 32 leaves, no lock-step list, and when disabled.
(b) The two forms of Quad::hit's inside test replayed in numpy f32 (element-wise operations, nothing fused), with the constants the
    header derives: on more than 10^6 (ray, quad) pairs - every axis, both u / v assignments, every sign combination, +-0 zeros; rays
    parallel to the plane, with zero direction components, from the quad's edges and corners, through points within an ulp of
    alpha, beta in {0, 1}, with t at t_min and at t_best, and with magnitudes up to 1e38 that overflow p in one, two and three
    components - both forms accept the same pairs and leave the same t bits."""
import os
import subprocess

import numpy as np
import pytest
from test_gpu_flat_reuse import box_stacks, signed_zero_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiny-raytracer_amd", "csrc")
F = np.float32
T_MIN = F(0.001)

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "axis_quads.h"
// driver flag   <records> <n_quads> <n_leaves> <flat_walk> <in_lds> <enabled>  -> the switch
// driver consts <records> <n_quads> <out>                                      -> per quad: u32 exact, 8 floats
int main(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<unsigned char> b;
    if (FILE* f = fopen(argv[2], "rb")) { int c; while ((c = fgetc(f)) != EOF) b.push_back((unsigned char)c); fclose(f); }
    const uint32_t nq = (uint32_t)strtoul(argv[3], nullptr, 10);
    if (argv[1][0] == 'f') {
        if (argc < 8) return 2;
        printf("%u\n", trt::axis_quads_flag(b.empty() ? nullptr : b.data(), nq, (uint32_t)strtoul(argv[4], nullptr, 10), atoi(argv[5]) != 0,
                                            atoi(argv[6]) != 0, atoi(argv[7]) != 0));
        return 0;
    }
    FILE* o = fopen(argv[4], "wb");
    if (!o) return 3;
    for (uint32_t i = 0; i < nq; i++) {
        float rec[20], out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        memcpy(rec, b.data() + 80u * (size_t)i, sizeof rec);
        const uint32_t ok = trt::axis_quad_constants(rec, out) ? 1u : 0u;
        fwrite(&ok, 4, 1, o);
        fwrite(out, 4, 8, o);
    }
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("axis_quads")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    count = [0]

    def write(records):
        rec = np.ascontiguousarray(records, np.float32).reshape(-1, 20)
        count[0] += 1
        f = d / ("quads%d.bin" % count[0])
        f.write_bytes(rec.tobytes())
        return f, len(rec)

    def flag(records, n_leaves=None, flat_walk=True, in_lds=True, enabled=True):
        f, n = write(records)
        out = subprocess.run([str(exe), "flag", str(f), str(n), str(n if n_leaves is None else n_leaves), str(int(flat_walk)), str(int(in_lds)),
                              str(int(enabled))], capture_output=True, text=True, check=True)
        return int(out.stdout)

    def consts(records):
        f, n = write(records)
        o = str(f) + ".out"
        subprocess.run([str(exe), "consts", str(f), str(n), o], check=True)
        raw = np.fromfile(o, np.uint32).reshape(n, 9)
        return raw[:, 0].astype(bool), raw[:, 1:].copy().view(np.float32)

    flag.consts = consts
    return flag


def packed_quads(trt, desc):
    """The quad records of the scene as the host compiler packs them: float32[n_quads, 20] (scene.h), and the leaf count."""
    s = trt.Scene(trt.world_from_description(desc)[0])
    info = s.info()
    off = 16 * (2 * info["num_cull_nodes"] + info["num_spheres"])                  # scene.h: culling nodes, spheres, quads
    rec = s.packed()[off:off + 80 * info["num_quads"]].view(np.float32).reshape(-1, 20).copy()
    return rec, info["num_quads"] + info["num_spheres"]


def with_quad(trt, corner, u, v):
    desc = box_stacks(trt)
    desc["geometries"] = desc["geometries"][:12] + [("quad", corner, u, v, "white")]
    return desc


# ---------------------------------------------------------------- (a) the switch

def test_on_for_cornell_and_the_axis_aligned_scenes(trt, driver):
    for desc in (trt.scenes.cornell(64, 64), box_stacks(trt), signed_zero_planes(trt)):
        rec, leaves = packed_quads(trt, desc)
        assert leaves <= 32 and len(rec) == len(desc["geometries"])
        assert driver(rec, leaves) == 1, desc["name"]
        ok, _ = driver.consts(rec)
        assert ok.all(), desc["name"]
    rec, _ = packed_quads(trt, signed_zero_planes(trt))
    assert np.any(np.signbit(rec[:, [8, 9, 10, 14, 15, 16]]) & (rec[:, [8, 9, 10, 14, 15, 16]] == 0)), "the scene holds -0 edge components"


def test_the_gpu_tests_scenes_are_what_they_claim(trt, driver):
    """tests/test_gpu_axis_quads.py: its twelve-quad scene takes the switch with twelve different constant patterns, its rotated scene does not."""
    import test_gpu_axis_quads as G
    rec, leaves = packed_quads(trt, G.twelve_combinations(trt))
    assert driver(rec, leaves) == 1
    ok, c = driver.consts(rec)
    assert ok.all() and len({tuple(np.sign(row[[0, 1, 2, 4, 5, 6]])) for row in c}) == 12
    rec, leaves = packed_quads(trt, G.box_stacks_rotated(trt))
    assert leaves == 27 and driver(rec, leaves) == 0 and driver(rec[:-1], leaves - 1) == 1


def test_off_for_a_rotated_quad(trt, driver):
    a = 1e-3
    rec, leaves = packed_quads(trt, with_quad(trt, (30.0, 0.0, 0.0), (5.0 * np.cos(a), 5.0 * np.sin(a), 0.0), (0.0, 0.0, 5.0)))
    ok, _ = driver.consts(rec)
    assert ok[:-1].all() and not ok[-1]
    assert driver(rec, leaves) == 0
    assert driver(rec[:-1], leaves - 1) == 1


def test_off_for_a_sheared_parallelogram(trt, driver):
    rec, leaves = packed_quads(trt, with_quad(trt, (30.0, 0.0, 0.0), (5.0, 0.0, 2.0), (0.0, 0.0, 5.0)))      # n stays on one axis, u does not
    assert np.count_nonzero(rec[-1, 0:3]) == 1 and np.count_nonzero(rec[-1, 14:17]) == 2
    assert driver(rec, leaves) == 0


def test_off_for_non_finite_components(trt, driver):
    rec, leaves = packed_quads(trt, trt.scenes.cornell(64, 64))
    for bad in (np.nan, np.inf, -np.inf):
        for k in [k for k in range(20) if k != 7]:                               # element 7 is the material index, not a float
            r = rec.copy()
            r[5, k] = bad
            assert driver(r, leaves) == 0, (bad, k)
    r = rec.copy()
    r[5, 7] = np.nan                                                             # any bit pattern is a material index
    assert driver(r, leaves) == 1


def test_off_beyond_32_leaves_without_the_list_and_when_disabled(trt, driver):
    rec, leaves = packed_quads(trt, trt.scenes.cornell(64, 64))
    assert driver(rec, leaves) == 1
    many = np.concatenate([rec, rec])[:33]
    assert driver(many, 33) == 0
    assert driver(many[:32], 32) == 1
    assert driver(rec, 33) == 0                                                   # spheres count as leaves too
    assert driver(rec, leaves, flat_walk=False) == 0
    assert driver(rec, leaves, in_lds=False) == 0
    assert driver(rec, leaves, enabled=False) == 0                                # TRT_AXIS_QUADS=0
    assert driver(rec[:0], 4) == 0                                                # no quads: nothing to switch


def test_structure_is_checked_component_by_component(driver):
    base = make_quads()
    assert driver(base[:1]) == 1
    a = int(np.flatnonzero(base[0, 0:3])[0])
    for k, val in (((a + 1) % 3, 1.0), ((a + 2) % 3, -1.0), (a, 0.0)):            # n: a second non-zero component / none at all
        r = base[:1].copy()
        r[0, k] = val
        assert driver(r) == 0, k
    for lo in (8, 11, 14):                                                        # v, w, u: a non-zero where a zero belongs
        r = base[:1].copy()
        z = lo + int(np.flatnonzero(r[0, lo:lo + 3] == 0)[0])
        r[0, z] = 1e-30
        assert driver(r) == 0, lo
    r = base[:1].copy()
    r[0, 14:17] = r[0, 8:11]                                                      # u on v's axis
    assert driver(r) == 0
    for lo in (8, 14):                                                            # the magnitude bound on the edges: [2^-64, 2^16]
        k = lo + int(np.flatnonzero(base[0, lo:lo + 3])[0])
        for val, want in ((65536.0, 1), (-65536.0, 1), (65540.0, 0), (2.0 ** -64, 1), (-2.0 ** -64, 1), (2.0 ** -65, 0), (1e-40, 0)):
            r = base[:1].copy()
            r[0, k] = val
            assert driver(r) == want, (lo, val)


# ---------------------------------------------------------------- (b) the replay

def make_quads(seed=11):
    """Quad records as scene_host.cpp packs them (n = u x v, w = n / n.n, d = n.corner in f32), for every axis, both u / v assignments and
    every sign combination, at several magnitudes; then the zero components of v, w, u and n get random signs."""
    rng = np.random.default_rng(seed)
    recs = []
    sizes = [(555.0, 555.0, 278.0), (130.0, 105.0, 343.0), (0.3, 7.0, 1.5), (1e-3, 2e-3, 3e38), (6.5e4, 1e-4, 5e37), (3.0, 1e4, -1e30),
             (2e-9, 3e-9, 1e-30)]
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for v_on_c in (True, False):
            for su in (1.0, -1.0):
                for sv in (1.0, -1.0):
                    for lu, lv, off in sizes:
                        for _ in range(2):
                            u, v = np.zeros(3, F), np.zeros(3, F)
                            u[b if v_on_c else c] = F(su * lu * rng.uniform(0.5, 1.0))
                            v[c if v_on_c else b] = F(sv * lv * rng.uniform(0.5, 1.0))
                            corner = np.array([F(off * rng.uniform(-1, 1)) if k == a else F(rng.uniform(-1, 1) * max(lu, lv)) for k in range(3)], F)
                            recs.append(pack_quad(corner, u, v))
    rec = np.array(recs, F)
    zero_slots = [0, 1, 2, 8, 9, 10, 11, 12, 13, 14, 15, 16]
    flip = rng.random((len(rec), len(zero_slots))) < 0.5
    for j, k in enumerate(zero_slots):
        z = (rec[:, k] == 0) & flip[:, j]
        rec[z, k] = F(-0.0)
    return rec


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def pack_quad(corner, u, v):
    with np.errstate(all="ignore"):
        n = np.array(cross(u, v), F)
        nn = F(dot(n, n))
        w = (n / nn).astype(F)
        d = F(dot(n, corner))
        nu = (n / F(np.sqrt(nn))).astype(F)
    return np.concatenate([n, [d], corner, [F(0)], v, w, u, nu]).astype(F)


def replay(rec, consts, o, d, t_best):
    """Both forms of rt_path.h trav_leaf's quad test on arrays of f32 (one quad record row and one constants row per ray).
    Returns (accept generic, accept specialised, t, in_range, p)."""
    q = [rec[:, k] for k in range(20)]
    n, dd, corner = q[0:3], q[3], q[4:7]
    v, w, u = q[8:11], q[11:14], q[14:17]
    A, wa, B = [consts[:, k] for k in range(3)], consts[:, 3], [consts[:, k] for k in range(4, 7)]
    with np.errstate(all="ignore"):
        dir_norm = dot(d, n)
        t = (dd - dot(o, n)) / dir_norm
        in_range = (T_MIN <= t) & (t < t_best)
        p = [(o[k] + t * d[k]) - corner[k] for k in range(3)]
        alpha = dot(cross(p, v), w)
        beta = dot(cross(u, p), w)
        gen = in_range & (0 <= alpha) & (alpha < 1) & (0 <= beta) & (beta < 1)
        alpha_s = wa * dot(p, A)
        beta_s = wa * dot(p, B)
        spe = in_range & (0 <= alpha_s) & (alpha_s < 1) & (0 <= beta_s) & (beta_s < 1)
    for x in (t, alpha, beta, alpha_s, beta_s, *p):
        assert x.dtype == np.float32
    return gen, spe, t, in_range, p, (alpha, beta, alpha_s, beta_s)


def ulps(x, k):
    """x moved by k ulps (k: integer array), through the bit pattern of |x| (x != 0)."""
    b = np.abs(x).astype(F).view(np.int32) + k.astype(np.int32)
    return np.copysign(b.view(np.float32), x)


def make_rays(rec, per_quad, seed):
    """per_quad rays for every quad record (rows repeated), of the classes the module docstring lists.  Returns (quad index, o, d, t_best, class)."""
    rng = np.random.default_rng(seed)
    nq = len(rec)
    qi = np.repeat(np.arange(nq), per_quad)
    r = rec[qi]
    m = len(qi)
    corner, v, u, nrm = r[:, 4:7], r[:, 8:11], r[:, 14:17], r[:, 0:3]
    axis = np.argmax(nrm != 0, axis=1)
    cls = np.tile(np.arange(per_quad) % 10, nq)
    with np.errstate(all="ignore"):
        # a target point on the quad's plane: parameters at, near and beyond the edges
        special = np.array([0.0, 1.0, 0.5, 1e-7, 1.0 - 6e-8, 1.0 + 1.2e-7, -1e-7, 0.25, 1.5, -0.5], F)
        al = np.where(rng.random(m) < 0.7, special[rng.integers(0, len(special), m)], rng.uniform(-0.3, 1.3, m)).astype(F)
        be = np.where(rng.random(m) < 0.7, special[rng.integers(0, len(special), m)], rng.uniform(-0.3, 1.3, m)).astype(F)
        target = (corner + al[:, None] * u + be[:, None] * v).astype(F)
        size = np.maximum(np.abs(u).max(axis=1), np.abs(v).max(axis=1)).astype(F)
        o = (target + (rng.uniform(-2, 2, (m, 3)) * size[:, None])).astype(F)
        rows = np.arange(m)
        height = (size * rng.uniform(0.01, 3.0, m) * rng.choice([-1.0, 1.0], m)).astype(F)
        o[rows, axis] = (corner[rows, axis] + height).astype(F)
        d = (target - o).astype(F)
        d = (d * rng.choice([1.0, 0.37, 1e-3, 40.0], m)[:, None].astype(F)).astype(F)
        t_best = np.full(m, np.inf, F)
        # 1: straight down the normal from above a point ON an edge / corner / inside: p's in-plane components are exact
        k = cls == 1
        o[k] = target[k]
        o[k, axis[k]] = (corner[k, axis[k]] + height[k]).astype(F)
        d[k] = 0
        d[k, axis[k]] = -height[k]
        z = k & (rng.random(m) < 0.5)
        d[z] = np.where(d[z] == 0, F(-0.0), d[z])
        # 2: parallel to the plane (d_a = +-0), from on and off the plane
        k = cls == 2
        d[k, axis[k]] = np.where(rng.random(k.sum()) < 0.5, F(0.0), F(-0.0))
        on = k & (rng.random(m) < 0.3)
        o[on, axis[on]] = corner[on, axis[on]]
        # 3: one or two zero direction components (never the normal's: those rays still hit)
        k = cls == 3
        other = (axis[k] + 1 + rng.integers(0, 2, k.sum())) % 3
        d[np.flatnonzero(k), other] = 0
        # 4: the origin ON the quad's edges and corners (t ~ 0) and just behind t_min
        k = cls == 4
        o[k] = target[k]
        far = k & (rng.random(m) < 0.5)                                   # 0.001 off the plane, unit direction back to it: t ~ t_min
        unit = np.zeros((m, 3), F)
        unit[rows, axis] = 1
        side = rng.choice([-1.0, 1.0], far.sum())[:, None].astype(F)
        o[far] = (target[far] + unit[far] * F(0.001) * side).astype(F)
        d[far] = (-side * unit[far] * ulps(np.ones(far.sum(), F), rng.integers(-3, 4, far.sum()))[:, None]).astype(F)   # |d| = 1 +- a few ulps
        # 5: the hit point moved by a few ulps around the edges (the direction's in-plane components nudged)
        k = cls == 5
        for c in range(3):
            nz = k & (d[:, c] != 0)
            d[nz, c] = ulps(d[nz, c], rng.integers(-3, 4, nz.sum()))
        # 6: magnitudes up to 1e38 in the direction: t d overflows in one, two or three components
        k = cls == 6
        idx = np.flatnonzero(k)
        scale = F(10.0) ** rng.uniform(30, 38.5, (len(idx), 3)).astype(F)
        mask = rng.random((len(idx), 3)) < 0.6
        d[idx] = np.where(mask, (np.where(d[idx] == 0, F(1), np.sign(d[idx])) * scale).astype(F), d[idx])
        #    ... along the normal too: from -3.2e38 towards a plane at up to +-3e38 (the tiny quads' corners), t ~ 4..12 stays finite
        #    (n.n is small there) while t d_a overflows
        na = idx[rng.random(len(idx)) < 0.5]
        side = np.where(corner[na, axis[na]] < 0, F(-1), F(1))
        o[na, axis[na]] = (-side * F(3.2e38)).astype(F)
        d[na, axis[na]] = (side * rng.uniform(0.5e38, 1.5e38, len(na))).astype(F)
        all3 = na[rng.random(len(na)) < 0.5]                              # ... with both in-plane components huge as well
        for c in (1, 2):
            d[all3, (axis[all3] + c) % 3] = (rng.choice([-1.0, 1.0], len(all3)) * rng.uniform(0.5e38, 1.5e38, len(all3))).astype(F)
        # 7: ... and in the origin
        k = cls == 7
        idx = np.flatnonzero(k)
        scale = F(10.0) ** rng.uniform(30, 38.5, (len(idx), 3)).astype(F)
        mask = rng.random((len(idx), 3)) < 0.5
        o[idx] = np.where(mask, (rng.choice([-1.0, 1.0], (len(idx), 3)) * scale).astype(F), o[idx])
        d[idx] = (target[idx] - o[idx]).astype(F)
        big_d = k & (rng.random(m) < 0.5)
        d[big_d] = (d[big_d] * F(0.25)).astype(F)
        # 8, 9: filled in by the caller (t at t_best needs t); 0: the plain rays above
    return qi, o.astype(F), d.astype(F), t_best, cls


def test_generic_and_specialised_forms_agree_on_a_million_pairs(driver):
    rec = make_quads()
    ok, consts = driver.consts(rec)
    assert ok.all() and len(rec) == 3 * 2 * 4 * 7 * 2
    # the set covers every (axis, assignment, sign of u, sign of v) and zeros of both signs
    axis = np.argmax(rec[:, 0:3] != 0, axis=1)
    v_axis = np.argmax(rec[:, 8:11] != 0, axis=1)
    su = np.sign(rec[:, 14:17].sum(axis=1))
    sv = np.sign(rec[:, 8:11].sum(axis=1))
    combos = {(int(a), int((va - a) % 3), float(x), float(y)) for a, va, x, y in zip(axis, v_axis, su, sv)}
    assert len(combos) == 3 * 2 * 2 * 2
    zeros = rec[:, [8, 9, 10, 11, 12, 13, 14, 15, 16]]
    assert np.any((zeros == 0) & np.signbit(zeros)) and np.any((zeros == 0) & ~np.signbit(zeros))
    # the header's constants are the single products' factors
    b, c = (axis + 1) % 3, (axis + 2) % 3
    rows = np.arange(len(rec))
    v, u, w = rec[:, 8:11], rec[:, 14:17], rec[:, 11:14]
    on_c = v[rows, c] != 0
    assert np.array_equal(consts[rows, 3].view(np.uint32), w[rows, axis].view(np.uint32))
    assert np.all(np.where(on_c, consts[rows, b] == v[rows, c], consts[rows, c] == -v[rows, b]))
    assert np.all(np.where(on_c, consts[rows, 4 + c] == u[rows, b], consts[rows, 4 + b] == -u[rows, c]))
    assert np.count_nonzero(consts[:, 0:3]) == len(rec) and np.count_nonzero(consts[:, 4:7]) == len(rec) and not consts[:, 7].any()

    per_quad = 3600
    qi, o, d, t_best, cls = make_rays(rec, per_quad, seed=5)
    assert len(qi) >= 1_000_000
    r, k = rec[qi], consts[qi]
    ov, dv = [o[:, j] for j in range(3)], [d[:, j] for j in range(3)]
    _, _, t0, _, _, _ = replay(r, k, ov, dv, t_best)
    # 8: t_best AT this quad's t (rejected: t < t_best is strict) and one ulp above it (accepted if inside); 9: a closer hit already found
    at = (cls == 8) & np.isfinite(t0) & (t0 > 0)
    t_best[at] = np.where(np.arange(at.sum()) % 2 == 0, t0[at], np.nextafter(t0[at], F(np.inf)))
    nearer = (cls == 9) & np.isfinite(t0)
    t_best[nearer] = (t0[nearer] * np.random.default_rng(3).uniform(0.2, 3.0, nearer.sum())).astype(F)
    gen, spe, t, in_range, p, planar = replay(r, k, ov, dv, t_best)

    # coverage of what the docstring promises
    finite_p = [np.isfinite(x) for x in p]
    n_bad = sum((~f).astype(int) for f in finite_p)
    for want in (1, 2, 3):
        assert np.count_nonzero(in_range & (n_bad == want)) > 100, want
    assert np.count_nonzero(gen) > 100_000 and np.count_nonzero(in_range & ~gen) > 100_000
    with np.errstate(all="ignore"):
        dn = dot(dv, [r[:, j] for j in range(3)])
    assert np.count_nonzero(dn == 0) > 50_000                                       # parallel
    assert np.count_nonzero((d == 0).sum(axis=1) == 2) > 10_000                     # two zero direction components
    near_min = np.abs(t - T_MIN) <= 4 * np.spacing(T_MIN)                           # t at t_min: within 4 ulps, accepted and rejected
    assert np.count_nonzero(near_min & (t >= T_MIN)) > 10 and np.count_nonzero(near_min & (t < T_MIN)) > 10
    assert np.count_nonzero(t == t_best) > 10_000 and np.count_nonzero(in_range & (np.nextafter(t, F(np.inf)) == t_best)) > 10_000
    alpha, beta, alpha_s, beta_s = planar
    for x in (alpha, beta):
        fin = np.isfinite(x) & in_range
        assert np.count_nonzero(fin & (x == 0)) > 1_000 and np.count_nonzero(fin & (x == 1)) > 100
        assert np.count_nonzero(fin & (x != 1) & (np.abs(x - 1) <= 2 * np.spacing(F(1)))) > 100      # within an ulp of 1
        assert np.count_nonzero(fin & (x != 0) & (np.abs(x) < 1e-6)) > 100                            # next to 0, both sides
    # the claim itself: the same value wherever p is finite (up to the sign of a zero), rejection by both forms wherever it is not
    allfin = finite_p[0] & finite_p[1] & finite_p[2]
    for g, s in ((alpha, alpha_s), (beta, beta_s)):
        same = (g == s) | (np.isnan(g) & np.isnan(s))
        assert np.all(same[allfin]), "the dot form is the cross form's value for a finite p"
    assert not np.any(gen[~allfin]) and not np.any(spe[~allfin])
    assert np.array_equal(gen, spe), "same accept decision for every pair"
    t_gen, t_spe = np.where(gen, t, t_best), np.where(spe, t, t_best)
    assert np.array_equal(t_gen.view(np.uint32), t_spe.view(np.uint32)), "same t bits for every pair"
