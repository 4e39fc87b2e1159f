// axis_quads.h — the inside test of an axis-aligned quad as two dot products (rt_path.h trav_leaf), and the scene-level switch for it.
//
// Quad::hit's inside test (quad.rs:38-41) is alpha = dot(cross(p, v), w), beta = dot(cross(u, p), w) with p = ray.at(t) - corner, and the
// quad is accepted iff 0 <= alpha < 1 and 0 <= beta < 1 (and t in range): 28 unfused f32 operations.  Call a quad AXIS-EXACT when every
// stored component of n, d, corner, v, w, u, n_unit is finite and
//   * n has exactly one non-zero component, on axis a (b = a + 1, c = a + 2 mod 3),
//   * w's components on b and c are +-0,
//   * u and v each have exactly one non-zero component, one on b and the other on c, of magnitude in [2^-64, 2^16].
// For such a quad and a FINITE p whose products with v's and u's components are finite (the magnitude bound is there for that: below):
//   (p x v)_a = fl(p_b v_c) - fl(p_c v_b), and one of the two products is +-0 (its v component is), so
//       v_c != 0:  (p x v)_a =  fl(p_b v_c)          A = v_c e_b
//       v_b != 0:  (p x v)_a = -fl(p_c v_b)          A = -v_b e_c          (negation is exact: -fl(x y) = fl(x (-y)))
//   the other two components of the cross product are finite and meet w's zeros in the dot product: they add +-0, which changes no
//   non-zero sum, so alpha = fl(w_a (p x v)_a) = fl(w_a dot(p, A)): dot(p, A) = p.x A.x + p.y A.y + p.z A.z, unfused, left to right, is
//   the one non-zero product plus two +-0.  Likewise
//       u_b != 0:  (u x p)_a =  fl(u_b p_c)          B = u_b e_c
//       u_c != 0:  (u x p)_a = -fl(u_c p_b)          B = -u_c e_b
//   and beta = fl(w_a dot(p, B)).  Where a value is zero its SIGN may differ between the two forms (x + -0 against x + +0, 0 - 0
//   against a lone product); it feeds only `0 <= .` and `. < 1`, which do not see the sign of zero.
// A NON-FINITE p (overflow of o + t d or of the subtraction of the corner: t itself is finite wherever in_range holds) is rejected by both
// forms.  Generic: every component of p is multiplied by a zero component of v somewhere in p x v (v has two), inf * 0 and NaN * 0 are NaN,
// and a NaN component of the cross product makes alpha NaN whatever w holds.  Dot form: the zero multiplications are kept - every
// component of p is multiplied by a component of A - so a non-finite p_k gives NaN (A_k zero) or +-inf (A_k not zero) in the sum, which
// ends NaN or +-inf, and so does its product with w_a (inf * 0 = NaN): neither passes 0 <= alpha < 1.
//   p_a     p_b / p_c     generic alpha                          dot-form alpha
//   finite  finite        fl(w_a fl(p_. v_.)) (sign of 0 free)   the same value
//   inf/NaN any           NaN (p_a v_. - .. with v_a = 0)        NaN (p_a * 0)
//   finite  one inf/NaN   NaN (times the zero of v)              NaN or +-inf
//   finite  both inf/NaN  NaN                                    NaN or +-inf
// THE MAGNITUDE BOUND.  The generic form also multiplies p_a, the component ALONG the normal, by v's (u's) non-zero component V - in a
// cross-product component that w's zero then turns into +-0 - and the dot form does not: were p_a V to overflow with p finite, the generic
// alpha would be NaN (inf * 0) where the dot form still accepts.  (Every other product of the generic form is either shared with the dot
// form - p_b V or p_c V, inf in both when it overflows - or has a zero factor.)  p_a is what rounding leaves of a point ON the plane: with
// n = N e_a, t = fl(fl(D - fl(o_a N)) / fl(d_a N)) and D = fl(N c_a), each rounding is worth at most 2^-24 of the largest of |o_a|, |c_a|,
// |t d_a| < 2^128 while t and p are finite, so |p_a| < 2^110 after the handful of them and |p_a V| < 2^126 for |V| <= 2^16.  Where a product
// with N is subnormal (absolute error 2^-150 instead of a relative one) the same chain gives |p_a V| < 2^-22 / |U| for a finite t: the lower
// bound keeps that far from overflow too.  Quads beyond the bound are simply not axis-exact; Cornell's edges are 20 to 100 long.
// t, in_range, t_best and prim_best are computed as before; nothing that reaches the frame changes.  tests/test_axis_quads.py replays both
// forms in f32 on millions of (ray, quad) pairs, overflowing p included, and compiles this header with g++.
//
// The constants (A.xyz, w_a) and (B.xyz, 0) replace elements 2 and 3 of the quad's record - (v.xyz, w.x) (w.y, w.z, u.x, u.y) - in the
// workgroup's LDS copy of the scene only (rt_path.h axis_quads_to_lds); the packed blob never changes.  Plain C++: the scene layer, the
// kernels and the host tests include it.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TRT_AQ_FN __host__ __device__ inline
#else
#define TRT_AQ_FN inline
#endif

namespace trt {

// `rec`: the 20 floats of one packed quad record (scene.h): n.xyz d | corner.xyz material | v.xyz w.x | w.yz u.xy | u.z n_unit.xyz.
// Returns whether the quad is axis-exact; if so out[0..3] = (A.xyz, w_a), out[4..7] = (B.xyz, 0).  No indexing by a run-time value:
// on the device everything stays in registers.
TRT_AQ_FN bool axis_quad_constants(const float* rec, float* out) {
    const float big = 3.4028234663852886e38f;                      // FLT_MAX: |x| <= big iff x is finite
    bool finite = true;
    for (int k = 0; k < 20; k++) finite = finite && (k == 7 || __builtin_fabsf(rec[k]) <= big);      // (element 7 is the material index)
    const bool nx = rec[0] != 0.0f, ny = rec[1] != 0.0f, nz = rec[2] != 0.0f;
    if (!finite || (nx ? 1 : 0) + (ny ? 1 : 0) + (nz ? 1 : 0) != 1) return false;
    // components in the order (a, b, c)
    const float vx = rec[8], vy = rec[9], vz = rec[10], wx = rec[11], wy = rec[12], wz = rec[13], ux = rec[14], uy = rec[15], uz = rec[16];
    const float va = nx ? vx : ny ? vy : vz, vb = nx ? vy : ny ? vz : vx, vc = nx ? vz : ny ? vx : vy;
    const float wa = nx ? wx : ny ? wy : wz, wb = nx ? wy : ny ? wz : wx, wc = nx ? wz : ny ? wx : wy;
    const float ua = nx ? ux : ny ? uy : uz, ub = nx ? uy : ny ? uz : ux, uc = nx ? uz : ny ? ux : uy;
    if (wb != 0.0f || wc != 0.0f || va != 0.0f || ua != 0.0f) return false;
    const float lo = 5.42101086e-20f, hi = 65536.0f;                                 // 2^-64, 2^16: the magnitude bound (above)
    auto edge = [&](float x) { return __builtin_fabsf(x) >= lo && __builtin_fabsf(x) <= hi; };
    const bool v_on_c = edge(vc) && vb == 0.0f && edge(ub) && uc == 0.0f;            // v along c, u along b
    const bool v_on_b = edge(vb) && vc == 0.0f && edge(uc) && ub == 0.0f;            // v along b, u along c
    if (!v_on_c && !v_on_b) return false;
    const float Ab = v_on_c ? vc : 0.0f, Ac = v_on_c ? 0.0f : -vb;
    const float Bb = v_on_c ? 0.0f : -uc, Bc = v_on_c ? ub : 0.0f;
    // back to (x, y, z): a = x -> (0, b, c); a = y -> (c, 0, b); a = z -> (b, c, 0)
    out[0] = nx ? 0.0f : ny ? Ac : Ab; out[1] = nx ? Ab : ny ? 0.0f : Ac; out[2] = nx ? Ac : ny ? Ab : 0.0f; out[3] = wa;
    out[4] = nx ? 0.0f : ny ? Bc : Bb; out[5] = nx ? Bb : ny ? 0.0f : Bc; out[6] = nx ? Bc : ny ? Bb : 0.0f; out[7] = 0.0f;
    return true;
}

// The scene-level switch: 1 iff the lock-step leaf list is in use (`flat_walk`, at most 32 leaves, scene copied to LDS: `in_lds`), the
// scene has quads and EVERY one of them is axis-exact; 0 when `enabled` is false (TRT_AXIS_QUADS=0).  `quads`: n_quads packed records
// of 80 bytes (scene.h off_quad).
inline uint32_t axis_quads_flag(const void* quads, uint32_t n_quads, uint32_t n_leaves, bool flat_walk, bool in_lds, bool enabled) {
    if (!enabled || !flat_walk || !in_lds || quads == nullptr || n_quads == 0u || n_leaves > 32u) return 0u;
    const unsigned char* p = static_cast<const unsigned char*>(quads);
    for (uint32_t i = 0; i < n_quads; i++) {
        float rec[20], out[8];
        memcpy(rec, p + 80u * (size_t)i, sizeof rec);
        if (!axis_quad_constants(rec, out)) return 0u;
    }
    return 1u;
}

}  // namespace trt
