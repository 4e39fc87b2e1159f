/* The nearest-first leaf phase (tiny-raytracer_amd/csrc/nearest_first.h) against the walk-order phase it replaces, on the CPU oracle
 * (test infrastructure, links liboracle the way ordered_theorem_check.c does).  The header is C++ and so is this program: it is built
 * with `g++ -x c++` (tests/test_nearest_first.py).  The margin, the host derivation of P and the decision procedure are the header's own
 * functions - the ones the kernel runs; the quad test is the oracle's Quad::hit, the boxes are the oracle's leaf boxes in walk order.
 *
 *   nearest_first_check <scene file> <rays> <mix|paths> [<cold rays out> [<cold rays to replay>]]
 * scene file: the camera position "x y z", then one quad per line, "cx cy cz ux uy uz vx vy vz light" (light: 0 / 1).  A path starts at
 * the camera towards a random point of the scene's extent and ends on a light, as the renderer's do (a path started INSIDE a closed
 * box would stay there).  Every ray runs ONE phase over all its pending leaves from (+inf, none), then the walk again in phases of 1 to
 * 4 pending leaves with the carried t_best (the leaf_slots = 2 situation); each phase is run both ways from the same (T0, P0) and must
 * give the same (t bits, primitive); the chained result must be the oracle's closest hit.  Prints one line of figures; exit status 1
 * on any mismatch.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "nearest_first.h"
#include "rt_oracle.h"

struct Quad { orc_vec3 c, u, v; int light; };
static const uint32_t QUAD_BIT = 0x40000000u, NONE = 0xFFFFFFFFu;

static uint32_t g_rng[2];
static float frand() { return orc_rng_random(g_rng); }
static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static orc_vec3 v3(float x, float y, float z) { orc_vec3 v = {x, y, z}; return v; }
static orc_vec3 cross(orc_vec3 a, orc_vec3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static float dot(orc_vec3 a, orc_vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

struct Scene {
    std::vector<Quad> quads;
    orc_world* w = nullptr;
    std::vector<int> order;                    /* leaf k (walk order) -> quad index */
    std::vector<float> box;                    /* 6 per leaf */
    float P[3];
    float lo[3], hi[3];                        /* the scene's extent */
    orc_vec3 camera;
};

struct Figures {
    long rays = 0, phases = 0, mismatches = 0, oracle_mismatches = 0, second = 0, residual = 0, rerun = 0, out_of_domain = 0, tests_ref = 0, tests_nf = 0,
         hits = 0;
    double worst_ratio = -1e30;
};

struct RayState {                              /* one ray against the scene: boxes and lazily computed intrinsic hits */
    const Scene* s;
    orc_ray ray;
    float start[32], far_[32], t[32];
    int known[32];                             /* 0 unknown, 1 miss, 2 hit */
    long tests;
    bool test(uint32_t leaf, float& t_out) {
        tests++;
        const int q = (int)(leaf & ~QUAD_BIT);
        int k = 0;
        while (s->order[k] != q) k++;
        if (!known[k]) {
            orc_hit_record h;
            const Quad& Q = s->quads[q];
            known[k] = orc_quad_hit(Q.c, Q.u, Q.v, &ray, 0.001f, INFINITY, &h) ? 2 : 1;
            t[k] = h.t;
        }
        t_out = t[k];
        return known[k] == 2;
    }
};

/* the reference phase: leaf_phase + trav_leaf */
static void reference_phase(RayState& rs, const std::vector<int>& pend, float& t_best, uint32_t& prim_best) {
    for (int k : pend) {
        float t;
        if (t_best > rs.start[k] && rs.test(QUAD_BIT | (uint32_t)rs.s->order[k], t) && t < t_best) { t_best = t; prim_best = QUAD_BIT | (uint32_t)rs.s->order[k]; }
    }
}

/* both phases from (t_best, prim_best); returns the nearest-first path bits, -1 on a mismatch */
static int both_phases(RayState& rs, const std::vector<int>& pend, float E, float& t_best, uint32_t& prim_best, Figures& f, bool count) {
    float tr = t_best, tn = t_best;
    uint32_t pr = prim_best, pn = prim_best;
    const float T0 = t_best;
    rs.tests = 0;
    reference_phase(rs, pend, tr, pr);
    f.tests_ref += rs.tests;
    rs.tests = 0;
    const uint32_t path = trt::nearest_first_phase((uint32_t)pend.size(),
        [&](uint32_t k, uint32_t& leaf, float& start) { leaf = QUAD_BIT | (uint32_t)rs.s->order[pend[k]]; start = rs.start[pend[k]]; },
        [&](uint32_t leaf, float& t) { return rs.test(leaf, t); }, E, tn, pn);
    f.tests_nf += rs.tests;
    f.phases++;
    if (count) {
        if (rs.tests >= 2) f.second++;
        if (path & 1u) f.residual++;
        if (path & 2u) f.rerun++;
        for (int k : pend) {                   /* the margin: every pending hit in [t_min, T0) */
            float t;
            if (rs.test(QUAD_BIT | (uint32_t)rs.s->order[k], t) && t < T0) {
                f.hits++;
                const double ratio = ((double)rs.start[k] - (double)t) / (double)E;
                if (ratio > f.worst_ratio) f.worst_ratio = ratio;
            }
        }
    }
    const bool same = bits(tr) == bits(tn) && pr == pn;
    if (!same) {
        if (f.mismatches++ < 5)
            fprintf(stderr, "mismatch: reference (%.9g, %08x) nearest-first (%.9g, %08x) path %u, %zu pending, T0 %.9g\n", tr, pr, tn, pn, path, pend.size(), T0);
    }
    t_best = tr; prim_best = pr;
    return same ? (int)path : -1;
}

/* returns the path bits of the single +inf phase (-1: mismatch, -2: ray outside the margin's domain) */
static int check_ray(const Scene& s, const orc_ray& ray, Figures& f) {
    const float o[3] = {ray.origin.x, ray.origin.y, ray.origin.z}, d[3] = {ray.direction.x, ray.direction.y, ray.direction.z};
    float inv[3];
    for (int a = 0; a < 3; a++) inv[a] = 1.0f / d[a];
    const bool finite = fabsf(o[0]) <= 3.4028234663852886e38f && fabsf(o[1]) <= 3.4028234663852886e38f && fabsf(o[2]) <= 3.4028234663852886e38f;
    if (!finite || !trt::nf_in_domain(inv[0], inv[1], inv[2])) { f.out_of_domain++; return -2; }       /* such rays walk the reference tree */
    const float E = trt::nf_margin(s.P[0], s.P[1], s.P[2], o[0], o[1], o[2], inv[0], inv[1], inv[2]);
    RayState rs;
    rs.s = &s; rs.ray = ray; rs.tests = 0;
    const int n = (int)s.order.size();
    for (int k = 0; k < n; k++) {              /* slab_fast_entry: min / max form */
        float tn = -INFINITY, tf = INFINITY;
        for (int a = 0; a < 3; a++) {
            const float x0 = (s.box[6 * k + a] - o[a]) * inv[a], x1 = (s.box[6 * k + 3 + a] - o[a]) * inv[a];
            tn = fmaxf(tn, fminf(x0, x1));
            tf = fminf(tf, fmaxf(x0, x1));
        }
        rs.start[k] = fmaxf(0.001f, tn);
        rs.far_[k] = tf;
        rs.known[k] = 0;
    }
    f.rays++;
    std::vector<int> pend;
    /* one phase from (+inf, none) */
    for (int k = 0; k < n; k++) if (!(rs.far_[k] <= rs.start[k])) pend.push_back(k);
    float t_best = INFINITY;
    uint32_t prim = NONE;
    const int path = both_phases(rs, pend, E, t_best, prim, f, true);
    orc_hit_record rec;
    int32_t index = -1;
    const int hit = orc_world_hit_index(s.w, &ray, 0.001f, INFINITY, &rec, &index, NULL);
    const bool agrees = hit ? (prim == (QUAD_BIT | (uint32_t)index) && bits(rec.t) == bits(t_best)) : prim == NONE;
    if (!agrees) f.oracle_mismatches++;
    /* the walk again in phases of 1..4 pending leaves with the carried t_best */
    float tb = INFINITY;
    uint32_t pb = NONE;
    pend.clear();
    size_t cap = 1u + (orc_rng_next_u32(g_rng) & 3u);
    for (int k = 0; k < n; k++) {
        if (!(fminf(tb, rs.far_[k]) <= rs.start[k])) pend.push_back(k);
        if (pend.size() == cap || (k == n - 1 && !pend.empty())) {
            both_phases(rs, pend, E, tb, pb, f, false);
            pend.clear();
            cap = 1u + (orc_rng_next_u32(g_rng) & 3u);
        }
    }
    if (bits(tb) != bits(t_best) || pb != prim) f.oracle_mismatches++;
    return path;
}

static float ulps(float x, int k) {
    for (; k > 0; k--) x = nextafterf(x, INFINITY);
    for (; k < 0; k++) x = nextafterf(x, -INFINITY);
    return x;
}
static orc_vec3 interior(const Scene& s) {
    return v3(s.lo[0] + (s.hi[0] - s.lo[0]) * frand(), s.lo[1] + (s.hi[1] - s.lo[1]) * frand(), s.lo[2] + (s.hi[2] - s.lo[2]) * frand());
}
static orc_ray primary(const Scene& s) {
    const orc_vec3 to = interior(s);
    return orc_ray_new(s.camera, v3(to.x - s.camera.x, to.y - s.camera.y, to.z - s.camera.z));
}
static orc_vec3 on_quad(const Quad& q, float a, float b) {
    return v3(q.c.x + a * q.u.x + b * q.v.x, q.c.y + a * q.u.y + b * q.v.y, q.c.z + a * q.u.z + b * q.v.z);
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: nearest_first_check <scene> <rays> <mix|paths> [<cold out> [<cold replay>]]\n"); return 2; }
    Scene s;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    Quad q;
    if (fscanf(in, "%f %f %f", &s.camera.x, &s.camera.y, &s.camera.z) != 3) return 2;
    while (fscanf(in, "%f %f %f %f %f %f %f %f %f %d", &q.c.x, &q.c.y, &q.c.z, &q.u.x, &q.u.y, &q.u.z, &q.v.x, &q.v.y, &q.v.z, &q.light) == 10) s.quads.push_back(q);
    fclose(in);
    const long n_rays = atol(argv[2]);
    const bool paths_only = strcmp(argv[3], "paths") == 0;
    const int n = (int)s.quads.size();
    if (n < 1 || n > 32) return 2;
    s.w = orc_world_new();
    for (int i = 0; i < n; i++) {
        char name[16];
        snprintf(name, sizeof name, "m%d", i);
        orc_world_add_quad(s.w, s.quads[i].c, s.quads[i].u, s.quads[i].v, orc_world_add_material(s.w, name, 0, v3(0.5f, 0.5f, 0.5f), 0.0f));
    }
    orc_world_build(s.w);
    std::vector<float> bbox(6 * 2 * n);
    std::vector<int32_t> prim(2 * n), sub(2 * n);
    const int nn = orc_world_bvh_dump(s.w, bbox.data(), prim.data(), sub.data(), 2 * n);
    for (int a = 0; a < 3; a++) { s.lo[a] = INFINITY; s.hi[a] = -INFINITY; }
    for (int i = 0; i < nn; i++)
        if (prim[i] >= 0) {
            s.order.push_back(prim[i]);
            for (int k = 0; k < 6; k++) s.box.push_back(bbox[6 * i + k]);
            for (int a = 0; a < 3; a++) { s.lo[a] = fminf(s.lo[a], bbox[6 * i + a]); s.hi[a] = fmaxf(s.hi[a], bbox[6 * i + 3 + a]); }
        }
    /* the packed leaf list and quad records (scene.h), for the host derivation */
    std::vector<uint32_t> leaves(8 * n);
    std::vector<float> recs(20 * n);
    for (int k = 0; k < n; k++) {
        memcpy(&leaves[8 * k], &s.box[6 * k], 24);
        leaves[8 * k + 6] = (uint32_t)k + 1u;
        leaves[8 * k + 7] = QUAD_BIT | (uint32_t)s.order[k];
    }
    for (int i = 0; i < n; i++) {              /* quad.rs:20-29, unfused */
        const Quad& Q = s.quads[i];
        const orc_vec3 nrm = cross(Q.u, Q.v);
        const float nn2 = dot(nrm, nrm), len = sqrtf(nn2);
        const float r[20] = {nrm.x, nrm.y, nrm.z, dot(nrm, Q.c), Q.c.x, Q.c.y, Q.c.z, 0.0f, Q.v.x, Q.v.y, Q.v.z, nrm.x / nn2,
                             nrm.y / nn2, nrm.z / nn2, Q.u.x, Q.u.y, Q.u.z, nrm.x / len, nrm.y / len, nrm.z / len};
        memcpy(&recs[20 * i], r, sizeof r);
    }
    const uint32_t flag = trt::nearest_first_flag(leaves.data(), (uint32_t)n, recs.data(), (uint32_t)n, 0u, 1u, true, s.P);
    if (flag != 1u) { fprintf(stderr, "the scene does not get the switch\n"); return 1; }

    Figures f;
    int fail = 0;
    if (argc > 5) {                            /* recorded cold-path rays take their recorded path */
        FILE* rp = fopen(argv[5], "r");
        if (!rp) return 2;
        uint32_t w[7];
        long replayed = 0;
        Figures g;
        while (fscanf(rp, "%x %x %x %x %x %x %x", &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6]) == 7) {
            orc_ray ray;
            memcpy(&ray, w, 24);
            const int path = check_ray(s, ray, g);
            if (path < 0 || ((uint32_t)path & w[6]) != w[6]) { fprintf(stderr, "recorded ray %ld: path %d, recorded %u\n", replayed, path, w[6]); fail = 1; }
            replayed++;
        }
        fclose(rp);
        if (replayed < 1 || g.mismatches || g.oracle_mismatches) fail = 1;
        printf("replayed %ld recorded rays\n", replayed);
    }
    FILE* out = argc > 4 && argv[4][0] ? fopen(argv[4], "w") : nullptr;
    int kept[2] = {0, 0};
    orc_rng_seed(20261017u, (uint32_t)n, 0u, g_rng);
    orc_ray ray = primary(s);
    int bounce = 0;
    while (f.rays + f.out_of_domain < n_rays) {
        const uint32_t kind = paths_only ? 0u : orc_rng_next_u32(g_rng) % 20u;
        bool path_ray = false;
        if (kind < 13u) {                      /* a bounced Lambertian path from the camera: the renderer's distribution */
            path_ray = true;
        } else if (kind < 16u) {               /* towards a point within a few ulps of a quad's edge or corner */
            const Quad& Q = s.quads[orc_rng_next_u32(g_rng) % (uint32_t)n];
            const uint32_t c = orc_rng_next_u32(g_rng);
            const float a = (c & 1u) ? (float)((c >> 1) & 1u) : frand(), b = ((c & 4u) || !(c & 1u)) ? (float)((c >> 3) & 1u) : frand();
            orc_vec3 target = on_quad(Q, a, b);
            target = v3(ulps(target.x, (int)((c >> 4) % 7u) - 3), ulps(target.y, (int)((c >> 8) % 7u) - 3), ulps(target.z, (int)((c >> 12) % 7u) - 3));
            const orc_vec3 from = interior(s);
            ray = orc_ray_new(from, v3(target.x - from.x, target.y - from.y, target.z - from.z));
        } else if (kind < 18u) {               /* one direction component down to 1e-7 */
            orc_vec3 dd = orc_random_unit_vector(g_rng);
            const uint32_t c = orc_rng_next_u32(g_rng);
            static const float decade[7] = {1e-1f, 1e-2f, 1e-3f, 1e-4f, 1e-5f, 1e-6f, 1e-7f};       /* (no libm call: the same rays on every machine) */
            const float tiny = ((c & 4u) ? 1.0f : -1.0f) * decade[(c >> 16) % 7u] * (1.0f + 8.0f * frand());
            if (c % 3u == 0u) dd.x = tiny; else if (c % 3u == 1u) dd.y = tiny; else dd.z = tiny;
            ray = orc_ray_new((c & 8u) ? interior(s) : on_quad(s.quads[(c >> 4) % (uint32_t)n], frand(), frand()), dd);
        } else {                               /* from a point on a quad */
            ray = orc_ray_new(on_quad(s.quads[orc_rng_next_u32(g_rng) % (uint32_t)n], frand(), frand()), orc_random_unit_vector(g_rng));
        }
        const int path = check_ray(s, ray, f);
        if (out && path > 0) {
            const int which = (path & 2) ? 1 : 0;
            if (kept[which] < 64) {
                uint32_t w[6];
                memcpy(w, &ray, 24);
                fprintf(out, "%08x %08x %08x %08x %08x %08x %x\n", w[0], w[1], w[2], w[3], w[4], w[5], which ? 2u : 1u);
                kept[which]++;
            }
        }
        /* the next segment of the path: Lambertian scatter at the hit (lambertian.rs), a fresh path after 12 bounces or a miss */
        orc_hit_record rec;
        int32_t at = -1;
        if (path_ray && bounce < 12 && orc_world_hit_index(s.w, &ray, 0.001f, INFINITY, &rec, &at, NULL) && !s.quads[at].light) {
            const orc_vec3 r = orc_random_unit_vector(g_rng);
            ray = orc_ray_new(rec.point, v3(rec.normal.x + r.x, rec.normal.y + r.y, rec.normal.z + r.z));
            bounce++;
        } else {
            ray = primary(s);
            bounce = 0;
        }
    }
    if (out) fclose(out);
    printf("%d quads %ld rays %ld phases: mismatches %ld oracle_mismatches %ld worst_ratio %.4f second %.3e rerun %.3e residual_count %ld rerun_count %ld "
           "out_of_domain %ld tests_ref %.4f tests_nf %.4f kept %d %d\n",
           n, f.rays, f.phases, f.mismatches, f.oracle_mismatches, f.worst_ratio, (double)f.second / (double)f.rays, (double)f.rerun / (double)f.rays, f.residual,
           f.rerun, f.out_of_domain, (double)f.tests_ref / (double)f.phases, (double)f.tests_nf / (double)f.phases, kept[0], kept[1]);
    orc_world_free(s.w);
    return (fail || f.mismatches || f.oracle_mismatches) ? 1 : 0;
}
