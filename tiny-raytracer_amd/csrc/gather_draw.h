// gather_draw.h - what the units that draw a sample's first ray about a caller-supplied surfel share: the gather queries (radiance.hip:
// the drawn ray starts a path), the ambient queries (ambient.hip: the drawn ray is an occlusion query), the probe queries (probe.hip) and the
// direct-light queries (direct.hip: the drawn ray is a shadow ray towards a drawn point on an emitter; nee.hip draws the same from a path's
// vertices: ONE body, direct_draw_from, behind both).  ONE copy of the item load and of the draws on the device, and on the host of the
// argument checks that more than one unit applies: trt_gather_params as a gather takes it (gather_check) and as passes.hip and nee.hip
// take it (gather_source_check), trt_radiance_params (radiance_check), the emitter table of direct.hip and nee.hip.  The device
// functions are pure functions of values (wave_run.h says why): moved here from radiance.hip as they stood, radiance_kernel compiles to
// the registers it had.
#pragma once

#include <type_traits>

#include "kernels.h"
#include "rt_path.h"

namespace trt {

TRT_DEV Ray rad_load_ray(const float* __restrict__ rays, uint32_t idx) {
    const float* r = rays + 6ull * idx;
    Ray ray;
    ray.o = v3(r[0], r[1], r[2]);
    ray.d = v3(r[3], r[4], r[5]);
    return ray;
}

// The first ray of a gather sample: the scatter rule of the lobe applied to the surfel (point, axis) = (item.o, item.d) with the draws
// of g, in the operations of rt_path.h shade_hit (hence of the oracle's material_scatter).  Three draws are taken from g.
// Cosine, lambertian.rs:16-22: axis + random_unit_vector, the axis itself if that is near zero; cone, metal.rs:18-25 with the axis in
// the place of the reflected direction: axis + spread * random_in_unit_sphere.  Ray::new normalises (ray.rs:12-14).
TRT_DEV Ray gather_ray(const float* __restrict__ items, uint32_t idx, uint32_t lobe, float spread, Rng& g) {
    const V3 in_sphere = random_in_unit_sphere_unit(g);
    const Ray item = rad_load_ray(items, idx);                              // after the draw: six registers less while it runs
    V3 dir;
    if (lobe == TRT_LOBE_COSINE) {
        dir = item.d + normalized(in_sphere);
        if (near_zero(dir)) dir = item.d;
    } else {
        dir = item.d + spread * in_sphere;
    }
    return ray_new(item.o, dir);
}

// The first ray of a probe sample (probe.hip): a direction uniform over the sphere, Vec3::new_random_unit_vector (vec3extend.rs:32-34), or
// over the hemisphere about the item's axis, Vec3::new_random_on_hemisphere (vec3extend.rs:36-43: the unit vector itself where its dot
// with the axis is > 0, else its negation - a zero or NaN dot flips).  Three draws are taken from g.  Ray::new normalises again
// (ray.rs:12-14), which changes the bits of about a quarter of the directions.  The axis is read by the hemisphere domain only.
TRT_DEV Ray probe_ray(const float* __restrict__ items, uint32_t idx, bool hemisphere, Rng& g) {
    const V3 u = normalized(random_in_unit_sphere_unit(g));
    const float* it = items + 6ull * idx;                                   // after the draw, as in gather_ray
    V3 dir = u;
    if (hemisphere) {
        const V3 axis = v3(it[3], it[4], it[5]);
        if (!(dot(u, axis) > 0.0f)) dir = -u;
    }
    return ray_new(v3(it[0], it[1], it[2]), dir);
}

// The shadow ray of a direct-light sample (direct.hip): a point y on one emitter of the caller's table (tinyrt.h trt_emitter: 20 words a
// record, read through the lane's own index - vector loads - once the first draw has chosen it), the ray from the surfel towards it and what
// an unoccluded sample folds.  In tinyrt.h's operation order, one IEEE f32 operation per operator:
//   u0 = random; e = min(uint32(u0 * float(E)), E - 1)
//   quad:    a = random; b = random; y = (corner + u * a) + v * b; nl = normal
//   sphere:  nl = random_unit_vector (probe_ray's); y = centre + nl * radius
//   w = y - x; d2 = w.w; cs = n.w; cl = |nl.w|; wgt = ((cs * cl) / (d2 * d2)) * ((area * float(E)) * (1 / pi))
// live: cs > 0, d2 > 0 and wgt finite - a NaN anywhere fails one of the three.  Three draws (quad) or four (sphere) are taken from g.
struct DirectSample {
    Ray ray;                         // Ray::new(x, w): normalised
    V3 c;                            // colour * wgt
    float t_max;                     // sqrt(d2) * shadow_end: the walk covers [0.001, t_max)
    bool live;
};
// ... with step 5's weight and the record's `geometry` word besides, which the weighted next-event kernels (nee.hip, MIS) weigh the
// sample by.  A type of its own, filled under `if constexpr`: the other callers' code is the code they had.
struct WeightedDirectSample : DirectSample {
    float wgt;
    uint32_t geometry;
};
// How step 2 chooses the emitter.  UniformPick: e = the slot of the first draw, probability 1 / E (trt_direct, trt_nee and their weighted
// forms).  AliasPick (trt_direct_pick, trt_direct_mis_pick): one draw more decides between the slot and its alias in a caller-supplied
// Walker/Vose table (tinyrt.h trt_emitter_pick: 4 words a record - q, alias, prob, reserved), and step 5 divides by the chosen record's
// `prob` where the uniform choice multiplies by E:
//   u0 = random; k = min(uint32(u0 * float(E)), E - 1); u1 = random; e = u1 < q[k] ? k : min(alias[k], E - 1)      (a NaN q takes the alias)
//   scale = (area / prob[e]) * (1 / pi)
// Two vector loads more through the lane's own index, both ahead of the emitter record's; the min keeps every read inside the E records
// whatever the table holds.
struct UniformPick {
    TRT_DEV uint32_t choose(uint32_t slot, uint32_t, Rng&, float&) const { return slot; }
    TRT_DEV float scale(float area, float fe, float) const { return (area * fe) * 0.318309886f; }
};
struct AliasPick {
    const float* __restrict__ table;
    TRT_DEV uint32_t choose(uint32_t slot, uint32_t n_emitters, Rng& g, float& prob) const {
        const float u1 = rng_random(g);
        const float* __restrict__ const rec = table + 4ull * slot;
        const uint32_t alias = __float_as_uint(rec[1]);
        const uint32_t e = u1 < rec[0] ? slot : (alias < n_emitters - 1u ? alias : n_emitters - 1u);
        prob = table[4ull * e + 2u];
        return e;
    }
    TRT_DEV float scale(float area, float, float prob) const { return (area / prob) * 0.318309886f; }
};
// ONE body for the surfel of an item (direct.hip) and for a surfel held in registers (nee.hip): `surfel()` returns (point, normal) as
// a Ray and is called after the draws, where an item is loaded so that its six registers are free while the draws run.  The choice and
// step 5's scale are the policy's, resolved at compile time: with the default policy the code is the code it was.
template <class Surfel, class Sample = DirectSample, class Pick = UniformPick>
TRT_DEV Sample direct_draw_from(Surfel surfel, const float* __restrict__ emitters, uint32_t n_emitters, float shadow_end, Rng& g, Pick policy = Pick{}) {
    const float fe = (float)n_emitters;
    const uint32_t pick = (uint32_t)(rng_random(g) * fe);
    float prob = 0.0f;
    const float* __restrict__ const em = emitters + 20ull * policy.choose(pick < n_emitters - 1u ? pick : n_emitters - 1u, n_emitters, g, prob);
    const V3 a = v3(em[2], em[3], em[4]);
    V3 y, nl;
    if (__float_as_uint(em[0]) == 1u) {
        const float ra = rng_random(g);
        const float rb = rng_random(g);
        y = (a + v3(em[5], em[6], em[7]) * ra) + v3(em[8], em[9], em[10]) * rb;
        nl = v3(em[11], em[12], em[13]);
    } else {
        nl = normalized(random_in_unit_sphere_unit(g));
        y = a + nl * em[5];
    }
    const Ray item = surfel();
    const V3 w = y - item.o;
    const float d2 = dot(w, w);
    const float cs = dot(item.d, w);
    const float cl = __builtin_fabsf(dot(nl, w));
    const float scale = policy.scale(em[17], fe, prob);
    const float wgt = ((cs * cl) / (d2 * d2)) * scale;
    Sample smp;
    smp.live = cs > 0.0f && d2 > 0.0f && __builtin_fabsf(wgt) < __builtin_inff();
    smp.ray = ray_new(item.o, w);
    smp.t_max = __builtin_sqrtf(d2) * shadow_end;
    smp.c = v3(em[14], em[15], em[16]) * wgt;
    if constexpr (std::is_same_v<Sample, WeightedDirectSample>) {
        smp.wgt = wgt;
        smp.geometry = __float_as_uint(em[1]);
    }
    return smp;
}
TRT_DEV DirectSample direct_draw(const float* __restrict__ items, uint32_t idx, const float* __restrict__ emitters, uint32_t n_emitters,
                                 float shadow_end, Rng& g) {
    return direct_draw_from([&] { return rad_load_ray(items, idx); }, emitters, n_emitters, shadow_end, g);
}
// ... with the weight and the `geometry` word, for the weighted direct-light kernel (direct.hip, direct_mis_kernel).
TRT_DEV WeightedDirectSample direct_draw_weighted(const float* __restrict__ items, uint32_t idx, const float* __restrict__ emitters,
                                                  uint32_t n_emitters, float shadow_end, Rng& g) {
    auto surfel = [&] { return rad_load_ray(items, idx); };
    return direct_draw_from<decltype(surfel), WeightedDirectSample>(surfel, emitters, n_emitters, shadow_end, g);
}
// The two draws of the direct-light kernels behind one name: PICK chooses the emitter through the alias table (direct.hip, PICK kernels).
template <bool PICK, class Sample>
TRT_DEV Sample direct_draw_item(const float* __restrict__ items, uint32_t idx, const float* __restrict__ emitters, const float* __restrict__ pick,
                                uint32_t n_emitters, float shadow_end, Rng& g) {
    auto surfel = [&] { return rad_load_ray(items, idx); };
    if constexpr (PICK) return direct_draw_from<decltype(surfel), Sample, AliasPick>(surfel, emitters, n_emitters, shadow_end, g, AliasPick{pick});
    else return direct_draw_from<decltype(surfel), Sample>(surfel, emitters, n_emitters, shadow_end, g);
}
// The same sample for a vertex of a path (nee.hip): x the point, n the unit normal on the side the light is gathered on.
TRT_DEV DirectSample direct_draw_at(const V3& x, const V3& n, const float* __restrict__ emitters, uint32_t n_emitters, float shadow_end, Rng& g) {
    return direct_draw_from([&] { Ray r; r.o = x; r.d = n; return r; }, emitters, n_emitters, shadow_end, g);
}
TRT_DEV WeightedDirectSample direct_draw_at_weighted(const V3& x, const V3& n, const float* __restrict__ emitters, uint32_t n_emitters,
                                                     float shadow_end, Rng& g) {
    auto surfel = [&] { Ray r; r.o = x; r.d = n; return r; };
    return direct_draw_from<decltype(surfel), WeightedDirectSample>(surfel, emitters, n_emitters, shadow_end, g);
}
// The two draws of the next-event kernels behind one name, as direct_draw_item is for the items: PICK chooses the emitter through the alias
// table (nee.hip, PICK kernels); without it the sample is direct_draw_at's / direct_draw_at_weighted's and `pick` is not read.
template <bool PICK, class Sample>
TRT_DEV Sample direct_draw_at(const V3& x, const V3& n, const float* __restrict__ emitters, const float* __restrict__ pick, uint32_t n_emitters,
                              float shadow_end, Rng& g) {
    auto surfel = [&] { Ray r; r.o = x; r.d = n; return r; };
    if constexpr (PICK) return direct_draw_from<decltype(surfel), Sample, AliasPick>(surfel, emitters, n_emitters, shadow_end, g, AliasPick{pick});
    else return direct_draw_from<decltype(surfel), Sample>(surfel, emitters, n_emitters, shadow_end, g);
}

// The lobe of a launch: 0 for a radiance query (the items are rays), else what trt_gather_params carries.
struct Lobe {
    uint32_t lobe;                   // 0: a radiance query
    float spread;
};

// Host side (defined in radiance.hip), declared here because only the units that include this header need it: a header for a handful of
// declarations would be a file more.
// What the forms that take a trt_gather_params check before any device work: trt_radiance's rules on p->path, then the lobe; and the
// kernel arguments of the parameters (radiance.hip).  `sums`: the required output buffer.
int gather_check(const trt_scene* s, const trt_ray* items, uint32_t n, const trt_gather_params* p, const float* sums, RenderArgs& ra, Lobe& lobe);
// trt_radiance's own rules on a trt_radiance_params, which gather_check applies to p->path and the probe queries (probe.hip) to theirs.
int radiance_check(const trt_scene* s, const trt_ray* rays, uint32_t n, const trt_radiance_params* p, const float* sums, RenderArgs& ra);
// The source, spread and reserved words of a trt_gather_params whose lobe word is an enum trt_passes_source (passes.hip, nee.hip).
int gather_source_check(const trt_gather_params& g);
// The emitter table's pointer and size (1 .. 2^20 where n > 0) and shadow_end, for both forms of direct.hip and nee.hip; and the table's
// entries, which only a host form can read.
int emitter_table_check(uint32_t n, const trt_emitter* emitters, uint32_t n_emitters, float shadow_end);
int emitter_entries_check(const trt_emitter* emitters, uint32_t n_emitters);

}  // namespace trt
