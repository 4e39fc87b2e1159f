// mis_weight.h - what the two weighted units share (nee.hip trt_nee_mis, direct.hip trt_direct_mis): ONE copy of the weight of a ray's own
// hit on a light, on the device, and of the table rule that makes the two strategies' weights sum to 1, on the host.  mis_hit_weight was
// moved here from nee.hip as it stood: nee_kernel compiles to the instructions it had.
#pragma once

#include <algorithm>
#include <vector>

#include "kernels.h"
#include "rt_path.h"
#include "scene_query.h"

namespace trt {

// The weight of a ray's own hit on a light (tinyrt.h trt_nee_mis, "light hit"; trt_direct_mis, step 2): wb for the hit primitive, reached at
// parameter t of `ray` from a surfel whose cosine with the ray was csh.  `normal` is the record's (unit; only |dot| is taken, so either
// facing gives the same bits).  The area is the primitive's own, in the bits trt_scene_emitters writes: |n| of the packed un-normalised
// quad normal, 4 pi r^2 with the header's constant for a sphere.
template <int MODE>
TRT_DEV float mis_hit_weight(const SceneAcc<MODE>& sc, uint32_t prim, const Ray& ray, const V3& normal, float t, float csh, uint32_t n_emitters,
                             uint32_t heuristic) {
    const uint32_t pidx = prim & PRIM_INDEX_MASK;
    float area;
    if (prim & PRIM_QUAD_BIT) {
        const float4 q0 = sc.quad(0, pidx);
        area = __builtin_sqrtf((q0.x * q0.x + q0.y * q0.y) + q0.z * q0.z);
    } else {
        const float r = sc.sphere(pidx).w;
        area = 12.566371f * (r * r);
    }
    const float clh = __builtin_fabsf(dot(normal, ray.d));
    const float g = ((csh * clh) / (t * t)) * ((area * (float)n_emitters) * 0.318309886f);
    const float qg = heuristic == TRT_MIS_POWER ? g * g : g;
    return csh > 0.0f && __builtin_fabsf(qg) < __builtin_inff() ? qg / (1.0f + qg) : 1.0f;
}
// ... where the emitter was chosen by power through an alias table (trt_direct_mis_pick): the light's choice probability is not 1 / E but
// ph = power / total_power, recomputed from the hit in the builder's operations (tinyrt.h trt_emitter_pick_build; `emission` is the hit
// material's colour) so that it has the bits of the table's prob for that light.  An overload, not a run-time branch: the uniform form
// above stands as it stood, and nee_kernel and direct_mis_kernel compile to the instructions they had.
template <int MODE>
TRT_DEV float mis_hit_weight(const SceneAcc<MODE>& sc, uint32_t prim, const Ray& ray, const V3& normal, float t, float csh, const V3& emission,
                             float total_power, uint32_t heuristic) {
    const uint32_t pidx = prim & PRIM_INDEX_MASK;
    float area;
    if (prim & PRIM_QUAD_BIT) {
        const float4 q0 = sc.quad(0, pidx);
        area = __builtin_sqrtf((q0.x * q0.x + q0.y * q0.y) + q0.z * q0.z);
    } else {
        const float r = sc.sphere(pidx).w;
        area = 12.566371f * (r * r);
    }
    const float clh = __builtin_fabsf(dot(normal, ray.d));
    const float pw = ((0.2126f * emission.x + 0.7152f * emission.y) + 0.0722f * emission.z) * area;
    const float ph = pw / total_power;
    const float g = ((csh * clh) / (t * t)) * ((area / ph) * 0.318309886f);
    const float qg = heuristic == TRT_MIS_POWER ? g * g : g;
    return csh > 0.0f && __builtin_fabsf(qg) < __builtin_inff() ? qg / (1.0f + qg) : 1.0f;
}

// The unit normal of HitRecord::new (hittable/mod.rs:28-48) for the primitive `ray` hits at t, as rt_path.h shade_body builds it, less the
// facing: the quad's n.normalized() as packed, the sphere's (ray.at(t) - centre).normalized().
template <int MODE>
TRT_DEV V3 hit_unit_normal(const SceneAcc<MODE>& sc, uint32_t prim, const Ray& ray, float t) {
    const uint32_t pidx = prim & PRIM_INDEX_MASK;
    if (prim & PRIM_QUAD_BIT) {
        const float4 q4 = sc.quad(4, pidx);
        return v3(q4.y, q4.z, q4.w);
    }
    const float4 sp = sc.sphere(pidx);
    return normalized(ray_at(ray, t) - v3(sp.x, sp.y, sp.z));
}

// The table rule of the weighted queries, which only a host form can check: the entries that name a geometry are exactly the scene's
// TRT_LIGHT geometries (trt_scene_emitters), each once, in any order.  The weights of a light's two strategies sum to 1 only then.
inline int nee_mis_table_check(const trt_scene* s, const trt_emitter* emitters, uint32_t n_emitters) {
    uint32_t count = 0;
    int rc = trt_scene_emitters(s, nullptr, 0u, &count);
    if (rc != TRT_OK) return rc;
    std::vector<trt_emitter> own(count);
    rc = trt_scene_emitters(s, own.data(), count, &count);
    if (rc != TRT_OK) return rc;
    std::vector<uint32_t> want, have;
    for (const trt_emitter& e : own) want.push_back(e.geometry);
    for (uint32_t i = 0; i < n_emitters; i++)
        if (emitters[i].geometry != 0xFFFFFFFFu) have.push_back(emitters[i].geometry);
    std::sort(want.begin(), want.end());
    std::sort(have.begin(), have.end());
    if (want != have)
        return query_fail(TRT_ERR_INVALID_ARG, "the table's entries with a geometry must be the scene's lights, each once (trt_scene_emitters)");
    return TRT_OK;
}

}  // namespace trt
