// wave_run.h - what the kernels that give every wave a contiguous run of work items share on the device: the ray queries (query.hip: a run
// of the caller's rays), the feature buffers (aov.hip: a run of the local image's pixels) and the sparse render (pixels.hip: a run of the
// pixel list).  ONE copy of the lane rank, the run of a wave, the place of the leaf stacks, the cursor step of the round loop's refill
// and the surface record of a closest hit; each kernel keeps its own loop body, because what a lane carries and does with a finished
// walk differs.  The host side of the same units is stream_plan.h (kernel table entry, launch rule) and query_plan.h (launch preamble).
// The sample queries - radiance.hip (radiance and gather: a run of the caller's rays or surfels), ambient.hip, probe.hip, passes.hip,
// direct.hip and nee.hip - take the run, the leaf stacks and the refill step from here too, and keep their own round loops for the same
// reason: the walk block of those loops (trav_begin / trav_unpark / closest_hit_resume | closest_hit) as a helper that takes walking,
// n_rays, prim and t by reference changes 3 000 to 19 000 lines of their assembly.  What surrounds the loops is shared: the shade body
// (rt_path.h shade_body), the draws (gather_draw.h), the launch (query_plan.h) and the two forms' scaffold (host_stage.h).
//
// Every function here is a pure function of values, and that is deliberate: with these the device assembly of all kernels that use them
// is, instruction for instruction, what their own copies gave.  Forms that did more were built and dropped because the compiler then
// emits other code, measurably slower in places (1 - 7 % on the sparse render and on occlusion queries): a run helper that returns
// through references with the early-out inside, a refill helper that holds the guard and updates the cursor, and a helper for a lane's
// offset into its leaf stack, `(threadIdx.x >> 6) * (64u * slots) + lane` - so that one expression stays in the kernels
// (stream_sample_kernel included), behind lds_behind_scene.  streamed.hip and wavefront.hip take wave_rank, streamed.hip lds_behind_scene.
#pragma once

#include "rt_path.h"

namespace trt {

// Number of set bits of a ballot mask below this lane.
TRT_DEV uint32_t wave_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The run of this wave: wave w owns items [w * per_wave, ...) of n.  wave_begin: its first item, in 64 bits - at or past n the wave owns
// none and returns (after the staging barriers); wave_count: the length of the run that begins at `begin` < n.
template <int THREADS>
TRT_DEV unsigned long long wave_begin(uint32_t per_wave) {
    const uint32_t wave = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    return (unsigned long long)wave * per_wave;
}
TRT_DEV uint32_t wave_count(uint32_t n, uint32_t per_wave, uint32_t begin) { return n - begin < per_wave ? n - begin : per_wave; }

// The dynamic LDS behind the scene copy (16-byte aligned): the backend-private area.  The postponed-leaf stacks (rt_path.h
// walk_fast_lds) begin here: slots x 64 x 8 bytes per wave, a lane's entries 64 apart.  The sizes of these parts, for the host: stream_plan.h
// LdsLayout (scene copy aligned to 16 | stacks); the address stays written out here and in the kernels (see the head of this file).
template <int MODE>
TRT_DEV char* lds_behind_scene(const SceneAcc<MODE>& sc) {
    return reinterpret_cast<char*>(g_lds) + ((sc.lds_bytes() + 15u) & ~15u);
}

// The refill step of a round: the lanes of the ballot `need` take the next items of the run in lane order - lane's item is
// cursor + wave_rank(need), taken if it is below count - and the wave-uniform cursor advances by their number, up to count.
TRT_DEV uint32_t wave_advance(uint32_t cursor, uint64_t need, uint32_t count) {
    cursor += (uint32_t)__builtin_popcountll(need);
    if (cursor > count) cursor = count;
    return cursor;
}

// The surface record of a closest hit (prim != PRIM_NONE) at ray.at(t): what HitRecord::new (hittable/mod.rs:28-48) makes of the winning
// primitive, from the lines of rt_path.h shade_hit that compute front_face, normal and the material index, in their operation order.
// `geometry` is the primitive's insertion index (scene_query.h geo_index).
struct HitSurface {
    V3 normal;                       // unit, facing the ray
    uint32_t geometry, material;
    bool front_face;
};
template <int MODE>
TRT_DEV HitSurface hit_surface(const SceneAcc<MODE>& sc, const uint32_t* __restrict__ geo_index, const Ray& ray, uint32_t prim, float t) {
    const uint32_t k = prim & PRIM_INDEX_MASK;
    HitSurface h;
    if (prim & PRIM_QUAD_BIT) {
        const float4 q0 = sc.quad(0, k), q1 = sc.quad(1, k), q4 = sc.quad(4, k);
        h.front_face = dot(ray.d, v3(q0.x, q0.y, q0.z)) < 0.0f;            // outward normal = n, un-normalised (quad.rs:45)
        const V3 nu = v3(q4.y, q4.z, q4.w);                                // n.normalized(), precomputed on the host
        h.normal = h.front_face ? nu : -nu;
        h.material = __float_as_uint(q1.w);
    } else {
        const float4 sp = sc.sphere(k);
        const V3 outward = ray_at(ray, t) - v3(sp.x, sp.y, sp.z);          // sphere.rs:47-51 (p = ray.at(t))
        h.front_face = dot(ray.d, outward) < 0.0f;
        const V3 nu = normalized(outward);
        h.normal = h.front_face ? nu : -nu;
        h.material = sc.sphere_material(k);
    }
    h.geometry = geo_index[k + ((prim & PRIM_QUAD_BIT) ? sc.L.n_spheres : 0u)];
    return h;
}

}  // namespace trt
