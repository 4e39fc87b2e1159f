// scene_facts.h - what the kernel compiled at run time for ONE scene (flat_literal.h, flat_literal_rtc.h, streamed.hip) is told about that
// scene beyond its leaf planes.  Host code only, plain C++.
//
// The unit's source is a handful of #defines in front of `#include "stream_pool.h"`.  The facts below are written there as further #defines
// (scene_facts_defines); rt_path.h reads them through constexpr values (kFactNoSphere ...) whose defaults - no define - say NOTHING, so every
// kernel built ahead of time, and a unit written without them, is the general kernel: any scene, any material, spheres or quads.
//
// A fact is claimed only where the host copy of the packed scene (scene.h) proves it; what cannot be read, or is out of range, claims nothing:
//   no_sphere      the scene has no sphere and every leaf of the walk-order list is a quad: no quad-bit test, no sphere branch.
//   kinds          bit k: some primitive references a material of trt_material_kind k.  A kind whose bit is clear cannot be hit
//                  (shade_straight drops the light compare of a scene without a light).  0: not claimed.
//   axis_exact     the scene's axis-exact-quads switch is on (FlatReuse::axis_quads: every quad axis-exact and the lock-step kernel rewrites
//                  the records of its LDS copy) AND no_sphere.  Reported; the kernel keeps the run-time switch.
//   nearest_first  the nearest-first switch (FlatReuse::nearest_first) is on, with axis_exact.  Reported; the kernel keeps the run-time switch.
//   lazy_color     SceneLayout::lazy_color (the unit is the LAZY instantiation whatever this says; a condition of straight_shade).
//   straight_shade kinds is a subset of {Lambertian, Light}, with no_sphere and lazy_color: every lane runs ONE straight-line shade body
//                  (rt_path.h shade_straight) and a path ends where kind == LIGHT or the budget is spent.
// The run-time switches the facts replace are launch arguments that never change for a scene handle (capi.hip: RenderArgs::flat_reuse is the
// handle's own), and the facts are part of what a LiteralKernel was compiled for: a launch whose facts differ does not take it.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

namespace trt {

struct SceneFacts {
    bool no_sphere = false;
    uint32_t kinds = 0u;
    bool axis_exact = false;
    bool nearest_first = false;
    bool lazy_color = false;
    bool straight_shade = false;
    bool any() const { return no_sphere || kinds != 0u || axis_exact || nearest_first || lazy_color || straight_shade; }
    bool operator==(const SceneFacts& o) const {
        return no_sphere == o.no_sphere && kinds == o.kinds && axis_exact == o.axis_exact && nearest_first == o.nearest_first &&
               lazy_color == o.lazy_color && straight_shade == o.straight_shade;
    }
    bool operator!=(const SceneFacts& o) const { return !(*this == o); }
    // one word: bit 0 no_sphere, 1 axis_exact, 2 nearest_first, 3 lazy_color, 4 straight_shade, bits 8 ... 11 kinds (tinyrt.h trt_scene_facts)
    uint32_t word() const {
        return (no_sphere ? 1u : 0u) | (axis_exact ? 2u : 0u) | (nearest_first ? 4u : 0u) | (lazy_color ? 8u : 0u) | (straight_shade ? 16u : 0u) | (kinds << 8);
    }
};

constexpr uint32_t kFactKindCount = 4u;              // trt_material_kind: Lambertian 0, Metal 1, Dielectric 2, Light 3
constexpr uint32_t kFactMaxLeaves = 32u;             // flat_literal.h kFlatLiteralMaxLeaves: a longer list has no kernel of its own

// TRT_SCENE_FACTS: 0 = none (the unit's text is the one without this header, byte for byte), 1 = the facts as constants alone, anything
// else and unset = those and the straight-line shade.
enum : uint32_t { SCENE_FACTS_NONE = 0u, SCENE_FACTS_CONSTANTS = 1u, SCENE_FACTS_ALL = 2u };

// The facts of a scene from its packed parts (scene.h): the walk-order leaf list (n_leaves x 32 bytes, link = word 7), the quad records
// (80 bytes each, the material index = word 7), the spheres' material indices and the materials' kinds (u32 each), and the switches the
// scene handle has derived (axis_quads.h, nearest_first.h) and SceneLayout::lazy_color.  Nothing is claimed for a null or empty list, a
// list of more than 32 leaves, a list that is not one leaf per primitive, or a link, material index or kind out of range.
inline SceneFacts scene_facts_derive(const void* leaf_list, uint32_t n_leaves, const void* quads, uint32_t n_quads, uint32_t n_spheres,
                                     const uint32_t* sphere_material, const uint32_t* material_kind, uint32_t n_materials, uint32_t axis_quads,
                                     uint32_t nearest_first, uint32_t lazy_color, uint32_t level = SCENE_FACTS_ALL) {
    SceneFacts f;
    if (level == SCENE_FACTS_NONE || leaf_list == nullptr || n_leaves == 0u || n_leaves > kFactMaxLeaves || material_kind == nullptr) return f;
    if ((uint64_t)n_quads + n_spheres != n_leaves) return f;                                // a primitive outside the list would have its kind left out
    const unsigned char* lp = static_cast<const unsigned char*>(leaf_list);
    bool all_quads = n_spheres == 0u;
    uint32_t kinds = 0u;
    for (uint32_t i = 0; i < n_leaves; i++) {
        uint32_t link, mat;
        memcpy(&link, lp + 32u * (size_t)i + 28u, sizeof link);
        const uint32_t idx = link & 0x3FFFFFFFu;                                            // PRIM_INDEX_MASK (scene.h)
        if (link & 0x80000000u) return SceneFacts{};                                        // NODE_INNER_BIT: not a leaf
        if (link & 0x40000000u) {                                                           // PRIM_QUAD_BIT
            if (quads == nullptr || idx >= n_quads) return SceneFacts{};
            memcpy(&mat, static_cast<const unsigned char*>(quads) + 80u * (size_t)idx + 28u, sizeof mat);
        } else {
            all_quads = false;
            if (sphere_material == nullptr || idx >= n_spheres) return SceneFacts{};
            mat = sphere_material[idx];
        }
        if (mat >= n_materials || material_kind[mat] >= kFactKindCount) return SceneFacts{};
        kinds |= 1u << material_kind[mat];
    }
    f.no_sphere = all_quads;
    f.kinds = kinds;
    f.axis_exact = f.no_sphere && axis_quads != 0u;
    f.nearest_first = f.axis_exact && nearest_first != 0u;
    f.lazy_color = lazy_color != 0u;
    f.straight_shade = level >= SCENE_FACTS_ALL && f.no_sphere && f.lazy_color && (kinds & ~((1u << 0) | (1u << 3))) == 0u;      // Lambertian and Light only
    return f;
}

// The #defines of the run-time compiled unit for the facts device code reads (rt_path.h: no sphere, the kinds, the straight-line shade);
// "" where none of them is claimed.  axis_exact, nearest_first and lazy_color are derived and reported (trt_scene_facts, the report tool)
// and stay run-time switches in the kernel.
inline std::string scene_facts_defines(const SceneFacts& f) {
    std::string s;
    if (f.no_sphere) s += "#define TRT_FACT_NO_SPHERE 1\n";
    if (f.kinds != 0u) { char b[48]; snprintf(b, sizeof b, "#define TRT_FACT_KINDS 0x%x\n", f.kinds); s += b; }
    if (f.straight_shade) s += "#define TRT_FACT_STRAIGHT_SHADE 1\n";
    return s;
}

}  // namespace trt
