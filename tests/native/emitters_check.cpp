// emitters_check.cpp - trt_scene_emitters and the two emitter init functions (tinyrt.h; capi.hip, scene_host.cpp) as a stand-alone host
// program for the sanitizers: the records are read back from the packed scene, so every index into it is exercised here - worlds of
// spheres only, quads only and both, with no light, one light and lights at both ends of the insertion order - with cap 0, a cap below
// the count and the exact count.  Prints "ok all".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/tinyrt.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static void run(int n_spheres, int n_quads, int light_every) {
    trt_world* w = nullptr;
    CHECK(trt_world_create(&w) == TRT_OK);
    trt_material grey{TRT_LAMBERTIAN, {0.5f, 0.5f, 0.5f}, 0.0f}, lamp{TRT_LIGHT, {3.0f, 2.0f, 1.0f}, 0.0f};
    CHECK(trt_world_add_material(w, "grey", &grey) == TRT_OK && trt_world_add_material(w, "lamp", &lamp) == TRT_OK);
    uint32_t m_grey = 0, m_lamp = 0;
    CHECK(trt_world_get_material(w, "grey", &m_grey) == TRT_OK && trt_world_get_material(w, "lamp", &m_lamp) == TRT_OK);
    std::vector<uint32_t> want;                       // insertion indices of the lights
    std::vector<uint32_t> want_kind;
    const int total = n_spheres + n_quads;
    for (int g = 0; g < total; g++) {
        const bool light = light_every > 0 && (g % light_every == 0 || g == total - 1);
        const uint32_t m = light ? m_lamp : m_grey;
        const bool quad = n_spheres == 0 || (n_quads > 0 && g % 2 == 1 && g / 2 < n_quads);
        const float f = (float)g;
        if (quad) CHECK(trt_world_add_quad(w, trt_vec3{f, 0.0f, 0.0f}, trt_vec3{0.5f, 0.0f, 0.25f}, trt_vec3{0.0f, 0.5f, f * 0.125f}, m) == TRT_OK);
        else CHECK(trt_world_add_sphere(w, trt_vec3{f, 2.0f, 1.0f}, 0.25f + f * 0.01f, m) == TRT_OK);
        if (light) { want.push_back((uint32_t)g); want_kind.push_back(quad ? 1u : 0u); }
    }
    trt_scene* s = nullptr;
    CHECK(trt_scene_create(w, &s) == TRT_OK);
    uint32_t count = 12345;
    CHECK(trt_scene_emitters(s, nullptr, 0, &count) == TRT_OK && count == want.size());
    CHECK(trt_scene_emitters(s, nullptr, 1, &count) == TRT_ERR_INVALID_ARG);
    CHECK(trt_scene_emitters(nullptr, nullptr, 0, &count) == TRT_ERR_INVALID_ARG && trt_scene_emitters(s, nullptr, 0, nullptr) == TRT_ERR_INVALID_ARG);
    for (size_t cap : {(size_t)1, want.size() / 2, want.size()}) {
        if (cap == 0 || cap > want.size()) continue;
        std::vector<trt_emitter> out(cap);                          // exactly cap entries: a write behind it is the sanitizer's to find
        CHECK(trt_scene_emitters(s, out.data(), (uint32_t)cap, &count) == TRT_OK && count == want.size());
        for (size_t k = 0; k < cap; k++) {
            CHECK(out[k].geometry == want[k] && out[k].kind == want_kind[k]);
            CHECK(out[k].color.x == 3.0f && out[k].color.y == 2.0f && out[k].color.z == 1.0f && out[k].reserved[0] == 0u && out[k].reserved[1] == 0u);
            trt_emitter again;
            memset(&again, 0xCD, sizeof again);
            if (out[k].kind == 1u) trt_emitter_init_quad(&again, out[k].a, out[k].b, out[k].c, out[k].color);
            else trt_emitter_init_sphere(&again, out[k].a, out[k].b.x, out[k].color);
            CHECK(again.geometry == 0xFFFFFFFFu);
            again.geometry = out[k].geometry;
            CHECK(memcmp(&again, &out[k], sizeof again) == 0);      // the scene's record is the init function's, byte for byte
            CHECK(out[k].area > 0.0f);
        }
    }
    trt_scene_destroy(s);
    trt_world_destroy(w);
}

int main() {
    trt_emitter_init_quad(nullptr, trt_vec3{0, 0, 0}, trt_vec3{1, 0, 0}, trt_vec3{0, 1, 0}, trt_vec3{1, 1, 1});
    trt_emitter_init_sphere(nullptr, trt_vec3{0, 0, 0}, 1.0f, trt_vec3{1, 1, 1});
    for (int every : {0, 1, 3, 1000}) {
        run(7, 0, every);
        run(0, 7, every);
        run(40, 40, every);
        run(1, 0, every);
        run(0, 1, every);
    }
    run(700, 300, 5);
    printf("ok all\n");
    return 0;
}
