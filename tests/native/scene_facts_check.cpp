// scene_facts_check.cpp - scene_facts.h on the host, without a device: the facts of small packed scenes built here, what is refused, the
// #defines, and a restatement of the unit's source text with and without facts (the real flat_literal_source is held against the same
// text in tests/test_scene_facts.py, on the files tools/literal_report.cpp writes).  tests/test_scene_facts.py compiles it with g++, plain and with
// -fsanitize=address,undefined.
//   scene_facts_check --self                         every case below; prints "self check ok"
//   scene_facts_check source <word>                  the source of the unit for a one-leaf list and the facts of <word> (trt_scene_facts' bits)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "flat_literal.h"
#include "scene_facts.h"

using trt::SceneFacts;

namespace {

int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); g_failed++; } } while (0)

// A packed scene's parts, exactly as large as they are said to be (the sanitizers see every read past an end).
struct Parts {
    std::vector<uint32_t> leaves;      // 8 words per leaf, word 7 = link
    std::vector<uint32_t> quads;       // 20 words per quad, word 7 = material
    std::vector<uint32_t> sphere_mat, kinds;
    uint32_t n_spheres = 0;
    void quad(uint32_t material) { leaves.resize(leaves.size() + 8u, 0u); leaves.back() = 0x40000000u | (uint32_t)(quads.size() / 20u); quads.resize(quads.size() + 20u, 0u); quads[quads.size() - 13u] = material; }
    void sphere(uint32_t material) { leaves.resize(leaves.size() + 8u, 0u); leaves.back() = n_spheres++; sphere_mat.push_back(material); }
    SceneFacts facts(uint32_t aq, uint32_t nf, uint32_t lazy, uint32_t level = trt::SCENE_FACTS_ALL) const {
        return trt::scene_facts_derive(leaves.empty() ? nullptr : leaves.data(), (uint32_t)(leaves.size() / 8u), quads.empty() ? nullptr : quads.data(),
                                       (uint32_t)(quads.size() / 20u), n_spheres, sphere_mat.empty() ? nullptr : sphere_mat.data(), kinds.data(),
                                       (uint32_t)kinds.size(), aq, nf, lazy, level);
    }
};
const uint32_t L = 0, M = 1, D = 2, E = 3;      // trt_material_kind

SceneFacts from_word(uint32_t w) {
    SceneFacts f;
    f.no_sphere = w & 1u; f.axis_exact = w & 2u; f.nearest_first = w & 4u; f.lazy_color = w & 8u; f.straight_shade = w & 16u; f.kinds = (w >> 8) & 0xFu;
    return f;
}

std::string unit_source(const SceneFacts& f) {      // flat_literal_rtc.h flat_literal_source, restated (that header needs the embedded headers)
    uint32_t leaf[8] = {0, 0, 0, 0x3f800000u, 0x3f800000u, 0x3f800000u, 1u, 0x40000000u}, masks[3] = {0, 0, 0};
    std::string text;
    if (!trt::flat_literal_asm(leaf, 1u, masks, text)) return "refused";
    return trt::flat_literal_define("TRT_FLAT_LITERAL_ASM", text) + "#define TRT_FLAT_LITERAL_EXTRA 0\n" + trt::scene_facts_defines(f) + "#include \"stream_pool.h\"\n";
}

void self_check() {
    {   // a Cornell-like scene: Lambertian and light quads, every switch on
        Parts p; p.kinds = {L, L, E}; for (int i = 0; i < 17; i++) p.quad(i % 2); p.quad(2);
        const SceneFacts f = p.facts(1, 1, 1);
        CHECK(f.no_sphere && f.axis_exact && f.nearest_first && f.lazy_color && f.straight_shade && f.kinds == 0x9u && f.word() == 0x91fu);
        CHECK(from_word(f.word()) == f);
        const SceneFacts c = p.facts(1, 1, 1, trt::SCENE_FACTS_CONSTANTS);
        CHECK(c.word() == 0x90fu && !c.straight_shade);
        CHECK(!p.facts(1, 1, 1, trt::SCENE_FACTS_NONE).any());
        CHECK(p.facts(0, 1, 1).word() == 0x919u);                      // nearest-first is claimed with axis-exact only
        CHECK(p.facts(1, 0, 0).word() == 0x903u);                      // no lazy colour: no straight-line shade
    }
    {   // quads and one sphere: nothing that depends on "no sphere"
        Parts p; p.kinds = {L, D, E}; p.quad(0); p.quad(0); p.sphere(1); p.quad(2);
        const SceneFacts f = p.facts(1, 1, 1);
        CHECK(!f.no_sphere && !f.axis_exact && !f.nearest_first && !f.straight_shade && f.lazy_color && f.kinds == 0xDu);
    }
    {   // one Metal quad, one Dielectric quad
        Parts p; p.kinds = {L, M, E}; p.quad(0); p.quad(1); p.quad(2);
        SceneFacts f = p.facts(1, 1, 1);
        CHECK(f.kinds == 0xBu && !f.straight_shade && f.no_sphere && f.nearest_first);
        p.kinds[1] = D; f = p.facts(1, 1, 1);
        CHECK(f.kinds == 0xDu && !f.straight_shade);
    }
    {   // Lambertian only; a light only; a material nobody references is not a kind of the scene
        Parts p; p.kinds = {L, E, M}; p.quad(0); p.quad(0);
        CHECK(p.facts(1, 1, 1).kinds == 0x1u && p.facts(1, 1, 1).straight_shade);
        Parts q; q.kinds = {M, E}; q.quad(1);
        CHECK(q.facts(1, 1, 1).kinds == 0x8u && q.facts(1, 1, 1).straight_shade);
    }
    {   // a tilted quad: the handle's switch is off
        Parts p; p.kinds = {L}; p.quad(0);
        const SceneFacts f = p.facts(0, 0, 1);
        CHECK(f.no_sphere && !f.axis_exact && !f.nearest_first && f.straight_shade);
    }
    {   // nothing claimed: empty, 33 leaves, an inner link, indices out of range, a kind beyond the enum
        Parts p; p.kinds = {L};
        CHECK(!p.facts(1, 1, 1).any());
        for (int i = 0; i < 32; i++) p.quad(0);
        CHECK(p.facts(1, 1, 1).any());
        p.quad(0);
        CHECK(!p.facts(1, 1, 1).any());
        Parts q; q.kinds = {L}; q.quad(0); q.leaves[7] |= 0x80000000u; CHECK(!q.facts(1, 1, 1).any());
        Parts r; r.kinds = {L}; r.quad(0); r.leaves[7] = 0x40000001u; CHECK(!r.facts(1, 1, 1).any());
        Parts s; s.kinds = {L}; s.quad(1); CHECK(!s.facts(1, 1, 1).any());
        Parts t; t.kinds = {4u}; t.quad(0); CHECK(!t.facts(1, 1, 1).any());
        Parts u; u.kinds = {L}; u.sphere(0); u.leaves[7] = 1u; CHECK(!u.facts(1, 1, 1).any());
        Parts v; v.kinds = {L, M}; v.quad(0); v.quad(1); v.leaves.resize(8u); CHECK(!v.facts(1, 1, 1).any());      // a quad no leaf names: not one leaf per primitive
        Parts w; w.kinds = {L}; w.quad(0); w.n_spheres = 1; w.sphere_mat = {0u}; CHECK(!w.facts(1, 1, 1).any());
    }
    // the defines, and the unit's text
    CHECK(trt::scene_facts_defines(SceneFacts{}).empty());
    CHECK(trt::scene_facts_defines(from_word(0x91fu)) == "#define TRT_FACT_NO_SPHERE 1\n#define TRT_FACT_KINDS 0x9\n#define TRT_FACT_STRAIGHT_SHADE 1\n");
    CHECK(trt::scene_facts_defines(from_word(0x00eu)).empty());                                 // the switches alone: reported, not compiled in
    const std::string off = unit_source(SceneFacts{}), on = unit_source(from_word(0x91fu));
    CHECK(off.find("TRT_FACT") == std::string::npos && on.find("TRT_FACT_KINDS 0x9") != std::string::npos);
    CHECK(on.size() > off.size() && on.compare(on.size() - 25u, 25u, off, off.size() - 25u, 25u) == 0);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "--self")) {
        self_check();
        if (g_failed) return 1;
        printf("self check ok\n");
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "source")) {
        fputs(unit_source(from_word((uint32_t)strtoul(argv[2], nullptr, 0))).c_str(), stdout);
        return 0;
    }
    fprintf(stderr, "usage: %s --self | source <word>\n", argv[0]);
    return 64;
}
