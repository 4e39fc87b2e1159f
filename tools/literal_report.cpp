// literal_report.cpp - compiles the lock-step kernel for one leaf list on the host (no device needed) the way streamed.hip does at run time,
// and reports what the unit costs: the generator's statistics, the scene facts it was told (scene_facts.h), the hiprtc compile time, the
// code object's size.  The code object is written next to the source of the unit, for `llvm-readelf --notes` (registers, scratch, spills)
// and `llvm-objdump -d` (tools/literal_isa_counts.py counts the VALU instructions and register copies of the kernel and its round loop).
//   literal_report <leaf file> <n_leaves> <pairs> <planes> <out prefix> [minw] [facts word]      writes <out prefix>.hip and <out prefix>.co
// `facts word`: what trt_scene_facts gives for the scene (tinyrt.h; 0 or absent: no facts, the unit's text is the one without them).
// Build (after `make -C tiny-raytracer_amd/csrc`, which writes rtc_headers.inc):
//   g++ -std=c++17 -O1 -I tiny-raytracer_amd/csrc tools/literal_report.cpp -ldl -o literal_report
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <string>
#include <vector>

#include "flat_literal_rtc.h"

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s <leaf file> <n_leaves> <pairs> <planes> <out prefix> [minw] [facts word]\n", argv[0]); return 64; }
    std::vector<unsigned char> bytes;
    if (FILE* f = fopen(argv[1], "rb")) { int c; while ((c = fgetc(f)) != EOF) bytes.push_back((unsigned char)c); fclose(f); }
    const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10);
    if (bytes.size() < 32u * (size_t)n) { fprintf(stderr, "file shorter than the list\n"); return 64; }
    const int minw = argc > 6 ? atoi(argv[6]) : 6;
    const uint32_t word = argc > 7 ? (uint32_t)strtoul(argv[7], nullptr, 0) : 0u;
    trt::SceneFacts facts;
    facts.no_sphere = (word & 1u) != 0u; facts.axis_exact = (word & 2u) != 0u; facts.nearest_first = (word & 4u) != 0u;
    facts.lazy_color = (word & 8u) != 0u; facts.straight_shade = (word & 16u) != 0u; facts.kinds = (word >> 8) & 0xFu;
    uint32_t m[3];
    trt::flat_reuse_masks(bytes.data(), n, true, m);
    std::string text;
    trt::FlatCacheStats st;
    if (!trt::flat_literal_cached_asm(bytes.data(), n, m, (uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]), text, st)) { fprintf(stderr, "refused\n"); return 2; }
    const std::string source = trt::flat_literal_source(text, st.extra_operands, facts);
    const std::string prefix = argv[5];
    if (FILE* f = fopen((prefix + ".hip").c_str(), "wb")) { fwrite(source.data(), 1, source.size(), f); fclose(f); }
    trt::FlatLiteralBuild built;
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = trt::flat_literal_compile(source, minw, "gfx950", nullptr, built);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!ok) { fprintf(stderr, "compile failed: %s\n", built.log.c_str()); return 1; }
    if (FILE* f = fopen((prefix + ".co").c_str(), "wb")) { fwrite(built.code.data(), 1, built.code.size(), f); fclose(f); }
    size_t lines = 0;
    for (char ch : text) lines += ch == '\n';
    printf("{\"pairs\": %s, \"planes\": %s, \"cached\": %d, \"intervals\": %u, \"plane_distances\": %u, \"evictions\": %u, \"far_reuses\": %u, \"extra_operands\": %u, "
           "\"text_lines\": %zu, \"facts\": {\"word\": %u, \"no_sphere\": %d, \"kinds\": %u, \"axis_exact\": %d, \"nearest_first\": %d, \"lazy_color\": %d, "
           "\"straight_shade\": %d}, \"hiprtc_seconds\": %.3f, \"code_object_bytes\": %zu, \"kernel\": \"%s\"}\n",
           argv[3], argv[4], st.cached ? 1 : 0, st.intervals, st.plane_distances, st.evictions, st.far_reuses, st.extra_operands, lines, facts.word(),
           facts.no_sphere ? 1 : 0, facts.kinds, facts.axis_exact ? 1 : 0, facts.nearest_first ? 1 : 0, facts.lazy_color ? 1 : 0, facts.straight_shade ? 1 : 0,
           secs, built.code.size(), built.kernel.c_str());
    return 0;
}
