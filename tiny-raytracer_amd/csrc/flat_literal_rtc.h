// flat_literal_rtc.h - compiles stream_pool_kernel for one scene at run time: the source is one #define (flat_literal.h: the scene's box
// phase) and `#include "stream_pool.h"`, the headers are the copies embedded at build time (rtc_headers.inc), the compiler is hiprtc, found
// at run time (dlopen: a machine without it renders through the kernels built ahead of time).  Host code only; needs no device - the
// result is a code object for the architecture named, which the caller loads (streamed.hip) or inspects (tools, tests).
#pragma once

#include <dlfcn.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "flat_literal.h"
#include "scene_facts.h"

namespace trt {

struct RtcHeader { const char* name; const char* text; };
// the project's headers, as the Makefile embedded them
inline const std::vector<RtcHeader>& rtc_project_headers() {
    static const std::vector<RtcHeader> h = {
#include "rtc_headers.inc"
    };
    return h;
}
// What the headers ask of the toolchain, as hiprtc wants it: its own built-in header already declares the HIP device API, the vector types and
// the fixed-width integers (in a namespace of its own), so these stand-ins are all there is behind the angle-bracket includes.
inline const std::vector<RtcHeader>& rtc_system_headers() {
    static const std::vector<RtcHeader> h = {
        {"hip/hip_runtime.h", "#pragma once\n"},
        {"stdint.h", "#pragma once\n"
                     "typedef signed char int8_t; typedef unsigned char uint8_t; typedef short int16_t; typedef unsigned short uint16_t;\n"
                     "typedef int int32_t; typedef unsigned int uint32_t; typedef long int64_t; typedef unsigned long uint64_t;\n"
                     "typedef unsigned long uintptr_t; typedef long intptr_t;\n"},
        {"stddef.h", "#pragma once\n#ifndef offsetof\n#define offsetof(t, m) __builtin_offsetof(t, m)\n#endif\n"},
        // (hiprtc's memcpy is a device function; the headers' host-side helpers, parsed but never emitted, name a host one)
        {"string.h", "#pragma once\ninline void* memcpy(void* d, const void* s, unsigned long n) { return __builtin_memcpy(d, s, n); }\n"},
        {"math.h", "#pragma once\n"},
    };
    return h;
}

// hiprtc's entry points, by name (the types are plain: the library is not linked and its header is not needed)
struct HiprtcApi {
    typedef void* Program;
    int (*create)(Program*, const char*, const char*, int, const char* const*, const char* const*) = nullptr;
    int (*destroy)(Program*) = nullptr;
    int (*add_name)(Program, const char*) = nullptr;
    int (*compile)(Program, int, const char* const*) = nullptr;
    int (*log_size)(Program, size_t*) = nullptr;
    int (*log)(Program, char*) = nullptr;
    int (*lowered)(Program, const char*, const char**) = nullptr;
    int (*code_size)(Program, size_t*) = nullptr;
    int (*code)(Program, char*) = nullptr;
    bool ok = false;
};
// `beside`: an address inside the HIP runtime's library (any HIP function), or null: hiprtc is looked for by name first, then next to it.
inline const HiprtcApi& hiprtc_api(const void* beside) {
    static const HiprtcApi api = [beside] {
        HiprtcApi a;
        void* h = nullptr;
        for (const char* name : {"libhiprtc.so", "libhiprtc.so.7", "libhiprtc.so.6"}) {
            h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (h) break;
        }
        Dl_info info;
        if (!h && beside && dladdr(beside, &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) h = dlopen((dir.substr(0, slash + 1) + "libhiprtc.so").c_str(), RTLD_NOW | RTLD_LOCAL);
        }
        if (!h) return a;
        auto sym = [&](auto& fn, const char* name) { fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name)); return fn != nullptr; };
        a.ok = sym(a.create, "hiprtcCreateProgram") && sym(a.destroy, "hiprtcDestroyProgram") && sym(a.add_name, "hiprtcAddNameExpression") &&
               sym(a.compile, "hiprtcCompileProgram") && sym(a.log_size, "hiprtcGetProgramLogSize") && sym(a.log, "hiprtcGetProgramLog") &&
               sym(a.lowered, "hiprtcGetLoweredName") && sym(a.code_size, "hiprtcGetCodeSize") && sym(a.code, "hiprtcGetCode");
        return a;
    }();
    return api;
}

struct FlatLiteralBuild {
    std::vector<char> code;          // the code object
    std::string kernel;              // the kernel's symbol in it
    std::string log;                 // why not, or the compiler's remarks
};

// The source of the unit for this asm text (flat_literal_asm, or flat_literal_cached_asm with the `extra_operands` of its statistics) and
// these scene facts (scene_facts.h; none: the text is the one without them, byte for byte).
inline std::string flat_literal_source(const std::string& asm_text, uint32_t extra_operands = 0u, const SceneFacts& facts = SceneFacts{}) {
    return flat_literal_define("TRT_FLAT_LITERAL_ASM", asm_text) + "#define TRT_FLAT_LITERAL_EXTRA " + std::to_string(extra_operands) + "\n" +
           scene_facts_defines(facts) + "#include \"stream_pool.h\"\n";
}

// stream_pool_kernel<MODE_LDS, false, minw, 256, WALK_FLAT, true> with this box phase, for `arch` ("gfx950"), with the library's flags.
// `source`: flat_literal_source(...) - or anything else, to see the failure path.  False with `log` set if hiprtc is missing or refuses.
inline bool flat_literal_compile(const std::string& source, int minw, const char* arch, const void* beside, FlatLiteralBuild& out) {
    const HiprtcApi& rtc = hiprtc_api(beside);
    if (!rtc.ok) { out.log = "hiprtc not found"; return false; }
    std::vector<const char*> names, texts;
    for (const auto* set : {&rtc_system_headers(), &rtc_project_headers()})
        for (const RtcHeader& h : *set) { names.push_back(h.name); texts.push_back(h.text); }
    HiprtcApi::Program prog = nullptr;
    if (rtc.create(&prog, source.c_str(), "stream_pool_literal.hip", (int)names.size(), texts.data(), names.data()) != 0) { out.log = "hiprtcCreateProgram failed"; return false; }
    const std::string expr = "&trt::stream_pool_kernel<1, false, " + std::to_string(minw) + ", 256, 2, true>";
    const std::string arch_opt = std::string("--offload-arch=") + arch;
    const char* opts[] = {arch_opt.c_str(), "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"};
    int rc = rtc.add_name(prog, expr.c_str());
    if (rc == 0) rc = rtc.compile(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
    size_t n = 0;
    if (rtc.log_size(prog, &n) == 0 && n > 1) { out.log.resize(n); rtc.log(prog, &out.log[0]); }
    bool ok = rc == 0;
    const char* lowered = nullptr;
    if (ok) ok = rtc.lowered(prog, expr.c_str(), &lowered) == 0 && lowered != nullptr;
    if (ok) out.kernel = lowered;
    if (ok) ok = rtc.code_size(prog, &n) == 0 && n > 0;
    if (ok) { out.code.resize(n); ok = rtc.code(prog, out.code.data()) == 0; }
    if (!ok && out.log.empty()) out.log = "hiprtc failed (" + std::to_string(rc) + ")";
    rtc.destroy(&prog);
    return ok;
}

}  // namespace trt
