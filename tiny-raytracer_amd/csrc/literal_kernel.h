// literal_kernel.h - where a scene keeps the kernel that was compiled for it at run time (flat_literal.h, streamed.hip), and how a render
// asks for it.  Host code only, and nothing of HIP by name: scene_cache.h holds one LiteralKernel per scene and device, the C ABI layer
// (capi.hip) says per render whether the scene wants one, and streamed.hip - the only unit that compiles, loads and launches it - finds
// the request in a thread-local for the length of the launch_streamed call.  The launchers' signatures stay as they are that way.
#pragma once

#include <stdint.h>

#include <condition_variable>
#include <mutex>

#include "scene_facts.h"

namespace trt {

// One scene's run-time compiled kernel on one device.  UNTRIED -> COMPILING (one thread; the others wait) -> READY or FAILED, for good: a
// scene compiles once, and one that could not be compiled renders through the kernels built ahead of time from then on.
struct LiteralKernel {
    enum State { UNTRIED, COMPILING, READY, FAILED };
    std::mutex mu;
    std::condition_variable cv;
    State state = UNTRIED;
    void* module = nullptr;                  // hipModule_t
    void* function = nullptr;                // hipFunction_t
    int minw = 0;                            // the launch bound it was instantiated with (stream_plan.h: the plan's row)
    SceneFacts facts;                        // the scene facts it was compiled with (scene_facts.h): a launch with other facts does not take it
    void (*unload)(void* module) = nullptr;  // set by the unit that loaded it
    // Call with no render of the scene in flight on the device (SceneCache's destructor has waited for them).
    void release() {
        if (module && unload) unload(module);
        module = function = nullptr;
        state = UNTRIED;
    }
};

// The interval cache of the scene's kernel: how many register pairs hold slab intervals and how many registers single plane distances.
// Measured on Cornell (profiles/ic_flat_cache_ab.txt): every further pair and every further plane register gained, 3 / 4 / 5 /
// 6 / 8 pairs and 8 pairs with 2 / 4 / 6 plane registers in one interleaved run; the 16 registers live only inside the box phase, below
// the kernel's register peak (70 VGPRs at every setting).
constexpr uint32_t kLiteralIntervalPairs = 8u, kLiteralPlaneRegs = 6u;

// What a render says about its scene: the host copy of the leaf list (n_leaves x 32 bytes, walk order) and whether the scene should run
// its own kernel now (TRT_FLAT_LITERAL: 0 never, 1 at the first streamed render, unset: at the first render large enough).
struct LiteralRequest {
    LiteralKernel* slot = nullptr;
    const void* leaf_list = nullptr;
    uint32_t n_leaves = 0;
    bool wanted = false;
    bool empty_source = false;               // TRT_FLAT_LITERAL_TEST_FAIL=1: the compiler is handed an empty source (tests of the fallback)
    uint32_t interval_pairs = kLiteralIntervalPairs;   // the cached stream's registers (flat_literal.h flat_literal_cached_asm):
    uint32_t plane_regs = kLiteralPlaneRegs;           //   TRT_FLAT_LITERAL_PAIRS 3 ... 8, TRT_FLAT_LITERAL_PLANES 0 ... 8; (3, 0): no cached stream
    SceneFacts facts;                        // what the handle has derived about the scene (scene_facts.h; TRT_SCENE_FACTS=0: nothing)
};
inline thread_local const LiteralRequest* t_literal_request = nullptr;
class LiteralScope {
  public:
    explicit LiteralScope(const LiteralRequest* r) { t_literal_request = r; }
    LiteralScope(const LiteralScope&) = delete;
    ~LiteralScope() { t_literal_request = nullptr; }
};

// The auto threshold: samples (width x rows x samples per pixel) of ONE render call from which a scene is compiled without being asked.
// Measured: the compilation takes 0.85 s of host time and the compiled kernel saves 6.6 ps per sample on Cornell (6.2 % of the
// kernel's time), so it has paid for itself after 1.3e11 samples - about 13 s of rendering, whatever the size of the calls; no single call
// amortises it.  The threshold therefore only tells a render loop from a test frame: a call of 2^26 samples (512 x 512 at 256 spp, 7 ms of
// kernel) is what a progressive or production render issues over and over - the bench's 1.07e9 per call is sixteen times that - while the
// parity and fuzz suites' frames end at 2048 x 2048 x 8 = 2^25 and never compile.
constexpr uint64_t kLiteralAutoSamples = 1ull << 26;

}  // namespace trt
