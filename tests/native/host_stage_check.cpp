// host_stage_check.cpp — drives tiny-raytracer_amd/csrc/host_stage.h (the staging helper of the host-buffer forms of the C ABI and their
// exception guard) on the simulated HIP runtime (tests/native/hipstub) under ASan+UBSan: the layout, a form that succeeds, every HIP call
// of the helper failing once at every position, and the guard.  The "kernel" is a task on the default stream.  Then the scaffold that
// the sample queries' two forms share (sample_query_on_host, sample_query_on_device) with a fake launcher on a real scene handle.
// TEST INFRASTRUCTURE: built and run by tests/test_host_sanitizers.py; prints "ok ..." lines and returns 0, or says what failed.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <atomic>
#include <new>
#include <vector>

#include "../../include/tinyrt.h"
#include "../../tiny-raytracer_amd/csrc/host_stage.h"

static int g_failures = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if (!(cond)) { printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); g_failures++; } \
    } while (0)

using trt::HostStage;

static size_t a16(size_t b) { return (b + 15u) / 16u * 16u; }

// ---- layout ----
static void layout() {
    {
        HostStage st("layout");
        const size_t r1 = st.reserve(1), r17 = st.reserve(17), none = st.reserve(1000, false), r0 = st.reserve(0), r16 = st.reserve(16);
        CHECK(r1 == 0 && r17 == 16 && r0 == 48 && r16 == 48 && st.total() == 64, "offsets %zu %zu %zu %zu total %zu", r1, r17, r0, r16, st.total());
        CHECK(none == HostStage::kNone && st.ptr<char>(none) == nullptr, "an unwanted region has a place");
    }
    // trt_radiance: rays | sums | second moments, if wanted | counters
    for (int m2 = 0; m2 < 2; m2++) {
        const size_t n = 1, rays_b = n * 24u, sums = n * 12u;
        HostStage st("layout");
        st.reserve(rays_b);
        const size_t r_rad = st.reserve(sums), r_m2 = st.reserve(sums, m2 != 0), r_ctr = st.reserve_counters();
        const size_t off_rad = a16(rays_b), off_m2 = off_rad + a16(sums), off_ctr = off_m2 + (m2 ? a16(sums) : 0u), total = off_ctr + trt::CTR_COUNT * 8u;
        CHECK(r_rad == off_rad && (m2 ? r_m2 == off_m2 : r_m2 == HostStage::kNone) && r_ctr == off_ctr && st.total() == total,
              "radiance layout, moment2 %d: total %zu, formula %zu", m2, st.total(), total);
    }
    // trt_select_pixels: sums | second moments | candidates, if given | selection | one word per tile of 256, whole 16s | count (16 bytes)
    const size_t ns[2] = {1, 257};
    for (size_t n : ns)
        for (int cand = 0; cand < 2; cand++) {
            const size_t npixels = n + 2, frame = npixels * 12u, list = n * 4u, scratch = a16((n + 255u) / 256u * 4u);
            HostStage st("layout");
            st.reserve(frame);
            st.reserve(frame);
            st.reserve(list, cand != 0);
            const size_t r_sel = st.reserve(list), r_scratch = st.reserve(scratch), r_count = st.reserve(16u);
            const size_t off_sel = 2u * a16(frame) + (cand ? a16(list) : 0u), off_scratch = off_sel + a16(list), off_count = off_scratch + scratch;
            CHECK(r_sel == off_sel && r_scratch == off_scratch && r_count == off_count && st.total() == off_count + 16u,
                  "selection layout, n %zu candidates %d: total %zu, formula %zu", n, cand, st.total(), off_count + 16u);
        }
    printf("ok layout\n");
}

// ---- a host form on the helper: two inputs go up, a flag word is zeroed, the task writes two outputs, both come down ----
constexpr size_t kN = 17;                       // bytes per buffer: no multiple of 16
constexpr uint8_t kSentinel = 0xEE;
enum Throw { NO_THROW, THROW_BAD_ALLOC };
static std::atomic<int> g_ran{0};

struct Step { const char* api; const char* what; };
// the calls of form() in order; "launch" is the step that takes the launcher's error
static std::vector<Step> steps(bool timed) {
    std::vector<Step> s = {{"hipMalloc", "check buffers: "}, {"hipMemcpy", "copy of input a"}, {"hipMemcpy", "copy of input b"}, {"hipMemset", "zero of the flag"}};
    if (timed) {
        s.push_back({"hipMemset", "hipMemset of the counters"});
        s.push_back({"hipEventCreate", "hipEventCreate"});
        s.push_back({"hipEventCreate", "hipEventCreate"});
        s.push_back({"hipEventRecord", "hipEventRecord"});
    }
    s.push_back({"launch", "check launch"});
    if (timed) s.push_back({"hipEventRecord", "hipEventRecord"});
    s.push_back({"hipMemcpy", "copy of output x"});
    s.push_back({"hipMemcpy", "copy of output y"});
    if (timed) {
        s.push_back({"hipMemcpy", "hipMemcpy of the counters"});
        s.push_back({"hipEventSynchronize", "hipEventElapsedTime"});
        s.push_back({"hipEventElapsedTime", "hipEventElapsedTime"});
    }
    return s;
}

static hipError_t launch(hipError_t refuse, const uint8_t* a, const uint8_t* b, const uint32_t* flag, uint8_t* x, uint8_t* y, unsigned long long* ctr) {
    if (refuse != hipSuccess) return refuse;
    hipstub_enqueue(nullptr, [=] {
        g_ran++;
        for (size_t i = 0; i < kN; i++) { x[i] = (uint8_t)(a[i] ^ b[i] ^ (uint8_t)*flag); y[i] = (uint8_t)(a[i] + 1u); }
        if (ctr) for (int c = 0; c < trt::CTR_COUNT; c++) ctr[c] += 100ull + (unsigned)c;
    });
    return hipSuccess;
}

// y's region is written by the task and never copied up: `y_up` stands for the running sums of a pass that starts them (a null pointer)
static int form(bool timed, const uint8_t* a, const uint8_t* b, const uint8_t* y_up, uint8_t* x, uint8_t* y, trt_stats* stats, hipError_t refuse, Throw thr) {
    return trt::host_form([&]() -> int {
        HostStage st("check buffers");
        const size_t r_a = st.reserve(kN), r_b = st.reserve(kN), r_none = st.reserve(kN, false), r_flag = st.reserve(4), r_x = st.reserve(kN), r_y = st.reserve(kN);
        if (timed) st.reserve_counters();
        st.alloc();
        st.up(r_a, a, kN, "copy of input a");
        st.up(r_b, b, kN, "copy of input b");
        if (y_up) st.up(r_y, y_up, kN, "copy of the running y");
        st.zero(r_flag, 4, "zero of the flag");
        if (timed) { st.zero_counters(); st.time_begin(); }
        if (thr == THROW_BAD_ALLOC) throw std::bad_alloc();
        if (st.ok())
            st.run(launch(refuse, st.ptr<uint8_t>(r_a), st.ptr<uint8_t>(r_b), st.ptr<uint32_t>(r_flag), st.ptr<uint8_t>(r_x), st.ptr<uint8_t>(r_y),
                          timed ? st.counters() : nullptr), "check launch");
        st.down(x, r_x, kN, "copy of output x");
        st.down(y, r_y, kN, "copy of output y");
        if (timed) st.read_stats(stats);
        (void)r_none;
        return st.finish();
    });
}

struct Buffers {
    uint8_t a[kN], b[kN], x[kN], y[kN];
    trt_stats stats;
    Buffers() {
        for (size_t i = 0; i < kN; i++) { a[i] = (uint8_t)(3u * i + 1u); b[i] = (uint8_t)(200u - 7u * i); }
        memset(x, kSentinel, kN);
        memset(y, kSentinel, kN);
        memset(&stats, kSentinel, sizeof(stats));
    }
    bool x_right() const { for (size_t i = 0; i < kN; i++) if (x[i] != (uint8_t)(a[i] ^ b[i])) return false; return true; }
    bool y_right() const { for (size_t i = 0; i < kN; i++) if (y[i] != (uint8_t)(a[i] + 1u)) return false; return true; }
    static bool untouched(const void* p, size_t n) { for (size_t i = 0; i < n; i++) if (static_cast<const uint8_t*>(p)[i] != kSentinel) return false; return true; }
    bool stats_right() const {
        trt_stats want{};
        want.samples = 100u + trt::CTR_SAMPLES;
        want.rays = 100u + trt::CTR_RAYS;
        want.kernel_ms = stats.kernel_ms;
        return stats.kernel_ms >= 0.0 && memcmp(&want, &stats, sizeof(stats)) == 0;           // samples, rays, kernel_ms and nothing else
    }
};

static void success() {
    const long allocs = hipstub_live_allocations(), events = hipstub_live_events();
    for (int timed = 0; timed < 2; timed++) {
        Buffers io;
        g_ran = 0;
        const int rc = form(timed != 0, io.a, io.b, nullptr, io.x, io.y, &io.stats, hipSuccess, NO_THROW);
        CHECK(rc == TRT_OK && g_ran == 1, "timed %d: rc %d %s, task ran %d times", timed, rc, trt_last_error(), g_ran.load());
        CHECK(io.x_right() && io.y_right(), "timed %d: the outputs differ from the task's", timed);
        if (timed) CHECK(io.stats_right(), "stats: samples %llu rays %llu kernel_ms %f", (unsigned long long)io.stats.samples, (unsigned long long)io.stats.rays, io.stats.kernel_ms);
        else CHECK(Buffers::untouched(&io.stats, sizeof(io.stats)), "the untimed form wrote stats");
    }
    {
        Buffers io;                                                 // stats == nullptr: nothing is written through it (ASan would see a null write)
        const int rc = form(true, io.a, io.b, nullptr, io.x, io.y, nullptr, hipSuccess, NO_THROW);
        CHECK(rc == TRT_OK && io.x_right() && io.y_right(), "timed, no stats: rc %d %s", rc, trt_last_error());
    }
    CHECK(hipstub_live_allocations() == allocs && hipstub_live_events() == events, "leak: %ld allocations, %ld events", hipstub_live_allocations() - allocs,
          hipstub_live_events() - events);
    printf("ok success\n");
}

// every HIP call of the helper failing once, at every position
static void failure_injection() {
    const long allocs = hipstub_live_allocations(), events = hipstub_live_events();
    const char* apis[] = {"hipMalloc", "hipMemcpy", "hipMemset", "hipEventCreate", "hipEventRecord", "hipEventSynchronize", "hipEventElapsedTime", "launch"};
    for (int timed = 0; timed < 2; timed++) {
        const std::vector<Step> seq = steps(timed != 0);
        size_t launch_at = 0, x_at = 0, y_at = 0;
        for (size_t k = 0; k < seq.size(); k++) {
            if (!strcmp(seq[k].api, "launch")) launch_at = k;
            if (!strcmp(seq[k].what, "copy of output x")) x_at = k;
            if (!strcmp(seq[k].what, "copy of output y")) y_at = k;
        }
        for (const char* api : apis) {
            long calls = 0, surfaced = 0;
            for (const Step& s : seq) calls += !strcmp(s.api, api);
            for (long at = 0; at <= calls; at++) {
                // the step this injection hits: the at-th of this API; none one past the last
                size_t hit = seq.size();
                long seen = 0;
                for (size_t k = 0; k < seq.size() && hit == seq.size(); k++)
                    if (!strcmp(seq[k].api, api) && seen++ == at) hit = k;
                const bool is_launch = !strcmp(api, "launch");
                Buffers io;
                g_ran = 0;
                if (!is_launch) hipstub_fail_after(api, at);
                const int rc = form(timed != 0, io.a, io.b, nullptr, io.x, io.y, &io.stats, is_launch && at == 0 ? hipErrorInvalidConfiguration : hipSuccess, NO_THROW);
                if (!is_launch) hipstub_fail_after(api, -1);
                if (hit == seq.size()) {
                    CHECK(rc == TRT_OK && io.x_right() && io.y_right() && g_ran == 1, "timed %d %s@%ld (past the last call): rc %d %s", timed, api, at, rc, trt_last_error());
                } else {
                    surfaced += rc != TRT_OK;
                    CHECK(rc == (hit == 0 ? TRT_ERR_OOM : TRT_ERR_HIP), "timed %d %s@%ld: rc %d", timed, api, at, rc);
                    CHECK(!strncmp(trt_last_error(), seq[hit].what, strlen(seq[hit].what)), "timed %d %s@%ld: message '%s', step '%s'", timed, api, at, trt_last_error(), seq[hit].what);
                    CHECK(g_ran == (hit > launch_at ? 1 : 0), "timed %d %s@%ld: the task ran %d times", timed, api, at, g_ran.load());
                    CHECK(hit > x_at ? io.x_right() : Buffers::untouched(io.x, kN), "timed %d %s@%ld: output x", timed, api, at);
                    CHECK(hit > y_at ? io.y_right() : Buffers::untouched(io.y, kN), "timed %d %s@%ld: output y", timed, api, at);
                    CHECK(Buffers::untouched(&io.stats, sizeof(io.stats)), "timed %d %s@%ld: a failed call wrote stats", timed, api, at);
                }
                CHECK(hipstub_live_allocations() == allocs && hipstub_live_events() == events, "timed %d %s@%ld: %ld allocations, %ld events left", timed, api, at,
                      hipstub_live_allocations() - allocs, hipstub_live_events() - events);
                CHECK(hipstub_errors() == 0, "timed %d %s@%ld: %ld protocol violations", timed, api, at, hipstub_errors());
                Buffers again;
                const int rc2 = form(timed != 0, again.a, again.b, nullptr, again.x, again.y, &again.stats, hipSuccess, NO_THROW);
                CHECK(rc2 == TRT_OK && again.x_right() && again.y_right() && (!timed || again.stats_right()), "timed %d %s@%ld: the form after the failure: rc %d %s", timed, api,
                      at, rc2, trt_last_error());
            }
            CHECK(surfaced == calls, "timed %d %s: %ld of %ld injected failures surfaced", timed, api, surfaced, calls);
            if (timed) CHECK(calls > 0, "the timed form never calls %s", api);
        }
    }
    printf("ok failure injection\n");
}

static void guard() {
    const long allocs = hipstub_live_allocations(), events = hipstub_live_events();
    for (int timed = 0; timed < 2; timed++) {
        Buffers io;
        g_ran = 0;
        const int rc = form(timed != 0, io.a, io.b, nullptr, io.x, io.y, &io.stats, hipSuccess, THROW_BAD_ALLOC);       // thrown with the allocation and the events alive
        CHECK(rc == TRT_ERR_OOM && !strcmp(trt_last_error(), "out of memory") && g_ran == 0, "timed %d: rc %d '%s'", timed, rc, trt_last_error());
        CHECK(hipstub_live_allocations() == allocs && hipstub_live_events() == events, "timed %d: %ld allocations, %ld events left behind the exception", timed,
              hipstub_live_allocations() - allocs, hipstub_live_events() - events);
    }
    CHECK(trt::host_form([] { return 42; }) == 42, "a status did not pass through the guard");
    CHECK(trt::host_form([]() -> int { return TRT_ERR_INVALID_ARG; }) == TRT_ERR_INVALID_ARG, "a status did not pass through the guard");
    CHECK(hipstub_errors() == 0, "%ld protocol violations", hipstub_errors());
    printf("ok guard\n");
}

// ---- the sample queries' scaffold: what goes up, what comes down, what a failure says and leaves ----
constexpr uint32_t kItems = 5;                  // items of 24 bytes: 120, a multiple of 8 and not of 16
constexpr float kScribble = -777.0f;
struct SampleIo {
    float items[kItems * 6], table[20], sums[kItems * 3], sums2[kItems];
    trt_stats stats;
    SampleIo() {
        for (uint32_t i = 0; i < kItems * 6; i++) items[i] = 0.5f * (float)i;
        for (uint32_t i = 0; i < 20; i++) table[i] = 100.0f + (float)i;
        for (uint32_t i = 0; i < kItems * 3; i++) sums[i] = 1000.0f + (float)i;
        for (uint32_t i = 0; i < kItems; i++) sums2[i] = 2000.0f + (float)i;
        memset(&stats, kSentinel, sizeof(stats));
    }
    // what the fake kernel leaves: (the sums as they went up | 0) + the item's first word (+ the table's first word); sums2 + 1
    float want_sum(uint32_t i, bool accumulate, bool with_table) const { return (accumulate ? 1000.0f + (float)i : 0.0f) + items[6 * (i / 3)] + (with_table ? table[0] : 0.0f); }
    float want_sum2(uint32_t i, bool accumulate) const { return (accumulate ? 2000.0f + (float)i : 0.0f) + 1.0f; }
};
struct SampleSeen { int calls = 0; bool table = false, sums2 = false, counters = false; };

// One call of the host form as a unit makes it.  The fake launcher behaves as the units' launchers do: with nothing to trace it launches
// nothing under accumulate - here it writes kScribble over the device sums instead, so that a download would show.
static int sample_form(trt_scene* s, uint32_t n, SampleIo& io, bool with_table, bool with_sums2, bool accumulate, bool nothing, hipError_t refuse, SampleSeen& seen,
                       trt_stats* stats) {
    return trt::host_form([&]() -> int {
        const trt::SampleHost h{io.items, (size_t)n * 24u, "copy of the items", with_table ? io.table : nullptr, sizeof(io.table), "copy of the table",
                                io.sums, (size_t)n * 12u, with_sums2 ? io.sums2 : nullptr, (size_t)n * 4u, "copy of the second sums"};
        return trt::sample_query_on_host(s, n, h, accumulate, nothing, "fake buffers", "fake launch", stats, [&](const trt::QueryScene& qs, const trt::SampleDev& d) {
            seen.calls++;
            seen.table = d.table != nullptr; seen.sums2 = d.sums2 != nullptr; seen.counters = d.counters != nullptr;
            if (refuse != hipSuccess) return refuse;
            CHECK(qs.scene.blob != nullptr, "the launcher got no scene");
            const trt::SampleDev dev = d;
            hipstub_enqueue(nullptr, [=] {
                g_ran++;
                for (uint32_t i = 0; i < 3u * n; i++) {
                    if (nothing) { dev.sums[i] = kScribble; continue; }
                    dev.sums[i] = (accumulate ? dev.sums[i] : 0.0f) + dev.items[6 * (i / 3)] + (dev.table ? dev.table[0] : 0.0f);
                }
                for (uint32_t i = 0; dev.sums2 && i < n; i++) dev.sums2[i] = nothing ? kScribble : (accumulate ? dev.sums2[i] : 0.0f) + 1.0f;
                if (!nothing) for (int c = 0; c < trt::CTR_COUNT; c++) dev.counters[c] += 100ull + (unsigned)c;
            });
            return hipSuccess;
        });
    });
}

static trt_scene* sample_scene() {
    trt_world* w = nullptr;
    trt_world_create(&w);
    trt_material m{TRT_LAMBERTIAN, {0.5f, 0.5f, 0.5f}, 0.0f};
    trt_world_add_material(w, "m", &m);
    for (int i = 0; i < 5; i++) trt_world_add_sphere(w, trt_vec3{(float)i, 0.0f, -3.0f}, 0.4f, 0);
    trt_scene* s = nullptr;
    if (trt_scene_create(w, &s) != TRT_OK) { printf("scene: %s\n", trt_last_error()); exit(2); }
    trt_world_destroy(w);
    return s;
}

static void sample_scaffold() {
    trt_scene* s = sample_scene();
    {
        SampleIo io;                                                // the first call uploads the scene: its allocations stay with the handle
        SampleSeen seen;
        const int rc = sample_form(s, kItems, io, false, false, false, false, hipSuccess, seen, &io.stats);
        CHECK(rc == TRT_OK, "first call: rc %d %s", rc, trt_last_error());
    }
    const long allocs = hipstub_live_allocations(), events = hipstub_live_events();
    const SampleIo fresh;
    // the second output and the table, wanted or not; a call that starts the sums and one that continues them
    for (int with_table = 0; with_table < 2; with_table++)
        for (int with_sums2 = 0; with_sums2 < 2; with_sums2++)
            for (int accumulate = 0; accumulate < 2; accumulate++) {
                SampleIo io;
                SampleSeen seen;
                g_ran = 0;
                const int rc = sample_form(s, kItems, io, with_table != 0, with_sums2 != 0, accumulate != 0, false, hipSuccess, seen, &io.stats);
                CHECK(rc == TRT_OK && g_ran == 1 && seen.calls == 1, "table %d sums2 %d accumulate %d: rc %d %s, ran %d", with_table, with_sums2, accumulate, rc, trt_last_error(), g_ran.load());
                CHECK(seen.table == (with_table != 0) && seen.sums2 == (with_sums2 != 0) && seen.counters, "table %d sums2 %d: the launcher saw table %d sums2 %d counters %d",
                      with_table, with_sums2, seen.table, seen.sums2, seen.counters);
                bool right = true;
                for (uint32_t i = 0; i < kItems * 3; i++) right = right && io.sums[i] == fresh.want_sum(i, accumulate != 0, with_table != 0);
                for (uint32_t i = 0; i < kItems; i++) right = right && io.sums2[i] == (with_sums2 ? fresh.want_sum2(i, accumulate != 0) : fresh.sums2[i]);
                CHECK(right, "table %d sums2 %d accumulate %d: the sums differ from the task's", with_table, with_sums2, accumulate);
                CHECK(io.stats.samples == 100u + trt::CTR_SAMPLES && io.stats.rays == 100u + trt::CTR_RAYS && io.stats.kernel_ms >= 0.0, "stats: samples %llu rays %llu",
                      (unsigned long long)io.stats.samples, (unsigned long long)io.stats.rays);
                CHECK(hipstub_live_allocations() == allocs && hipstub_live_events() == events, "leak: %ld allocations, %ld events", hipstub_live_allocations() - allocs,
                      hipstub_live_events() - events);
            }
    // the copies of a call, in order: the k-th hipMemcpy failing names the k-th of them, one past the last fails nothing
    for (int cfg = 0; cfg < 16; cfg++) {
        const bool with_table = cfg & 1, with_sums2 = cfg & 2, accumulate = cfg & 4, nothing = cfg & 8;
        std::vector<const char*> want = {"copy of the items"};
        if (with_table) want.push_back("copy of the table");
        if (accumulate) want.push_back("hipMemcpy of the sums");
        if (accumulate && with_sums2) want.push_back("copy of the second sums");
        if (!(accumulate && nothing)) want.push_back("hipMemcpy of the results");
        if (!(accumulate && nothing) && with_sums2) want.push_back("hipMemcpy of the results");
        want.push_back("hipMemcpy of the counters");
        for (size_t k = 0; k <= want.size(); k++) {
            SampleIo io;
            SampleSeen seen;
            hipstub_fail_after("hipMemcpy", (long)k);
            const int rc = sample_form(s, kItems, io, with_table, with_sums2, accumulate, nothing, hipSuccess, seen, &io.stats);
            hipstub_fail_after("hipMemcpy", -1);
            if (k == want.size()) CHECK(rc == TRT_OK, "copies of configuration %d: more than %zu", cfg, want.size());
            else CHECK(rc == TRT_ERR_HIP && !strncmp(trt_last_error(), want[k], strlen(want[k])), "configuration %d, copy %zu: rc %d '%s', expected '%s'", cfg, k, rc, trt_last_error(), want[k]);
            CHECK(hipstub_live_allocations() == allocs && hipstub_live_events() == events, "configuration %d, copy %zu: leak", cfg, k);
        }
    }
    printf("ok sample scaffold: outputs and copies\n");
    // accumulate with nothing to trace: both sums go up, nothing comes down, the host buffers keep their bytes (the device copies were scribbled over)
    for (int nothing_accumulates = 0; nothing_accumulates < 2; nothing_accumulates++) {
        SampleIo io;
        SampleSeen seen;
        const int rc = sample_form(s, kItems, io, true, true, nothing_accumulates != 0, true, hipSuccess, seen, &io.stats);
        CHECK(rc == TRT_OK && seen.calls == 1, "nothing, accumulate %d: rc %d %s", nothing_accumulates, rc, trt_last_error());
        if (nothing_accumulates) {
            CHECK(!memcmp(io.sums, fresh.sums, sizeof(io.sums)) && !memcmp(io.sums2, fresh.sums2, sizeof(io.sums2)), "accumulate with nothing: the host sums were written");
        } else {
            CHECK(io.sums[0] == kScribble && io.sums2[kItems - 1] == kScribble, "nothing without accumulate: what the launcher wrote did not arrive");
        }
        CHECK(io.stats.samples == 0u && io.stats.rays == 0u, "nothing: stats %llu %llu", (unsigned long long)io.stats.samples, (unsigned long long)io.stats.rays);
        CHECK(hipstub_live_allocations() == allocs && hipstub_live_events() == events, "nothing: leak");
    }
    printf("ok sample scaffold: nothing to trace\n");
    {
        SampleIo io;                                                // a failing launch: its label, no download, no stats, the allocation freed
        SampleSeen seen;
        g_ran = 0;
        const int rc = sample_form(s, kItems, io, true, true, true, false, hipErrorInvalidConfiguration, seen, &io.stats);
        CHECK(rc == TRT_ERR_HIP && !strncmp(trt_last_error(), "fake launch", 11) && seen.calls == 1 && g_ran == 0, "failing launch: rc %d '%s'", rc, trt_last_error());
        CHECK(!memcmp(io.sums, fresh.sums, sizeof(io.sums)) && !memcmp(io.sums2, fresh.sums2, sizeof(io.sums2)) && Buffers::untouched(&io.stats, sizeof(io.stats)),
              "failing launch: the outputs or the stats were written");
        CHECK(hipstub_live_allocations() == allocs && hipstub_live_events() == events, "failing launch: %ld allocations, %ld events left", hipstub_live_allocations() - allocs,
              hipstub_live_events() - events);
    }
    {
        SampleIo io;                                                // a failing allocation: TRT_ERR_OOM under the buffers' label, no launch
        SampleSeen seen;
        hipstub_fail_after("hipMalloc", 0);
        const int rc = sample_form(s, kItems, io, true, true, false, false, hipSuccess, seen, &io.stats);
        hipstub_fail_after("hipMalloc", -1);
        CHECK(rc == TRT_ERR_OOM && !strncmp(trt_last_error(), "fake buffers: ", 14) && seen.calls == 0, "failing allocation: rc %d '%s', %d launches", rc, trt_last_error(), seen.calls);
        CHECK(!memcmp(io.sums, fresh.sums, sizeof(io.sums)) && Buffers::untouched(&io.stats, sizeof(io.stats)), "failing allocation: the outputs or the stats were written");
        CHECK(hipstub_live_allocations() == allocs && hipstub_live_events() == events, "failing allocation: leak");
    }
    {
        SampleIo io;                                                // n == 0: no device work at all, stats zeroed
        SampleSeen seen;
        const long mallocs = hipstub_malloc_calls();
        const int rc = sample_form(s, 0, io, true, true, true, false, hipSuccess, seen, &io.stats);
        CHECK(rc == TRT_OK && seen.calls == 0 && hipstub_malloc_calls() == mallocs && io.stats.samples == 0u && io.stats.kernel_ms == 0.0, "n == 0: rc %d, %d launches", rc, seen.calls);
        CHECK(sample_form(s, 0, io, true, true, true, false, hipSuccess, seen, nullptr) == TRT_OK, "n == 0 without stats");
    }
    // the device form: n == 0 launches nothing; a launch's error comes back under its label
    int launches = 0;
    CHECK(trt::sample_query_on_device(s, 0, "fake launch", [&](const trt::QueryScene&) { launches++; return hipSuccess; }) == TRT_OK && launches == 0, "device form, n == 0");
    CHECK(trt::sample_query_on_device(s, 3, "fake launch", [&](const trt::QueryScene& qs) { launches += qs.scene.blob != nullptr; return hipSuccess; }) == TRT_OK && launches == 1,
          "device form: %s", trt_last_error());
    CHECK(trt::sample_query_on_device(s, 3, "fake launch", [&](const trt::QueryScene&) { return hipErrorInvalidConfiguration; }) == TRT_ERR_HIP &&
              !strncmp(trt_last_error(), "fake launch", 11), "device form, failing launch: '%s'", trt_last_error());
    CHECK(hipstub_errors() == 0, "%ld protocol violations", hipstub_errors());
    trt_scene_destroy(s);
    printf("ok sample scaffold: failures and the device form\n");
}

int main() {
    layout();
    success();
    failure_injection();
    guard();
    sample_scaffold();
    if (g_failures) { printf("%d check(s) failed\n", g_failures); return 1; }
    printf("ok all\n");
    return 0;
}
