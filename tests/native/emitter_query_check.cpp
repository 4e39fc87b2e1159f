// emitter_query_check.cpp — drives tiny-raytracer_amd/csrc/emitter_query.h (the host side the eight direct / nee queries share) on the
// simulated HIP runtime (tests/native/hipstub): the step runner - the listed order, the stop at the first failure, what only a host form
// with n > 0 runs, what sets pick / total_power - and the two forms with a fake launcher on a real scene handle: what the launcher is
// handed, where the pick table is staged, n == 0.  The two steps the header only declares (emitter_entries_check, nee_mis_table_check:
// their definitions need the device compiler) are this file's own: they note that they ran and fail on demand.  The pick table's steps
// are emitter_pick.h's real ones.
// TEST INFRASTRUCTURE: built and run by tests/test_emitter_query_native.py; prints "ok ..." lines and returns 0, or says what failed.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/tinyrt.h"
#include "../../tiny-raytracer_amd/csrc/emitter_query.h"

static int g_failures = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if (!(cond)) { printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); g_failures++; } \
    } while (0)

// ---- the two declared steps: which ran, in which order; a table whose first record has kind 7 / geometry 7 breaks the step's rule ----
static std::string g_ran;
namespace trt {
int emitter_entries_check(const trt_emitter* emitters, uint32_t n_emitters) {
    g_ran += 'E';
    return n_emitters > 0u && emitters[0].kind == 7u ? query_fail(TRT_ERR_INVALID_ARG, "fake: emitter entries") : TRT_OK;
}
inline int nee_mis_table_check(const trt_scene* s, const trt_emitter* emitters, uint32_t n_emitters) {
    g_ran += 'R';
    return !s || (n_emitters > 0u && emitters[0].geometry == 7u) ? query_fail(TRT_ERR_INVALID_ARG, "fake: table rule") : TRT_OK;
}
}  // namespace trt

using namespace trt;

constexpr EmitterStep kPlain[] = {STEP_EMITTER_ENTRIES};
constexpr EmitterStep kMis[] = {STEP_EMITTER_ENTRIES, STEP_TABLE_RULE};
constexpr EmitterStep kPick[] = {STEP_PICK_POINTER, STEP_EMITTER_ENTRIES, STEP_PICK_ENTRIES};
constexpr EmitterStep kRuleFirst[] = {STEP_PICK_POINTER, STEP_EMITTER_ENTRIES, STEP_TABLE_RULE, STEP_PICK_ENTRIES, STEP_PICK_POWER};
constexpr EmitterStep kRecordsFirst[] = {STEP_PICK_POINTER, STEP_EMITTER_ENTRIES, STEP_PICK_ENTRIES, STEP_TABLE_RULE, STEP_PICK_POWER};

constexpr uint32_t kE = 3;
struct Tables {
    trt_emitter emitters[kE];
    trt_emitter_pick pick[kE];
    float total = 0.0f;
    Tables() {
        memset(emitters, 0, sizeof(emitters));
        for (uint32_t e = 0; e < kE; e++) {
            emitters[e].geometry = 0xFFFFFFFFu;
            emitters[e].color = trt_vec3{1.0f, 1.0f, 1.0f};
            emitters[e].area = 1.0f + (float)e;
        }
        if (pick_build(emitters, kE, nullptr, pick, &total) != TRT_OK) { printf("pick_build: %s\n", trt_last_error()); exit(2); }
    }
    EmitterTables view(bool with_pick = true) const { return EmitterTables{emitters, with_pick ? pick : nullptr, kE, total}; }
};

template <size_t K>
static int run(const EmitterStep (&steps)[K], const trt_scene* s, uint32_t n, const EmitterTables& t, EmitterForm form, EmitterVariant& v) {
    g_ran.clear();
    v = EmitterVariant{};
    return emitter_steps_run(s, n, t, form, steps, v);
}
static bool says(const char* fragment) { return strstr(trt_last_error(), fragment) != nullptr; }

static void step_runner(const trt_scene* s) {
    EmitterVariant v;
    {
        const Tables ok;                                            // a clean call: every step in the listed order, and what the steps set
        CHECK(run(kPlain, s, 1, ok.view(false), FORM_HOST, v) == TRT_OK && g_ran == "E" && !v.pick && v.total_power == 0.0f, "plain: ran '%s'", g_ran.c_str());
        CHECK(run(kMis, s, 1, ok.view(false), FORM_HOST, v) == TRT_OK && g_ran == "ER" && !v.pick, "mis: ran '%s'", g_ran.c_str());
        CHECK(run(kPick, s, 1, ok.view(), FORM_HOST, v) == TRT_OK && g_ran == "E" && v.pick && v.total_power == 0.0f, "pick: ran '%s' pick %d", g_ran.c_str(), v.pick);
        CHECK(run(kRuleFirst, s, 1, ok.view(), FORM_HOST, v) == TRT_OK && g_ran == "ER" && v.pick && v.total_power == ok.total, "mis pick: %s", trt_last_error());
        CHECK(run(kRecordsFirst, s, 1, ok.view(), FORM_HOST, v) == TRT_OK && g_ran == "ER" && v.pick && v.total_power == ok.total, "mis pick: %s", trt_last_error());
        CHECK(!v.mis && v.heuristic == 0u, "the steps touched the weighting");
    }
    {
        Tables bad;                                                 // every step's rule broken at once: the first listed step that fails is reported
        bad.emitters[0].kind = 7u;
        bad.emitters[0].geometry = 7u;
        bad.pick[1].q = 2.0f;
        EmitterTables t = bad.view();
        t.total_power = -1.0f;
        t.pick = nullptr;
        CHECK(run(kRuleFirst, s, 1, t, FORM_HOST, v) == TRT_ERR_INVALID_ARG && says("null argument") && g_ran.empty(), "pointer first: '%s' ran '%s'", trt_last_error(), g_ran.c_str());
        t.pick = bad.pick;
        CHECK(run(kRuleFirst, s, 1, t, FORM_HOST, v) == TRT_ERR_INVALID_ARG && says("fake: emitter entries") && g_ran == "E", "entries: '%s' ran '%s'", trt_last_error(), g_ran.c_str());
        bad.emitters[0].kind = 0u;
        // the two orders that differ: the table rule before the pick records, and behind them
        CHECK(run(kRuleFirst, s, 1, t, FORM_HOST, v) == TRT_ERR_INVALID_ARG && says("fake: table rule") && g_ran == "ER", "rule first: '%s' ran '%s'", trt_last_error(), g_ran.c_str());
        CHECK(run(kRecordsFirst, s, 1, t, FORM_HOST, v) == TRT_ERR_INVALID_ARG && says("pick: q") && g_ran == "E", "records first: '%s' ran '%s'", trt_last_error(), g_ran.c_str());
        const Tables fresh;                                         // the records mended: the rule behind them is reached
        memcpy(bad.pick, fresh.pick, sizeof(bad.pick));
        CHECK(run(kRecordsFirst, s, 1, t, FORM_HOST, v) == TRT_ERR_INVALID_ARG && says("fake: table rule") && g_ran == "ER", "records first, rule: '%s'", trt_last_error());
        bad.emitters[0].geometry = 0xFFFFFFFFu;
        CHECK(run(kRuleFirst, s, 1, t, FORM_HOST, v) == TRT_ERR_INVALID_ARG && says("total_power must") && g_ran == "ER", "total: '%s'", trt_last_error());
        t.total_power = bad.total * 2.0f;
        CHECK(run(kRuleFirst, s, 1, t, FORM_HOST, v) == TRT_ERR_INVALID_ARG && says("power / total_power"), "prob: '%s'", trt_last_error());
        t.total_power = bad.total;
        CHECK(run(kRuleFirst, s, 1, t, FORM_HOST, v) == TRT_OK, "mended: '%s'", trt_last_error());
    }
    {
        Tables bad;                                                 // what reads a table runs in a host form with n > 0 only
        bad.emitters[0].kind = 7u;
        bad.emitters[0].geometry = 7u;
        bad.pick[0].alias = kE;
        EmitterTables t = bad.view();
        t.total_power = -1.0f;
        CHECK(run(kRuleFirst, s, 1, t, FORM_DEVICE, v) == TRT_OK && g_ran.empty() && v.pick && v.total_power == -1.0f, "device form: '%s' ran '%s'", trt_last_error(), g_ran.c_str());
        CHECK(run(kRuleFirst, s, 0, t, FORM_HOST, v) == TRT_OK && g_ran.empty() && v.pick, "n == 0: '%s' ran '%s'", trt_last_error(), g_ran.c_str());
        CHECK(run(kPlain, s, 0, t, FORM_HOST, v) == TRT_OK && g_ran.empty(), "n == 0, plain: ran '%s'", g_ran.c_str());
        CHECK(run(kMis, s, 1, t, FORM_DEVICE, v) == TRT_OK && g_ran.empty() && !v.pick, "device form, mis: ran '%s'", g_ran.c_str());
        t.pick = nullptr;                                           // the pointer is looked at in both forms, where n > 0
        CHECK(run(kPick, s, 1, t, FORM_DEVICE, v) == TRT_ERR_INVALID_ARG && says("null argument"), "device form, no pick table");
        CHECK(run(kPick, s, 0, t, FORM_DEVICE, v) == TRT_OK && run(kPick, s, 0, t, FORM_HOST, v) == TRT_OK, "n == 0 needs no pick table");
    }
    {
        trt_direct_mis_params p{};                                  // the weighted parameters' own check
        EmitterVariant w;
        p.heuristic = 2u;
        p.reserved[0] = 1u;
        CHECK(emitter_mis_check(p, w) == TRT_ERR_INVALID_ARG && says("heuristic must") && !w.mis, "heuristic: '%s'", trt_last_error());
        p.heuristic = TRT_MIS_POWER;
        CHECK(emitter_mis_check(p, w) == TRT_ERR_INVALID_ARG && says("reserved words must be zero") && !w.mis, "reserved: '%s'", trt_last_error());
        p.reserved[0] = 0u;
        CHECK(emitter_mis_check(p, w) == TRT_OK && w.mis && w.heuristic == TRT_MIS_POWER && !w.pick, "a clean struct: '%s'", trt_last_error());
        trt_nee_mis_params q{};
        CHECK(emitter_mis_check(q, w) == TRT_OK && w.heuristic == TRT_MIS_BALANCE, "the other family's struct");
    }
    printf("ok step runner\n");
}

// ---- the two forms: a family's call and launcher, faked ----
struct FakeCall : EmitterVariant {
    struct { uint32_t accumulate = 0u; } ra;
    bool empty = false;
    bool nothing() const { return empty; }
};
struct Seen {
    int calls = 0;
    const float *items = nullptr, *emitters = nullptr, *pick = nullptr;
    float *radiance = nullptr, *moment2 = nullptr;
    unsigned long long* counters = nullptr;
    hipStream_t stream = nullptr;
    bool call_pick = false;
    float call_total = 0.0f;
    size_t bytes = 0;
};
static Seen g_seen;
static size_t g_bytes_before = 0;
constexpr uint32_t kItems = 5;                  // 120 bytes of items: not a multiple of 16
static trt_emitter_pick g_pick_on_device[kE];

static hipError_t fake_launch(const QueryScene& qs, const FakeCall& c, const float* d_items, uint32_t n, const float* d_emitters, const float* d_pick,
                              float* d_radiance, float* d_moment2, unsigned long long* d_counters, hipStream_t stream) {
    CHECK(qs.scene.blob != nullptr && n == kItems, "the launcher got no scene, or %u items", n);
    g_seen = Seen{g_seen.calls + 1, d_items, d_emitters, d_pick, d_radiance, d_moment2, d_counters, stream, c.pick, c.total_power, hipstub_live_bytes() - g_bytes_before};
    hipstub_enqueue(stream, [=] {
        for (uint32_t i = 0; i < 3u * n; i++) d_radiance[i] = d_items[6u * (i / 3u)] + 1.0f;
        if (d_counters) d_counters[CTR_SAMPLES] += n;
        if (d_pick) memcpy(g_pick_on_device, d_pick, sizeof(g_pick_on_device));
    });
    return hipSuccess;
}

static size_t a16(size_t b) { return (b + 15u) / 16u * 16u; }
constexpr EmitterLabels kFake{"fake buffers", "fake launch"};

static trt_scene* a_scene() {
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

static void two_forms(trt_scene* s) {
    const Tables tables;
    trt_ray items[kItems];
    memset(items, 0, sizeof(items));
    for (uint32_t i = 0; i < kItems; i++) items[i].origin.x = 10.0f * (float)i;
    float radiance[kItems * 3], moment2[kItems * 3];
    trt_stats stats;
    {
        FakeCall c;                                                 // the first call uploads the scene: its allocations stay with the handle
        CHECK(emitter_query_on_host(s, c, kPlain, kFake, fake_launch, items, kItems, tables.view(false), radiance, nullptr, &stats) == TRT_OK, "first call: %s", trt_last_error());
    }
    const long allocs = hipstub_live_allocations();
    // the host form: the pick table goes behind the counters, and only where the query has one; the other regions lie where they lay
    const size_t off_table = a16(sizeof(items)), off_sums = off_table + a16(sizeof(tables.emitters)), off_m2 = off_sums + a16(sizeof(radiance)),
                 off_ctr = off_m2 + a16(sizeof(moment2)), off_pick = off_ctr + a16(CTR_COUNT * 8u);
    for (int with_pick = 0; with_pick < 2; with_pick++) {
        FakeCall c;
        g_seen = Seen{};
        g_bytes_before = hipstub_live_bytes();
        memset(g_pick_on_device, 0, sizeof(g_pick_on_device));
        memset(&stats, 0xEE, sizeof(stats));
        g_ran.clear();
        const int rc = with_pick ? emitter_query_on_host(s, c, kRuleFirst, kFake, fake_launch, items, kItems, tables.view(), radiance, moment2, &stats)
                                 : emitter_query_on_host(s, c, kMis, kFake, fake_launch, items, kItems, tables.view(false), radiance, moment2, &stats);
        CHECK(rc == TRT_OK && g_seen.calls == 1 && g_ran == "ER", "host form, pick %d: rc %d '%s' ran '%s'", with_pick, rc, trt_last_error(), g_ran.c_str());
        const char* const base = reinterpret_cast<const char*>(g_seen.items);
        CHECK(reinterpret_cast<const char*>(g_seen.emitters) == base + off_table && reinterpret_cast<const char*>(g_seen.radiance) == base + off_sums &&
                  reinterpret_cast<const char*>(g_seen.moment2) == base + off_m2 && reinterpret_cast<const char*>(g_seen.counters) == base + off_ctr,
              "host form, pick %d: the regions moved", with_pick);
        CHECK(g_seen.stream == nullptr && g_seen.call_pick == (with_pick != 0) && g_seen.call_total == (with_pick ? tables.total : 0.0f), "host form, pick %d: the call", with_pick);
        if (with_pick) {
            CHECK(reinterpret_cast<const char*>(g_seen.pick) == base + off_pick && g_seen.bytes == off_pick + sizeof(tables.pick), "the pick table is not behind the counters: %zu bytes", g_seen.bytes);
            CHECK(!memcmp(g_pick_on_device, tables.pick, sizeof(tables.pick)), "the pick table's bytes did not arrive");
        } else {
            CHECK(g_seen.pick == nullptr && g_seen.bytes == off_ctr + CTR_COUNT * 8u, "no pick table, but %zu bytes", g_seen.bytes);
        }
        CHECK(radiance[0] == 1.0f && radiance[3 * (kItems - 1)] == 10.0f * (float)(kItems - 1) + 1.0f && stats.samples == kItems, "host form, pick %d: the results", with_pick);
        CHECK(hipstub_live_allocations() == allocs, "host form, pick %d: leak", with_pick);
    }
    {
        Tables bad;                                                 // a failing step: no launch, no allocation, the outputs and stats untouched
        bad.emitters[0].geometry = 7u;
        FakeCall c;
        g_seen = Seen{};
        const long mallocs = hipstub_malloc_calls();
        radiance[0] = -5.0f;
        memset(&stats, 0xEE, sizeof(stats));
        const int rc = emitter_query_on_host(s, c, kRuleFirst, kFake, fake_launch, items, kItems, bad.view(), radiance, moment2, &stats);
        CHECK(rc == TRT_ERR_INVALID_ARG && says("fake: table rule") && g_seen.calls == 0 && hipstub_malloc_calls() == mallocs && radiance[0] == -5.0f,
              "failing step: rc %d '%s'", rc, trt_last_error());
        CHECK(reinterpret_cast<const unsigned char*>(&stats)[0] == 0xEE, "failing step: stats were written");
        CHECK(emitter_query_on_device(s, c, kPick, kFake, fake_launch, items, kItems, bad.view(false), radiance, nullptr, nullptr, nullptr) == TRT_ERR_INVALID_ARG &&
                  says("null argument") && g_seen.calls == 0, "device form, failing step: '%s'", trt_last_error());
    }
    {
        Tables bad;                                                 // n == 0: nothing is launched, stats are zeroed, no table is read (in either form)
        bad.emitters[0].kind = 7u;
        FakeCall c;
        g_seen = Seen{};
        const long mallocs = hipstub_malloc_calls();
        memset(&stats, 0xEE, sizeof(stats));
        g_ran.clear();
        EmitterTables t = bad.view();
        t.pick = nullptr;
        CHECK(emitter_query_on_host(s, c, kRuleFirst, kFake, fake_launch, nullptr, 0, t, nullptr, nullptr, &stats) == TRT_OK && g_seen.calls == 0 && g_ran.empty() &&
                  hipstub_malloc_calls() == mallocs && stats.samples == 0u && stats.rays == 0u && stats.kernel_ms == 0.0, "n == 0, host form: '%s'", trt_last_error());
        CHECK(c.pick, "n == 0: the query is still a PICK query");
        CHECK(emitter_query_on_host(s, c, kRuleFirst, kFake, fake_launch, nullptr, 0, t, nullptr, nullptr, nullptr) == TRT_OK, "n == 0 without stats");
        CHECK(emitter_query_on_device(s, c, kRuleFirst, kFake, fake_launch, nullptr, 0, t, nullptr, nullptr, nullptr, nullptr) == TRT_OK && g_seen.calls == 0,
              "n == 0, device form: '%s'", trt_last_error());
    }
    {
        Tables bad;                                                 // the device form: the caller's pointers as they are, on the caller's stream, no table read
        bad.emitters[0].kind = 7u;
        bad.pick[0].alias = kE;
        FakeCall c;
        g_seen = Seen{};
        hipStream_t stream = nullptr;
        CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess, "hipStreamCreateWithFlags");
        unsigned long long counters[CTR_COUNT] = {0};
        EmitterTables t = bad.view();
        t.total_power = 3.5f;
        const long mallocs = hipstub_malloc_calls();
        g_ran.clear();
        const int rc = emitter_query_on_device(s, c, kRecordsFirst, kFake, fake_launch, items, kItems, t, radiance, moment2, reinterpret_cast<uint64_t*>(counters), stream);
        CHECK(hipStreamSynchronize(stream) == hipSuccess, "hipStreamSynchronize");
        CHECK(rc == TRT_OK && g_seen.calls == 1 && g_ran.empty() && hipstub_malloc_calls() == mallocs, "device form: rc %d '%s' ran '%s'", rc, trt_last_error(), g_ran.c_str());
        CHECK(g_seen.items == reinterpret_cast<const float*>(items) && g_seen.emitters == reinterpret_cast<const float*>(bad.emitters) &&
                  g_seen.pick == reinterpret_cast<const float*>(bad.pick) && g_seen.radiance == radiance && g_seen.moment2 == moment2 && g_seen.counters == counters &&
                  g_seen.stream == stream, "device form: the launcher's pointers");
        CHECK(g_seen.call_pick && g_seen.call_total == 3.5f && counters[CTR_SAMPLES] == kItems, "device form: the call");
        g_seen = Seen{};
        CHECK(emitter_query_on_device(s, c, kMis, kFake, fake_launch, items, kItems, bad.view(false), radiance, nullptr, nullptr, stream) == TRT_OK && g_seen.calls == 1 &&
                  g_seen.pick == nullptr && g_seen.moment2 == nullptr && g_seen.counters == nullptr, "device form, no pick table: '%s'", trt_last_error());
        CHECK(hipStreamSynchronize(stream) == hipSuccess && hipStreamDestroy(stream) == hipSuccess, "the stream");
        const auto refuse = [](const QueryScene&, const FakeCall&, const float*, uint32_t, const float*, const float*, float*, float*, unsigned long long*, hipStream_t) {
            return hipErrorInvalidConfiguration;
        };
        CHECK(emitter_query_on_device(s, c, kPlain, kFake, refuse, items, kItems, bad.view(false), radiance, nullptr, nullptr, nullptr) == TRT_ERR_HIP &&
                  !strncmp(trt_last_error(), "fake launch", 11), "device form, failing launch: '%s'", trt_last_error());
        Tables ok;
        CHECK(emitter_query_on_host(s, c, kPlain, kFake, refuse, items, kItems, ok.view(false), radiance, nullptr, nullptr) == TRT_ERR_HIP &&
                  !strncmp(trt_last_error(), "fake launch", 11) && hipstub_live_allocations() == allocs, "host form, failing launch: '%s'", trt_last_error());
        hipstub_fail_after("hipMalloc", 0);
        const int oom = emitter_query_on_host(s, c, kPlain, kFake, fake_launch, items, kItems, ok.view(false), radiance, nullptr, nullptr);
        hipstub_fail_after("hipMalloc", -1);
        CHECK(oom == TRT_ERR_OOM && !strncmp(trt_last_error(), "fake buffers: ", 14), "host form, failing allocation: rc %d '%s'", oom, trt_last_error());
    }
    CHECK(hipstub_errors() == 0, "%ld protocol violations", hipstub_errors());
    printf("ok the two forms\n");
}

int main() {
    trt_scene* s = a_scene();
    step_runner(s);
    two_forms(s);
    trt_scene_destroy(s);
    if (g_failures) { printf("%d check(s) failed\n", g_failures); return 1; }
    printf("ok all\n");
    return 0;
}
