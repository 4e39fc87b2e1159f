// host_stage.h - what the host-buffer forms of the C ABI (trt_intersect, trt_radiance, trt_render_aov, ...) share: host code only, no kernel.
// Such a form stages the caller's buffers through ONE device allocation of its own on the default stream and returns when the answer is
// back.  HostStage is that allocation for the length of one call; host_form is the guard the form runs in.  The sample queries
// (radiance, gather, ambient, probe, passes, direct, nee) stage the same buffers in the same order, so the body of their host form and
// of their device form is here too, with the unit's launcher as a callable: sample_query_on_host, sample_query_on_device.  Needs
// scene_query.h (query_fail, query_fail_hip, the scene on the device) and nothing of the kernel units: tests/native/host_stage_check.cpp
// drives all of it on the simulated runtime.
#pragma once

#include <new>
#include <string>

#include "scene_query.h"

namespace trt {

// Runs the body of a host form: no std::bad_alloc leaves the C ABI (if even the message cannot be set, the old one stays).
template <class Body>
int host_form(Body&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        try { return query_fail(TRT_ERR_OOM, "out of memory"); } catch (...) { return TRT_ERR_OOM; }
    }
}

// Regions at multiples of 16 bytes in one hipMalloc, then the steps of the form in order.  The first step that fails is kept with its
// `what` and every later one does nothing; finish() reports it.  The destructor frees the allocation and the events on every path.
class HostStage {
  public:
    static constexpr size_t kNone = ~(size_t)0;                     // the region of a buffer that is not wanted: ptr() is null
    explicit HostStage(const char* label) : label_(label) {}        // what the allocation is called when it fails
    HostStage(const HostStage&) = delete;
    ~HostStage() { if (ev0_) (void)hipEventDestroy(ev0_); if (ev1_) (void)hipEventDestroy(ev1_); if (base_) (void)hipFree(base_); }
    // before alloc(): the next region (0 bytes are legal); returns its offset
    size_t reserve(size_t bytes, bool wanted = true) {
        const size_t off = q_align16(total_);
        if (wanted) total_ = off + bytes;
        return wanted ? off : kNone;
    }
    size_t total() const { return total_; }
    void alloc() {
        e_ = hipMalloc(reinterpret_cast<void**>(&base_), total_);
        if (e_ != hipSuccess) { (void)hipGetLastError(); base_ = nullptr; oom_ = true; }
    }
    template <class T> T* ptr(size_t region) const { return region == kNone ? nullptr : reinterpret_cast<T*>(base_ + region); }
    // a launcher is only called while ok():  if (st.ok()) st.run(launch_x(...), "x launch");  A copy for a region that is not wanted does nothing.
    bool ok() const { return e_ == hipSuccess; }
    void up(size_t region, const void* host, size_t bytes, const char* what) { if (ok() && region != kNone) note(hipMemcpy(base_ + region, host, bytes, hipMemcpyHostToDevice), what); }
    void zero(size_t region, size_t bytes, const char* what) { if (ok()) note(hipMemset(base_ + region, 0, bytes), what); }
    void run(hipError_t launched, const char* what) {
        if (ok()) note(launched, what);
        if (ok() && ev1_) note(hipEventRecord(ev1_, nullptr), "hipEventRecord");
    }
    void down(void* host, size_t region, size_t bytes, const char* what) { if (ok() && region != kNone) note(hipMemcpy(host, base_ + region, bytes, hipMemcpyDeviceToHost), what); }      // (waits for the kernel: same stream)
    // TRT_OK, TRT_ERR_OOM for the allocation, or the first failed step as query_fail_hip reports it
    int finish() const {
        if (oom_) return query_fail(TRT_ERR_OOM, std::string(label_) + ": " + hipGetErrorString(e_));
        return ok() ? TRT_OK : query_fail_hip(e_, what_);
    }
    // The forms that report trt_stats: CTR_COUNT counters behind the other regions, zeroed before the launch; two events on the default
    // stream, the first recorded by time_begin() and the second by run() behind the launch; read_stats() is the form's last step.
    size_t reserve_counters() { return ctr_ = reserve(sizeof(h_ctr_)); }
    unsigned long long* counters() const { return ptr<unsigned long long>(ctr_); }
    void zero_counters() { zero(ctr_, sizeof(h_ctr_), "hipMemset of the counters"); }
    void time_begin() {
        if (ok()) note(hipEventCreate(&ev0_), "hipEventCreate");
        if (ok()) note(hipEventCreate(&ev1_), "hipEventCreate");
        if (ok()) note(hipEventRecord(ev0_, nullptr), "hipEventRecord");
    }
    void read_stats(trt_stats* stats) {
        float ms = 0.0f;
        down(h_ctr_, ctr_, sizeof(h_ctr_), "hipMemcpy of the counters");
        if (ok()) note(hipEventSynchronize(ev1_), "hipEventElapsedTime");
        if (ok()) note(hipEventElapsedTime(&ms, ev0_, ev1_), "hipEventElapsedTime");
        if (ok() && stats) { *stats = trt_stats{}; stats->samples = h_ctr_[CTR_SAMPLES]; stats->rays = h_ctr_[CTR_RAYS]; stats->kernel_ms = ms; }
    }

  private:
    void note(hipError_t e, const char* what) { if (e != hipSuccess) { e_ = e; what_ = what; } }
    const char *label_, *what_ = "";
    char* base_ = nullptr;
    size_t total_ = 0, ctr_ = kNone;
    hipError_t e_ = hipSuccess;
    bool oom_ = false;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    unsigned long long h_ctr_[CTR_COUNT] = {0};
};

// ---- the sample queries (radiance, gather, ambient, direct, nee, probe, passes): ONE copy of what their two forms do around the launch ----

// The device form after the unit's checks: buffers in HBM, asynchronous on the caller's stream.  launch(qs) is the unit's launcher.
template <class Launch>
int sample_query_on_device(trt_scene* s, uint32_t n, const char* what, Launch&& launch) {
    if (n == 0u) return TRT_OK;
    int rc = query_require_device();
    if (rc != TRT_OK) return rc;
    QueryScene qs;
    rc = query_scene_on_device(s, qs);
    if (rc != TRT_OK) return rc;
    const hipError_t e = launch(qs);
    if (e != hipSuccess) return query_fail_hip(e, what);
    return TRT_OK;
}

// The caller's buffers of a host form, and the device copies its launcher is given.
struct SampleHost {
    const void* items; size_t items_b; const char* items_what;      // the rays or surfels, and what their copy is called
    const void* table; size_t table_b; const char* table_what;      // a second input (the emitter table), or nullptr
    float* sums; size_t sums_b;                                      // the required output
    float* sums2; size_t sums2_b; const char* sums2_what;            // the optional output (nullptr: not wanted), and what its upload is called
    const void* table2 = nullptr; size_t table2_b = 0; const char* table2_what = "";      // a third input (the emitter pick table), or nullptr
};
struct SampleDev {
    const float *items, *table;
    float *sums, *sums2;             // sums2: nullptr where the caller's is
    unsigned long long* counters;
    const float* table2;             // nullptr where the caller's is
};
// The host form after the unit's checks (inside host_form).  Device copies of the inputs and of the sums are the call's own (one
// allocation), one stream-ordered sequence on the default stream, complete when the call returns.  The running sums go up only when
// the call continues them (accumulate), and come down unless it continues them with nothing to trace.  launch(qs, dev) is the unit's
// launcher on the default stream.
template <class Launch>
int sample_query_on_host(trt_scene* s, uint32_t n, const SampleHost& h, bool accumulate, bool nothing, const char* buffers, const char* what,
                         trt_stats* stats, Launch&& launch) {
    if (n == 0u) {
        if (stats) *stats = trt_stats{};
        return TRT_OK;
    }
    int rc = query_require_device();
    if (rc != TRT_OK) return rc;
    QueryScene qs;
    rc = query_scene_on_device(s, qs);
    if (rc != TRT_OK) return rc;
    HostStage st(buffers);
    const size_t r_items = st.reserve(h.items_b), r_table = st.reserve(h.table_b, h.table != nullptr), r_sums = st.reserve(h.sums_b),
                 r_sums2 = st.reserve(h.sums2_b, h.sums2 != nullptr);
    st.reserve_counters();
    const size_t r_table2 = st.reserve(h.table2_b, h.table2 != nullptr);    // behind the counters: the other regions lie where they lay
    st.alloc();
    st.up(r_items, h.items, h.items_b, h.items_what);
    st.up(r_table, h.table, h.table_b, h.table_what);
    st.up(r_table2, h.table2, h.table2_b, h.table2_what);
    st.zero_counters();
    // the running sums a pass continues go up; a pass that starts them reads nothing
    if (accumulate) st.up(r_sums, h.sums, h.sums_b, "hipMemcpy of the sums");
    if (accumulate) st.up(r_sums2, h.sums2, h.sums2_b, h.sums2_what);
    st.time_begin();
    if (st.ok())
        st.run(launch(qs, SampleDev{st.ptr<float>(r_items), st.ptr<float>(r_table), st.ptr<float>(r_sums), st.ptr<float>(r_sums2), st.counters(),
                                st.ptr<float>(r_table2)}), what);
    const bool wrote = !(accumulate && nothing);
    if (wrote) st.down(h.sums, r_sums, h.sums_b, "hipMemcpy of the results");
    if (wrote) st.down(h.sums2, r_sums2, h.sums2_b, "hipMemcpy of the results");
    st.read_stats(stats);
    return st.finish();
}

}  // namespace trt
