// scene_cache.h - what a scene handle keeps on its devices, and the scaffold of the blocking entry points that borrow from it: host code
// only, no kernel.  Included by capi.hip alone.  Needs scene_query.h (query_fail, query_fail_hip) and nothing of the kernel units: the
// host-only build of capi.hip against tests/native/hipstub drives it on the simulated runtime (tests/native/capi_host_check.cpp).
//
// Everything a render needs on a device besides the caller's buffers is cached on the scene handle (SceneCache), per device, and lives until
// trt_scene_destroy / trt_scene_trim: the packed scene and the ray queries' index table (each uploaded on first use), WORKSPACES and RENDER
// CONTEXTS (below).  CtxRun is one blocking entry point's use of a context.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "literal_kernel.h"
#include "scene_query.h"

namespace trt {

// Puts the calling thread's current device back when it goes out of scope.  If the device cannot be read nothing is put back; error() says why.
class DeviceRestore {
  public:
    DeviceRestore() : e_(hipGetDevice(&prev_)) {}
    DeviceRestore(const DeviceRestore&) = delete;
    ~DeviceRestore() { if (e_ == hipSuccess) (void)hipSetDevice(prev_); }
    hipError_t error() const { return e_; }
    int device() const { return prev_; }
  private:
    int prev_ = 0;
    hipError_t e_;
};

// Device scratch of one render (streamed: radiance records of a chunk + batch counter; wavefront: path state).  A render owns its workspace
// from acquire to release; release records an event behind the render's last kernel and a workspace is handed out again only to a stream
// that first waits for that event.  busy: a host thread owns the entry (between acquire and release, or while the pool itself
// regrows / frees it); recorded: `done` has been recorded behind the last kernel that used the buffer.
struct Workspace {
    void* ptr = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    hipStream_t last_stream = nullptr;            // the stream `done` was recorded on (valid while recorded)
    bool recorded = false;
    bool busy = false;
};
// Everything a blocking entry point (trt_render, trt_render_multi*, trt_sample_batch) needs on one device besides its workspace.  One call
// owns a context from acquire to release and has synchronised `stream` before it releases, so an idle context has no work in flight.
struct RenderCtx {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    unsigned long long* d_ctr = nullptr;          // CTR_COUNT counters
    float* d_accum = nullptr;                     // device frame (or band) buffer, grown on demand
    size_t accum_bytes = 0;
    bool busy = false;
};
constexpr size_t kMaxWorkspacesPerDevice = 8;      // beyond that, renders queue behind each other on the device

// The per-device cache of one scene handle.  THE LOCKING RULE: the mutex guards only the bookkeeping.  An entry is marked busy under the lock
// and every HIP call that can block (hipMalloc, hipFree, hipMemcpy, hipEventSynchronize, hipStreamSynchronize) runs with the lock released;
// a busy entry's fields belong to its owner.  Streams are created once and never destroyed while the cache lives, so an event recorded on
// one (a workspace's `done`) never outlives its stream.
class SceneCache {
  public:
    enum Upload { PACKED_SCENE, GEO_INDEX };
    // Must not run while another host thread is inside a call on this cache.  Renders that are still running on a device are waited for
    // (their workspace events) before anything is freed.
    ~SceneCache() {
        DeviceRestore restore;
        for (auto& kv : dev_) {
            if (hipSetDevice(kv.first) != hipSuccess) continue;
            DeviceCache& dc = kv.second;
            for (Workspace* w : dc.ws) {
                if (w->recorded) (void)hipEventSynchronize(w->done);      // a render may still be using it
                if (w->ptr) (void)hipFree(w->ptr);
                if (w->done) (void)hipEventDestroy(w->done);
                delete w;
            }
            for (RenderCtx* c : dc.ctx) context_destroy(c);               // after the workspaces: their events were recorded on these streams
            for (Cached& u : dc.up) if (u.ptr) (void)hipFree(u.ptr);
            dc.literal.release();                                         // the scene's own kernel (literal_kernel.h): no render is in flight any more
        }
    }
    // idle scratch (workspaces + context frames) kept per device: trt_scene_options.scratch_cap_bytes.  Set before the handle is shared.
    void set_cap(size_t bytes) { cap_ = bytes; }
    // `out`: the buffer `which` on the current device, uploaded from `host` on first use (0 bytes, an empty index table: 4 bytes, nothing copied).  One
    // thread uploads (lock released during the copy), the others wait for it.  `label` names the upload when it fails.
    template <class T>
    int on_device(Upload which, const void* host, size_t bytes, const char* label, T*& out) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return query_fail_hip(e, "hipGetDevice");
        std::unique_lock<std::mutex> lock(mu_);
        Cached& u = dev_[dev].up[which];                            // references into an unordered_map stay valid across inserts
        while (u.ptr == nullptr && u.busy) cv_.wait(lock);
        if (u.ptr == nullptr) {
            u.busy = true;
            lock.unlock();
            void* d = nullptr;
            e = hipMalloc(&d, bytes ? bytes : sizeof(uint32_t));
            if (e == hipSuccess && bytes) {
                e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
                if (e != hipSuccess) { (void)hipFree(d); d = nullptr; }
            }
            lock.lock();
            u.busy = false;
            u.ptr = d;
            cv_.notify_all();
            if (e != hipSuccess) return query_fail_hip(e, label);
        }
        out = static_cast<T*>(u.ptr);
        return TRT_OK;
    }
    // A packed scene that is already in HBM on `dev` (the device scene compiler's): the first render there does not upload again.
    void adopt_packed_scene(int dev, void* d_blob) { std::lock_guard<std::mutex> lock(mu_); dev_[dev].up[PACKED_SCENE].ptr = d_blob; }
    // Takes a workspace of at least `need` bytes for a render that will be enqueued on `stream` of device `dev`.
    int workspace_acquire(int dev, size_t need, hipStream_t stream, Workspace** out) {
        std::unique_lock<std::mutex> lock(mu_);
        DeviceCache& dc = dev_[dev];
        bool may_grow = true;
        for (;;) {
            // 1. an idle one whose last render has finished (no dependency at all): the smallest that fits, else one to regrow
            Workspace* pick = nullptr;
            Workspace* regrow = nullptr;
            for (Workspace* w : dc.ws) {
                if (w->busy || !ws_finished(w)) continue;
                if (w->bytes >= need) { if (!pick || w->bytes < pick->bytes) pick = w; }
                else if (!regrow) regrow = w;
            }
            enum { USE, REGROW, CREATE, QUEUE, DRAIN } what = USE;
            // 1b. one whose last render is still in flight ON THIS STREAM: stream order already puts this render behind it - no wait, no second
            //     buffer.  (Back-to-back renders enqueued on one stream - bench.py's steps, a progressive viewer - otherwise grew the pool to its
            //     eight workspaces, 16 GB each at full size, and sent the idle ones through the byte cap: a 13 GB hipMalloc + hipFree per render.)
            //     hipStreamPerThread is one handle for many streams and never matches.
            //     The wait on `done` is still enqueued (SAME_STREAM below): behind its own stream's work it costs nothing, and it keeps the reuse
            //     safe should a caller destroy a stream with work pending and get the same handle back for a new one.
            bool same_stream = false;
            if (!pick && stream != hipStreamPerThread) {
                for (Workspace* w : dc.ws) if (!w->busy && w->recorded && w->last_stream == stream && w->bytes >= need && (!pick || w->bytes < pick->bytes)) pick = w;
                same_stream = pick != nullptr;
            }
            if (same_stream) what = QUEUE;
            if (!pick && regrow) { pick = regrow; what = REGROW; }
            // 2. a new one while the pool may grow
            if (!pick && may_grow && dc.ws.size() < kMaxWorkspacesPerDevice) {
                pick = new (std::nothrow) Workspace();
                if (!pick) return query_fail(TRT_ERR_OOM, "out of memory");
                dc.ws.push_back(pick);
                what = CREATE;
            }
            // 3. an idle one that is still in flight and large enough: this render queues behind it on the device
            if (!pick) {
                for (Workspace* w : dc.ws) if (!w->busy && w->bytes >= need) { pick = w; what = QUEUE; break; }
            }
            if (!pick) {
                // 4. every workspace is owned by another host thread: wait for a release
                bool any_busy = false;
                for (Workspace* w : dc.ws) any_busy = any_busy || w->busy;
                if (any_busy) { cv_.wait(lock); continue; }
                if (dc.ws.empty()) return query_fail(TRT_ERR_OOM, "no device memory for a render workspace");
                // 5. all idle, all in flight, all too small: wait for the first to finish, then regrow it
                pick = dc.ws.front();
                what = DRAIN;
            }
            pick->busy = true;
            lock.unlock();
            // ---- HIP calls, lock released; `pick` is ours ----
            hipError_t e = hipSuccess;
            const char* where = "";
            if (what == CREATE) {
                e = hipEventCreateWithFlags(&pick->done, hipEventDisableTiming); where = "hipEventCreate(workspace)";
                if (e == hipSuccess) { e = hipMalloc(&pick->ptr, need); where = "hipMalloc(workspace)"; if (e == hipSuccess) pick->bytes = need; else pick->ptr = nullptr; }
            } else if (what == DRAIN || what == REGROW) {
                if (what == DRAIN) { e = hipEventSynchronize(pick->done); where = "hipEventSynchronize(workspace)"; }
                if (e == hipSuccess && pick->ptr) { e = hipFree(pick->ptr); where = "hipFree(workspace)"; pick->ptr = nullptr; pick->bytes = 0; }
                if (e == hipSuccess) { e = hipMalloc(&pick->ptr, need); where = "hipMalloc(workspace)"; if (e == hipSuccess) pick->bytes = need; else pick->ptr = nullptr; }
                if (e == hipSuccess) pick->recorded = false;
            } else if (what == QUEUE) {
                e = hipStreamWaitEvent(stream, pick->done, 0); where = "hipStreamWaitEvent(workspace)";
            }
            if (e == hipSuccess) { *out = pick; return TRT_OK; }
            (void)hipGetLastError();
            lock.lock();
            if (what == CREATE) {
                dc.ws.erase(std::find(dc.ws.begin(), dc.ws.end(), pick));
                if (pick->done) (void)hipEventDestroy(pick->done);
                delete pick;
                cv_.notify_all();
                if (e == hipErrorOutOfMemory) {
                    // out of HBM for another copy: queue behind a running render whose buffer is large enough, if there is one; else the caller
                    // may ask for less (TRT_ERR_OOM: enqueue_render halves the samples per launch)
                    bool fits = false;                                 // (a busy entry's fields belong to its owner: it may fit once released)
                    for (Workspace* w : dc.ws) fits = fits || w->busy || w->bytes >= need;
                    if (fits) { may_grow = false; continue; }
                    return query_fail(TRT_ERR_OOM, std::string(where) + ": " + hipGetErrorString(e));
                }
                return query_fail_hip(e, where);
            }
            pick->busy = false;                                       // (a failed regrow leaves an empty, reusable entry)
            cv_.notify_all();
            if (e == hipErrorOutOfMemory) return query_fail(TRT_ERR_OOM, std::string(where) + ": " + hipGetErrorString(e));
            return query_fail_hip(e, where);
        }
    }
    // Gives the workspace back; `stream` has all of the render's launches enqueued.
    int workspace_release(int dev, Workspace* w, hipStream_t stream) {
        hipError_t e = hipEventRecord(w->done, stream);
        bool recorded = e == hipSuccess;
        if (!recorded) {
            // without the event nothing orders the next user behind this render: wait for the render itself
            (void)hipGetLastError();
            (void)hipStreamSynchronize(stream);
            (void)hipGetLastError();
        }
        {
            std::unique_lock<std::mutex> lock(mu_);
            w->recorded = recorded;
            w->last_stream = stream;
            w->busy = false;
            trim_locked(lock, dev_[dev], cap_);
        }
        cv_.notify_all();
        if (e != hipSuccess) return query_fail_hip(e, "hipEventRecord(workspace)");
        return TRT_OK;
    }

    // A render context on device `dev` (the current one) with a device frame of at least `accum_bytes` (0: none needed).
    int context_acquire(int dev, size_t accum_bytes, RenderCtx** out) {
        RenderCtx* c = nullptr;
        bool fresh = false;
        {
            std::lock_guard<std::mutex> lock(mu_);
            DeviceCache& dc = dev_[dev];
            RenderCtx* fits = nullptr;                                 // the smallest idle frame that fits, else the largest idle one (regrown)
            RenderCtx* any = nullptr;
            for (RenderCtx* k : dc.ctx) {
                if (k->busy) continue;
                if (k->accum_bytes >= accum_bytes && (!fits || k->accum_bytes < fits->accum_bytes)) fits = k;
                if (!any || k->accum_bytes > any->accum_bytes) any = k;
            }
            c = fits ? fits : any;
            if (!c) {
                c = new (std::nothrow) RenderCtx();
                if (!c) return query_fail(TRT_ERR_OOM, "out of memory");
                dc.ctx.push_back(c);
                fresh = true;
            }
            c->busy = true;
        }
        hipError_t e = hipSuccess;
        const char* where = "";
        if (fresh) {
            e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking); where = "hipStreamCreate";
            if (e == hipSuccess) { e = hipEventCreate(&c->ev0); where = "hipEventCreate"; }
            if (e == hipSuccess) { e = hipEventCreate(&c->ev1); where = "hipEventCreate"; }
            if (e == hipSuccess) { e = hipMalloc(reinterpret_cast<void**>(&c->d_ctr), CTR_COUNT * sizeof(unsigned long long)); where = "hipMalloc(counters)"; }
        }
        if (e == hipSuccess && c->accum_bytes < accum_bytes) {
            if (c->d_accum) { e = hipFree(c->d_accum); where = "hipFree(frame)"; c->d_accum = nullptr; c->accum_bytes = 0; }
            if (e == hipSuccess) { e = hipMalloc(reinterpret_cast<void**>(&c->d_accum), accum_bytes); where = "hipMalloc(frame)"; if (e == hipSuccess) c->accum_bytes = accum_bytes; else c->d_accum = nullptr; }
        }
        if (e == hipSuccess) { *out = c; return TRT_OK; }
        (void)hipGetLastError();
        const int rc = query_fail_hip(e, where);
        std::lock_guard<std::mutex> lock(mu_);
        if (fresh) {                                                  // half-built: take it out of the pool again (nothing was enqueued on its stream)
            DeviceCache& dc = dev_[dev];
            dc.ctx.erase(std::find(dc.ctx.begin(), dc.ctx.end(), c));
            context_destroy(c);
        } else {
            c->busy = false;
        }
        return rc;
    }
    // The caller has synchronised c->stream (or nothing was enqueued on it).  The context stays in the pool whatever the pool's size:
    // its stream and events live until the cache is destroyed (a workspace's `done` event may have been recorded on that stream and is
    // queried by later acquires, so destroying the stream here - round 3 did, beyond 16 idle contexts - brought back the very pattern
    // DESIGN.md's audit of round 2's abort removed).  What a burst of shards leaves behind is bounded by the byte cap: idle contexts'
    // frames are freed largest first by trim_locked; a context without a frame is a stream, two events and 128 bytes of counters.
    void context_release(int dev, RenderCtx* c) {
        std::unique_lock<std::mutex> lock(mu_);
        c->busy = false;
        trim_locked(lock, dev_[dev], cap_);
    }
    // Frees idle scratch on `dev` (the current device) until at most `cap` bytes of it stay cached.  Safe while renders run: what they own is skipped.
    void trim(int dev, size_t cap) { std::unique_lock<std::mutex> lock(mu_); trim_locked(lock, dev_[dev], cap); }
    // ... all of it, on every device the cache has been used on
    void trim_all() {
        DeviceRestore restore;
        std::vector<int> devices;
        {
            std::lock_guard<std::mutex> lock(mu_);
            for (auto& kv : dev_) devices.push_back(kv.first);
        }
        for (int d : devices) if (hipSetDevice(d) == hipSuccess) trim(d, 0);
    }
    // What enqueue_render's halving loop remembers and asks: the bytes of this cache's idle workspaces on `dev` (a regrow frees them first), and
    // the short grant - != 0: the last streamed render of a full-size launch was granted scratch for this many samples only.
    size_t idle_workspace_bytes(int dev) {
        std::lock_guard<std::mutex> lock(mu_);
        size_t idle = 0;
        for (Workspace* w : dev_[dev].ws) if (!w->busy) idle += w->bytes;
        return idle;
    }
    uint32_t short_samples(int dev) { std::lock_guard<std::mutex> lock(mu_); return dev_[dev].short_samples; }
    void set_short_samples(int dev, uint32_t samples) { std::lock_guard<std::mutex> lock(mu_); dev_[dev].short_samples = samples; }
    // The scene's run-time compiled kernel on `dev` (literal_kernel.h): compiled at most once per scene and device, it has its own lock.
    LiteralKernel* literal_kernel(int dev) { std::lock_guard<std::mutex> lock(mu_); return &dev_[dev].literal; }      // (references into an unordered_map stay valid)
  private:
    struct Cached { void* ptr = nullptr; bool busy = false; };      // ptr: in HBM once uploaded; busy: a thread is uploading it
    struct DeviceCache {
        Cached up[2];                                 // [PACKED_SCENE], [GEO_INDEX]
        std::vector<Workspace*> ws;
        std::vector<RenderCtx*> ctx;
        uint32_t short_samples = 0;
        LiteralKernel literal;
    };
    static bool ws_finished(Workspace* w) {                           // call with the lock held, entry not busy
        if (!w->recorded) return true;
        const bool done = hipEventQuery(w->done) == hipSuccess;
        (void)hipGetLastError();                                      // hipErrorNotReady is not an error
        return done;
    }
    static void context_destroy(RenderCtx* c) {                       // idle context: nothing in flight on its stream
        if (c->d_accum) (void)hipFree(c->d_accum);
        if (c->d_ctr) (void)hipFree(c->d_ctr);
        if (c->ev0) (void)hipEventDestroy(c->ev0);
        if (c->ev1) (void)hipEventDestroy(c->ev1);
        if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
        (void)hipGetLastError();
        delete c;
    }
    // Frees idle scratch on `dc` until at most `cap` bytes of IDLE scratch stay cached (largest first).  Called with the lock held; the
    // hipFree calls run with the lock released (the entries are marked busy meanwhile).
    void trim_locked(std::unique_lock<std::mutex>& lock, DeviceCache& dc, size_t cap) {
        for (;;) {
            size_t total = 0;                                         // idle entries only: a busy entry's fields belong to its owner
            for (Workspace* w : dc.ws) if (!w->busy) total += w->bytes;
            for (RenderCtx* c : dc.ctx) if (!c->busy) total += c->accum_bytes;
            if (total <= cap) return;
            Workspace* bw = nullptr;
            RenderCtx* bc = nullptr;
            for (Workspace* w : dc.ws) if (!w->busy && w->bytes && ws_finished(w) && (!bw || w->bytes > bw->bytes)) bw = w;
            for (RenderCtx* c : dc.ctx) if (!c->busy && c->accum_bytes && (!bc || c->accum_bytes > bc->accum_bytes)) bc = c;
            if (!bw && !bc) return;                                   // everything left is in use
            void* victim;
            if (bw && (!bc || bw->bytes >= bc->accum_bytes)) { bw->busy = true; victim = bw->ptr; bw->ptr = nullptr; bw->bytes = 0; bw->recorded = false; bc = nullptr; }
            else { bc->busy = true; victim = bc->d_accum; bc->d_accum = nullptr; bc->accum_bytes = 0; bw = nullptr; }
            lock.unlock();
            (void)hipFree(victim);
            (void)hipGetLastError();
            lock.lock();
            if (bw) bw->busy = false; else bc->busy = false;
            cv_.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::unordered_map<int, DeviceCache> dev_;        // device ordinal -> cached device resources
    size_t cap_ = (size_t)32 << 30;
};

inline void counters_to_stats(const unsigned long long* c, trt_stats* st) {
    st->samples = c[CTR_SAMPLES]; st->rays = c[CTR_RAYS]; st->node_tests = c[CTR_NODE]; st->sphere_tests = c[CTR_SPHERE];
    st->quad_plane_tests = c[CTR_QUAD_PLANE]; st->quad_inside_tests = c[CTR_QUAD_INSIDE]; st->shades = c[CTR_SHADE];
    for (int i = 0; i < 4; i++) st->wave_trips[i] = c[CTR_W_ROUNDS + i];
    st->gather_per_band = 0;
}

// One blocking call on a render context of the current device: acquire, the call's steps in order, finish.  The first step that fails is
// kept (status and thread-local message) and every later one does nothing; a HIP call handed to step() is made only while ok():
//   if (run.ok()) run.step(hipMemcpyAsync(...), "hipMemcpyAsync(...)");
// The destructor synchronises the stream (unless finish() already has), then frees the call's own device allocations, then gives the
// context back: on every path the stream is drained before the context is reused.
class CtxRun {
  public:
    explicit CtxRun(SceneCache& cache, int dev = -1) : cache_(cache), dev_(dev) { if (dev < 0) step(hipGetDevice(&dev_), "hipGetDevice"); }     // -1: the current device
    CtxRun(const CtxRun&) = delete;
    ~CtxRun() {
        if (!c_) return;
        if (!drained_) (void)hipStreamSynchronize(c_->stream);
        for (int k = 0; k < n_owned_; k++) (void)hipFree(owned_[k]);
        if (!ok()) (void)hipGetLastError();
        cache_.context_release(dev_, c_);
    }
    bool ok() const { return rc_ == TRT_OK; }
    // the context, with a device frame of at least `frame_bytes` (0: none needed)
    void acquire(size_t frame_bytes) { if (ok()) rc_ = cache_.context_acquire(dev_, frame_bytes, &c_); }
    hipStream_t stream() const { return c_ ? c_->stream : nullptr; }
    float* frame() const { return c_ ? c_->d_accum : nullptr; }
    unsigned long long* counters() const { return c_ ? c_->d_ctr : nullptr; }
    // a device allocation of this call's own (at most two), freed by the destructor behind the synchronise; failing, it is `code` with "`what`: " in front
    template <class T>
    void alloc(T** p, size_t bytes, const char* what, int code) {
        if (!ok()) return;
        const hipError_t e = n_owned_ < 2 ? hipMalloc(reinterpret_cast<void**>(p), bytes) : hipErrorInvalidValue;
        if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; rc_ = query_fail(code, std::string(what) + ": " + hipGetErrorString(e)); return; }
        owned_[n_owned_++] = *p;
    }
    void zero_counters() { if (ok()) step(hipMemsetAsync(c_->d_ctr, 0, CTR_COUNT * sizeof(unsigned long long), c_->stream), "hipMemsetAsync(counters)"); }
    void step(hipError_t e, const char* what) { if (ok() && e != hipSuccess) rc_ = query_fail_hip(e, what); }
    void step(int status) { if (ok()) rc_ = status; }                 // of a callee that has set the message itself (enqueue_render)
    void time_begin() { if (ok()) step(hipEventRecord(c_->ev0, c_->stream), "hipEventRecord(ev0)"); }
    void time_end() { if (ok()) step(hipEventRecord(c_->ev1, c_->stream), "hipEventRecord(ev1)"); }
    // the last step: the counters come down (`h_ctr` lives longer than this object), the stream is synchronised, `*ms` is the time between time_begin()
    // and time_end().  Returns the call's status.
    int finish(unsigned long long (&h_ctr)[CTR_COUNT], float* ms) {
        if (ok()) step(hipMemcpyAsync(h_ctr, c_->d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, c_->stream), "hipMemcpyAsync(counters)");
        if (ok()) { step(hipStreamSynchronize(c_->stream), "hipStreamSynchronize"); drained_ = ok(); }
        if (ok()) step(hipEventElapsedTime(ms, c_->ev0, c_->ev1), "hipEventElapsedTime");
        return rc_;
    }
    // ... into `stats` (may be null), with the time as kernel_ms.  (The counters land in a member: where they land must outlive the destructor's drain.)
    int finish(trt_stats* stats) {
        float ms = 0.0f;
        if (finish(h_ctr_, &ms) == TRT_OK && stats) { counters_to_stats(h_ctr_, stats); stats->kernel_ms = ms; }
        return rc_;
    }
  private:
    SceneCache& cache_;
    int dev_ = 0;
    RenderCtx* c_ = nullptr;
    int rc_ = TRT_OK, n_owned_ = 0;
    bool drained_ = false;
    void* owned_[2] = {nullptr, nullptr};
    unsigned long long h_ctr_[CTR_COUNT] = {0};
};

}  // namespace trt
