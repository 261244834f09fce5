// The engine's auxiliary streams: the probe that tells which hardware queue a new stream landed on, the streams created on first use,
// and the event waits that order one stream behind another.
#include "engine_internal.h"

// Auxiliary streams.  The HIP runtime maps streams onto a handful of hardware queues PER PRIORITY LEVEL (GPU_MAX_HW_QUEUES = 4),
// round-robin in creation order, and two streams on one queue run their kernels strictly one after the other: a kernel trace showed
// the second compute lane and the collective's stream sharing the main stream's queue (no overlap at all) depending on how many
// streams the process had created before.  Every auxiliary stream has the main stream's (normal) priority and is probed instead:
// streams of another priority level come from another queue pool, but measured no faster.
// ---- which hardware queue did a new stream land on? ----
// Not visible through the API, but observable: a kernel on stream b cannot finish while a kernel on stream a spins if both sit
// on one queue.  probe_spin_kernel waits on the constant-rate clock for a bounded time (always exits), probe_nop_kernel is empty.
extern "C" {
__global__ void probe_spin_kernel(long long ticks) {
    const long long t0 = (long long)wall_clock64();
    while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
__global__ void probe_nop_kernel() {}
}
// One probe: 1 = kernels of a and b run concurrently (different hardware queues), 0 = b's kernel finished only after a's, -1 = API
// error.  Decided by the ORDER of two device-side timestamps (the event behind the spin on a, the event behind the empty kernel
// on b), not by host wall time: if b's kernel ended while a was still spinning, the queues are different.
static int streams_overlap_once(hipStream_t a, hipStream_t b, long long ticks) {
    hipEvent_t e0 = nullptr, ea = nullptr, eb = nullptr;
    if (hipEventCreate(&e0) != hipSuccess) return -1;
    if (hipEventCreate(&ea) != hipSuccess) { hipEventDestroy(e0); return -1; }
    if (hipEventCreate(&eb) != hipSuccess) { hipEventDestroy(e0); hipEventDestroy(ea); return -1; }
    int res = -1;
    if (hipEventRecord(e0, a) == hipSuccess) {
        hipLaunchKernelGGL(probe_spin_kernel, dim3(1), dim3(64), 0, a, ticks);
        if (hipEventRecord(ea, a) == hipSuccess) {
            hipLaunchKernelGGL(probe_nop_kernel, dim3(1), dim3(64), 0, b);
            float ta = 0.f, tb = 0.f;       // both measured from e0, which precedes both kernels: never a negative interval
            if (hipEventRecord(eb, b) == hipSuccess && hipStreamSynchronize(b) == hipSuccess && hipStreamSynchronize(a) == hipSuccess &&
                hipEventElapsedTime(&ta, e0, ea) == hipSuccess && hipEventElapsedTime(&tb, e0, eb) == hipSuccess)
                res = tb < ta - 0.02f ? 1 : 0;        // b's kernel was over >= 20 us before the spin ended
        }
    }
    hipStreamSynchronize(a);
    hipEventDestroy(e0); hipEventDestroy(ea); hipEventDestroy(eb);
    (void)hipGetLastError();
    return res;
}
// true: kernels of a and b run concurrently; on any API error: true (no reason to reject the stream).  The candidate gets an untimed
// first launch (a new stream's first launch can take longer than the spin), and a "shares a queue" verdict is confirmed once with a
// ten times longer spin: a host that needed more than 300 us to submit the empty kernel (loaded box, profiler attached) would
// otherwise reject a good candidate.
bool streams_overlap(hipStream_t a, hipStream_t b) {
    hipLaunchKernelGGL(probe_nop_kernel, dim3(1), dim3(64), 0, b);
    if (hipStreamSynchronize(b) != hipSuccess) { (void)hipGetLastError(); return true; }
    int r = streams_overlap_once(a, b, 30000LL);              // 300 us at the 100 MHz constant clock
    if (r == 0) r = streams_overlap_once(a, b, 300000LL);     // 3 ms
    return r != 0;
}
// A new auxiliary stream that shares its hardware queue with none of `avoid`.  The runtime gives a new stream the least-loaded
// queue (round-robin in a fresh process; in a process that has created and destroyed many streams the main stream's queue can be the
// emptiest for many creations in a row), so the rejected candidates stay alive until a keeper is found -- every reject loads the
// queue it sits on and steers the next candidate elsewhere -- and up to 32 candidates are tried (0.3 ms each per stream to avoid).
// If every candidate collides the last one is kept.
hipError_t make_aux_stream(hipStream_t* out, const char* label, std::initializer_list<hipStream_t> avoid) {
    std::vector<hipStream_t> rejected;
    hipStream_t s = nullptr;
    hipError_t rc = hipSuccess;
    constexpr int kAttempts = 32;
    for (int attempt = 0; attempt < kAttempts; ++attempt) {
        s = nullptr;
        rc = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (rc != hipSuccess) break;
        bool ok = true;
        for (hipStream_t a : avoid) if (a != s && !streams_overlap(a, s)) { ok = false; break; }      // a == nullptr is the null stream: probed too
        if (getenv("SGV_STREAM_LOG")) fprintf(stderr, "[sgvae] %s stream: candidate %d %s\n", label, attempt, ok ? "kept" : "shares a hardware queue with a stream it must not, rejected");
        if (ok) break;
        if (attempt == kAttempts - 1) {
            // kept all the same: the engine stays correct, but this stream's kernels now run between the other stream's instead of
            // beside them (no lane / optimizer / communication overlap) -- say so once, the bench line reports it as well
            fprintf(stderr, "[sgvae] warning: %s stream: all %d candidate streams share a hardware queue with a stream they must avoid "
                            "(GPU_MAX_HW_QUEUES too small for this process?); overlap on this stream is lost\n", label, kAttempts);
            break;
        }
        rejected.push_back(s);
    }
    for (hipStream_t r : rejected) hipStreamDestroy(r);
    *out = rc == hipSuccess ? s : nullptr;
    return rc;
}
// the engine's on-demand streams: made at first use, nullptr if that failed (make_aux_stream leaves nullptr behind)
static hipStream_t ensure(hipStream_t* slot, const char* label, std::initializer_list<hipStream_t> avoid) {
    if (!*slot) make_aux_stream(slot, label, avoid);
    return *slot;
}
// never on the main stream's queue: an AdamW launch that waits for a collective there would hold back every kernel behind it
hipStream_t ensure_opt(sgv_engine* e) { return ensure(&e->opt, "optimizer", {e->stream, e->side, e->lane2}); }
// a communication stream for sgv_set_rccl that is guaranteed not to sit on the main stream's hardware queue (a collective there
// would run strictly between the main stream's kernels instead of beside them)
hipStream_t ensure_comm_own(sgv_engine* e) { return ensure(&e->comm_own, "communication", {e->stream, e->side, e->lane2}); }
hipStream_t ensure_wire(sgv_engine* e) { return ensure(&e->wire, "wire", {e->stream, e->side}); }
hipEvent_t next_event(sgv_engine* e) {
    if (e->ev_next == e->ev_pool.size()) {
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return nullptr;
        e->ev_pool.push_back(ev);
    }
    return e->ev_pool[e->ev_next++];
}
// `waiter` waits for everything enqueued on `of` so far
int stream_wait(sgv_engine* e, hipStream_t waiter, hipStream_t of) {
    hipEvent_t ev = next_event(e);
    if (!ev) return fail(SGV_ERR_HIP, "event creation failed");
    HIPCHK(hipEventRecord(ev, of));
    HIPCHK(hipStreamWaitEvent(waiter, ev, 0));
    return 0;
}
// make the main stream wait for every weight-gradient GEMM issued so far on the side stream
int join_side(sgv_engine* e) {
    if (!e->side_dirty) return 0;
    CHK(stream_wait(e, e->stream, e->side));
    e->side_dirty = false;
    return 0;
}

// the three getters of the C ABI: the stream `get` makes or finds goes to *stream; `err` if there is none
static int stream_out(sgv_engine* e, void** stream, hipStream_t (*get)(sgv_engine*), const char* err) {
    if (!e || !stream) return fail(SGV_ERR_ARG, "null argument");
    hipStream_t s = get(e);
    if (s) *stream = (void*)s;
    return s ? SGV_OK : fail(SGV_ERR_HIP, "%s", err);
}
int sgv_comm_stream(sgv_engine* e, void** stream) { return stream_out(e, stream, ensure_comm_own, "stream creation failed"); }
int sgv_wire_stream(sgv_engine* e, void** stream) { return stream_out(e, stream, ensure_wire, "the engine has no wire stream"); }
int sgv_opt_stream(sgv_engine* e, void** stream) { return stream_out(e, stream, ensure_opt, "the engine has no optimizer stream"); }
