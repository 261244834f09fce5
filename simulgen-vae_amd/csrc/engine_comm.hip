// Data-parallel plumbing: RCCL resolved with dlopen, the fake collective of the tests, the per-bucket all-reduce, the calls that register a communicator.
#include <dlfcn.h>
#include "engine_internal.h"

// ---- RCCL, resolved at run time --------------------------------------------------------------------------------
RcclApi g_rccl;
namespace {
int rccl_load() {
    if (g_rccl.h) return 0;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) return fail(SGV_ERR_STATE, "RCCL not found (dlopen librccl.so.1): %s", dlerror());
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(h, "ncclAllReduce");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(h, "ncclGetErrorString");
    g_rccl.CommCount = (decltype(g_rccl.CommCount))dlsym(h, "ncclCommCount");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllReduce)
        return fail(SGV_ERR_STATE, "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllReduce");
    g_rccl.h = h;
    return 0;
}
// ---- test double for the collective (sgv_test_fake_collective): "all-reduce" = multiply the range in place by k on the given
// stream.  With k a power of two every element the engine hands to a collective is scaled exactly, so a step through the fake must
// leave bitwise the state of a plain step at (k alpha, k beta) -- if and only if every gradient element and every <G,W> slot went
// through exactly one collective (backward is linear in (alpha, beta); tests/test_modules_gpu.py).
float g_fake_k = 0.f;
long g_fake_calls = 0, g_fake_elems = 0;
extern "C" {
__global__ void fake_scale_f32_kernel(float* p, size_t n, float k) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] *= k;
}
__global__ void fake_scale_bf16_kernel(bf16_t* p, size_t n, float k) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = (bf16_t)((float)p[i] * k);
}
}
int fake_allreduce(const void* in, void* out, size_t count, int dtype, int op, void* comm, hipStream_t st) {
    (void)comm;
    if (in != out || op != kNcclAvg || (dtype != kNcclFloat32 && dtype != kNcclBfloat16)) return 1;
    ++g_fake_calls; g_fake_elems += (long)count;
    if (!count) return 0;
    const int blocks = (int)std::min<size_t>((count + 255) / 256, 4096);
    if (dtype == kNcclFloat32) hipLaunchKernelGGL(fake_scale_f32_kernel, dim3(blocks), dim3(256), 0, st, (float*)out, count, g_fake_k);
    else hipLaunchKernelGGL(fake_scale_bf16_kernel, dim3(blocks), dim3(256), 0, st, (bf16_t*)out, count, g_fake_k);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
int rccl_rc(const char* what, int rc) {       // an RCCL call's return code as the library's: SGV_OK, or the error with RCCL's message
    return rc ? fail(SGV_ERR_HIP, "%s failed: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error") : SGV_OK;
}
}  // namespace

static std::map<void*, int> g_comm_ranks;      // communicator -> number of ranks (one rank: the mean is the identity, nothing is issued)
// a one-rank communicator exchanges nothing: its all-reduces are skipped -- unless SGV_FORCE_COLLECTIVE=1 asks for the one-GPU
// rehearsal of the N > 1 path (every bucket packed, handed to ncclAllReduce and unpacked as with more ranks)
bool comm_is_single(void* comm) {
    const char* f = getenv("SGV_FORCE_COLLECTIVE");      // read per call: tests switch it inside one process
    if (f && atoi(f) == 1) return false;
    auto it = g_comm_ranks.find(comm);
    return it != g_comm_ranks.end() && it->second == 1;
}
// bucket b: wait (on the communication stream) for what the engine stream holds so far, average it over the ranks.
// split_dots: the <G,W_eff> slots of a weight bucket's conv layers travel with the bucket (a second, tiny fp32 all-reduce of
// bucket_dots[b]) and the small bucket leaves them out -- the bucket's AdamW then needs nothing from the end of backward.
int rccl_bucket(sgv_engine* e, void* comm, hipStream_t cs, int b, hipEvent_t done, bool split_dots) {
    CHK(stream_wait(e, cs, e->stream));
    float* g = e->grads + e->buckets[b].first;
    if (!comm_is_single(comm)) {
        const bool small = b == (int)e->buckets.size() - 1;
        const bool lp = b < (int)e->bucket_packed.size() && e->bucket_packed[b];
        void* w = lp ? (void*)((char*)e->grads_lp + 2 * e->buckets[b].first) : (void*)g;
        size_t cnt = e->buckets[b].second;
        if (small && split_dots) { w = (void*)(g + e->dots_total); cnt -= e->dots_total; }
        int rc = g_rccl.AllReduce(w, w, cnt, lp ? kNcclBfloat16 : kNcclFloat32, kNcclAvg, comm, cs);
        if (rc) return rccl_rc("ncclAllReduce", rc);
        if (!small && split_dots && e->bucket_dots[b].second) {
            float* d = e->grads + e->bucket_dots[b].first;
            rc = g_rccl.AllReduce(d, d, e->bucket_dots[b].second, kNcclFloat32, kNcclAvg, comm, cs);
            if (rc) return rccl_rc("ncclAllReduce(<G,W> slots)", rc);
        }
    }
    if (done) HIPCHK(hipEventRecord(done, cs));
    return 0;
}

int sgv_rccl_probe(void) { return rccl_load(); }
int sgv_rccl_comm_count(void* comm, int* nranks) {
    if (!comm || !nranks) return fail(SGV_ERR_ARG, "null argument");
    CHK(rccl_load());
    if (g_fake_k != 0.f) { *nranks = 0; return SGV_OK; }                  // the test double has no ranks
    if (!g_rccl.CommCount) return fail(SGV_ERR_STATE, "librccl lacks ncclCommCount");
    return rccl_rc("ncclCommCount", g_rccl.CommCount(comm, nranks));
}
int sgv_test_fake_collective(float k, long* calls, long* elems) {
    if (calls) *calls = g_fake_calls;
    if (elems) *elems = g_fake_elems;
    g_fake_calls = 0; g_fake_elems = 0;
    if (k != 0.f) {
        g_fake_k = k;
        g_rccl.AllReduce = fake_allreduce;
        if (!g_rccl.h) g_rccl.h = (void*)&g_fake_k;                     // rccl_load: nothing to resolve while the double is installed
    } else if (g_fake_k != 0.f) {
        const bool own = g_rccl.h == (void*)&g_fake_k;
        g_fake_k = 0.f;
        if (own) g_rccl = RcclApi();                                    // the next rccl_load resolves the real library
        else g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(g_rccl.h, "ncclAllReduce");
    }
    return SGV_OK;
}
int sgv_rccl_unique_id(void* id128) {
    if (!id128) return fail(SGV_ERR_ARG, "null argument");
    CHK(rccl_load());
    return rccl_rc("ncclGetUniqueId", g_rccl.GetUniqueId(id128));
}
int sgv_rccl_comm_init(void** comm_out, int nranks, const void* id128, int rank) {
    if (!comm_out || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(SGV_ERR_ARG, "bad argument");
    CHK(rccl_load());
    RcclApi::Id128 id;
    memcpy(id.b, id128, 128);
    const int rc = g_rccl.CommInitRank(comm_out, nranks, id, rank);
    if (!rc) g_comm_ranks[*comm_out] = nranks;
    return rccl_rc("ncclCommInitRank", rc);
}
int sgv_rccl_allreduce(void* comm, void* dev_buf, size_t count, int dtype, void* stream) {
    if (!comm || !dev_buf) return fail(SGV_ERR_ARG, "null argument");
    if (dtype != SGV_DTYPE_F32 && dtype != SGV_DTYPE_BF16) return fail(SGV_ERR_ARG, "bad dtype");
    CHK(rccl_load());
    return rccl_rc("ncclAllReduce", g_rccl.AllReduce(dev_buf, dev_buf, count, dtype == SGV_DTYPE_BF16 ? kNcclBfloat16 : kNcclFloat32, kNcclAvg, comm, (hipStream_t)stream));
}
int sgv_rccl_comm_destroy(void* comm) {
    if (!comm) return SGV_OK;
    CHK(rccl_load());
    return rccl_rc("ncclCommDestroy", g_rccl.CommDestroy(comm));
}
int sgv_allreduce_grads(sgv_engine* e, void* rccl_comm, void* comm_stream) {
    if (!e || !rccl_comm) return fail(SGV_ERR_ARG, "null argument");
    CHK(rccl_load());
    CHK(join_side(e));
    const hipStream_t cs = comm_stream ? (hipStream_t)comm_stream : e->stream;
    for (int b = 0; b < (int)e->buckets.size(); ++b) CHK(rccl_bucket(e, rccl_comm, cs, b, nullptr));
    if (cs != e->stream) CHK(stream_wait(e, e->stream, cs));
    return SGV_OK;
}
int sgv_set_rccl(sgv_engine* e, void* rccl_comm, void* comm_stream) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (rccl_comm && e->cb) return fail(SGV_ERR_STATE, "a bucket callback is registered: use one of the two data-parallel paths");
    if (rccl_comm) {
        if (!comm_stream) return fail(SGV_ERR_ARG, "sgv_set_rccl needs a communication stream of its own");
        CHK(rccl_load());
        while (e->bucket_done.size() < e->buckets.size()) {
            hipEvent_t ev = nullptr;
            HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            e->bucket_done.push_back(ev);
        }
        e->bucket_pending.assign(e->buckets.size(), 0);
        if (!e->tn_sched) HIPCHK(hipMalloc((void**)&e->tn_sched, 8 * 520 * sizeof(int)));
    }
    e->comm = rccl_comm;
    e->comm_stream = (hipStream_t)comm_stream;
    return SGV_OK;
}

int sgv_set_bucket_callback(sgv_engine* e, sgv_bucket_cb cb, void* user) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (cb && e->comm) return fail(SGV_ERR_STATE, "an RCCL communicator is registered: use one of the two data-parallel paths");
    if (cb && !e->tn_sched) HIPCHK(hipMalloc((void**)&e->tn_sched, 8 * 520 * sizeof(int)));
    e->cb = cb; e->cb_user = user;
    return SGV_OK;
}
