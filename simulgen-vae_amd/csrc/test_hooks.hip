// Test hooks (sgv_test_* of include/sgvae.h): caller-owned device buffers in, the launcher the engine calls, a sync, an error code out.
// Only sgv_test_stream_overlap looks inside an engine (the others take fail / HIPCHK / CHK / align_up / sum_slabs from the private header, the recon-tail hooks their tails from recon_tails.h);
// sgv_test_fake_collective lives with the collective it replaces (engine_comm.hip).
#include "engine_internal.h"
#include "recon_tails.h"

// a dense NT problem on caller-owned buffers: A [M][K], W [taps][N][K], C and addend [M][N]
static GemmNT dense_nt(const void* A, const void* W, void* C, const float* bias, const float* scale, const void* addend, int M, int N,
                       int K, int taps, int Tlen, int splitk, int out_f32) {
    GemmNT p; memset(&p, 0, sizeof(p));
    p.A = A; p.lda = K; p.W = W; p.ldw = K; p.w_tap_stride = (long)N * K; p.C = C; p.ldc = N;
    p.addend = addend; p.ldadd = N; p.bias = bias; p.scale = scale;
    p.M = M; p.N = N; p.K = K; p.taps = taps; p.pad = (taps - 1) / 2; p.Tlen = Tlen; p.splitk = splitk < 1 ? 1 : splitk; p.out_f32 = out_f32;
    return p;
}
// tail of the GEMM hooks: sync, free the hook's scratch, then report what `launcher` returned and how `kernel` ended
static int gemm_hook_done(int r, const char* launcher, const char* kernel, void* stream, std::initializer_list<void*> scratch) {
    const hipError_t se = hipStreamSynchronize((hipStream_t)stream);
    for (void* p : scratch) if (p) hipFree(p);
    if (r) return fail(SGV_ERR_ARG, "%s rejected the arguments (%d)", launcher, r);
    if (se != hipSuccess) return fail(SGV_ERR_HIP, "%s failed: %s", kernel, hipGetErrorString(se));
    return SGV_OK;
}
// tail of the two fused Conv + GroupNorm hooks
static int conv_gn_hook_done(int r, const char* what, void* stream) {
    const hipError_t se = hipStreamSynchronize((hipStream_t)stream);
    return r || se != hipSuccess ? fail(SGV_ERR_HIP, "%s launch failed (%d, %s)", what, r, hipGetErrorString(se)) : SGV_OK;
}

extern "C" {
int sgv_test_gemm_nt(int dtype, const void* A, const void* W, void* C, const float* bias, const float* scale, const void* addend,
                     int M, int N, int K, int taps, int Tlen, int splitk, int out_f32, void* stream) {
    GemmNT p = dense_nt(A, W, C, bias, scale, addend, M, N, K, taps, Tlen, splitk, out_f32);
    if (p.splitk > 1) HIPCHK(hipMalloc((void**)&p.partial, sizeof(float) * (size_t)p.splitk * M * N));
    return gemm_hook_done(launch_gemm_nt(dtype, p, (hipStream_t)stream), "launch_gemm_nt", "gemm_nt", stream, {p.partial});
}

int sgv_test_gemm_nt_stats(const void* A, const void* W, void* C, const float* bias, const void* addend, int M, int N, int K,
                           int taps, int Tlen, int Cg, double* sums, void* stream) {
    if (Cg < 1 || N % Cg) return fail(SGV_ERR_ARG, "N must be a multiple of Cg");
    GemmNT p = dense_nt(A, W, C, bias, nullptr, addend, M, N, K, taps, Tlen, 1, 0);
    p.gn_sums = sums; p.gn_Cg = Cg; p.gn_G = N / Cg;
    return gemm_hook_done(launch_gemm_nt(SGV_DTYPE_BF16, p, (hipStream_t)stream), "launch_gemm_nt", "gemm_nt", stream, {});
}

int sgv_test_conv_gn_fwd(const void* A, const void* W, const float* bias, const float* scale, const void* res, const float* gamma,
                         const float* beta, void* y, void* out, double* sums, int B, int T, int N, int K, int taps, int G, float rscale,
                         void* stream) {
    ConvGN q; memset(&q, 0, sizeof(q));
    q.A = A; q.lda = K; q.W = W; q.ldw = K; q.w_tap_stride = (long)N * K; q.bias = bias; q.scale = scale;
    q.y = y; q.ldy = N; q.out = out; q.ldout = N; q.res = res; q.ldres = N; q.rscale = rscale; q.gamma = gamma; q.beta = beta; q.sums = sums;
    q.B = B; q.T = T; q.N = N; q.K = K; q.taps = taps; q.pad = (taps - 1) / 2; q.G = G; q.Cg = G > 0 ? N / G : 0;
    if (!conv_gn_fused_eligible(SGV_DTYPE_BF16, q)) return fail(SGV_ERR_ARG, "shape not taken by the fused conv + GroupNorm kernel");
    return conv_gn_hook_done(launch_conv_gn_fwd(q, (hipStream_t)stream), "conv_gn", stream);
}
int sgv_test_conv_gn_bwd(const void* A, const void* W, const float* scale, const void* addend, const void* premul, void* da, const void* y,
                         const double* sums, const float* gamma,
                         const float* beta, const float* cbias, void* dy, double* sums2, float* ptot, float* cdot_part, int B, int T,
                         int N, int K, int taps, int G, void* stream) {
    ConvGNBwd q; memset(&q, 0, sizeof(q));
    q.A = A; q.lda = K; q.W = W; q.ldw = K; q.w_tap_stride = (long)N * K; q.scale = scale; q.addend = addend; q.ldadd = N;
    q.premul = premul; q.ldpre = N; q.da = da; q.ldda = N;
    q.y = y; q.ldy = N; q.sums = sums; q.gamma = gamma; q.beta = beta; q.cbias = cbias; q.dy = dy; q.lddy = N;
    q.sums2 = sums2; q.ptot = ptot; q.cdot_part = cdot_part; q.rscale = 1.f; q.gscale = 1.f;
    q.B = B; q.T = T; q.N = N; q.K = K; q.taps = taps; q.pad = (taps - 1) / 2; q.G = G; q.Cg = G > 0 ? N / G : 0;
    if (!conv_gn_bwd_eligible(SGV_DTYPE_BF16, q)) return fail(SGV_ERR_ARG, "shape not taken by the fused input-gradient + GroupNorm backward kernel");
    return conv_gn_hook_done(launch_conv_gn_bwd(q, (hipStream_t)stream), "conv_gn_bwd", stream);
}
// 256x256 persistent kernel (gemm256.hip), bf16.  mode 0: forced (launch_gemm_nt256, split-K as given), 1: the engine's plan
// (gemm_nt_plan: kernel choice, split-K, main + tail rows).  sums != null: fused GroupNorm statistics (mode 0, split-K 1).
int sgv_test_gemm_nt256(const void* A, const void* W, void* C, const float* bias, const float* scale, const void* addend, int M, int N,
                        int K, int taps, int Tlen, int splitk, int out_f32, int mode, int Cg, double* sums, int* plan_kind, void* stream) {
    GemmNT p = dense_nt(A, W, C, bias, scale, addend, M, N, K, taps, Tlen, splitk, out_f32);
    const size_t cap = (size_t)32 << 20;
    float* part = nullptr;
    HIPCHK(hipMalloc((void**)&p.partial, sizeof(float) * std::max(cap, (size_t)p.splitk * M * N)));
    if (sums) {
        if (Cg < 1 || N % Cg) { hipFree(p.partial); return fail(SGV_ERR_ARG, "N must be a multiple of Cg"); }
        HIPCHK(hipMalloc((void**)&part, sizeof(float) * gemm_nt256_part_floats(M, N, 1)));
        p.gn_part = part; p.gn_sums = sums; p.gn_Cg = Cg; p.gn_G = N / Cg;
    }
    const int band_code = (mode >> 8) & 0xff, strm_code = (mode >> 16) & 7;
    p.band = band_code == 255 ? -1 : band_code;
    p.strm = strm_code == 7 ? -1 : strm_code;
    const int ts_code = (mode >> 19) & 3;
    p.ts = ts_code == 1 ? 1 : ts_code == 2 ? -1 : 0;
    const bool split_tail = (mode >> 21) & 1;          // planned launch with the 128-row tail as its own 128 x 512 launch (the engine runs it beside the main one)
    mode &= 0xff;
    int r;
    if (split_tail) {
        // the split is forced here (the planner's cost comparison and the "tail shorter than the main launch" rule decide speed, not results)
        GemmPlan pl = gemm_nt_plan(SGV_DTYPE_BF16, p, cap, 0);
        if (M % 256 != 128 || M < 384) { hipFree(p.partial); return fail(SGV_ERR_ARG, "split-tail test mode needs M = 128 (mod 256)"); }
        pl.kind = 2; pl.m_main = M - 128; pl.fuse_stats = 0;
        pl.sk_main = std::max(1, std::min(p.splitk, 8));
        if (plan_kind) *plan_kind = pl.kind;
        float* tp = nullptr;
        HIPCHK(hipMalloc((void**)&tp, sizeof(float) * cap));
        int sk_t = gemm_nt_tail_split(SGV_DTYPE_BF16, p, pl, cap);
        if (sk_t <= 0) {
            const long tkt = (long)taps * ((K + 63) / 64);
            sk_t = (int)std::max(1L, std::min((long)(16 / std::max(1, (N + 511) / 512)), tkt / 24));
        }
        if (N < 512) r = -4;
        else {
            r = launch_gemm_nt_main(p, pl, (hipStream_t)stream);
            if (!r) r = launch_gemm_nt_tail(p, pl, sk_t, tp, (hipStream_t)stream);
        }
        hipStreamSynchronize((hipStream_t)stream);
        hipFree(tp);
    } else if (mode == 0) {
        if (plan_kind) *plan_kind = p.ts == 1 ? 3 : 1;
        if (p.ts < 0) p.ts = 0;
        r = launch_gemm_nt256(p, (hipStream_t)stream);
    } else {
        const GemmPlan pl = gemm_nt_plan(SGV_DTYPE_BF16, p, cap, sums != nullptr);
        if (plan_kind) *plan_kind = pl.kind;
        if (sums && !pl.fuse_stats) r = -3;
        else r = launch_gemm_nt_planned(SGV_DTYPE_BF16, p, pl, (hipStream_t)stream);
    }
    return gemm_hook_done(r, "the 256x256 GEMM path", "gemm_nt256", stream, {p.partial, part});
}

int sgv_test_stream_overlap(sgv_engine* e, int which, int* overlaps) {
    if (!e || !overlaps) return fail(SGV_ERR_ARG, "null argument");
    hipStream_t s = which == 0 ? e->lane2 : which == 1 ? e->side : which == 2 ? ensure_opt(e) : which == 3 ? ensure_comm_own(e) : nullptr;
    if (which < 0 || which > 3) return fail(SGV_ERR_ARG, "which must be 0..3");
    if (!s) { *overlaps = -1; return SGV_OK; }
    HIPCHK(hipStreamSynchronize(e->stream));
    *overlaps = streams_overlap(e->stream, s) ? 1 : 0;
    return SGV_OK;
}
// Test hook: occupy part of the chip for a bounded time (what a resident collective's channel workgroups do): `blocks` workgroups
// of `threads` threads and `lds_bytes` of LDS each spin on the constant-rate clock for `ticks` (100 MHz) on `stream`; returns at once.
__global__ void occupy_spin_kernel(long long ticks) {
    extern __shared__ char occ_lds[];
    if (threadIdx.x == 0xFFFFFF) occ_lds[0] = 1;
    const long long t0 = (long long)wall_clock64();
    while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
int sgv_test_occupy(void* stream, int blocks, int threads, int lds_bytes, long long ticks) {
    if (blocks < 1 || blocks > 1024 || threads < 64 || threads > 1024 || lds_bytes < 0 || lds_bytes > 160 * 1024 || ticks < 0 || ticks > 1000000)
        return fail(SGV_ERR_ARG, "sgv_test_occupy: argument out of range (at most 1024 workgroups, 10 ms)");
    hipLaunchKernelGGL(occupy_spin_kernel, dim3(blocks), dim3(threads), (size_t)lds_bytes, (hipStream_t)stream, ticks);
    return hipGetLastError() == hipSuccess ? SGV_OK : fail(SGV_ERR_HIP, "occupy launch failed");
}
int sgv_test_gemm_tn(int dtype, const void* A, const void* Bm, float* dW, int M, int N1, int N2, int taps, int Tlen, int splitk,
                     int use_tr, void* stream) {
    GemmTN p; memset(&p, 0, sizeof(p));
    p.A = A; p.lda = N1; p.B = Bm; p.ldb = N2; p.out = dW; p.ldo = N2; p.out_tap_stride = (long)N1 * N2;
    p.M = M; p.N1 = N1; p.N2 = N2; p.taps = taps; p.pad = (taps - 1) / 2; p.Tlen = Tlen; p.splitk = splitk < 1 ? 1 : splitk; p.use_tr = use_tr != 0; p.force_w2 = use_tr == 2 ? 1 : use_tr == 3 ? 2 : (use_tr == 4 || use_tr == 6 || use_tr == 7) ? 3 : use_tr == 5 ? -1 : 0;
    p.out_bf16 = use_tr == 6 ? 1 : 0;          // 6: the 256 x 256 kernel with bf16 output (dW is then a bf16 array; splitk 1)
    // 7: the 256 x 256 kernel in its work-stealing form
    static int* test_sched = nullptr;          // allocated once: an allocation per call would wait for whatever else runs on the device
    if (use_tr == 7) { if (!test_sched) HIPCHK(hipMalloc((void**)&test_sched, 513 * sizeof(int))); p.sched = test_sched; }
    if (p.out_bf16 && (splitk > 1 || !gemm_tn256_eligible(dtype, p))) return fail(SGV_ERR_ARG, "sgv_test_gemm_tn: bf16 output needs the 256 x 256 kernel and splitk 1");
    float* partial = nullptr;
    const long nw = (long)taps * N1 * N2;
    if (p.splitk > 1) {
        HIPCHK(hipMalloc((void**)&partial, sizeof(float) * (size_t)p.splitk * nw));
        p.out = partial; p.out_slab_stride = nw;
    }
    int r = launch_gemm_tn(dtype, p, (hipStream_t)stream);
    if (!r && p.splitk > 1) sum_slabs(dW, partial, p.splitk, nw, (hipStream_t)stream);
    return gemm_hook_done(r, "launch_gemm_tn", "gemm_tn", stream, {partial});
}

// ---- test hooks for the non-GEMM kernels (ew.hip, recon_out.hip): argument checks, the launcher the engine calls, sync ----
static int ew_hook_done(int r, const char* what, void* stream) {
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipStreamSynchronize((hipStream_t)stream);
    if (r) return fail(SGV_ERR_ARG, "%s: the launcher rejected the arguments (%d)", what, r);
    if (le != hipSuccess) return fail(SGV_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(le));
    if (se != hipSuccess) return fail(SGV_ERR_HIP, "%s failed: %s", what, hipGetErrorString(se));
    return SGV_OK;
}
static int gn_hook_shape(const char* what, int dtype, int B, int T, int C, int G, const float* work, size_t work_floats) {
    if (dtype != SGV_DTYPE_F32 && dtype != SGV_DTYPE_BF16) return fail(SGV_ERR_ARG, "%s: dtype must be SGV_DTYPE_F32 or SGV_DTYPE_BF16", what);
    if (B < 1 || T < 1 || C < 8 || C % 8) return fail(SGV_ERR_ARG, "%s: B, T >= 1 and C %% 8 == 0 required (B %d, T %d, C %d)", what, B, T, C);
    if (G < 1 || G > SGV_GN_MAX_GROUPS || C % G) return fail(SGV_ERR_ARG, "%s: 1 <= G <= %d and C %% G == 0 required (C %d, G %d)", what, SGV_GN_MAX_GROUPS, C, G);
    if (!work || work_floats < ew_gn_part_floats(B, T, C))
        return fail(SGV_ERR_ARG, "%s: workspace of %zu floats given, %zu needed", what, work ? work_floats : (size_t)0, ew_gn_part_floats(B, T, C));
    return SGV_OK;
}
static bool ld_ok(long ld, int C) { return ld >= C && ld % 8 == 0; }
size_t sgv_test_gn_workspace_floats(int B, int T, int C) {
    if (B < 1 || T < 1 || C < 8 || C % 8) return 0;
    return ew_gn_part_floats(B, T, C);
}
int sgv_test_gn_fwd(int dtype, int act, const void* y, long ldy, const void* res, long ldres, float rscale, void* out, long ldout,
                    const float* gamma, const float* beta, double* sums, float* work, size_t work_floats, int B, int T, int C, int G,
                    int* path, void* stream) {
    CHK(gn_hook_shape("sgv_test_gn_fwd", dtype, B, T, C, G, work, work_floats));
    if (!y || !out || !gamma || !beta || !sums) return fail(SGV_ERR_ARG, "sgv_test_gn_fwd: null argument");
    if (act < 0 || act > 3) return fail(SGV_ERR_ARG, "sgv_test_gn_fwd: act must be 0 none, 1 gelu, 2 tanh or 3 relu");
    if (!ld_ok(ldy, C) || !ld_ok(ldout, C) || (res && !ld_ok(ldres, C))) return fail(SGV_ERR_ARG, "sgv_test_gn_fwd: row strides must be >= C and multiples of 8");
    GNParams p;
    p.y = y; p.ldy = ldy; p.res = res; p.ldres = ldres; p.rscale = rscale; p.out = out; p.ldout = ldout;
    p.gamma = gamma; p.beta = beta; p.sums = sums; p.part = work; p.B = B; p.T = T; p.C = C; p.G = G; p.Cg = C / G;
    if (path) *path = gn_fused_ok(p) ? 1 : 0;
    return ew_hook_done(ew_gn_fwd(dtype, act, p, (hipStream_t)stream), "sgv_test_gn_fwd", stream);
}
int sgv_test_gn_bwd(int dtype, int act, const void* y, long ldy, const void* dout, long lddout, float rscale, float gscale,
                    const float* gamma, const float* beta, const double* sums, void* dy, long lddy, double* sums2, float* dgamma,
                    float* dbeta, float* dbias, float* cdot, const float* cbias, int accum_affine, float* work, size_t work_floats,
                    int B, int T, int C, int G, int* path, void* stream) {
    CHK(gn_hook_shape("sgv_test_gn_bwd", dtype, B, T, C, G, work, work_floats));
    if (!y || !dout || !gamma || !beta || !sums || !dy || !sums2) return fail(SGV_ERR_ARG, "sgv_test_gn_bwd: null argument");
    if (act != 0 && act != 1 && act != 3) return fail(SGV_ERR_ARG, "sgv_test_gn_bwd: act must be 0 none, 1 gelu or 3 relu");
    if (!ld_ok(ldy, C) || !ld_ok(lddout, C) || !ld_ok(lddy, C)) return fail(SGV_ERR_ARG, "sgv_test_gn_bwd: row strides must be >= C and multiples of 8");
    GNParams p;
    p.y = y; p.ldy = ldy; p.dout = dout; p.lddout = lddout; p.rscale = rscale; p.gscale = gscale; p.out = dy; p.ldout = lddy;
    p.gamma = gamma; p.beta = beta; p.sums = const_cast<double*>(sums); p.sums2 = sums2; p.dgamma = dgamma; p.dbeta = dbeta; p.dbias = dbias;
    p.cdot = cdot; p.cbias = cbias; p.accum_affine = accum_affine ? 1 : 0; p.part = work;
    p.B = B; p.T = T; p.C = C; p.G = G; p.Cg = C / G;
    if (path) *path = gn_fused_bwd_ok(p) ? 1 : 0;
    return ew_hook_done(ew_gn_bwd(dtype, act, p, (hipStream_t)stream), "sgv_test_gn_bwd", stream);
}
int sgv_test_recon_loss(int dtype, int train, int loss_type, const void* y, long ldy, const void* x, long ldx, void* xhat, long ldxhat,
                        const float* gamma, const float* beta, double* sums, double* loss_sums, double* sums2, float* unit, float gscale,
                        void* dy, long lddy, float* cdot, const float* cbias, float* work, size_t work_floats, int B, int T, int C,
                        int G, void* stream) {
    CHK(gn_hook_shape("sgv_test_recon_loss", dtype, B, T, C, G, work, work_floats));
    if (!y || !x || !gamma || !beta || !sums || !loss_sums) return fail(SGV_ERR_ARG, "sgv_test_recon_loss: null argument");
    if (loss_type < SGV_LOSS_MSE || loss_type > SGV_LOSS_HUBER) return fail(SGV_ERR_ARG, "sgv_test_recon_loss: unknown loss kind %d", loss_type);
    if (train && (!sums2 || !unit || !dy)) return fail(SGV_ERR_ARG, "sgv_test_recon_loss: training needs sums2, unit and dy");
    if (!ld_ok(ldy, C) || !ld_ok(ldx, C) || (xhat && !ld_ok(ldxhat, C)) || (train && !ld_ok(lddy, C)))
        return fail(SGV_ERR_ARG, "sgv_test_recon_loss: row strides must be >= C and multiples of 8");
    hipStream_t s = (hipStream_t)stream;
    // forward half, as decoder_fwd: statistics, then tanh + loss (+ the backward reductions)
    GNParams p;
    p.B = B; p.T = T; p.C = C; p.G = G; p.Cg = C / G; p.gamma = gamma; p.beta = beta;
    p.y = y; p.ldy = ldy; p.sums = sums; p.part = work;
    int r = ew_gn_stats(dtype, p, s);
    p.dout = x; p.lddout = ldx; p.loss_type = loss_type; p.loss_sums = loss_sums;
    if (xhat) { p.out = xhat; p.ldout = ldxhat; }
    if (train) { p.sums2 = sums2; p.dgamma = unit; p.dbeta = unit + C; p.dbias = unit + 2L * C; p.gscale = 1.0f; }
    if (!r) r = ew_recon_loss(dtype, train ? 1 : 0, p, s);
    if (!r && train) {
        // backward half, as the recon-head block of the backward pass (immediate sum of the <G, W_eff> partials)
        GNParams q;
        q.B = B; q.T = T; q.C = C; q.G = G; q.Cg = C / G; q.gamma = gamma; q.beta = beta;
        q.y = y; q.ldy = ldy; q.sums = sums; q.sums2 = sums2; q.dout = x; q.lddout = ldx; q.loss_type = loss_type; q.gscale = gscale;
        q.out = dy; q.ldout = lddy; q.cdot = cdot; q.cbias = cbias; q.part = work;
        r = ew_recon_bwd_apply(dtype, q, s);
    }
    return ew_hook_done(r, "sgv_test_recon_loss", stream);
}
// The recon-tail hooks (recon_out.hip), each three steps.  Front: the checks on what they all take, the model's group rule
// G = min(8, max(1, C / 4)) and the GNParams of the recon head's map.  The tail's builder (recon_tails.h), the one the entry point calls.
// Back: a workspace [statistics | extra_floats for the pass], the statistics of y, the pass itself -- pass(dtype, p, extra, s) -> the
// launcher's code -- the sync and the free.
static int recon_hook_front(const char* me, int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                            const float* scale, const float* min, int B, int T, int C, GNParams& p) {
    if (dtype != SGV_DTYPE_F32 && dtype != SGV_DTYPE_BF16) return fail(SGV_ERR_ARG, "%s: dtype must be SGV_DTYPE_F32 or SGV_DTYPE_BF16", me);
    if (!y || !sums || !gamma || !beta || !scale || !min) return fail(SGV_ERR_ARG, "%s: null argument", me);
    if (B < 1 || T < 1 || C < 8 || C % 8) return fail(SGV_ERR_ARG, "%s: B, T >= 1 and C %% 8 == 0 required (B %d, T %d, C %d)", me, B, T, C);
    if (!ld_ok(ldy, C)) return fail(SGV_ERR_ARG, "%s: the row stride must be >= C and a multiple of 8", me);
    if ((uintptr_t)y & 15) return fail(SGV_ERR_ARG, "%s: misaligned pointer (y 16 bytes)", me);
    p.B = B; p.T = T; p.C = C; p.G = std::min(8, std::max(1, C / 4)); p.Cg = C / p.G; p.gamma = gamma; p.beta = beta;
    if (C % p.G) return fail(SGV_ERR_ARG, "%s: C = %d is not a multiple of its %d groups", me, C, p.G);
    p.y = y; p.ldy = ldy; p.sums = sums;
    return SGV_OK;
}
extern "C++" template <typename Pass>
static int recon_hook_run(const char* me, int dtype, GNParams& p, size_t extra_floats, void* stream, const Pass& pass) {
    const size_t stat_floats = align_up(ew_gn_part_floats(p.B, p.T, p.C), 4);
    float* work = nullptr;
    HIPCHK(hipMalloc((void**)&work, sizeof(float) * (stat_floats + extra_floats)));
    p.part = work;
    hipStream_t s = (hipStream_t)stream;
    int r = ew_gn_stats(dtype, p, s);
    if (!r) r = pass(dtype, p, work + stat_floats, s);
    const int rc = ew_hook_done(r, me, stream);
    hipFree(work);
    return rc;
}
int sgv_test_recon_physical(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                            const float* scale, const float* min, int layout, float* out, int B, int T, int C, void* stream) {
    const char* me = "sgv_test_recon_physical";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_field(me, "out", scale, min, layout, out, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_recon_summary(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                           const float* scale, const float* min, const sgv_summary_out* out, const int32_t* probes_host,
                           int n_probes, int B, int T, int C, void* stream) {
    const char* me = "sgv_test_recon_summary";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(summary_out_ok(me, "pointer", out));
    if (out->probes && (!probes_host || n_probes < 1)) return fail(SGV_ERR_ARG, "%s: probes asked for, but no probe nodes are given", me);
    if (!out->probes) n_probes = 0;
    if (n_probes > SGV_MAX_PROBES) return fail(SGV_ERR_ARG, "%s: %d probe nodes, at most %d", me, n_probes, SGV_MAX_PROBES);
    const int bad = first_bad_probe(probes_host, n_probes, C);
    if (bad >= 0) return fail(SGV_ERR_ARG, "%s: probe nodes[%d] = %d is outside [0, %d)", me, bad, (int)probes_host[bad], C);
    int* nodes = nullptr;
    if (n_probes) {
        HIPCHK(hipMalloc((void**)&nodes, sizeof(int32_t) * n_probes));
        if (hipMemcpy(nodes, probes_host, sizeof(int32_t) * n_probes, hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(nodes);
            return fail(SGV_ERR_HIP, "%s: the probe nodes could not be copied to the device", me);
        }
    }
    int rc = tail_summary(me, "pointer", scale, min, out, nodes, n_probes, tail);       // the outputs were checked above: fills the tail
    if (!rc) rc = recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
    hipFree(nodes);          // after the sync of recon_hook_run
    return rc;
}
int sgv_test_recon_score(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                         const float* scale, const float* min, const float* truth, const sgv_score_out* out, int B, int T, int C,
                         void* stream) {
    const char* me = "sgv_test_recon_score";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_score(me, "truth", scale, min, truth, out, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_recon_ensemble(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                            const float* scale, const float* min, long count_before, const sgv_ensemble_state* st, int B, int T,
                            int C, void* stream) {
    const char* me = "sgv_test_recon_ensemble";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_ensemble(me, "B", scale, min, count_before, st, B, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_recon_sobol(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                         const float* scale, const float* min, int n_params, long blocks_before, const sgv_sobol_state* st, int B,
                         int T, int C, void* stream) {
    const char* me = "sgv_test_recon_sobol";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_sobol(me, "B", scale, min, n_params, blocks_before, st, B, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_recon_distribution(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                                const float* scale, const float* min, long count_before, const sgv_distribution_state* st, int B,
                                int T, int C, void* stream) {
    const char* me = "sgv_test_recon_distribution";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_distribution(me, "B", scale, min, count_before, st, B, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_recon_regress(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                           const float* scale, const float* min, int n_cov, const float* weights, long count_before,
                           const sgv_regress_state* st, int B, int T, int C, void* stream) {
    const char* me = "sgv_test_recon_regress";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_regress(me, "B", scale, min, n_cov, weights, count_before, st, B, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_recon_project(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                           const float* scale, const float* min, const float* weights, int n_func, float* out, int B, int T, int C,
                           void* stream) {
    const char* me = "sgv_test_recon_project";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_project(me, scale, min, weights, n_func, out, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_recon_temporal(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                            const float* scale, const float* min, const float* weights, int n_func, float* out, int B, int T, int C,
                            void* stream) {
    const char* me = "sgv_test_recon_temporal";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_temporal(me, scale, min, weights, n_func, out, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_recon_gram(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta, const float* scale,
                        const float* min, const float* node_weights, const float* offset, float* out, int B, int T, int C, void* stream) {
    const char* me = "sgv_test_recon_gram";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_gram(me, scale, min, T, node_weights, offset, out, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_recon_exceedance(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                              const float* scale, const float* min, const float* levels, int n_level, int side, int32_t* stats,
                              float* excess, int B, int T, int C, void* stream) {
    const char* me = "sgv_test_recon_exceedance";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_exceedance(me, scale, min, T, levels, n_level, side, stats, excess, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_recon_cycles(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta, const float* scale,
                          const float* min, const float* gate, int exponent, const sgv_cycles_out* out, int B, int T, int C, void* stream) {
    const char* me = "sgv_test_recon_cycles";
    GNParams p; ReconTail tail;
    CHK(recon_hook_front(me, dtype, y, ldy, sums, gamma, beta, scale, min, B, T, C, p));
    CHK(tail_cycles(me, scale, min, T, gate, exponent, out, tail));
    return recon_hook_run(me, dtype, p, tail.work_floats(B, T, C), stream, tail.run);
}
int sgv_test_act(int dtype, int mode, const void* y, long ldy, const void* dout, long lddout, float rscale, void* out, long ldout,
                 float* dbias, float* cdot, const float* cbias, const float* yf32, long ldyf, float* work, size_t work_floats, int B,
                 int T, int C, void* stream) {
    CHK(gn_hook_shape("sgv_test_act", dtype, B, T, C, 1, work, work_floats));
    if (mode < 0 || mode > 2) return fail(SGV_ERR_ARG, "sgv_test_act: mode must be 0, 1 or 2");
    if (!y || !ld_ok(ldy, C)) return fail(SGV_ERR_ARG, "sgv_test_act: y missing or its row stride not >= C and a multiple of 8");
    if (mode != 2 && (!out || !ld_ok(ldout, C))) return fail(SGV_ERR_ARG, "sgv_test_act: modes 0 and 1 need out (row stride >= C, multiple of 8)");
    if (mode == 1 && (!dout || !ld_ok(lddout, C))) return fail(SGV_ERR_ARG, "sgv_test_act: mode 1 needs dout (row stride >= C, multiple of 8)");
    if (mode == 2 && cdot && (!yf32 || !ld_ok(ldyf, C))) return fail(SGV_ERR_ARG, "sgv_test_act: mode 2 with cdot needs yf32 (row stride >= C, multiple of 8)");
    GNParams p;
    p.B = B; p.T = T; p.C = C; p.G = 1; p.Cg = C;
    p.y = y; p.ldy = ldy; p.dout = dout; p.lddout = lddout; p.rscale = rscale; p.out = out; p.ldout = ldout;
    p.dbias = dbias; p.cdot = cdot; p.cbias = cbias; p.yf32 = mode == 2 && cdot ? yf32 : nullptr; p.ldyf = ldyf; p.part = work;
    return ew_hook_done(ew_act(dtype, mode, p, (hipStream_t)stream), "sgv_test_act", stream);
}
int sgv_test_latent(const float* last, const float* eps, float* z, double* kl, const float* dz, float* dlast, float coef, int B, int Z,
                    void* stream) {
    if (!last || !eps || B < 1 || Z < 1 || (long)B * Z > (1L << 24)) return fail(SGV_ERR_ARG, "sgv_test_latent: null argument or bad shape");
    if (!z != !kl || !dz != !dlast || (!z && !dz)) return fail(SGV_ERR_ARG, "sgv_test_latent: give z and kl (forward) and / or dz and dlast (backward)");
    int r = 0;
    if (z) r = ew_latent_fwd(last, eps, z, B, Z, kl, (hipStream_t)stream);
    if (!r && dz) r = ew_latent_bwd(last, eps, dz, dlast, B, Z, coef, (hipStream_t)stream);
    return ew_hook_done(r, "sgv_test_latent", stream);
}
int sgv_test_stage(int dtype, const float* pz, const float* qz, const float* eps, const void* dec_out, long ldd, void* zs_next,
                   long ldz, float* zmap, float std_scale, float inv_b, double* kl, double* kl_part, const void* dzs, long lddzs,
                   void* g_p, void* g_q, float coef, int M, int C, void* stream) {
    if (dtype != SGV_DTYPE_F32 && dtype != SGV_DTYPE_BF16) return fail(SGV_ERR_ARG, "sgv_test_stage: dtype must be SGV_DTYPE_F32 or SGV_DTYPE_BF16");
    if (!pz || !qz || !eps || M < 1 || C < 1) return fail(SGV_ERR_ARG, "sgv_test_stage: null argument or bad shape");
    if (!zs_next && !dzs) return fail(SGV_ERR_ARG, "sgv_test_stage: give zs_next (forward) and / or dzs (backward)");
    if (zs_next && (!dec_out || !kl || !kl_part || ldd < C || ldz < C)) return fail(SGV_ERR_ARG, "sgv_test_stage: forward needs dec_out, kl, kl_part and row strides >= C");
    if (dzs && (!g_p || !g_q || lddzs < C)) return fail(SGV_ERR_ARG, "sgv_test_stage: backward needs g_p, g_q and a row stride >= C");
    int r = 0;
    if (zs_next) r = ew_stage_fwd(dtype, pz, qz, eps, dec_out, ldd, zs_next, ldz, zmap, M, C, std_scale, kl, inv_b, kl_part, (hipStream_t)stream);
    if (!r && dzs) r = ew_stage_bwd(dtype, pz, qz, eps, dzs, lddzs, g_p, g_q, M, C, coef, (hipStream_t)stream);
    return ew_hook_done(r, "sgv_test_stage", stream);
}
int sgv_test_linear_head(int xdtype, const void* X, const float* W, const float* bias, const float* scale, float* Y, float* part,
                         size_t part_floats, const float* dY, const void* addend, void* dX, float* dW, float* db, int B, int K, int O,
                         void* stream) {
    if (xdtype != SGV_DTYPE_F32 && xdtype != SGV_DTYPE_BF16) return fail(SGV_ERR_ARG, "sgv_test_linear_head: xdtype must be SGV_DTYPE_F32 or SGV_DTYPE_BF16");
    if (!X || !W || B < 1 || O < 1 || K < 8 || K % 8) return fail(SGV_ERR_ARG, "sgv_test_linear_head: X, W, B, O >= 1 and K %% 8 == 0 required");
    if (!Y && !dY) return fail(SGV_ERR_ARG, "sgv_test_linear_head: give Y (forward) and / or dY (backward)");
    if (Y && (!part || part_floats < (size_t)128 * B * O)) return fail(SGV_ERR_ARG, "sgv_test_linear_head: forward needs a workspace of 128 * B * O floats");
    if (dY && ((!dX && !dW) || (addend && !dX) || (db && !dW))) return fail(SGV_ERR_ARG, "sgv_test_linear_head: backward needs dX or dW (addend goes with dX, db with dW)");
    int r = 0;
    if (Y) r = ew_linear_head_fwd(xdtype, X, W, bias, scale, Y, B, K, O, part, (hipStream_t)stream);
    if (!r && dY) r = ew_linear_head_bwd(xdtype, dY, X, W, scale, addend, dX, dW, db, B, K, O, (hipStream_t)stream);
    return ew_hook_done(r, "sgv_test_linear_head", stream);
}
int sgv_test_linear_expand(int dtype, const float* X, const float* W, const float* bias, const float* scale, void* Y, const void* dY,
                           float* dX, float* dW, float* db, int B, int K, int O, void* stream) {
    if (dtype != SGV_DTYPE_F32 && dtype != SGV_DTYPE_BF16) return fail(SGV_ERR_ARG, "sgv_test_linear_expand: dtype must be SGV_DTYPE_F32 or SGV_DTYPE_BF16");
    if (!X || !W || B < 1 || O < 1 || K < 1) return fail(SGV_ERR_ARG, "sgv_test_linear_expand: null argument or bad shape");
    if (!Y && !dY) return fail(SGV_ERR_ARG, "sgv_test_linear_expand: give Y (forward) and / or dY (backward)");
    if (Y && !bias) return fail(SGV_ERR_ARG, "sgv_test_linear_expand: forward needs bias");
    if (dY && (!dW || !db)) return fail(SGV_ERR_ARG, "sgv_test_linear_expand: backward needs dW and db");
    int r = 0;
    if (Y) r = ew_linear_expand_fwd(dtype, X, W, bias, scale, Y, B, K, O, (hipStream_t)stream);
    if (!r && dY) r = ew_linear_expand_bwd(dtype, dY, X, W, scale, dX, dW, db, B, K, O, (hipStream_t)stream);
    return ew_hook_done(r, "sgv_test_linear_expand", stream);
}

// ---- test hook for the multi-tensor optimizer / spectral-norm passes (optim.hip; tests/test_optim_kernels_gpu.py) ----
// Descriptor and work-item tables over caller-owned device buffers, built by the OptTables of sgv_ew.h like the engine's and the
// parameter-set object's; scratch (tmp_t, tmp_s, tpart, spart, the per-item partials) is the object's own and starts as NaN.
struct sgv_optset {
    int dt = 0;
    OptTables tab;                               // one group
    std::vector<int> tiled;                      // per AdamDesc
    float* tmp = nullptr;
    double* gnorm = nullptr;
};
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int optset_done(int r, const char* what, hipStream_t s) {
    const hipError_t se = hipStreamSynchronize(s);
    if (r) return fail(SGV_ERR_HIP, "%s: launch failed", what);
    if (se != hipSuccess) return fail(SGV_ERR_HIP, "%s failed: %s", what, hipGetErrorString(se));
    return SGV_OK;
}
static int optset_read(const double* dev, double* host, const char* what, hipStream_t s) {
    if (hipMemcpyAsync(host, dev, sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess) { hipStreamSynchronize(s); return fail(SGV_ERR_HIP, "%s: read-back failed", what); }
    return SGV_OK;
}
int sgv_test_optset_destroy(sgv_optset* os) {
    if (!os) return SGV_OK;
    if (os->tmp) hipFree(os->tmp);
    if (os->gnorm) hipFree(os->gnorm);
    os->tab.release();
    delete os;
    return SGV_OK;
}
int sgv_test_optset_create(int dtype, const sgv_optset_entry* entries, int n, sgv_optset** out) {
    const char* me = "sgv_test_optset_create";
    if (dtype != SGV_DTYPE_F32 && dtype != SGV_DTYPE_BF16) return fail(SGV_ERR_ARG, "%s: dtype must be SGV_DTYPE_F32 or SGV_DTYPE_BF16", me);
    if (!entries || n < 1 || !out) return fail(SGV_ERR_ARG, "%s: null argument or no entries", me);
    size_t n_tmp = 0;
    for (int i = 0; i < n; ++i) {
        const sgv_optset_entry& e = entries[i];
        if (!e.p || !e.g || !e.m || !e.v) return fail(SGV_ERR_ARG, "%s: entry %d needs p, g, m and v", me, i);
        if (!al16(e.p) || !al16(e.g) || !al16(e.m) || !al16(e.v)) return fail(SGV_ERR_ARG, "%s: entry %d: p, g, m and v must be 16-byte aligned", me, i);
        if (e.n < 4 || e.n % 4) return fail(SGV_ERR_ARG, "%s: entry %d: n = %ld is not a positive multiple of 4", me, i, e.n);
        if (e.rows < 0 || (e.rows == 0 && e.tiled)) return fail(SGV_ERR_ARG, "%s: entry %d: the tiled pass takes spectrally-normalised weights only (rows > 0)", me, i);
        if (e.rows == 0 && (e.wct || e.g_bf16)) return fail(SGV_ERR_ARG, "%s: entry %d: wct and g_bf16 go with a spectrally-normalised weight", me, i);
        if (e.wc && !al16(e.wc)) return fail(SGV_ERR_ARG, "%s: entry %d: wc must be 16-byte aligned", me, i);
        if (e.rows > 0) {
            if (e.taps < 1 || e.cols < 4 || e.cols % 4) return fail(SGV_ERR_ARG, "%s: entry %d: taps >= 1 and cols %% 4 == 0 required (taps %d, cols %d)", me, i, e.taps, e.cols);
            if ((long)e.taps * e.rows * e.cols != e.n) return fail(SGV_ERR_ARG, "%s: entry %d: taps * rows * cols = %ld but n = %ld", me, i, (long)e.taps * e.rows * e.cols, e.n);
            if (!e.u || !e.v_sn || !e.sigma || !e.dot || !al16(e.v_sn)) return fail(SGV_ERR_ARG, "%s: entry %d: a spectrally-normalised weight needs u, v_sn (16-byte aligned), sigma and dot", me, i);
            if (e.g_bf16 && ((uintptr_t)e.g_bf16 & 7)) return fail(SGV_ERR_ARG, "%s: entry %d: g_bf16 must be 8-byte aligned", me, i);
            n_tmp += sn_scratch_floats(e.taps, e.rows, e.cols);
        }
    }
    sgv_optset* os = new sgv_optset();
    os->dt = dtype;
    auto bad = [&](const char* what) { sgv_test_optset_destroy(os); return fail(SGV_ERR_HIP, "%s: %s failed", me, what); };
    auto nan_alloc = [&](void** dst, size_t bytes) {      // all-ones bytes are a NaN in float and in double
        return hipMalloc(dst, bytes ? bytes : 256) == hipSuccess && hipMemset(*dst, 0xFF, bytes ? bytes : 256) == hipSuccess;
    };
    if (!nan_alloc((void**)&os->tmp, n_tmp * sizeof(float))) return bad("scratch allocation");
    OptTables& t = os->tab;
    float* scratch = os->tmp;
    for (int i = 0; i < n; ++i) {
        const sgv_optset_entry& e = entries[i];
        AdamDesc a; memset(&a, 0, sizeof(a));
        a.p = e.p; a.g = e.g; a.m = e.m; a.v = e.v; a.n = e.n; a.sn = -1; a.rows = 1; a.cols = (int)e.n; a.taps = 1;
        a.wc = e.wc; a.wct = e.wct; a.glp = (const unsigned short*)e.g_bf16;
        if (e.rows > 0) {
            SNDesc d; memset(&d, 0, sizeof(d));
            d.W = e.p; d.u = e.u; d.v = e.v_sn; d.sigma = e.sigma; d.dot = e.dot; d.G = e.g;
            d.taps = e.taps; d.rows = e.rows; d.cols = e.cols; d.active = e.active ? 1 : 0;
            sn_scratch_carve(d, scratch);
            d.wc = sn_compute_copy(dtype == SGV_DTYPE_BF16, e.wc, e.cols);
            a.sn = t.add_sn(d, e.tiled != 0, !e.tiled);
            a.rows = e.rows; a.cols = e.cols; a.taps = e.taps;
        }
        const int id = t.add_adam(a, e.tiled != 0);
        os->tiled.push_back(e.tiled ? 1 : 0);
        if (e.wc || e.wct) t.add_copy(id);
    }
    t.finish();
    if (!t.upload(0xFF)) return bad("table upload");
    if (!nan_alloc((void**)&os->gnorm, sizeof(double))) return bad("workspace allocation");
    *out = os;
    return SGV_OK;
}
int sgv_test_optset_power_iteration(sgv_optset* os, int train, int reuse_tpart, void* stream) {
    if (!os) return fail(SGV_ERR_ARG, "sgv_test_optset_power_iteration: null object");
    const OptTables& t = os->tab;
    if (t.sn.empty()) return SGV_OK;
    hipStream_t s = (hipStream_t)stream;
    const bool reuse = train && reuse_tpart;         // run_sn with wtu_fresh: the tiled entries' tpart comes from the last AdamW pass
    const OptTables::List l1 = reuse ? OptTables::SN_UNF : OptTables::SN;
    const int r = opt_sn_power_iteration(t.sn_dev, t.dev[l1], t.n(l1), t.dev[OptTables::SN], t.n(OptTables::SN), t.dev[OptTables::TSUM], t.n(OptTables::TSUM),
                                         t.dev[OptTables::SSUM], t.n(OptTables::SSUM), (int)t.sn.size(), train, s);
    return optset_done(r, "sgv_test_optset_power_iteration", s);
}
int sgv_test_optset_grad_dot(sgv_optset* os, void* stream) {
    if (!os) return fail(SGV_ERR_ARG, "sgv_test_optset_grad_dot: null object");
    hipStream_t s = (hipStream_t)stream;
    const OptTables& t = os->tab;
    int r = opt_sn_grad_dot(t.sn_dev, t.dev[OptTables::DOT], t.n(OptTables::DOT), t.dot_part, s);
    if (!r && !t.fin.empty()) r = ew_fin_dots(t.fin.data(), (int)t.fin.size(), s);
    return optset_done(r, "sgv_test_optset_grad_dot", s);
}
int sgv_test_optset_grad_norm(sgv_optset* os, double* gnorm_sq_out, void* stream) {
    if (!os || !gnorm_sq_out) return fail(SGV_ERR_ARG, "sgv_test_optset_grad_norm: null argument");
    hipStream_t s = (hipStream_t)stream;
    const OptTables& t = os->tab;
    int r = opt_grad_norm(t.adam_dev, t.sn_dev, t.dev[OptTables::ADAM], t.n(OptTables::ADAM), t.gnorm_part, s);
    if (!r) r = ew_rowsum_d(t.gnorm_part, t.n(OptTables::ADAM), 1, os->gnorm, 1.0, s);
    if (!r) CHK(optset_read(os->gnorm, gnorm_sq_out, "sgv_test_optset_grad_norm", s));
    return optset_done(r, "sgv_test_optset_grad_norm", s);
}
int sgv_test_optset_adamw(sgv_optset* os, float lr, float wd, int step, const float* gscale_dev, int grad_source, const float* g_base,
                          const void* g_wire, size_t g_wire_elems, double* gnorm_sq_out, void* stream) {
    const char* me = "sgv_test_optset_adamw";
    if (!os) return fail(SGV_ERR_ARG, "%s: null object", me);
    if (step < 1 || lr < 0.f) return fail(SGV_ERR_ARG, "%s: step >= 1 and lr >= 0 required", me);
    if (grad_source < 0 || grad_source > 2) return fail(SGV_ERR_ARG, "%s: grad_source must be 0 (fp32), 1 (per-entry bf16 mirror) or 2 (bf16 wire copy)", me);
    if (grad_source == 2) {
        if (!g_base || !g_wire || ((uintptr_t)g_wire & 7)) return fail(SGV_ERR_ARG, "%s: the wire copy needs g_base and an 8-byte aligned g_wire", me);
        for (size_t i = 0; i < os->tab.adam.size(); ++i) {
            if (!os->tiled[i]) continue;
            const long off = os->tab.adam[i].g - g_base;
            if (off < 0 || off % 4 || (size_t)(off + os->tab.adam[i].n) > g_wire_elems)
                return fail(SGV_ERR_ARG, "%s: tiled entry %zu: its gradient must lie in [g_base, g_base + g_wire_elems) at a multiple of 4 elements", me, i);
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const AdamCoef c = adam_coef(step);
    const OptTables& t = os->tab;
    const int n_flat = t.n(OptTables::FLAT), n_tile = t.n(OptTables::TILE);
    int r = opt_adamw(t.adam_dev, t.sn_dev, t.dev[OptTables::FLAT], n_flat, lr, c.b1, c.b2, 1e-8f, wd, c.bc1, c.bc2s, t.gnorm_part, os->dt, s, gscale_dev);
    if (!r) r = opt_adamw_sn(t.adam_dev, t.sn_dev, t.dev[OptTables::TILE], n_tile, lr, c.b1, c.b2, 1e-8f, wd, c.bc1, c.bc2s, t.gnorm_part + n_flat, os->dt, s,
                             g_base, grad_source == 2 ? g_wire : nullptr, grad_source == 1 ? 1 : 0);
    if (!r && gnorm_sq_out) {
        r = ew_rowsum_d(t.gnorm_part, n_flat + n_tile, 1, os->gnorm, 1.0, s);
        if (!r) CHK(optset_read(os->gnorm, gnorm_sq_out, me, s));
    }
    return optset_done(r, me, s);
}
int sgv_test_optset_make_copies(sgv_optset* os, void* stream) {
    if (!os) return fail(SGV_ERR_ARG, "sgv_test_optset_make_copies: null object");
    hipStream_t s = (hipStream_t)stream;
    return optset_done(opt_make_copies(os->tab.adam_dev, os->tab.dev[OptTables::COPY], os->tab.n(OptTables::COPY), os->dt, s), "sgv_test_optset_make_copies", s);
}
}  // extern "C"
