// libsgvae engine: parameter/optimizer arenas, layer graph of the hierarchical VAE, forward /
// backward orchestration on one HIP stream, and the engine's part of the C ABI of include/sgvae.h.
// Beside it, sharing engine_internal.h: engine_build.hip (what runs once at creation), engine_optim.hip (gradient buckets, AdamW), engine_comm.hip (RCCL),
// engine_streams.hip (auxiliary streams), engine_input.hip, engine_ckpt.hip, engine_surrogate.hip (the surrogate entry points), test_hooks.hip.
//
// Graph restated from the reference (channels-last, weights [tap][Cout][Cin]):
//   VAE.forward modules/VAE_network.py:79-121 ; Encoder modules/encoder.py:96-167 ;
//   Decoder modules/decoder.py:84-223 ; blocks modules/common.py:78-162 ; losses modules/losses.py:8-48 ;
//   training step modules/train.py:139-168.
// The backward pass is written out by hand (the reference uses autograd).
#include "engine_internal.h"
#include "recon_tails.h"

// ---- error state of the library: one thread-local message, written through sgv_set_error by every translation unit ----
static thread_local char g_err[1024] = "";
int sgv_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char* sgv_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------
// timing helpers
// ------------------------------------------------------------------------------------------------
static int tag_id(sgv_engine* e, const std::string& name) {
    auto it = e->tag_ids.find(name);
    if (it != e->tag_ids.end()) return it->second;
    int id = (int)e->tag_names.size();
    e->tag_ids[name] = id; e->tag_names.push_back(name);
    return id;
}
// Times the MAIN kernel of a GEMM launch (split-K combine passes are excluded so the numbers line up with the
// rocprofv3 per-kernel averages in profiles/).
struct ScopedTimer {
    sgv_engine* e; TimerRec r; bool on; bool ended = false; std::string name;
    void end_now() { if (on && !ended) { hipEventRecord(r.b, e->stream); ended = true; } }
    // detail only: a fact the launch decided after the timer started (e.g. " out=bf16": the 256 x 256 kernel's bf16 epilogue)
    void retag(const char* suffix) { if (on && e->timing_detail) r.tag = tag_id(e, name + suffix); }
    // detail (sgv_kernel_time_reset(e, 2)): one tag per (class, layer, shape) instead of one per class
    ScopedTimer(sgv_engine* e_, const char* cls, const Layer* l, int M = 0, int N = 0, int K = 0, int taps = 0, int sk = 0)
        : e(e_), on(e_->timing) {
        if (!on) return;
        hipEventCreate(&r.a); hipEventCreate(&r.b);
        name = cls;
        if (e->timing_detail && l) {
            char buf[160];
            snprintf(buf, sizeof(buf), "|%s|M=%d N=%d K=%d taps=%d splitk=%d", l->prefix.c_str(), M, N, K, taps, sk);
            name += buf;
        }
        r.tag = tag_id(e, name);
        hipEventRecord(r.a, e->stream);
        // 128-row kernels: the launcher records the end event right after the main kernel; the 256x256 path (main kernel, its
        // split-K combine, the 128-row tail launch) is timed as a whole
        if (!strncmp(cls, "gemm_nt", 7) && strncmp(cls, "gemm_nt_t256", 12)) { gemm_nt_main_done_event(r.b); ended = true; }
    }
    ~ScopedTimer() { if (on) { end_now(); e->timers.push_back(r); } }
};
// total time and number of the recorded launches that carry `tag` (none carries a negative one)
static void tag_total(sgv_engine* e, int tag, float* total_ms, int* calls) {
    float tot = 0.f; int n = 0;
    for (auto& t : e->timers) if (t.tag == tag) { float ms = 0.f; hipEventElapsedTime(&ms, t.a, t.b); tot += ms; ++n; }
    if (total_ms) *total_ms = tot;
    if (calls) *calls = n;
}

// ------------------------------------------------------------------------------------------------
// op wrappers
// ------------------------------------------------------------------------------------------------
static const void* wc_ptr(sgv_engine* e, const Layer& l) {
    if (e->dt == SGV_DTYPE_BF16) return e->copies + l.wc * e->esz;
    return e->params + l.w;
}
static const void* wct_ptr(sgv_engine* e, const Layer& l) { return e->copies + l.wct * e->esz; }

// Y = conv(X) * (1/sigma) + bias
// want_stats: let the GEMM epilogue produce the GroupNorm (sum, sum of squares) of the output per (sample, group) when the
// planned kernel can (256x256 kernel: deterministic partials + finalize; 128x128 kernel: its fp64-atomic epilogue) --
// callers check conv_fwd_fuses_stats first and skip ew_gn_stats
static void conv_fwd_params(sgv_engine* e, const Layer& l, const Tensor& x, const Tensor& y, long M, GemmNT& p) {
    memset(&p, 0, sizeof(p));
    p.A = x.p; p.lda = x.ld;
    p.W = wc_ptr(e, l); p.ldw = l.cin; p.w_tap_stride = (long)l.cout * l.cin;
    p.C = y.p; p.ldc = y.ld; p.out_f32 = y.f32 ? 1 : 0;
    p.bias = e->params + l.b;
    p.scale = e->sn_sigma + 2 * l.sn + 1;
    p.M = (int)M; p.N = l.cout; p.K = l.cin; p.taps = l.k; p.pad = (l.k - 1) / 2; p.Tlen = e->T;
    p.partial = e->partial;
}
// 0: separate statistics pass; 1: 128x128 kernel epilogue (fp64 atomics); 2: 256x256 kernel (deterministic)
static int conv_fwd_stats_mode(sgv_engine* e, const Layer& l, const Tensor& x, const Tensor& y, long M, int Cg, int G) {
    if (y.f32 || e->dt != SGV_DTYPE_BF16) return 0;
    GemmNT q; conv_fwd_params(e, l, x, y, M, q);
    q.gn_Cg = Cg; q.gn_G = G;
    const GemmPlan pl = gemm_nt_plan(e->dt, q, e->partial_floats, 1);
    if (pl.kind == 1 && pl.fuse_stats && gemm_nt256_part_floats((int)M, l.cout, 1) <= e->gn_part_floats) return 2;
    if (pl.kind == 0 && !e->deterministic && gemm_nt_can_fuse_stats(e->dt, (int)M, l.cout, l.cin, l.k, e->T, Cg)) return 1;
    return 0;
}
static bool conv_fwd_fuses_stats(sgv_engine* e, const Layer& l, const Tensor& x, const Tensor& y, long M, int Cg, int G) {
    return conv_fwd_stats_mode(e, l, x, y, M, Cg, G) != 0;
}
// A planned 256 x 256 launch whose 128-row tail would follow it as a second launch (M = 3200: rows 3072..3199): when the main
// launch leaves CUs free -- 240 work items on 256 CUs, the K = 95 008 products -- the tail runs BESIDE it instead, on the lane
// stream, as one round of <= 16 items of the 128 x 512 tile shape (each workgroup of either launch needs a CU of its own, and
// 240 + 16 = 256, so both are resident whatever the order they are placed in).  The tail is addressed by shifted row pointers
// (GemmNT::trow0 keeps the tap windows of a multi-tap product on the absolute rows); gemm_nt_tail_split decides.
static int launch_nt(sgv_engine* e, const GemmNT& p, const GemmPlan& pl) {
    // not while a collective may be resident: the tail takes exactly the CUs the main launch leaves free, and a static item list that
    // finds fewer CUs than items runs a second round
    // (kernel-timing passes take it too: the timer brackets the launch group on the main stream, join included)
    if (e->use_lanes && e->lane2 && e->tail_fork && e->stream != e->lane2 && !e->coll_inflight) {
        const int sk_t = gemm_nt_tail_split(e->dt, p, pl, e->partial_floats);
        if (sk_t > 0) {
            HIPCHK(hipEventRecord(e->tail_fork, e->stream));
            HIPCHK(hipStreamWaitEvent(e->lane2, e->tail_fork, 0));
            int r = launch_gemm_nt_main(p, pl, e->stream);
            if (r) return r;
            r = launch_gemm_nt_tail(p, pl, sk_t, e->partial2, e->lane2);
            if (r) return r;
            HIPCHK(hipEventRecord(e->tail_join, e->lane2));
            HIPCHK(hipStreamWaitEvent(e->stream, e->tail_join, 0));
            return 0;
        }
    }
    return launch_gemm_nt_planned(e->dt, p, pl, e->stream);
}
static int conv_fwd(sgv_engine* e, const Layer& l, const Tensor& x, const Tensor& y, long M, double* gn_sums = nullptr, int gn_Cg = 0,
                    int gn_G = 0) {
    GemmNT p; conv_fwd_params(e, l, x, y, M, p);
    const int smode = gn_sums ? conv_fwd_stats_mode(e, l, x, y, M, gn_Cg, gn_G) : 0;
    if (gn_sums && !smode) return fail(SGV_ERR_STATE, "conv_fwd: statistics requested from a GEMM that cannot produce them (%s)", l.prefix.c_str());
    p.gn_Cg = gn_Cg; p.gn_G = gn_G;
    GemmPlan pl = gemm_nt_plan(e->dt, p, e->partial_floats, smode == 2);
    if (smode == 2) { p.gn_sums = gn_sums; p.gn_part = e->gn_part; }
    else if (smode == 1) { p.gn_sums = gn_sums; }
    ScopedTimer tm(e, pl.kind ? "gemm_nt_t256" : gemm_nt_uses_wide(e->dt, p.N, p.K, p.taps) ? "gemm_nt_wide" : "gemm_nt", &l, p.M, p.N, p.K, p.taps, pl.sk_main);
    int r = launch_nt(e, p, pl);
    if (r) return fail(SGV_ERR_ARG, "gemm_nt launch failed for %s (M=%d N=%d K=%d, kind %d)", l.prefix.c_str(), p.M, p.N, p.K, pl.kind);
    return 0;
}
// dX = conv^T(dY) * (1/sigma) (+ addend)
static int conv_bwd_dx(sgv_engine* e, const Layer& l, const Tensor& dy, const Tensor& dx, const Tensor* addend, long M) {
    GemmNT p; memset(&p, 0, sizeof(p));
    p.A = dy.p; p.lda = dy.ld;
    p.W = wct_ptr(e, l); p.ldw = l.cout; p.w_tap_stride = (long)l.cout * l.cin;
    p.C = dx.p; p.ldc = dx.ld; p.out_f32 = 0;
    if (addend) { p.addend = addend->p; p.ldadd = addend->ld; }
    p.scale = e->sn_sigma + 2 * l.sn + 1;
    p.M = (int)M; p.N = l.cin; p.K = l.cout; p.taps = l.k; p.pad = (l.k - 1) / 2; p.Tlen = e->T;
    p.partial = e->partial;
    const GemmPlan pl = gemm_nt_plan(e->dt, p, e->partial_floats, 0);
    ScopedTimer tm(e, pl.kind ? "gemm_nt_t256" : gemm_nt_uses_wide(e->dt, p.N, p.K, p.taps) ? "gemm_nt_wide" : "gemm_nt", &l, p.M, p.N, p.K, p.taps, pl.sk_main);
    int r = launch_nt(e, p, pl);
    if (r) return fail(SGV_ERR_ARG, "gemm_nt(dX) launch failed for %s", l.prefix.c_str());
    return 0;
}
__global__ void sum_slabs_kernel(float* out, const float* partial, int splitk, long n) {
    if ((n & 3) == 0 && ((((uintptr_t)out) | ((uintptr_t)partial)) & 15) == 0) {      // 16-byte path (every conv weight)
        const long n4 = n >> 2;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            float4 v = reinterpret_cast<const float4*>(partial)[i];
            for (int z = 1; z < splitk; ++z) {
                const float4 w = reinterpret_cast<const float4*>(partial + (long)z * n)[i];
                v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
            }
            reinterpret_cast<float4*>(out)[i] = v;
        }
        return;
    }
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float v = 0.f;
        for (int z = 0; z < splitk; ++z) v += partial[(long)z * n + i];
        out[i] = v;
    }
}
// its one launcher (the weight-gradient path below, sgv_test_gemm_tn): four elements per thread (grid-stride either way)
void sum_slabs(float* out, const float* partial, int splitk, long n, hipStream_t stream) {
    int blocks = (int)((n / 4 + 255) / 256); if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sum_slabs_kernel, dim3(blocks), dim3(256), 0, stream, out, partial, splitk, n);
}
// dW[tap][co][ci] = sum_m dY[m][co] X[m+tap-pad][ci]
static int conv_bwd_dw(sgv_engine* e, const Layer& l, const Tensor& dy, const Tensor& x, long M) {
    GemmTN p; memset(&p, 0, sizeof(p));
    p.A = dy.p; p.lda = dy.ld; p.B = x.p; p.ldb = x.ld;
    p.M = (int)M; p.N1 = l.cout; p.N2 = l.cin; p.taps = l.k; p.pad = (l.k - 1) / 2; p.Tlen = e->T;
    p.use_tr = e->use_tr;
    p.ldo = l.cin; p.out_tap_stride = (long)l.cout * l.cin;
    int sk = e->use_tr ? gemm_tn_pick_splitk(p.M, p.N1, p.N2, p.taps, e->dt, e->T) : gemm_tn_pick_splitk(p.M, p.N1, p.N2, p.taps, e->dt);
    const long nw = l.nw();
    if ((size_t)sk * nw > e->partial_tn_floats) sk = 1;
    float* G = e->grads + l.gw;
    // side stream: dY and X are final once the kernels enqueued so far on the main stream have run; nothing on the
    // main stream reads G before join_side().  (Kernel-timing passes keep everything on one stream.)
    // only the small launches go to the side stream: big GEMMs fill every CU on their own and co-running them costs L2
    const bool side = e->use_side && !e->timing && 2.0e-9 * p.M * p.N1 * p.N2 * p.taps <= DW_SIDE_MAX_GF;
    hipStream_t st = e->stream;
    float* slabs = e->partial;
    if (side) {
        CHK(stream_wait(e, e->side, e->stream));
        st = e->side; slabs = e->partial_tn; e->side_dirty = true;
    } else if ((size_t)sk * nw > e->partial_floats) sk = 1;
    if (e->dw_chunks > 1 && (int)(&l - e->layers.data()) == e->dw_chunk_layer && sk == 1 && !side && l.k == 1 && l.cout % (128 * e->dw_chunks) == 0) {
        const int rows = l.cout / e->dw_chunks;
        GemmTN q0 = p; q0.splitk = 1; q0.N1 = rows;
        q0.out = reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(e->grads_lp) + l.gw); q0.out_bf16 = 1;
        const bool direct = l.lp && wire_lp_active(e) && gemm_tn_uses_t256(e->dt, q0) && gemm_tn256_accepts(q0);     // the chunks' wire copy straight from the GEMM
        e->dw_chunk_direct = direct;
        e->lp_dirty[(int)(&l - e->layers.data())] = direct ? 1 : 0;
        for (int c = 0; c < e->dw_chunks; ++c) {
            GemmTN q = p;
            q.splitk = 1; q.N1 = rows;
            q.A = (const char*)dy.p + (size_t)c * rows * e->esz;
            q.out = G + (size_t)c * rows * l.cin;
            if (direct) { q.out = reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(e->grads_lp) + l.gw + (size_t)c * rows * l.cin); q.out_bf16 = 1; }
            if (e->coll_inflight && e->tn_sched) q.sched = e->tn_sched + 520 * (e->tn_sched_next++ & 7);
            if (launch_gemm_tn(e->dt, q, st)) return fail(SGV_ERR_ARG, "gemm_tn launch failed for %s (rows %d..%d)", l.prefix.c_str(), c * rows, (c + 1) * rows);
            if (e->release && e->release->after_chunk(c, e->dw_chunks, c * rows, (c + 1) * rows)) return fail(SGV_ERR_HIP, "weight-gradient chunk exchange failed for %s", l.prefix.c_str());
        }
        return 0;
    }
    ScopedTimer tm(e, "gemm_tn", &l, p.M, p.N1, p.N2, p.taps, sk);
    const int li_ = (int)(&l - e->layers.data());
    if (sk == 1) {
        p.splitk = 1; p.out = G;
        // grad_bf16: the 256 x 256 kernel rounds its accumulators to bf16 on the way out; the AdamW pass reads them there
        // a resident collective may keep some of the persistent kernel's workgroups off the chip: the work-stealing form (gemm256tn.hip)
        if (e->coll_inflight && e->tn_sched) p.sched = e->tn_sched + 520 * (e->tn_sched_next++ & 7);
        const bool opt_lp = l.lp && grad_lp_active(e), wire_lp = l.lp && !opt_lp && wire_lp_active(e);
        GemmTN plp = p;
        plp.out = reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(e->grads_lp) + l.gw); plp.out_bf16 = 1;
        const bool lp = (opt_lp || wire_lp) && gemm_tn_uses_t256(e->dt, plp) && gemm_tn256_accepts(plp);
        if (lp) { p = plp; tm.retag(" out=bf16"); }
        if (launch_gemm_tn(e->dt, p, st)) return fail(SGV_ERR_ARG, "gemm_tn launch failed for %s", l.prefix.c_str());
        // a smaller batch than the one the layer was classified at took another kernel: the optimizer still reads the mirror, so the
        // fp32 result goes there in a pass (the wire copy gets it with the rest of the bucket: pack_bucket)
        if (opt_lp && !lp) ew_pack_bf16(G, (char*)e->grads_lp + 2 * l.gw, nw, st);
        e->lp_dirty[li_] = lp ? 1 : 0;
    } else {
        // split-K over the batch*time rows: each slice writes its own fp32 slab (plain stores), then one sum pass
        p.splitk = sk; p.out = slabs; p.out_slab_stride = nw;
        if (launch_gemm_tn(e->dt, p, st)) return fail(SGV_ERR_ARG, "gemm_tn launch failed for %s", l.prefix.c_str());
        tm.end_now();
        sum_slabs(G, slabs, sk, nw, st);
        if (l.lp && grad_lp_active(e)) ew_pack_bf16(G, (char*)e->grads_lp + 2 * l.gw, nw, st);
        e->lp_dirty[li_] = 0;
    }
    return 0;
}

static GNParams gn_base(sgv_engine* e, const GNLayer& g, int B) {
    GNParams p;
    p.gamma = e->params + g.gamma; p.beta = e->params + g.beta;
    p.B = B; p.T = e->T; p.C = g.C; p.G = g.G; p.Cg = g.C / g.G;
    return p;
}

// Scope that runs the calls it encloses on the second compute lane (stream + split-K / reduction workspaces swapped in); the lane
// first waits for everything enqueued on the main stream so far.  lane2_join() makes the main stream wait for the lane.
struct Lane2 {
    sgv_engine* e; hipStream_t s0; float* p0; float* c0; float* g0; bool on;
    explicit Lane2(sgv_engine* e_) : e(e_), s0(e_->stream), p0(e_->partial), c0(e_->colpart), g0(e_->gn_part) {
        on = e->use_lanes && e->lane2 && !e->timing;
        if (!on) return;
        hipEventRecord(e->lane_fork, e->stream);
        hipStreamWaitEvent(e->lane2, e->lane_fork, 0);
        e->stream = e->lane2; e->partial = e->partial2; e->colpart = e->colpart2; e->gn_part = e->gn_part2;
    }
    ~Lane2() {
        if (!on) return;
        hipEventRecord(e->lane_join, e->lane2);
        e->stream = s0; e->partial = p0; e->colpart = c0; e->gn_part = g0;
    }
};
static void lane2_join(sgv_engine* e) {
    if (e->use_lanes && e->lane2 && !e->timing) hipStreamWaitEvent(e->stream, e->lane_join, 0);
}

static int block_fwd(sgv_engine* e, Block& b, const Tensor& in, int B) {
    const long M = (long)B * e->T;
    Tensor x = in;
    for (size_t s = 0; s < b.st.size(); ++s) {
        Stage& S = b.st[s];
        const Layer& L = e->layers[S.layer];
        Tensor cin = x;
        if (S.pre_gelu) {
            GNParams p; p.y = x.p; p.ldy = x.ld; p.out = S.pre.p; p.ldout = S.pre.ld; p.B = B; p.T = e->T; p.C = x.C;
            ew_act(e->dt, 0, p, e->stream);
            cin = S.pre;
        }
        if (S.gn >= 0 && S.act == 1 && e->use_convgn && e->dt == SGV_DTYPE_BF16 && !S.y.f32 && (long)L.cin * L.k <= CONVGN_MAXK) {
            // one workgroup per (group, sample): convolution, statistics, normalise + GELU (+ residual) in one launch
            const GNLayer& g = e->gns[S.gn];
            ConvGN q; memset(&q, 0, sizeof(q));
            q.A = cin.p; q.lda = cin.ld; q.W = wc_ptr(e, L); q.ldw = L.cin; q.w_tap_stride = (long)L.cout * L.cin;
            q.bias = e->params + L.b; q.scale = e->sn_sigma + 2 * L.sn + 1;
            q.y = S.y.p; q.ldy = S.y.ld; q.out = S.a.p; q.ldout = S.a.ld;
            if (b.residual && s + 1 == b.st.size()) { q.res = in.p; q.ldres = in.ld; q.rscale = 0.1f; } else q.rscale = 1.f;
            q.gamma = e->params + g.gamma; q.beta = e->params + g.beta; q.sums = e->stats + S.sums;
            q.B = B; q.T = e->T; q.N = L.cout; q.K = L.cin; q.taps = L.k; q.pad = (L.k - 1) / 2; q.G = g.G; q.Cg = g.C / g.G;
            if (g.C == L.cout && conv_gn_fused_eligible(e->dt, q)) {
                ScopedTimer tm(e, "conv_gn", &L, (int)M, L.cout, L.cin, L.k, 1);
                if (launch_conv_gn_fwd(q, e->stream)) return fail(SGV_ERR_ARG, "conv_gn launch failed for %s", L.prefix.c_str());
                x = S.a;
                continue;
            }
        }
        CHK(conv_fwd(e, L, cin, S.y, M));
        if (S.gn >= 0) {
            const GNLayer& g = e->gns[S.gn];
            GNParams p = gn_base(e, g, B);
            p.y = S.y.p; p.ldy = S.y.ld; p.sums = e->stats + S.sums; p.part = e->colpart;
            p.out = S.a.p; p.ldout = S.a.ld;
            if (b.residual && s + 1 == b.st.size()) { p.res = in.p; p.ldres = in.ld; p.rscale = 0.1f; }
            ew_gn_fwd(e->dt, S.act, p, e->stream);
        } else if (S.act) {
            GNParams p; p.y = S.y.p; p.ldy = S.y.ld; p.out = S.a.p; p.ldout = S.a.ld; p.B = B; p.T = e->T; p.C = L.cout;
            ew_act(e->dt, 0, p, e->stream);
        }
        x = S.a;
    }
    return 0;
}

// dOut: gradient wrt the block output; dIn (nullable): gradient wrt the block input (overwritten).
// before_first_dw (optional): its release_small() runs after the last dY of the block exists, right before the weight-gradient GEMM of
// the block's first conv (sgv_backward uses it to release the small-gradient bucket early).
// Input gradient of convolution L (its dY given) + GroupNorm / GELU backward of stage P below it in one launch (convgn.hip);
// `addend` (residual path) is added to the input gradient before it is rounded; `premul` = x when L reads GELU(x) (the gradient
// is multiplied by gelu'(x)); rscale = the residual scale of P's block when P is its last stage.  Returns 1 when the fused kernel ran (P.dy,
// the group sums, the per-sample column totals and the <G, W_eff> partials of P's layer are written and their fixed-order sums
// queued), 0 when the shapes are not taken, < 0 on error.
static int fused_dx_gn_bwd(sgv_engine* e, const Layer& L, const Tensor& dY, const Tensor* addend, Stage& P, int B, long M,
                           const Tensor* premul = nullptr, float rscale = 1.f, const Tensor* da_out = nullptr) {
    if (!e->use_convgn || e->dt != SGV_DTYPE_BF16 || !L.need_wct || (long)L.cout * L.k > CONVGN_MAXK) return 0;
    if (P.gn < 0 || P.act != 1 || P.y.f32) return 0;
    const Layer& LP = e->layers[P.layer];
    const GNLayer& g = e->gns[P.gn];
    ConvGNBwd q; memset(&q, 0, sizeof(q));
    q.A = dY.p; q.lda = dY.ld; q.W = wct_ptr(e, L); q.ldw = L.cout; q.w_tap_stride = (long)L.cin * L.cout;
    q.scale = e->sn_sigma + 2 * L.sn + 1;
    if (addend) { q.addend = addend->p; q.ldadd = addend->ld; }
    if (premul) { q.premul = premul->p; q.ldpre = premul->ld; }
    if (da_out) { q.da = da_out->p; q.ldda = da_out->ld; }
    q.y = P.y.p; q.ldy = P.y.ld; q.sums = e->stats + P.sums; q.gamma = e->params + g.gamma; q.beta = e->params + g.beta;
    q.cbias = e->params + LP.b; q.dy = P.dy.p; q.lddy = P.dy.ld; q.sums2 = e->stats + P.sums2; q.ptot = e->red + g.ptot;
    q.cdot_part = e->red + LP.dot_part; q.rscale = rscale; q.gscale = 1.f;
    q.B = B; q.T = e->T; q.N = L.cin; q.K = L.cout; q.taps = L.k; q.pad = (L.k - 1) / 2; q.G = g.G; q.Cg = g.C / g.G;
    if (g.C != L.cin || LP.cout != L.cin || !conv_gn_bwd_eligible(e->dt, q)) return 0;
    ScopedTimer tm(e, "conv_gn_bwd", &L, (int)M, L.cin, L.cout, L.k, 1);
    if (launch_conv_gn_bwd(q, e->stream)) return fail(SGV_ERR_ARG, "conv_gn_bwd launch failed for %s", L.prefix.c_str());
    int* cntp = &e->dot_counts[e->fin_dots.size() % 512];
    *cntp = g.G * B;
    e->fin_dots.push_back({q.cdot_part, e->grads + LP.gdot, *cntp, 0});
    e->fin_affine.push_back({q.ptot, e->grads + g.gbeta, e->grads + g.ggamma, e->grads + LP.gb, g.C, B, 0, 0});
    return 1;
}

// below / below_done (optional): the last stage of the block that consumes dIn as its incoming gradient; when the fused kernel
// can take (this block's first convolution, that stage) together, it writes dIn AND that stage's dY, *below_done is set and the
// caller passes last_dy_ready = true to that block's block_bwd (below_rscale: that block's residual scale).
static int block_bwd(sgv_engine* e, Block& b, const Tensor& in, const Tensor& dOut, const Tensor* dIn, int B,
                     GradRelease* before_first_dw = nullptr, Stage* below = nullptr, bool* below_done = nullptr,
                     bool last_dy_ready = false, float below_rscale = 1.f) {
    const long M = (long)B * e->T;
    Tensor dA = dOut;
    float sc = b.residual ? 0.1f : 1.0f;
    bool dy_ready = last_dy_ready;  // the stage's dY was produced by the fused kernel launched from the stage above
    for (int s = (int)b.st.size() - 1; s >= 0; --s) {
        Stage& S = b.st[s];
        const Layer& L = e->layers[S.layer];
        const Tensor x_raw = (s == 0) ? in : b.st[s - 1].a;
        const Tensor x_conv = S.pre_gelu ? S.pre : x_raw;
        Tensor dY;
        // <G,W_eff> and the GroupNorm affine / bias gradients leave these kernels as block / per-sample partials in e->red; the
        // fixed-order sums run once per bucket (GradRelease::flush_fin)
        int* cnt = &e->dot_counts[e->fin_dots.size() % 512];
        if (e->recompute_act && S.gn >= 0 && !S.y.f32) {
            // regenerate this stage's output map exactly as block_fwd's unfused path writes it (the fused forward kernel normalises the
            // same stored values): the map is read below as the next stage's convolution input (weight gradient) and by the
            // residual adds; a recompute build would not have kept it
            const GNLayer& g = e->gns[S.gn];
            GNParams p = gn_base(e, g, B);
            p.y = S.y.p; p.ldy = S.y.ld; p.sums = e->stats + S.sums; p.part = e->colpart;
            p.out = S.a.p; p.ldout = S.a.ld;
            if (b.residual && s + 1 == (int)b.st.size()) { p.res = in.p; p.ldres = in.ld; p.rscale = 0.1f; }
            if (ew_gn_apply(e->dt, S.act, p, e->stream)) return fail(SGV_ERR_HIP, "activation recompute launch failed (%s)", L.prefix.c_str());
            e->recompute_bytes += (size_t)M * g.C * e->esz;
        }
        if (dy_ready) {
            dY = S.dy;
            dy_ready = false;
        } else if (S.gn >= 0) {
            const GNLayer& g = e->gns[S.gn];
            GNParams p = gn_base(e, g, B);
            p.y = S.y.p; p.ldy = S.y.ld; p.sums = e->stats + S.sums; p.sums2 = e->stats + S.sums2;
            p.dout = dA.p; p.lddout = dA.ld; p.rscale = sc;
            p.part = e->colpart;
            p.ptot = e->red + g.ptot;
            p.out = S.dy.p; p.ldout = S.dy.ld;
            p.cdot = e->grads + L.gdot; p.cbias = e->params + L.b;   // <G,W_eff> = sum dY*(y - bias)
            p.cdot_part = e->red + L.dot_part; p.cdot_blocks = cnt;
            if (ew_gn_bwd(e->dt, 1, p, e->stream)) return fail(SGV_ERR_STATE, "GroupNorm backward launch failed (%s)", L.prefix.c_str());           // sums2, dY (GELU), partials
            e->fin_dots.push_back({p.cdot_part, p.cdot, *cnt, 0});
            e->fin_affine.push_back({p.ptot, e->grads + g.gbeta, e->grads + g.ggamma, e->grads + L.gb, g.C, B, 0, 0});
            dY = S.dy;
        } else if (S.act) {
            GNParams p; p.y = S.y.p; p.ldy = S.y.ld; p.dout = dA.p; p.lddout = dA.ld; p.rscale = sc;
            p.out = S.dy.p; p.ldout = S.dy.ld; p.dbias = e->grads + L.gb; p.part = e->colpart; p.B = B; p.T = e->T; p.C = L.cout;
            p.cdot = e->grads + L.gdot; p.cbias = e->params + L.b;
            p.cdot_part = e->red + L.dot_part; p.cdot_blocks = cnt;
            if (L.col_part != NPOS) { p.part = e->red + L.col_part; p.defer_colsum = 1; }     // bias gradient: summed with the small bucket's other sums
            ew_act(e->dt, 1, p, e->stream);
            if (L.col_part != NPOS) e->fin_affine.push_back({p.part, p.dbias, nullptr, nullptr, L.cout, ew_act_part_rows(B, e->T, L.cout), 0, 1});
            e->fin_dots.push_back({p.cdot_part, p.cdot, *cnt, 0});
            dY = S.dy;
        } else {
            GNParams p; p.y = dA.p; p.ldy = dA.ld; p.dbias = e->grads + L.gb; p.part = e->colpart; p.B = B; p.T = e->T; p.C = L.cout;
            if (!S.y.f32) return fail(SGV_ERR_STATE, "conv without norm/activation must have an fp32 output (%s)", L.prefix.c_str());
            p.cdot = e->grads + L.gdot; p.cbias = e->params + L.b; p.yf32 = (const float*)S.y.p; p.ldyf = S.y.ld;
            p.cdot_part = e->red + L.dot_part; p.cdot_blocks = cnt;
            if (L.col_part != NPOS) { p.part = e->red + L.col_part; p.defer_colsum = 1; }
            ew_act(e->dt, 2, p, e->stream);
            if (L.col_part != NPOS) e->fin_affine.push_back({p.part, p.dbias, nullptr, nullptr, L.cout, ew_act_part_rows(B, e->T, L.cout), 0, 1});
            e->fin_dots.push_back({p.cdot_part, p.cdot, *cnt, 0});
            dY = dA;
        }
        sc = 1.0f;
        if (s == 0 && before_first_dw) before_first_dw->release_small();
        CHK(conv_bwd_dw(e, L, dY, x_conv, M));
        const bool need = (s > 0) || (dIn != nullptr);
        if (need && (s > 0 ? !S.pre_gelu : (below && below_done))) {
            Stage& P = s > 0 ? b.st[s - 1] : *below;
            const Tensor* add = (s == 0 && b.residual) ? &dOut : nullptr;
            // across blocks the input gradient itself is stored too (dIn): a residual block below adds it to its own input gradient
            const int fr = fused_dx_gn_bwd(e, L, dY, add, P, B, M, S.pre_gelu ? &x_raw : nullptr, s > 0 ? 1.f : below_rscale, s > 0 ? nullptr : dIn);
            if (fr < 0) return fr;
            if (fr > 0) {
                if (s > 0) { dy_ready = true; dA = P.da; }
                else *below_done = true;
                continue;
            }
        }
        if (need) {
            const Tensor target = (s > 0) ? b.st[s - 1].da : *dIn;
            if (S.pre_gelu) {
                CHK(conv_bwd_dx(e, L, dY, S.dpre, nullptr, M));
                GNParams p; p.y = x_raw.p; p.ldy = x_raw.ld; p.dout = S.dpre.p; p.lddout = S.dpre.ld; p.rscale = 1.f;
                p.out = target.p; p.ldout = target.ld; p.B = B; p.T = e->T; p.C = x_raw.C;
                ew_act(e->dt, 1, p, e->stream);
            } else {
                const Tensor* add = (s == 0 && b.residual) ? &dOut : nullptr;
                CHK(conv_bwd_dx(e, L, dY, target, add, M));
            }
            dA = target;
        }
    }
    return 0;
}

// the environment's switches (A/B runs and tests), read once per engine, in front of everything sgv_create builds
static void env_switches(sgv_engine* e) {
    if (const char* v = getenv("SGV_DDP_EARLY")) e->ddp_early = atoi(v);
    if (const char* v = getenv("SGV_DDP_LAST_CHUNKS")) e->ddp_last_chunks = atoi(v);
    if (const char* v = getenv("SGV_DDP_CHUNK_MIN_GF")) e->ddp_chunk_min_gf = atof(v);
    if (const char* v = getenv("SGV_LANES")) e->use_lanes = atoi(v);
    if (const char* v = getenv("SGV_CONVGN")) e->use_convgn = atoi(v);
    if (const char* v = getenv("SGV_DW_SIDE")) e->use_side = atoi(v) != 0;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int sgv_create(const sgv_config* cfg, void* hip_stream, sgv_engine** out) {
    if (!cfg || !out) return fail(SGV_ERR_ARG, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(SGV_ERR_NOGPU, "no HIP device visible: libsgvae has no CPU fallback");
    if (cfg->n_levels < 2 || cfg->n_levels > SGV_MAX_LEVELS) return fail(SGV_ERR_ARG, "n_levels must be in [2,%d]", SGV_MAX_LEVELS);
    if (cfg->n_levels - 1 + 2 > SGV_MAX_SCALARS) return fail(SGV_ERR_ARG, "too many levels");
    if (cfg->compute_dtype != SGV_DTYPE_F32 && cfg->compute_dtype != SGV_DTYPE_BF16) return fail(SGV_ERR_ARG, "bad compute_dtype");
    if (cfg->num_node % 8 || cfg->latent_dim % 8 || cfg->hierarchical_dim % 8)
        return fail(SGV_ERR_ARG, "num_node, latent_dim and hierarchical_dim must be multiples of 8 (16-byte channel vectors)");
    for (int i = 0; i < cfg->n_levels; ++i)
        if (cfg->num_filter_enc[i] % 8 || cfg->num_filter_enc[i] <= 0) return fail(SGV_ERR_ARG, "num_filter_enc[%d]=%d must be a positive multiple of 8", i, cfg->num_filter_enc[i]);
    if (cfg->max_batch < 1 || cfg->num_time < 1) return fail(SGV_ERR_ARG, "bad batch/time");
    if (cfg->loss_type < 0 || cfg->loss_type > 3) return fail(SGV_ERR_ARG, "bad loss_type");
    sgv_engine* e = new sgv_engine();
    env_switches(e);
    e->cfg = *cfg;
    e->stream = (hipStream_t)hip_stream;
    e->dt = cfg->compute_dtype; e->esz = e->dt == SGV_DTYPE_BF16 ? 2 : 4;
    e->n = cfg->n_levels; e->n_st = e->n - 1; e->T = cfg->num_time; e->N = cfg->num_node;
    e->Z = cfg->latent_dim; e->H = cfg->hierarchical_dim; e->maxB = cfg->max_batch;
    e->use_tr = (cfg->flags & 1) ? 0 : 1;
    for (int i = 0; i < e->n; ++i) e->enc.push_back(cfg->num_filter_enc[i]);
    e->dec.assign(e->enc.rbegin(), e->enc.rend());
    int r;
    if ((r = build_layout(e))) { delete e; return r; }
    // workspace for split-K slabs: enough for the largest split GEMM
    const long M = (long)e->maxB * e->T;
    size_t pf = 0, pf_tn = 0;
    for (auto& l : e->layers) {
        if (!l.used || l.op == OP_LINEAR) continue;
        int sk = gemm_nt_pick_splitk((int)M, l.cout, l.cin, l.k, e->dt);
        if (sk > 1) pf = std::max(pf, (size_t)sk * M * l.cout);
        sk = gemm_nt_pick_splitk((int)M, l.cin, l.cout, l.k, e->dt);
        if (sk > 1 && l.need_wct) pf = std::max(pf, (size_t)sk * M * l.cin);
        sk = std::max(gemm_tn_pick_splitk((int)M, l.cout, l.cin, l.k, e->dt, e->T), gemm_tn_pick_splitk((int)M, l.cout, l.cin, l.k, e->dt));
        if (sk > 1) pf_tn = std::max(pf_tn, (size_t)sk * l.nw());
    }
    if (pf < ((size_t)32 << 20)) pf = (size_t)32 << 20;   // batch < max_batch can pick deeper splits
    if (pf_tn < ((size_t)32 << 20)) pf_tn = (size_t)32 << 20;
    e->partial_floats = pf;
    e->partial_tn_floats = pf_tn;
    e->colpart_floats = 0;
    for (auto& g : e->gns) e->colpart_floats = std::max(e->colpart_floats, ew_gn_part_floats(e->maxB, e->T, g.C));
    for (auto& l : e->layers) if (l.op != OP_LINEAR) e->colpart_floats = std::max(e->colpart_floats, ew_gn_part_floats(e->maxB, e->T, l.cout));
    e->colpart_floats = std::max(e->colpart_floats, ew_recon_summary_work_floats(e->maxB, e->T, e->N));   // sgv_summarize's frame partials (smaller up to T of several hundred)
    e->colpart_floats = std::max(e->colpart_floats, ew_recon_project_work_floats(e->maxB, e->T, e->N, SGV_MAX_FUNCTIONALS));   // sgv_project's partials at 32 rows
    e->colpart_floats = std::max(e->colpart_floats, ew_recon_temporal_work_floats(e->T));   // sgv_temporal's transposed weights [T_pad][32]
    if (e->T <= SGV_MAX_GRAM_T) e->colpart_floats = std::max(e->colpart_floats, ew_recon_gram_work_floats(e->maxB, e->T, e->N));   // sgv_gram's per-block tile partials
    e->xpose_floats = (size_t)M * std::max(e->N, 8);
    for (int i = 0; i < e->n; ++i) e->xpose_floats = std::max(e->xpose_floats, (size_t)M * e->enc[i] * 2);
#define ALLOC(ptr, bytes)                                                                                      \
    do {                                                                                                       \
        size_t b_ = (bytes);                                                                                   \
        if (b_ == 0) b_ = 256;                                                                                 \
        if (hipMalloc((void**)&(ptr), b_) != hipSuccess) { int rc = fail(SGV_ERR_HIP, "hipMalloc(%zu bytes) failed for " #ptr, b_); sgv_destroy(e); return rc; } \
        hipMemsetAsync((ptr), 0, b_, e->stream);                                                               \
    } while (0)
    ALLOC(e->params, e->n_params * 4);
    ALLOC(e->grads, e->n_grads * 4);
    e->lp_dirty.assign(e->layers.size(), 0);
    ALLOC(e->adam_m, e->n_grads * 4);
    ALLOC(e->adam_v, e->n_grads * 4);
    ALLOC(e->copies, e->n_copies * e->esz);
    ALLOC(e->act, e->act_bytes);
    ALLOC(e->stats, e->n_stats * 8);
    ALLOC(e->sn_tmp, e->n_sn_tmp * 4);
    ALLOC(e->sn_sigma, e->layers.size() * 2 * 4);
    ALLOC(e->sn_dot_dummy, SGV_DOT_SLOTS * sizeof(float));
    ALLOC(e->scal, 32 * 8);
    ALLOC(e->partial, e->partial_floats * 4);
    ALLOC(e->partial_tn, e->partial_tn_floats * 4);
    e->gn_part_floats = 0;
    for (auto& l : e->layers) if (l.used && l.op != OP_LINEAR) e->gn_part_floats = std::max(e->gn_part_floats, gemm_nt256_part_floats((int)M, l.cout, 1));
    ALLOC(e->gn_part, e->gn_part_floats * 4);
    if (e->use_lanes && make_aux_stream(&e->lane2, "lane", {e->stream}) == hipSuccess &&
        hipEventCreateWithFlags(&e->lane_fork, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&e->lane_join, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&e->tail_fork, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&e->tail_join, hipEventDisableTiming) == hipSuccess) {
        ALLOC(e->partial2, e->partial_floats * 4);
        ALLOC(e->gn_part2, e->gn_part_floats * 4);
    } else {
        e->use_lanes = 0;
    }
    {
        size_t nr = 0;
        for (auto& g : e->gns) { g.ptot = nr; nr += align_up((size_t)e->maxB * 3 * g.C, 4); }
        for (auto& l : e->layers) if (l.op != OP_LINEAR) { l.dot_part = nr; nr += align_up((size_t)ew_gn_max_blocks(e->maxB, e->T, l.cout), 4); }
        for (auto& l : e->layers) if (l.op != OP_LINEAR && l.used && l.cout <= 8192) { l.col_part = nr; nr += align_up((size_t)ew_act_part_rows(e->maxB, e->T, l.cout) * l.cout, 4); }
        e->red_floats = nr;
    }
    ALLOC(e->red, e->red_floats * 4);
    if (make_aux_stream(&e->side, "side", {e->stream, e->lane2}) != hipSuccess) e->side = nullptr;
    e->use_side = e->use_side && e->side != nullptr;          // SGV_DW_SIDE applies once the side stream exists
    // the optimizer and wire streams of the data-parallel step are created on first use (ensure_opt / ensure_wire): every stream a
    // process creates shifts the runtime's stream -> hardware-queue assignment of the ones created after it
    ALLOC(e->xpose_tmp, e->xpose_floats * 4);
    ALLOC(e->colpart, e->colpart_floats * 4);
    if (e->use_lanes) ALLOC(e->colpart2, e->colpart_floats * 4);
#undef ALLOC
    if ((r = build_bind(e))) { sgv_destroy(e); return r; }
    if (hipStreamSynchronize(e->stream) != hipSuccess) { sgv_destroy(e); return fail(SGV_ERR_HIP, "stream sync failed in create"); }
    *out = e;
    return SGV_OK;
}

int sgv_destroy(sgv_engine* e) {
    if (!e) return SGV_OK;
    hipStreamSynchronize(e->stream);
    void* ptrs[] = {e->params, e->grads, e->adam_m, e->adam_v, e->copies, e->act, e->stats, e->sn_tmp, e->sn_sigma, e->sn_dot_dummy,
                    e->scal, e->partial, e->partial_tn, e->partial2, e->colpart2, e->gn_part2, e->gn_part, e->red, e->xpose_tmp, e->colpart};
    for (void* p : ptrs) if (p) hipFree(p);
    e->tab.release();
    if (e->side) { hipStreamSynchronize(e->side); hipStreamDestroy(e->side); }
    if (e->opt) { hipStreamSynchronize(e->opt); hipStreamDestroy(e->opt); }
    if (e->wire) { hipStreamSynchronize(e->wire); hipStreamDestroy(e->wire); }
    if (e->comm_own) { hipStreamSynchronize(e->comm_own); hipStreamDestroy(e->comm_own); }
    if (e->lane2) { hipStreamSynchronize(e->lane2); hipStreamDestroy(e->lane2); }
    if (e->aug_stream) {
        hipStreamSynchronize(e->aug_stream); hipStreamDestroy(e->aug_stream);
        hipEventDestroy(e->aug_done); hipEventDestroy(e->aug_gate); hipEventDestroy(e->x_free[0]); hipEventDestroy(e->x_free[1]); hipFree(e->aug_ctl);
    }
    if (e->lane_fork) hipEventDestroy(e->lane_fork);
    if (e->tail_fork) hipEventDestroy(e->tail_fork);
    if (e->tail_join) hipEventDestroy(e->tail_join);
    if (e->lane_join) hipEventDestroy(e->lane_join);
    for (auto ev : e->ev_pool) hipEventDestroy(ev);
    for (auto& t : e->timers) { hipEventDestroy(t.a); hipEventDestroy(t.b); }
    if (e->grads_lp) hipFree(e->grads_lp);
    if (e->tn_sched) hipFree(e->tn_sched);
    if (e->probes_dev) hipFree(e->probes_dev);
    ckpt_release(e);
    delete e;
    return SGV_OK;
}

int sgv_param_count(const sgv_engine* e) { return e ? (int)e->entries.size() : 0; }

int sgv_param_info(const sgv_engine* e, int index, const char** name, int* ndim, int64_t shape[4], int* kind, int* has_grad) {
    if (!e || index < 0 || index >= (int)e->entries.size()) return fail(SGV_ERR_ARG, "bad index");
    const StateEntry& s = e->entries[index];
    if (name) *name = s.name.c_str();
    if (ndim) *ndim = (int)s.shape.size();
    if (shape) for (size_t i = 0; i < s.shape.size() && i < 4; ++i) shape[i] = s.shape[i];
    if (kind) *kind = s.kind;
    if (has_grad) *has_grad = s.has_grad ? 1 : 0;
    return SGV_OK;
}

}  // extern "C"

// ---- reference layout <-> internal layout (host) ---------------------------------------------
// dir = +1: ref -> internal; -1: internal -> ref
static void permute_entry(const sgv_engine* e, const StateEntry& s, const float* src, float* dst, int dir) {
    const long cnt = s.count();
    if (s.gn >= 0) { memcpy(dst, src, cnt * 4); return; }
    const Layer& l = e->layers[s.layer];
    const int T = e->T;
    auto mov = [&](long iref, long iint) { if (dir > 0) dst[iint] = src[iref]; else dst[iref] = src[iint]; };
    if (s.kind == 1) {
        if (l.op == OP_CONV) {
            for (int co = 0; co < l.cout; ++co) for (int ci = 0; ci < l.cin; ++ci) for (int j = 0; j < l.k; ++j)
                mov(((long)co * l.cin + ci) * l.k + j, ((long)j * l.cout + co) * l.cin + ci);
        } else if (l.op == OP_CONVT) {
            for (int ci = 0; ci < l.cin; ++ci) for (int co = 0; co < l.cout; ++co) for (int j = 0; j < l.k; ++j)
                mov(((long)ci * l.cout + co) * l.k + j, ((long)(l.k - 1 - j) * l.cout + co) * l.cin + ci);
        } else if (l.lin_kind == LIN_HEAD) {
            const int C = l.lin_C;
            for (int o = 0; o < l.cout; ++o) for (int c = 0; c < C; ++c) for (int t = 0; t < T; ++t)
                mov((long)o * l.cin + (long)c * T + t, (long)o * l.cin + (long)t * C + c);
        } else {  // LIN_EXPAND: rows permuted
            const int C = l.lin_C;
            for (int c = 0; c < C; ++c) for (int t = 0; t < T; ++t) for (int k = 0; k < l.cin; ++k)
                mov(((long)c * T + t) * l.cin + k, ((long)t * C + c) * l.cin + k);
        }
    } else if (s.kind == 3) {  // v over matrix columns
        if (l.op == OP_CONV) { for (int ci = 0; ci < l.cin; ++ci) for (int j = 0; j < l.k; ++j) mov((long)ci * l.k + j, (long)j * l.cin + ci); }
        else if (l.op == OP_CONVT) { for (int ci = 0; ci < l.cin; ++ci) for (int j = 0; j < l.k; ++j) mov((long)ci * l.k + j, (long)(l.k - 1 - j) * l.cin + ci); }
        else if (l.lin_kind == LIN_HEAD) { const int C = l.lin_C; for (int c = 0; c < C; ++c) for (int t = 0; t < T; ++t) mov((long)c * T + t, (long)t * C + c); }
        else memcpy(dst, src, cnt * 4);
    } else {  // bias (0) or u (2): per output row
        if (l.op == OP_LINEAR && l.lin_kind == LIN_EXPAND) { const int C = l.lin_C; for (int c = 0; c < C; ++c) for (int t = 0; t < T; ++t) mov((long)c * T + t, (long)t * C + c); }
        else memcpy(dst, src, cnt * 4);
    }
}
size_t entry_param_offset(const sgv_engine* e, const StateEntry& s) {
    if (s.gn >= 0) return s.kind == 4 ? e->gns[s.gn].gamma : e->gns[s.gn].beta;
    const Layer& l = e->layers[s.layer];
    switch (s.kind) { case 0: return l.b; case 1: return l.w; case 2: return l.u; default: return l.v; }
}
size_t entry_grad_offset(const sgv_engine* e, const StateEntry& s) {
    if (!s.has_grad) return NPOS;
    if (s.gn >= 0) return s.kind == 4 ? e->gns[s.gn].ggamma : e->gns[s.gn].gbeta;
    const Layer& l = e->layers[s.layer];
    return s.kind == 0 ? l.gb : (s.kind == 1 ? l.gw : NPOS);
}
static const StateEntry* find_entry(sgv_engine* e, const char* name) {
    auto it = e->entry_index.find(name);
    if (it == e->entry_index.end()) return nullptr;
    return &e->entries[it->second];
}

static int refresh_copies(sgv_engine* e) {
    int r = opt_make_copies(e->tab.adam_dev, e->tab.dev[OptTables::COPY], e->tab.n(OptTables::COPY), e->dt, e->stream);
    if (r) return fail(SGV_ERR_HIP, "make_copies launch failed");
    e->copies_fresh = true;
    return 0;
}

static int run_sn(sgv_engine* e, int train) {
    // tpart of the fused layers may already hold the 64-row-block partials of W^T u from the last AdamW pass (still valid:
    // neither W nor u changed since); eval forwards never read or clobber it
    const bool reuse = train && e->wtu_fresh;
    const OptTables& t = e->tab;
    const OptTables::List l1 = reuse ? OptTables::SN_UNF : OptTables::SN;
    if (opt_sn_power_iteration(t.sn_dev, t.dev[l1], t.n(l1), t.dev[OptTables::SN], t.n(OptTables::SN), t.dev[OptTables::TSUM], t.n(OptTables::TSUM),
                               t.dev[OptTables::SSUM], t.n(OptTables::SSUM), (int)e->layers.size(), train, e->stream))
        return fail(SGV_ERR_HIP, "spectral-norm launch failed");
    if (train) e->wtu_fresh = false;     // u moved
    return 0;
}

static int export_act(sgv_engine* e, const Tensor& t, int B, float* host) {
    // [B][T][C] compute dtype -> [B][C][T] fp32
    const long cnt = (long)B * e->T * t.C;
    if ((size_t)cnt > e->xpose_floats) return fail(SGV_ERR_ARG, "activation too large for the export buffer");
    ew_transpose(t.f32 ? 0 : e->dt, 0, t.p, e->xpose_tmp, B, e->T, t.C, t.ld, e->T, (long)e->T * t.ld, (long)t.C * e->T, e->stream);
    HIPCHK(hipMemcpyAsync(host, e->xpose_tmp, cnt * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" {

int sgv_load_state(sgv_engine* e, const char* name, const float* host, size_t count) {
    if (!e || !name || !host) return fail(SGV_ERR_ARG, "null argument");
    const StateEntry* s = find_entry(e, name);
    if (!s) return fail(SGV_ERR_NAME, "unknown state key '%s'", name);
    if ((long)count != s->count()) return fail(SGV_ERR_ARG, "size mismatch for '%s': got %zu expected %ld", name, count, s->count());
    std::vector<float> tmp(count);
    permute_entry(e, *s, host, tmp.data(), +1);
    HIPCHK(hipMemcpy(e->params + entry_param_offset(e, *s), tmp.data(), count * 4, hipMemcpyHostToDevice));
    e->copies_fresh = false;
    e->wtu_fresh = false;
    return SGV_OK;
}

int sgv_export_state(sgv_engine* e, const char* name, float* host, size_t count) {
    if (!e || !name || !host) return fail(SGV_ERR_ARG, "null argument");
    const StateEntry* s = find_entry(e, name);
    if (!s) return fail(SGV_ERR_NAME, "unknown state key '%s'", name);
    if ((long)count != s->count()) return fail(SGV_ERR_ARG, "size mismatch for '%s'", name);
    std::vector<float> tmp(count);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(tmp.data(), e->params + entry_param_offset(e, *s), count * 4, hipMemcpyDeviceToHost));
    permute_entry(e, *s, tmp.data(), host, -1);
    return SGV_OK;
}

int sgv_export_grad(sgv_engine* e, const char* name, float* host, size_t count, int* is_none) {
    if (!e || !name || !host) return fail(SGV_ERR_ARG, "null argument");
    const StateEntry* s = find_entry(e, name);
    if (!s) return fail(SGV_ERR_NAME, "unknown state key '%s'", name);
    if ((long)count != s->count()) return fail(SGV_ERR_ARG, "size mismatch for '%s'", name);
    const size_t go = entry_grad_offset(e, *s);
    if (is_none) *is_none = (go == NPOS);
    if (go == NPOS) { memset(host, 0, count * 4); return SGV_OK; }
    std::vector<float> g(count);
    CHK(lp_sync(e));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(g.data(), e->grads + go, count * 4, hipMemcpyDeviceToHost));
    if (s->kind == 1) {
        // spectral-norm chain rule on the host (fp64): g_orig = (G - <G,W>/sigma * u v^T) / sigma
        const Layer& l = e->layers[s->layer];
        std::vector<float> w(count), u(l.cout), v((size_t)l.cin * l.k);
        float sig[2];
        HIPCHK(hipMemcpy(w.data(), e->params + l.w, count * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(u.data(), e->params + l.u, u.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(v.data(), e->params + l.v, v.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(sig, e->sn_sigma + 2 * l.sn, 8, hipMemcpyDeviceToHost));
        double dot = 0.0;
        for (size_t i = 0; i < count; ++i) dot += (double)g[i] * (double)w[i];
        const double c = dot / sig[0];
        for (int j = 0; j < l.k; ++j) for (int r = 0; r < l.cout; ++r) for (int cc = 0; cc < l.cin; ++cc) {
            const size_t i = ((size_t)j * l.cout + r) * l.cin + cc;
            g[i] = (float)(((double)g[i] - c * (double)u[r] * (double)v[(size_t)j * l.cin + cc]) / sig[0]);
        }
    }
    permute_entry(e, *s, g.data(), host, -1);
    return SGV_OK;
}

int sgv_export_adam(sgv_engine* e, const char* name, float* host_m, float* host_v, size_t count) {
    if (!e || !name) return fail(SGV_ERR_ARG, "null argument");
    const StateEntry* s = find_entry(e, name);
    if (!s) return fail(SGV_ERR_NAME, "unknown state key '%s'", name);
    const size_t go = entry_grad_offset(e, *s);
    if (go == NPOS) return fail(SGV_ERR_ARG, "'%s' has no optimizer state", name);
    if ((long)count != s->count()) return fail(SGV_ERR_ARG, "size mismatch for '%s'", name);
    std::vector<float> t(count);
    HIPCHK(hipStreamSynchronize(e->stream));
    if (host_m) { HIPCHK(hipMemcpy(t.data(), e->adam_m + go, count * 4, hipMemcpyDeviceToHost)); permute_entry(e, *s, t.data(), host_m, -1); }
    if (host_v) { HIPCHK(hipMemcpy(t.data(), e->adam_v + go, count * 4, hipMemcpyDeviceToHost)); permute_entry(e, *s, t.data(), host_v, -1); }
    return SGV_OK;
}

int sgv_load_adam(sgv_engine* e, const char* name, const float* host_m, const float* host_v, size_t count) {
    if (!e || !name) return fail(SGV_ERR_ARG, "null argument");
    const StateEntry* s = find_entry(e, name);
    if (!s) return fail(SGV_ERR_NAME, "unknown state key '%s'", name);
    const size_t go = entry_grad_offset(e, *s);
    if (go == NPOS) return fail(SGV_ERR_ARG, "'%s' has no optimizer state", name);
    if ((long)count != s->count()) return fail(SGV_ERR_ARG, "size mismatch for '%s': got %zu expected %ld", name, count, s->count());
    std::vector<float> t(count);
    HIPCHK(hipStreamSynchronize(e->stream));
    if (host_m) { permute_entry(e, *s, host_m, t.data(), +1); HIPCHK(hipMemcpy(e->adam_m + go, t.data(), count * 4, hipMemcpyHostToDevice)); }
    if (host_v) { permute_entry(e, *s, host_v, t.data(), +1); HIPCHK(hipMemcpy(e->adam_v + go, t.data(), count * 4, hipMemcpyHostToDevice)); }
    return SGV_OK;
}

int sgv_get_train_state(const sgv_engine* e, uint64_t state[4]) {
    if (!e || !state) return fail(SGV_ERR_ARG, "null argument");
    state[0] = (uint64_t)e->step; state[1] = e->seed; state[2] = e->draw; state[3] = 0;
    return SGV_OK;
}
int sgv_set_train_state(sgv_engine* e, const uint64_t state[4]) {
    if (!e || !state) return fail(SGV_ERR_ARG, "null argument");
    if (e->adam_open) return fail(SGV_ERR_STATE, "sgv_set_train_state: an AdamW step is open");
    if (state[3] != 0) return fail(SGV_ERR_ARG, "sgv_set_train_state: the reserved slot must be 0");
    if (state[0] > (uint64_t)1 << 62) return fail(SGV_ERR_ARG, "sgv_set_train_state: step count out of range");
    e->step = (long)state[0]; e->seed = state[1]; e->draw = state[2];     // unlike sgv_seed, the draw position is kept
    return SGV_OK;
}

int sgv_prepare(sgv_engine* e) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    return refresh_copies(e);
}

int sgv_set_input(sgv_engine* e, const float* x_dev, int batch) {
    if (!e || !x_dev) return fail(SGV_ERR_ARG, "null argument");
    if (batch < 1 || batch > e->maxB) return fail(SGV_ERR_ARG, "batch %d outside [1,%d]", batch, e->maxB);
    CHK(aug_join(e));
    // [B][N][T] fp32 -> [B][T][N] compute dtype
    ew_transpose(0, e->dt, x_dev, e->x_in.p, batch, e->N, e->T, e->T, e->x_in.ld, (long)e->N * e->T, (long)e->T * e->x_in.ld, e->stream);
    x_release(e);
    e->batch = batch;
    e->have_fwd = false;
    return SGV_OK;
}

int sgv_set_eps(sgv_engine* e, int site, const float* eps_dev, int batch) {
    if (!e || !eps_dev) return fail(SGV_ERR_ARG, "null argument");
    if (site < 0 || site >= e->n_st) return fail(SGV_ERR_ARG, "eps site %d outside [0,%d)", site, e->n_st);
    if (batch < 1 || batch > e->maxB) return fail(SGV_ERR_ARG, "bad batch");
    if (site == 0) {
        HIPCHK(hipMemcpyAsync(e->eps[0], eps_dev, (size_t)batch * e->Z * 4, hipMemcpyDeviceToDevice, e->stream));
    } else {
        const int C = e->dec[site];
        ew_transpose(0, 0, eps_dev, e->eps[site], batch, C, e->T, e->T, C, (long)C * e->T, (long)e->T * C, e->stream);
    }
    e->eps_set[site] = 1;
    return SGV_OK;
}

int sgv_set_shard(sgv_engine* e, int rank, int world) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (world < 1 || rank < 0 || rank >= world) return fail(SGV_ERR_ARG, "bad shard %d of %d", rank, world);
    e->shard_rank = rank; e->shard_world = world;
    return SGV_OK;
}
int sgv_set_draw_row(sgv_engine* e, long first_row) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (first_row < 0) return fail(SGV_ERR_ARG, "sgv_set_draw_row: first_row = %ld is negative", first_row);
    e->draw_row = first_row;
    return SGV_OK;
}
int sgv_seed(sgv_engine* e, uint64_t seed) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    e->seed = seed; e->draw = 0;
    return SGV_OK;
}

int sgv_set_option(sgv_engine* e, const char* key, int value) {
    if (!e || !key) return fail(SGV_ERR_ARG, "null argument");
    if (!strcmp(key, "write_xhat")) e->write_xhat = value != 0;
    else if (!strcmp(key, "use_tr")) e->use_tr = value != 0;
    else if (!strcmp(key, "dw_side_stream")) e->use_side = value != 0 && e->side != nullptr;
    else if (!strcmp(key, "ddp_early_adamw")) e->ddp_early = value != 0;
    else if (!strcmp(key, "wire_stream")) e->use_wire = value != 0 && ensure_wire(e) != nullptr;
    else if (!strcmp(key, "vendor_gemm")) { if (value) return fail(SGV_ERR_ARG, "vendor_gemm: the library GEMM back end was removed from libsgvae.so (comparator: tests/micro/vendor)"); }
    else if (!strcmp(key, "deterministic")) e->deterministic = value != 0;
    else if (!strcmp(key, "lanes")) e->use_lanes = value != 0 && e->lane2 != nullptr;          // second compute lane (schedule only: results are bitwise the same)
    else if (!strcmp(key, "grad_bf16")) CHK(set_grad_bf16(e, value));                            // see the member
    else if (!strcmp(key, "recompute_activations")) e->recompute_act = value != 0;               // measurement only, see block_bwd
    else if (!strcmp(key, "fused_stages")) e->use_convgn = value != 0;                          // csrc/convgn.hip kernels for the small Conv -> GroupNorm -> GELU stages
    else return fail(SGV_ERR_ARG, "unknown option '%s'", key);
    return SGV_OK;
}

static int encoder_fwd(sgv_engine* e, int B, bool join_lane) {
    const int n = e->n;
    CHK(aug_join(e));
    Tensor x = e->x_in;
    for (int i = 0; i < n; ++i) {
        CHK(block_fwd(e, e->encA[i], x, B));
        if (i == 0) CHK(aug_fire(e));          // a staged next batch: built beside the short kernels from here on
        CHK(block_fwd(e, e->encR[i], e->encA[i].st.back().a, B));
        x = e->enc_h[i];
        if (i < n - 1) {
            // the xs head of this level feeds only the decoder's posterior branch, which runs on the second lane: it goes there
            // too, beside the next encoder block (in-order on that lane, so the posterior branch needs no extra wait)
            Lane2 lane(e);
            const Layer& l = e->layers[e->xs_lin[i]];
            ew_linear_head_fwd(e->dt, x.p, e->params + l.w, e->params + l.b, e->sn_sigma + 2 * l.sn + 1, e->xs_raw[i], B, l.cin, l.cout, e->colpart, e->stream);
        }
    }
    const Layer& l = e->layers[e->last_lin];
    ew_linear_head_fwd(e->dt, x.p, e->params + l.w, e->params + l.b, e->sn_sigma + 2 * l.sn + 1, e->last, B, l.cin, l.cout, e->colpart, e->stream);
    if (join_lane) lane2_join(e);
    return 0;
}

// Decoder.forward (decoder.py:170-216) from e->zlat / e->xs_raw, then the recon head + loss pass -- or, with `tail`, the recon head's
// convolution and statistics followed by that recon tail instead of the loss tail (a surrogate pass: recon_tails.h).
extern "C++" int decoder_fwd(sgv_engine* e, int B, int train, int mode_fix, const ReconTail* tail) {
    const int n = e->n, n_st = e->n_st;
    const long M = (long)B * e->T;
    // A tail with members_before >= 0: the noise of member m is a function of (seed, m, site) alone -- the rows members_before + b of the streams
    // the first call after sgv_seed draws from -- and the draw position is left where it is: a study gives the same bits at any batch size.
    // The other surrogate passes draw per call, from row e->draw_row on (sgv_set_draw_row; 0 unless a caller cuts a study into batches itself)
    const bool ens = tail && tail->members_before >= 0;
    uint64_t ens_draw = 0;
    for (int s = 1; s < n_st; ++s) {
        if (!e->eps_set[s]) ew_randn(e->eps[s], M * e->dec[s], e->seed, (ens ? ens_draw++ : e->draw++) * 8 + s, e->stream, (long)e->T * e->dec[s], e->shard_world, e->shard_rank,
                                     ens ? tail->members_before : tail ? e->draw_row : 0);
    }
    {
        const Layer& l = e->layers[e->start_lin];
        ew_linear_expand_fwd(e->dt, e->zlat, e->params + l.w, e->params + l.b, e->sn_sigma + 2 * l.sn + 1, e->sbuf.p, B, l.cin, l.cout, e->stream);
    }
    CHK(block_fwd(e, e->decS, e->sbuf, B));
    for (int i = 0; i < n_st; ++i) {
        const bool post = i < n_st - 1;
        auto xs_lift = [&]() -> int {       // xs lift of the posterior branch: depends on the encoder only
            const Layer& l = e->layers[e->xs_exp[i]];
            const int lvl = n - 2 - i;
            ew_linear_expand_fwd(e->dt, e->xs_raw[lvl], e->params + l.w, e->params + l.b, e->sn_sigma + 2 * l.sn + 1, e->xl[i].p, B, l.cin, l.cout, e->stream);
            return block_fwd(e, e->decX[i], e->xl[i], B);
        };
        if (post) {
            // hoisted onto the second lane beside this stage's up-sampling and residual blocks: the lane's chain (lift, condition_xz) was
            // twice as long as the prior branch it ran beside, and the main stream waited for it at the join
            Lane2 lane(e);
            CHK(xs_lift());
        }
        CHK(block_fwd(e, e->decU[i], e->zs[i], B));
        CHK(block_fwd(e, e->decD[i], e->decU[i].st.back().a, B));
        if (!post) break;
        const int C = e->dec[i + 1];
        {   // posterior branch (xs lift -> condition_xz) on the second lane, beside the prior branch below
            Lane2 lane(e);
            CHK(block_fwd(e, e->decQ1[i], e->cat[i], B));
            CHK(block_fwd(e, e->decQ2[i], e->decQ1[i].st.back().a, B));
        }
        CHK(block_fwd(e, e->decP1[i], e->dec_out[i], B));
        CHK(block_fwd(e, e->decP2[i], e->decP1[i].st.back().a, B));
        lane2_join(e);
        ew_stage_fwd(e->dt, (const float*)e->decP2[i].st[0].y.p, (const float*)e->decQ2[i].st[0].y.p, e->eps[i + 1], e->dec_out[i].p, e->dec_out[i].ld,
                     e->zs[i + 1].p, e->zs[i + 1].ld, e->zmap[i], (int)M, C, mode_fix ? 1e-10f : 1.0f, e->scal + 3 + i, 1.0f / B, (double*)e->colpart, e->stream);
    }
    // recon head: conv -> GroupNorm stats -> tanh + loss (+ backward reductions in training)
    Stage& S = e->recon.st[0];
    const Layer& L = e->layers[S.layer];
    const GNLayer& g = e->gns[S.gn];
    GNParams p = gn_base(e, g, B);
    p.y = S.y.p; p.ldy = S.y.ld; p.sums = e->stats + S.sums; p.part = e->colpart;
    if (conv_fwd_fuses_stats(e, L, e->dec_out[n_st - 1], S.y, M, p.Cg, p.G)) {        // statistics from the GEMM epilogue: one 608 MB pass less
        CHK(conv_fwd(e, L, e->dec_out[n_st - 1], S.y, M, p.sums, p.Cg, p.G));
    } else {
        CHK(conv_fwd(e, L, e->dec_out[n_st - 1], S.y, M));
        ew_gn_stats(e->dt, p, e->stream);
    }
    if (tail) {
        // the tail's workspace is e->colpart, which nothing uses once the statistics are done (sized in sgv_create); the field and the
        // running states go straight to the caller's buffers (no loss, no read of x_in, no x_hat)
        ScopedTimer tm(e, tail->tag, nullptr);
        const int r = tail->run(e->dt, p, e->colpart, e->stream);
        return r ? fail(SGV_ERR_ARG, tail->rejected, r) : 0;
    }
    p.dout = e->x_in.p; p.lddout = e->x_in.ld; p.loss_type = e->cfg.loss_type;
    p.loss_sums = e->scal;
    if (e->write_xhat || !train) { p.out = e->xhat.p; p.ldout = e->xhat.ld; }
    if (train) {
        p.sums2 = e->stats + S.sums2; p.dgamma = e->recon_unit; p.dbeta = e->recon_unit + e->N;
        p.dbias = e->recon_unit + 2L * e->N; p.gscale = 1.0f;
    }
    ew_recon_loss(e->dt, train, p, e->stream);
    return 0;
}

static int read_scalars(sgv_engine* e, int B, float* scalars_host) {
    double h[16];
    HIPCHK(hipMemcpyAsync(h, e->scal, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const double numel = (double)B * e->T * e->N;
    for (int i = 0; i < SGV_MAX_SCALARS; ++i) scalars_host[i] = 0.f;
    scalars_host[0] = (float)(h[0] / numel);
    scalars_host[1] = (float)h[2];
    for (int i = 0; i + 1 < e->n_st; ++i) scalars_host[2 + i] = (float)h[3 + i];
    scalars_host[1 + e->n_st] = (float)(h[1] / numel);
    return 0;
}

int sgv_forward(sgv_engine* e, int train, int mode_fix, float* scalars_host) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (e->batch < 1) return fail(SGV_ERR_STATE, "no input set");
    if (train && mode_fix) return fail(SGV_ERR_ARG, "mode_fix is an inference path");
    if (!e->copies_fresh) CHK(refresh_copies(e));
    const int B = e->batch;
    if (!e->deterministic) HIPCHK(hipMemsetAsync(e->stats, 0, e->n_stats_fwd * 8, e->stream));   // only the fp64-atomic statistics epilogue accumulates
    HIPCHK(hipMemsetAsync(e->scal, 0, 16 * 8, e->stream));
    CHK(run_sn(e, train));
    CHK(encoder_fwd(e, B, false));
    if (!e->eps_set[0]) ew_randn(e->eps[0], (long)B * e->Z, e->seed, (e->draw++) * 8, e->stream, e->Z, e->shard_world, e->shard_rank);
    ew_latent_fwd(e->last, e->eps[0], e->zlat, B, e->Z, e->scal + 2, e->stream);
    CHK(decoder_fwd(e, B, train, mode_fix));
    e->have_fwd = true;
    e->fwd_train = train != 0;
    for (int s = 0; s < e->n_st; ++s) e->eps_set[s] = 0;
    x_release(e);                        // re-recorded at the end of the backward pass, which reads the batch again
    if (scalars_host) CHK(read_scalars(e, B, scalars_host));
    return SGV_OK;
}

// what sgv_decode and the surrogate entry points (engine_surrogate.hip) share in front of decoder_fwd: argument checks, fresh weight copies, eval-mode spectral norm,
// the caller's latents into e->zlat / e->xs_raw
extern "C++" int decode_begin(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, const char* who) {
    if (!e || !z_dev) return fail(SGV_ERR_ARG, "null argument");
    if (batch < 1 || batch > e->maxB) return fail(SGV_ERR_ARG, "batch %d outside [1,%d]", batch, e->maxB);
    if (!xs_dev)
        return fail(SGV_ERR_ARG, "%s needs xs (Decoder.forward with xs=None leaves z unchanged between stages in the reference; not supported)", who);
    if (!e->copies_fresh) CHK(refresh_copies(e));
    const int B = batch;
    e->batch = B;
    if (!e->deterministic) HIPCHK(hipMemsetAsync(e->stats, 0, e->n_stats_fwd * 8, e->stream));   // only the fp64-atomic statistics epilogue accumulates
    HIPCHK(hipMemsetAsync(e->scal, 0, 16 * 8, e->stream));
    CHK(run_sn(e, 0));
    HIPCHK(hipMemcpyAsync(e->zlat, z_dev, (size_t)B * e->Z * 4, hipMemcpyDeviceToDevice, e->stream));
    // list order of Encoder.forward's return: [xs_{n-2}, ..., xs_0]
    for (int j = 0; j < e->n - 1; ++j)
        HIPCHK(hipMemcpyAsync(e->xs_raw[e->n - 2 - j], xs_dev + (size_t)j * B * e->H, (size_t)B * e->H * 4, hipMemcpyDeviceToDevice, e->stream));
    return 0;
}

int sgv_decode(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, float* scalars_host) {
    CHK(decode_begin(e, z_dev, xs_dev, batch, "sgv_decode"));
    CHK(decoder_fwd(e, batch, 0, mode_fix));
    e->have_fwd = true;
    e->fwd_train = false;
    for (int s = 0; s < e->n_st; ++s) e->eps_set[s] = 0;
    if (scalars_host) CHK(read_scalars(e, batch, scalars_host));
    return SGV_OK;
}

int sgv_encode(sgv_engine* e, float* mu_host, float* logvar_host, float* xs_host) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (e->batch < 1) return fail(SGV_ERR_STATE, "no input set");
    if (!e->copies_fresh) CHK(refresh_copies(e));
    const int B = e->batch;
    if (!e->deterministic) HIPCHK(hipMemsetAsync(e->stats, 0, e->n_stats_fwd * 8, e->stream));   // only the fp64-atomic statistics epilogue accumulates
    CHK(run_sn(e, 0));
    CHK(encoder_fwd(e, B, true));
    x_release(e);
    std::vector<float> last((size_t)B * 2 * e->Z);
    HIPCHK(hipMemcpyAsync(last.data(), e->last, last.size() * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int b = 0; b < B; ++b) {
        if (mu_host) memcpy(mu_host + (size_t)b * e->Z, &last[(size_t)b * 2 * e->Z], e->Z * 4);
        if (logvar_host) memcpy(logvar_host + (size_t)b * e->Z, &last[(size_t)b * 2 * e->Z + e->Z], e->Z * 4);
    }
    if (xs_host) {
        // list order of Encoder.forward's return: [xs_{n-2}, ..., xs_0]
        for (int j = 0; j < e->n - 1; ++j)
            HIPCHK(hipMemcpy(xs_host + (size_t)j * B * e->H, e->xs_raw[e->n - 2 - j], (size_t)B * e->H * 4, hipMemcpyDeviceToHost));
    }
    return SGV_OK;
}

int sgv_get_xhat(sgv_engine* e, float* xhat_dev) {
    if (!e || !xhat_dev) return fail(SGV_ERR_ARG, "null argument");
    if (!e->have_fwd) return fail(SGV_ERR_STATE, "no forward pass to read from");
    ew_transpose(e->dt, 0, e->xhat.p, xhat_dev, e->batch, e->T, e->N, e->xhat.ld, e->T, (long)e->T * e->xhat.ld, (long)e->N * e->T, e->stream);
    return SGV_OK;
}

int sgv_get_activation(sgv_engine* e, const char* name, float* host, size_t count) {
    if (!e || !name || !host) return fail(SGV_ERR_ARG, "null argument");
    const int B = e->batch;
    std::string s(name);
    if (s == "x_in") {     // the input batch as the engine holds it (after sgv_set_input / sgv_augment_collate)
        CHK(aug_join(e));
        if (B < 1) return fail(SGV_ERR_STATE, "no input batch");
        if ((long)count != (long)B * e->T * e->N) return fail(SGV_ERR_ARG, "size mismatch for activation 'x_in'");
        return export_act(e, e->x_in, B, host);
    }
    if (!e->have_fwd) return fail(SGV_ERR_STATE, "no forward pass to read from");
    if (s.rfind("eps", 0) == 0 && s.size() == 4) {      // the noise of the last forward: eps0 [B][latent], eps{i} [B*T][C_i] (channels-last rows)
        const int site = s[3] - '0';
        if (site < 0 || site >= e->n_st) return fail(SGV_ERR_NAME, "bad noise site");
        const long want = site == 0 ? (long)B * e->Z : (long)B * e->T * e->dec[site];
        if ((long)count != want) return fail(SGV_ERR_ARG, "size mismatch for activation '%s': got %zu expected %ld", name, count, want);
        HIPCHK(hipMemcpy(host, e->eps[site], count * 4, hipMemcpyDeviceToHost));
        return SGV_OK;
    }
    auto chk = [&](long want) { return (long)count == want ? 0 : fail(SGV_ERR_ARG, "size mismatch for activation '%s': got %zu expected %ld", name, count, want); };
    auto idx = [&](const char* pre) { return atoi(s.c_str() + strlen(pre)); };
    HIPCHK(hipStreamSynchronize(e->stream));
    if (s.rfind("enc_h", 0) == 0) { int i = idx("enc_h"); if (i < 0 || i >= e->n) return fail(SGV_ERR_NAME, "bad index"); CHK(chk((long)B * e->T * e->enc[i])); return export_act(e, e->enc_h[i], B, host); }
    if (s.rfind("dec_out", 0) == 0) { int i = idx("dec_out"); if (i < 0 || i >= e->n_st) return fail(SGV_ERR_NAME, "bad index"); CHK(chk((long)B * e->T * e->dec[i + 1])); return export_act(e, e->dec_out[i], B, host); }
    if (s.rfind("zmap", 0) == 0) {
        int i = idx("zmap"); if (i < 0 || i + 1 >= e->n_st) return fail(SGV_ERR_NAME, "bad index");
        Tensor t; t.p = e->zmap[i]; t.C = e->dec[i + 1]; t.ld = t.C; t.f32 = true;
        CHK(chk((long)B * e->T * t.C)); return export_act(e, t, B, host);
    }
    if (s == "x_hat") { CHK(chk((long)B * e->T * e->N)); return export_act(e, e->xhat, B, host); }
    if (s == "mu" || s == "log_var") {
        CHK(chk((long)B * e->Z));
        std::vector<float> last((size_t)B * 2 * e->Z);
        HIPCHK(hipMemcpy(last.data(), e->last, last.size() * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) memcpy(host + (size_t)b * e->Z, &last[(size_t)b * 2 * e->Z + (s == "mu" ? 0 : e->Z)], e->Z * 4);
        return SGV_OK;
    }
    if (s == "z") { CHK(chk((long)B * e->Z)); HIPCHK(hipMemcpy(host, e->zlat, count * 4, hipMemcpyDeviceToHost)); return SGV_OK; }
    if (s.rfind("xs", 0) == 0) {
        int j = idx("xs"); if (j < 0 || j >= e->n - 1) return fail(SGV_ERR_NAME, "bad index");
        CHK(chk((long)B * e->H)); HIPCHK(hipMemcpy(host, e->xs_raw[e->n - 2 - j], count * 4, hipMemcpyDeviceToHost)); return SGV_OK;
    }
    return fail(SGV_ERR_NAME, "unknown activation '%s'", name);
}

// The backward traversal of the model: recon head, decoder stages, latent, encoder.  When a gradient bucket is complete and what
// happens to it then (transport, wire format, where its AdamW runs; fuse_lr >= 0: the optimizer step too) is GradRelease's
// business (engine_optim.hip): the traversal only says where a bucket's last gradient has been enqueued.
static int backward_impl(sgv_engine* e, float alpha, float beta, float fuse_lr) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (!e->have_fwd || !e->fwd_train) return fail(SGV_ERR_STATE, "sgv_backward needs a preceding sgv_forward(train=1)");
    e->lp_fp32 = false;                  // grad_bf16: this backward's gradients of the mirrored layers go to the mirror again
    GradRelease rel(e, fuse_lr);
    CHK(rel.begin());
    const int B = e->batch, n = e->n, n_st = e->n_st;
    const long M = (long)B * e->T;
    const float coefB = beta / (float)B;
    e->ev_next = 0;
    e->recompute_bytes = 0;
    e->fin_dots.clear(); e->fin_affine.clear();
    // no zero-fills: every gradient of the small zone (biases, GroupNorm affine, <G,W_eff> slot 0) and every backward group sum
    // is written, not accumulated, by its fixed-order reduction; tensors that get no gradient stay at their initial zero
    // ---- recon head ----
    {
        Stage& S = e->recon.st[0];
        const Layer& L = e->layers[S.layer];
        const GNLayer& g = e->gns[S.gn];
        const float gs = alpha / (float)((double)M * e->N);
        GNParams p = gn_base(e, g, B);
        p.y = S.y.p; p.ldy = S.y.ld; p.sums = e->stats + S.sums; p.sums2 = e->stats + S.sums2;
        p.dout = e->x_in.p; p.lddout = e->x_in.ld; p.loss_type = e->cfg.loss_type; p.gscale = gs;
        p.out = e->dy_recon.p; p.ldout = e->dy_recon.ld;
        p.cdot = e->grads + L.gdot; p.cbias = e->params + L.b;
        p.cdot_part = e->red + L.dot_part; p.cdot_blocks = &e->dot_counts[0];
        ew_recon_bwd_apply(e->dt, p, e->stream);
        e->fin_dots.push_back({p.cdot_part, p.cdot, e->dot_counts[0], 0});
        ew_scale3(e->grads + g.ggamma, e->grads + g.gbeta, e->grads + L.gb, e->recon_unit, gs, e->N, e->stream);
        CHK(conv_bwd_dw(e, L, e->dy_recon, e->dec_out[n_st - 1], M));
        CHK(conv_bwd_dx(e, L, e->dy_recon, e->d_out[n_st - 1], nullptr, M));
        rel.fire();
    }
    // ---- decoder stages ----
    for (int i = n_st - 1; i >= 0; --i) {
        const int C = e->dec[i + 1];
        if (i < n_st - 1) {
            ew_stage_bwd(e->dt, (const float*)e->decP2[i].st[0].y.p, (const float*)e->decQ2[i].st[0].y.p, e->eps[i + 1], e->dzs[i + 1].p, e->dzs[i + 1].ld,
                         e->gp[i].p, e->gq[i].p, (int)M, C, coefB, e->stream);
            Tensor d_xs = e->dcat[i]; d_xs.C = C;
            Tensor d_oq = e->dcat[i]; d_oq.C = C; d_oq.p = (char*)d_oq.p + (size_t)C * e->esz;
            {   // posterior branch on the second lane, beside the prior branch below (they meet in the add3 after the join)
                Lane2 lane(e);
                bool q_ready = false;      // condition_xz: the output convolution's input gradient went straight into the residual block's GroupNorm backward
                CHK(block_bwd(e, e->decQ2[i], e->decQ1[i].st.back().a, e->gq[i], &e->d_qres[i], B, nullptr, &e->decQ1[i].st.back(), &q_ready, false, 0.1f));
                CHK(block_bwd(e, e->decQ1[i], e->cat[i], e->d_qres[i], &e->dcat[i], B, nullptr, nullptr, nullptr, q_ready));
            }
            bool p_ready = false;
            CHK(block_bwd(e, e->decP2[i], e->decP1[i].st.back().a, e->gp[i], &e->d_pres[i], B, nullptr, &e->decP1[i].st.back(), &p_ready, false, 0.1f));
            CHK(block_bwd(e, e->decP1[i], e->dec_out[i], e->d_pres[i], &e->d_outp[i], B, nullptr, nullptr, nullptr, p_ready));
            lane2_join(e);
            ew_add3(e->dt, e->d_outp[i].p, e->d_outp[i].ld, e->dzs[i + 1].p, e->dzs[i + 1].ld, d_oq.p, d_oq.ld, e->d_out[i].p, e->d_out[i].ld, (int)M, C, e->stream);
            {
                // the xs lift's backward needs d_xs only: deferred onto the lane beside the residual / up-sampling blocks' backward
                // below (the mirror of the forward hoist); joined before the stage's bucket is released
                Lane2 lane(e);
                CHK(block_bwd(e, e->decX[i], e->xl[i], d_xs, &e->d_xl[i], B));
                const Layer& l = e->layers[e->xs_exp[i]];
                const int lvl = n - 2 - i;
                ew_linear_expand_bwd(e->dt, e->d_xl[i].p, e->xs_raw[lvl], e->params + l.w, e->sn_sigma + 2 * l.sn + 1, e->d_xs_raw[lvl],
                                     e->grads + l.gw, e->grads + l.gb, B, l.cin, l.cout, e->stream);
            }
        }
        CHK(block_bwd(e, e->decD[i], e->decU[i].st.back().a, e->d_out[i], &e->d_u[i], B));
        CHK(block_bwd(e, e->decU[i], e->zs[i], e->d_u[i], &e->dzs[i], B));
        if (i < n_st - 1) lane2_join(e);
        if (i == 0) {
            CHK(block_bwd(e, e->decS, e->sbuf, e->dzs[0], &e->d_sbuf, B));
            const Layer& l = e->layers[e->start_lin];
            ew_linear_expand_bwd(e->dt, e->d_sbuf.p, e->zlat, e->params + l.w, e->sn_sigma + 2 * l.sn + 1, e->d_z, e->grads + l.gw, e->grads + l.gb,
                                 B, l.cin, l.cout, e->stream);
        }
        rel.fire();
    }
    // ---- latent + encoder ----
    ew_latent_bwd(e->last, e->eps[0], e->d_z, e->d_last, B, e->Z, coefB, e->stream);
    {
        const Layer& l = e->layers[e->last_lin];
        ew_linear_head_bwd(e->dt, e->d_last, e->enc_h[n - 1].p, e->params + l.w, e->sn_sigma + 2 * l.sn + 1, nullptr, e->d_h[n - 1].p,
                           e->grads + l.gw, e->grads + l.gb, B, l.cin, l.cout, e->stream);
    }
    for (int i = n - 1; i >= 0; --i) {
        const Layer& xl = e->layers[e->xs_lin[i]];
        if (xl.has_grad) {
            ew_linear_head_bwd(e->dt, e->d_xs_raw[i], e->enc_h[i].p, e->params + xl.w, e->sn_sigma + 2 * xl.sn + 1, e->d_h[i].p, e->d_h[i].p,
                               e->grads + xl.gw, e->grads + xl.gb, B, xl.cin, xl.cout, e->stream);
        }
        bool a_ready = false;       // the residual block's input gradient went straight into the GroupNorm backward of encA[i]'s last stage
        CHK(block_bwd(e, e->encR[i], e->encA[i].st.back().a, e->d_h[i], &e->enc_a_dummy[i], B, nullptr, &e->encA[i].st.back(), &a_ready));
        const Tensor x_prev = i == 0 ? e->x_in : e->enc_h[i - 1];
        if (i == 0) {
            // the small bucket is released from inside the block, in front of its first layer's weight-gradient GEMM (release_small)
            CHK(rel.before_first_block());
            CHK(rel.after_first_block(block_bwd(e, e->encA[0], x_prev, e->enc_a_dummy[0], nullptr, B, &rel, nullptr, nullptr, a_ready)));
        } else {
            CHK(block_bwd(e, e->encA[i], x_prev, e->enc_a_dummy[i], &e->d_h[i - 1], B, nullptr, nullptr, nullptr, a_ready));
        }
    }
    return rel.finish();
}
// every path out of backward_impl has joined the side stream: the main stream's position is past the last reader of the batch
static int backward_done(sgv_engine* e, int rc) { e->coll_inflight = false; if (rc == SGV_OK) x_release(e); return rc; }
int sgv_backward(sgv_engine* e, float alpha, float beta) { return backward_done(e, backward_impl(e, alpha, beta, -1.f)); }
int sgv_backward_step(sgv_engine* e, float alpha, float beta, float lr) {
    if (lr < 0.f) return fail(SGV_ERR_ARG, "negative learning rate");
    if (e && e->cb) return fail(SGV_ERR_STATE, "sgv_backward_step is the single-GPU path: with a bucket callback use sgv_backward + sgv_adamw_step_range");
    return backward_done(e, backward_impl(e, alpha, beta, lr));
}

// device memory held by the engine, bytes: [0] fp32 master parameters, [1] gradient arena, [2] Adam m + v, [3] compute-dtype weight
// copies, [4] activations (every map of forward and backward at max_batch: nothing is recomputed), [5] split-K / reduction workspaces
int sgv_memory_info(const sgv_engine* e, size_t out[6]) {
    if (!e || !out) return fail(SGV_ERR_ARG, "null argument");
    out[0] = e->n_params * 4; out[1] = e->n_grads * 4; out[2] = e->n_grads * 8; out[3] = e->n_copies * e->esz; out[4] = e->act_bytes;
    out[5] = ((e->use_lanes ? 2 : 1) * (e->partial_floats + e->colpart_floats + e->gn_part_floats) + e->partial_tn_floats + e->red_floats + e->n_sn_tmp + e->xpose_floats) * 4;
    return SGV_OK;
}
int sgv_recompute_bytes(const sgv_engine* e, size_t* bytes) {
    if (!e || !bytes) return fail(SGV_ERR_ARG, "null argument");
    *bytes = e->recompute_bytes;
    return SGV_OK;
}
// ---- per-epoch statistics without a host sync per step (reference loop: modules/train.py:171-174 reads four scalars and
// one gradient norm per parameter tensor with .item() after every step; here the step's scalars are added to a device-side
// accumulator by a one-thread kernel and read once per epoch) ----
__global__ void scalars_accumulate_kernel(const double* scal, double* acc, int n_st, double numel) {
    // acc: [0] recon (selected loss, mean), [1] kl, [2..] kl2 per stage, [8] mse, [9] gradient norm, [10] steps
    acc[0] += scal[0] / numel;
    acc[1] += scal[2];
    for (int i = 0; i + 1 < n_st; ++i) acc[2 + i] += scal[3 + i];
    acc[8] += scal[1] / numel;
    acc[9] += sqrt(scal[15]);
    acc[10] += 1.0;
}
int sgv_scalars_accumulate(sgv_engine* e) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (e->batch < 1) return fail(SGV_ERR_STATE, "no step to accumulate");
    hipLaunchKernelGGL(scalars_accumulate_kernel, dim3(1), dim3(1), 0, e->stream, e->scal, e->scal + 16, e->n_st,
                       (double)e->batch * e->T * e->N);
    return SGV_OK;
}
int sgv_scalars_read(sgv_engine* e, double* host16, int reset) {
    if (!e || !host16) return fail(SGV_ERR_ARG, "null argument");
    HIPCHK(hipMemcpyAsync(host16, e->scal + 16, 16 * 8, hipMemcpyDeviceToHost, e->stream));
    if (reset) HIPCHK(hipMemsetAsync(e->scal + 16, 0, 16 * 8, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGV_OK;
}

int sgv_kernel_time_reset(sgv_engine* e, int enable) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    hipStreamSynchronize(e->stream);
    for (auto& t : e->timers) { hipEventDestroy(t.a); hipEventDestroy(t.b); }
    e->timers.clear();
    e->timing = enable != 0;
    e->timing_detail = enable == 2;
    return SGV_OK;
}
int sgv_kernel_time_tag(sgv_engine* e, int index, char* name, size_t cap, float* total_ms, int* calls) {
    if (!e || !name || cap == 0) return fail(SGV_ERR_ARG, "null argument");
    if (index < 0 || index >= (int)e->tag_names.size()) return SGV_ERR_ARG;   // end of the list: not an error message
    HIPCHK(hipStreamSynchronize(e->stream));
    snprintf(name, cap, "%s", e->tag_names[index].c_str());
    tag_total(e, index, total_ms, calls);
    return SGV_OK;
}
int sgv_kernel_time(sgv_engine* e, const char* which, float* total_ms, int* calls) {
    if (!e || !which) return fail(SGV_ERR_ARG, "null argument");
    HIPCHK(hipStreamSynchronize(e->stream));
    auto it = e->tag_ids.find(which);
    tag_total(e, it != e->tag_ids.end() ? it->second : -1, total_ms, calls);
    return SGV_OK;
}
}  // extern "C"
