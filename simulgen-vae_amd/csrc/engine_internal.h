// Private to engine*.hip and test_hooks.hip: the engine's data model and the few helpers that more than one of those files calls.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "../../include/sgvae.h"
#include "sgv_ew.h"

#define fail sgv_set_error      // the library's error helper (sgv_common.h) under the name the engine's code uses
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return fail(SGV_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define CHK(x)                                  \
    do {                                        \
        int r_ = (x);                           \
        if (r_ != 0) return r_ < 0 ? r_ : -r_;  \
    } while (0)

static const size_t NPOS = (size_t)-1;

struct Tensor {
    void* p = nullptr;
    int C = 0;
    long ld = 0;
    bool f32 = false;
};

enum { OP_CONV = 0, OP_CONVT = 1, OP_LINEAR = 2 };
enum { LIN_NONE = 0, LIN_HEAD = 1, LIN_EXPAND = 2 };

struct Layer {
    std::string prefix;
    int op = OP_CONV, cin = 0, cout = 0, k = 1;
    bool used = true, has_grad = true, need_wct = true;
    int lin_kind = LIN_NONE, lin_C = 0;      // head: K = lin_C*T; expand: O = lin_C*T
    size_t w = NPOS, b = NPOS, u = NPOS, v = NPOS;  // param arena (floats)
    size_t gw = NPOS, gb = NPOS, gdot = NPOS;       // grad arena (floats); gdot: <G,W_eff> scalar (small zone)
    size_t wc = NPOS, wct = NPOS;                   // compute-copy arena (elements)
    int sn = -1;
    int splitk_tn = 1;
    size_t dot_part = NPOS;                         // per-block <G,W_eff> partials of the layer's dY kernel (e->red arena)
    size_t col_part = NPOS;                         // per-block column sums of dY (bias gradient of a conv without GroupNorm), same arena
    bool lp = false;                                // option grad_bf16: this layer's weight gradient lives in the bf16 mirror arena (fixed at creation:
                                                    //   its weight-gradient GEMM takes the 256 x 256 kernel at the engine's full batch)
    long nw() const { return (long)cout * cin * k; }
};
struct GNLayer {
    std::string prefix;
    int C = 0, G = 1;
    bool used = true, has_grad = true;
    size_t gamma = NPOS, beta = NPOS, ggamma = NPOS, gbeta = NPOS;
    size_t ptot = NPOS;                             // [B][3][C] per-sample column totals of the backward pass (e->red arena)
};
struct Stage {
    int layer = -1, gn = -1, act = 0;
    bool pre_gelu = false, out_f32 = false;
    Tensor pre, y, a, dy, da, dpre;
    size_t sums = NPOS, sums2 = NPOS;   // stats arena (doubles)
};
struct Block {
    std::vector<Stage> st;
    bool residual = false;
};
struct StateEntry {
    std::string name;
    int kind;  // 0 bias,1 weight_orig,2 u,3 v,4 gn w,5 gn b
    int layer = -1, gn = -1;
    std::vector<int64_t> shape;
    bool has_grad;
    long count() const { long n = 1; for (auto s : shape) n *= s; return n; }
};

struct TimerRec { hipEvent_t a, b; int tag; };

constexpr double DW_SIDE_MAX_GF = 250.0;   // weight-gradient GEMMs up to this size go to the side stream (sgv_engine::side)
constexpr long CONVGN_MAXK = 4096;         // widest K * taps of a fused Conv -> GroupNorm -> GELU stage (sgv_engine::use_convgn)

struct sgv_engine {
    sgv_config cfg;
    hipStream_t stream = nullptr;
    int dt = 0;         // compute dtype
    size_t esz = 4;     // bytes per compute element
    int n = 0, n_st = 0, T = 0, N = 0, Z = 0, H = 0, maxB = 0;
    std::vector<int> enc, dec;
    std::vector<Layer> layers;
    std::vector<GNLayer> gns;
    std::vector<StateEntry> entries;
    std::map<std::string, int> entry_index;
    // arenas
    float* params = nullptr; size_t n_params = 0;
    float* grads = nullptr; size_t n_grads = 0, n_grads_w = 0;   // weights zone first, small zone after
    float* adam_m = nullptr; float* adam_v = nullptr;
    char* copies = nullptr; size_t n_copies = 0;
    char* act = nullptr; size_t act_bytes = 0, act_used = 0;
    double* stats = nullptr; size_t n_stats = 0, n_stats_fwd = 0;  // [fwd sums | bwd sums2]
    float* sn_tmp = nullptr; size_t n_sn_tmp = 0;   // power-iteration scratch, four blocks per layer (sn_scratch_carve)
    bool wtu_fresh = false;                          // tpart of the fused layers holds the W^T u partials for the current weights
    // descriptor and work-item tables of the optimizer / spectral-norm kernels, groups = gradient buckets.  DOT / fin hold the Linear
    // layers' <G,W> (per-item partials in tab.dot_part), tab.gnorm_part the per-item sums of squared gradients of the AdamW passes
    OptTables tab;
    float* sn_sigma = nullptr;
    float* sn_dot_dummy = nullptr;
    double* scal = nullptr;        // device doubles: [0..1] loss sums, [2] kl, [3..] kl2, [15] grad norm^2
    float* partial = nullptr; size_t partial_floats = 0;
    // weight-gradient GEMMs are off the critical path of backward: the SMALL ones (<= 250 GFLOP, i.e. everything but
    // the five largest layers) run on a second stream next to the dX GEMMs and normalisation passes of the following
    // layers, which fills the CUs those 100-200-block launches leave idle (measured 16.14 -> 15.83 ms/step).  Putting
    // the big ones there too loses 2.5 %: they fill every CU on their own and co-running kernels evict each other's
    // L2 tiles.  Option "dw_side_stream" / SGV_DW_SIDE=0 turns it off; kernel-timing passes always run on one stream.
    hipStream_t side = nullptr;
    std::vector<char> aug_host[4]; int aug_turn = 0;                  // staging of sgv_augment_collate's control arrays
    void* comm = nullptr; hipStream_t comm_stream = nullptr;          // native RCCL path (sgv_set_rccl)
    std::vector<hipEvent_t> bucket_done; std::vector<char> bucket_pending;
    // data-parallel wire format of the weight buckets: 0 = the fp32 arena itself, 1 = a bf16 copy (packed at the bucket's fire point,
    // averaged by the collective, unpacked into the arena in front of the bucket's AdamW).  The small bucket always travels in fp32.
    int payload_bf16 = 0; void* grads_lp = nullptr; std::vector<char> bucket_packed;
    // option "grad_bf16" (bf16 engines, single-GPU path: no communicator, no bucket callback): the 256 x 256 weight-gradient kernel
    // stores its result as bf16 into the mirror arena grads_lp and the AdamW pass reads it there (AdamDesc::glp) -- 4 B less
    // written and read per parameter of the big layers.  The fp32 arena of those layers is refreshed on demand (lp_sync) for the
    // calls that read it (sgv_export_grad, sgv_grad_norm).
    // With the bf16 wire format of the data-parallel step the same kernel writes the wire copy directly (bit for bit what the pack
    // pass produced from the fp32 result; that pass then skips those layers).
    int grad_bf16 = 0;
    bool lp_classified = false;
    std::vector<char> lp_dirty;          // per layer: its gradient of the last backward was stored as bf16 into grads_lp (not into the fp32 arena)
    // sgv_scale_grads / sgv_grad_buffer changed or exposed the fp32 arena after an lp_sync: until the next backward the AdamW pass
    // reads the fp32 arena for every layer (the mirror no longer holds the gradient)
    bool lp_fp32 = false;
    std::vector<std::vector<int>> bucket_lp_layers;     // per weight bucket: its Layer::lp layers in arena order
    bool dw_chunk_direct = false;        // chunked first-layer gradient (data-parallel): the chunk GEMMs write the wire copy themselves
    // data-parallel optimizer overlap: the <G,W_eff> scalars of a weight bucket's layers sit together at the head of the small zone
    // (bucket_dots[b] = their range), so they can be averaged WITH the bucket instead of with the small bucket at the end of backward;
    // the bucket's conv-weight AdamW then runs on `opt` as soon as both collectives have landed, under the rest of backward
    // (sgv_adamw_bucket_async; the engine's own RCCL path does it by itself in sgv_backward_step).  bucket_updated[b]: done this step.
    std::vector<std::pair<size_t, size_t>> bucket_dots; size_t dots_total = 0;
    hipStream_t opt = nullptr; bool opt_dirty = false, adam_open = false;
    hipStream_t comm_own = nullptr;                   // sgv_comm_stream: a probed communication stream the engine owns
    hipStream_t wire = nullptr; int use_wire = 0;     // callback path: buckets are complete (and packed) on this stream, not on the engine stream
    std::vector<char> bucket_updated;
    int ddp_early = 1;                                // SGV_DDP_EARLY; this and the other environment switches: env_switches (engine.hip)
    // BASELINE configs[3] "+ grad-checkpoint": what recomputing the GroupNorm + GELU outputs in backward would cost.  With the option on,
    // block_bwd regenerates every stage's activation a = act(GN(y)) from the stored pre-normalisation map and statistics right before
    // the stage's backward reads it (one extra streaming pass per stage).  The buffers themselves stay allocated -- this times the
    // recompute, it does not free the memory (sgv_memory_info's "activations" minus what recompute_bytes reports is what a
    // recompute build would keep); `use_checkpointing` stays forced off as in the reference
    bool recompute_act = false;
    size_t recompute_bytes = 0;
    // the last weight bucket (the first encoder layer: 97 M gradients that exist only when backward ends) is produced, exchanged and
    // updated in row chunks of the weight-gradient GEMM: chunk c's pack / all-reduce / AdamW run under chunk c + 1's GEMM, so only
    // the last chunk's exchange is exposed (engine-issued path; SGV_DDP_LAST_CHUNKS=1 turns it off).  Two chunks: 512 rows keep the
    // GEMM's 128 x 256 tiles at whole rounds of the chip, four chunks of 256 rows would cost 27 % of the GEMM
    int ddp_last_chunks = 2;
    double ddp_chunk_min_gf = 250.0;                  // SGV_DDP_CHUNK_MIN_GF: tests lower it to chunk a small first layer
    int dw_chunks = 1, dw_chunk_layer = -1;
    struct GradRelease* release = nullptr;            // non-null only while backward_impl runs: conv_bwd_dw reports each chunk's GEMM to it (after_chunk)
    // bf16 wire format: the conv-weight AdamW reads a packed bucket straight from the averaged bf16 copy (no unpack pass; the fp32
    // arena keeps this rank's own gradients); only the few weights of a bucket that the flat pass updates (Linear heads:
    // bucket_flat_w) are unpacked.  bucket_packed[b]: bit 0 = conv-weight part still packed, bit 1 = flat part still packed.
    std::vector<std::vector<std::pair<size_t, size_t>>> bucket_flat_w;
    float* partial_tn = nullptr; size_t partial_tn_floats = 0;
    std::vector<hipEvent_t> ev_pool; size_t ev_next = 0;
    bool use_side = true, side_dirty = false;
    float* xpose_tmp = nullptr; size_t xpose_floats = 0;
    float* recon_unit = nullptr;   // [3][N] unit-scale dgamma/dbeta/dbias of the recon head
    float* colpart = nullptr; size_t colpart_floats = 0;   // per-block column-sum workspace (also the frame partials of sgv_summarize, the partials of sgv_project and sgv_gram and the transposed weights of sgv_temporal)
    int* probes_dev = nullptr; int n_probes = 0;           // sgv_set_probes: SGV_MAX_PROBES checked node indices (allocated on first use)
    std::vector<int32_t> probes_host;                      // the source of the last upload stays alive until the next one
    // graph
    std::vector<Block> encA, encR, decU, decD, decP1, decP2, decX, decQ1, decQ2;
    Block decS, recon;
    std::vector<int> xs_lin, xs_exp;   // layer ids: encoder.xs_linear.i ; decoder.xs_sequence.i.0
    int last_lin = -1, start_lin = -1;
    // tensors
    Tensor x_in, xhat, sbuf, d_sbuf, dy_recon;
    // Prefetched augmentation (sgv_augment_stage / sgv_augment_advance): the NEXT batch is built in the spare input buffer on a
    // stream of its own, in launches of a few samples, beside the short kernels that follow the first encoder layer's GEMM (the
    // chip's HBM is idle there); the reference hides the same work in DataLoader worker processes.
    Tensor x_bufs[2];
    int x_cur = 0;
    hipStream_t aug_stream = nullptr;
    hipEvent_t aug_done = nullptr, aug_gate = nullptr, x_free[2] = {nullptr, nullptr};
    bool x_free_set[2] = {false, false};
    bool aug_staged = false, aug_fired = false, aug_pending = false;   // staged: control arrays on the device; fired: kernels enqueued; pending: the current batch's kernels may still run
    const void* aug_data = nullptr;
    int aug_next_batch = 0;
    char* aug_ctl = nullptr;           // control arrays of the staged batch
    std::vector<Tensor> enc_h, d_h, enc_a_dummy, zs, dzs, cat, dcat, dec_out, d_out, d_u, d_pres, d_qres, d_outp, gp, gq, xl, d_xl;
    std::vector<float*> xs_raw, d_xs_raw, eps, zmap;
    std::vector<int> eps_set;
    float *last = nullptr, *d_last = nullptr, *zlat = nullptr, *d_z = nullptr;
    int batch = 0;
    bool have_fwd = false, fwd_train = false, write_xhat = true, copies_fresh = false;
    int deterministic = 1;             // 1: no float-atomic accumulation anywhere in the step; option "deterministic"
    float* gn_part = nullptr; size_t gn_part_floats = 0;   // per-(tile, wave) GroupNorm partial sums of the 256x256 GEMM epilogue
    // deterministic reductions: block partials that nobody needs before the optimizer (GroupNorm affine / bias gradients,
    // <G,W_eff>) stay in this arena until the bucket they belong to is released, then two table-driven passes sum them
    // second compute lane: the posterior branch of a decoder stage (xs lift, condition_xz) is independent of the prior branch
    // (condition_z) between the residual block and the KL / reparameterisation kernel, in forward and in backward; both are chains
    // of small kernels that leave most of the chip idle, so they run side by side on two streams with workspaces of their own
    hipStream_t lane2 = nullptr; float* partial2 = nullptr; float* colpart2 = nullptr; float* gn_part2 = nullptr;
    hipEvent_t lane_fork = nullptr, lane_join = nullptr;
    hipEvent_t tail_fork = nullptr, tail_join = nullptr;      // concurrent 128-row tail of a 256 x 256 launch (launch_nt)
    bool coll_inflight = false;        // data-parallel backward, from the first released bucket on: a collective's channel workgroups may hold CUs
    int* tn_sched = nullptr;           // 8 x 520 ints: work-stealing state of the 256 x 256 weight-gradient launches issued while coll_inflight
    unsigned tn_sched_next = 0;
    int use_lanes = 1;                 // SGV_LANES
    // small Conv1d -> GroupNorm -> GELU stages in one launch (convgn.hip, K * taps <= CONVGN_MAXK); SGV_CONVGN=0 restores GEMM +
    // combine + GroupNorm kernels
    int use_convgn = 1;
    float* red = nullptr; size_t red_floats = 0;
    std::vector<FinDot> fin_dots; std::vector<FinAffine> fin_affine;
    int dot_counts[512];
    uint64_t seed = 0x5347564145ull, draw = 0;
    long draw_row = 0;                          // sgv_set_draw_row: sample b of a per-call draw takes row draw_row + b of its stream
    int shard_rank = 0, shard_world = 1;        // sgv_set_shard: sample b of this engine's batch is sample b * world + rank of the global batch
    long step = 0;
    float scalars_host[SGV_MAX_SCALARS];
    sgv_bucket_cb cb = nullptr; void* cb_user = nullptr;
    std::vector<std::pair<size_t, size_t>> buckets;   // (offset, count) in grad arena, backward order
    bool timing = false, timing_detail = false;
    std::vector<TimerRec> timers;
    std::map<std::string, int> tag_ids;
    std::vector<std::string> tag_names;
    int use_tr = 1;
    // whole-state snapshot / restore (engine_ckpt.hip): one flat fp32 buffer in reference layout, filled by table-driven permute
    // kernels into a device staging buffer (allocated on first use, not counted by sgv_memory_info) and copied to the caller's
    // pinned host buffer on a stream of the engine's own, so the main stream can go on with the next step at once
    struct CkptState* ckpt = nullptr;
};

constexpr int SGV_MAX_PROBES = 4096;
// position of the first probe node outside [0, N), -1 if none (sgv_set_probes, sgv_test_recon_summary)
static inline int first_bad_probe(const int32_t* nodes, int count, int N) {
    for (int i = 0; i < count; ++i) if (nodes[i] < 0 || nodes[i] >= N) return i;
    return -1;
}
// The output structs of the surrogate passes, checked and converted in one place for the entry points (engine.hip) and the kernel
// hooks (test_hooks.hip).  *_ok: 0, or SGV_ERR_ARG with the message set; `who` is the caller's name, the prefix of the message, and the
// second string the one word in which the texts of an entry point and of its hook differ.
static inline int summary_out_ok(const char* who, const char* noun, const sgv_summary_out* o) {
    if (!o) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!o->node_stats && !o->node_when && !o->frame_stats && !o->frame_where && !o->probes) return fail(SGV_ERR_ARG, "%s: all five outputs are NULL", who);
    if ((((uintptr_t)o->node_stats | (uintptr_t)o->node_when) & 15) || (((uintptr_t)o->frame_stats | (uintptr_t)o->frame_where) & 7) || ((uintptr_t)o->probes & 3))
        return fail(SGV_ERR_ARG, "%s: misaligned %s (node_stats / node_when 16 bytes, frame_stats / frame_where 8, probes 4)", who, noun);
    return 0;
}
static inline ReconSummary recon_summary_of(const sgv_summary_out& o, const int* probe_nodes, int n_probes, float* work) {
    ReconSummary r;
    r.node_stats = o.node_stats; r.node_when = o.node_when; r.frame_stats = o.frame_stats; r.frame_where = o.frame_where;
    r.probes = o.probes; r.probe_nodes = probe_nodes; r.n_probes = n_probes; r.work = work;
    return r;
}
static inline int score_out_ok(const char* who, const char* truth_name, const float* truth, const sgv_score_out* o) {
    if (!truth || !o) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!o->node_err && !o->node_when && !o->frame_err && !o->frame_where) return fail(SGV_ERR_ARG, "%s: all four outputs are NULL", who);
    if ((((uintptr_t)truth | (uintptr_t)o->node_err | (uintptr_t)o->node_when) & 15) || (((uintptr_t)o->frame_err | (uintptr_t)o->frame_where) & 3))
        return fail(SGV_ERR_ARG, "%s: misaligned pointer (%s, node_err / node_when 16 bytes, frame_err / frame_where 4)", who, truth_name);
    return 0;
}
static inline ReconScore recon_score_of(const sgv_score_out& o, float* work) {
    ReconScore r;
    r.node_err = o.node_err; r.node_when = o.node_when; r.frame_err = o.frame_err; r.frame_where = o.frame_where; r.work = work;
    return r;
}
static inline int ensemble_state_ok(const char* who, const char* batch_name, const sgv_ensemble_state* st, long count_before, int batch) {
    if (!st) return fail(SGV_ERR_ARG, "%s: null argument", who);
    const bool mo = st->mean || st->m2, ex = st->max || st->min || st->arg_max || st->arg_min, ec = st->exceed || st->limit;
    if (!mo && !ex && !ec) return fail(SGV_ERR_ARG, "%s: no group of the state is given", who);
    if ((mo && !(st->mean && st->m2)) || (ex && !(st->max && st->min && st->arg_max && st->arg_min)) || (ec && !(st->exceed && st->limit)))
        return fail(SGV_ERR_ARG, "%s: half a group (mean + m2, max + min + arg_max + arg_min, limit + exceed go together)", who);
    if ((((uintptr_t)st->mean | (uintptr_t)st->m2 | (uintptr_t)st->max | (uintptr_t)st->min | (uintptr_t)st->arg_max | (uintptr_t)st->arg_min |
          (uintptr_t)st->exceed) & 15) || ((uintptr_t)st->limit & 3))
        return fail(SGV_ERR_ARG, "%s: misaligned pointer (the state arrays 16 bytes, limit 4)", who);
    if (count_before < 0 || batch < 1 || count_before + batch > (1L << 24))
        return fail(SGV_ERR_ARG, "%s: count_before = %ld with %s = %d is outside [0, 2^24]", who, count_before, batch_name, batch);
    return 0;
}
static inline ReconEnsemble recon_ensemble_of(const sgv_ensemble_state& st) {
    ReconEnsemble r;
    r.mean = st.mean; r.m2 = st.m2; r.vmax = st.max; r.vmin = st.min; r.imax = st.arg_max; r.imin = st.arg_min;
    r.limit = st.limit; r.exceed = st.exceed;
    return r;
}
constexpr int SGV_DISTRIBUTION_MIN_BINS = 2, SGV_DISTRIBUTION_MAX_BINS = 64;      // HI_MIN_BINS, HI_MAX_BINS of recon_out.hip: the block's byte histogram fits the LDS
static inline int distribution_state_ok(const char* who, const char* batch_name, const sgv_distribution_state* st, long count_before, int batch) {
    if (!st) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!st->lo || !st->hi || !st->counts) return fail(SGV_ERR_ARG, "%s: lo, hi and counts are all required", who);
    if (st->bins < SGV_DISTRIBUTION_MIN_BINS || st->bins > SGV_DISTRIBUTION_MAX_BINS)
        return fail(SGV_ERR_ARG, "%s: bins = %d is outside [%d, %d]", who, st->bins, SGV_DISTRIBUTION_MIN_BINS, SGV_DISTRIBUTION_MAX_BINS);
    if (((uintptr_t)st->lo | (uintptr_t)st->hi | (uintptr_t)st->counts) & 15) return fail(SGV_ERR_ARG, "%s: misaligned pointer (lo, hi and counts 16 bytes)", who);
    if (count_before < 0 || batch < 1 || count_before + batch > (1L << 24))
        return fail(SGV_ERR_ARG, "%s: count_before = %ld with %s = %d is outside [0, 2^24]", who, count_before, batch_name, batch);
    return 0;
}
static inline ReconDistribution recon_distribution_of(const sgv_distribution_state& st) {
    ReconDistribution r;
    r.lo = st.lo; r.hi = st.hi; r.counts = st.counts; r.bins = st.bins;
    return r;
}
constexpr int SGV_REGRESS_MAX_COVARIATES = 32;      // RG_MAX_K of recon_out.hip: the launch's weights fit the block's LDS table
static inline int regress_state_ok(const char* who, const char* batch_name, const sgv_regress_state* st, int n_cov, const float* weights, long count_before,
                                   int batch) {
    if (!st || !weights) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!st->mean || !st->m2 || !st->comoment) return fail(SGV_ERR_ARG, "%s: mean, m2 and comoment are all required", who);
    if (n_cov < 1 || n_cov > SGV_REGRESS_MAX_COVARIATES) return fail(SGV_ERR_ARG, "%s: n_cov = %d is outside [1, %d]", who, n_cov, SGV_REGRESS_MAX_COVARIATES);
    if ((((uintptr_t)st->mean | (uintptr_t)st->m2 | (uintptr_t)st->comoment) & 15) || ((uintptr_t)weights & 3))
        return fail(SGV_ERR_ARG, "%s: misaligned pointer (the state arrays 16 bytes, weights 4)", who);
    if (count_before < 0 || batch < 1 || count_before + batch > (1L << 24))
        return fail(SGV_ERR_ARG, "%s: count_before = %ld with %s = %d is outside [0, 2^24]", who, count_before, batch_name, batch);
    return 0;
}
static inline ReconRegress recon_regress_of(const sgv_regress_state& st, const float* weights) {
    ReconRegress r;
    r.mean = st.mean; r.m2 = st.m2; r.co = st.comoment; r.w = weights;
    return r;
}
// sgv_project and its test hook: SGV_MAX_FUNCTIONALS (sgv_ew.h) weight rows at most
static inline int project_args_ok(const char* who, const float* weights, int n_func, const float* out) {
    if (!weights || !out) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (n_func < 1 || n_func > SGV_MAX_FUNCTIONALS) return fail(SGV_ERR_ARG, "%s: n_func = %d is outside [1, %d]", who, n_func, SGV_MAX_FUNCTIONALS);
    if (((uintptr_t)weights & 15) || ((uintptr_t)out & 3)) return fail(SGV_ERR_ARG, "%s: misaligned pointer (weights 16 bytes, out 4)", who);
    return 0;
}
// sgv_temporal and its test hook: SGV_MAX_TEMPORAL (sgv_ew.h) weight rows at most; the rows of out are written 32 bytes at a time
static inline int temporal_args_ok(const char* who, const float* weights, int n_func, const float* out) {
    if (!weights || !out) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (n_func < 1 || n_func > SGV_MAX_TEMPORAL) return fail(SGV_ERR_ARG, "%s: n_func = %d is outside [1, %d]", who, n_func, SGV_MAX_TEMPORAL);
    if (((uintptr_t)weights & 3) || ((uintptr_t)out & 15)) return fail(SGV_ERR_ARG, "%s: misaligned pointer (weights 4 bytes, out 16)", who);
    return 0;
}
// sgv_gram and its test hook: T <= SGV_MAX_GRAM_T (sgv_ew.h) row tiles fit the kernel's accumulators; the weights and the offset may be null
static inline int gram_args_ok(const char* who, int T, const float* node_weights, const float* offset, const float* out) {
    if (!out) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (T > SGV_MAX_GRAM_T) return fail(SGV_ERR_ARG, "%s: T = %d is beyond the limit of %d time steps", who, T, SGV_MAX_GRAM_T);
    if ((((uintptr_t)node_weights | (uintptr_t)offset) & 15) || ((uintptr_t)out & 3)) return fail(SGV_ERR_ARG, "%s: misaligned pointer (node_weights and offset 16 bytes, out 4)", who);
    return 0;
}
// sgv_exceedance and its test hook: SGV_MAX_EXCEED_LEVELS (sgv_ew.h) levels at most, T within the kernel's packed 16-bit counters; the
// rows of both outputs are written 32 bytes at a time
static inline int exceedance_args_ok(const char* who, int T, const float* levels, int n_level, int side, const int32_t* stats, const float* excess) {
    if (!levels) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!stats && !excess) return fail(SGV_ERR_ARG, "%s: no output (stats and excess are both null)", who);
    if (n_level < 1 || n_level > SGV_MAX_EXCEED_LEVELS) return fail(SGV_ERR_ARG, "%s: n_level = %d is outside [1, %d]", who, n_level, SGV_MAX_EXCEED_LEVELS);
    if (side != SGV_SIDE_ABOVE && side != SGV_SIDE_BELOW) return fail(SGV_ERR_ARG, "%s: unknown side %d", who, side);
    if (T > 65535) return fail(SGV_ERR_ARG, "%s: T = %d is beyond the limit of 65535 time steps", who, T);
    if (((uintptr_t)levels & 3) || (((uintptr_t)stats | (uintptr_t)excess) & 15)) return fail(SGV_ERR_ARG, "%s: misaligned pointer (levels 4 bytes, stats and excess 16)", who);
    return 0;
}
constexpr int SGV_SOBOL_MAX_PARAMS = 30;   // SB_MAX_D of recon_out.hip: a block of n_params + 2 members fits the kernel's member table
static inline int sobol_state_ok(const char* who, const char* batch_name, const sgv_sobol_state* st, int n_params, long blocks_before, int batch) {
    if (!st) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!st->mean || !st->m2) return fail(SGV_ERR_ARG, "%s: mean and m2 are required", who);
    if (!st->first_sq && !st->total_sq) return fail(SGV_ERR_ARG, "%s: neither first_sq nor total_sq is given", who);
    if (((uintptr_t)st->mean | (uintptr_t)st->m2 | (uintptr_t)st->first_sq | (uintptr_t)st->total_sq) & 15)
        return fail(SGV_ERR_ARG, "%s: misaligned pointer (the state arrays 16 bytes)", who);
    if (n_params < 1 || n_params > SGV_SOBOL_MAX_PARAMS) return fail(SGV_ERR_ARG, "%s: n_params = %d is outside [1, %d]", who, n_params, SGV_SOBOL_MAX_PARAMS);
    if (batch < 1 || batch % (n_params + 2))
        return fail(SGV_ERR_ARG, "%s: %s = %d is not a positive multiple of n_params + 2 = %d (whole blocks A, B, AB_1 .. AB_d)", who, batch_name, batch, n_params + 2);
    if (blocks_before < 0 || blocks_before > (1L << 23) || 2 * (blocks_before + batch / (n_params + 2)) > (1L << 24))
        return fail(SGV_ERR_ARG, "%s: blocks_before = %ld with %d blocks: 2 (blocks_before + blocks) is outside [0, 2^24]", who, blocks_before, batch / (n_params + 2));
    return 0;
}
static inline ReconSobol recon_sobol_of(const sgv_sobol_state& st) {
    ReconSobol r;
    r.mean = st.mean; r.m2 = st.m2; r.first_sq = st.first_sq; r.total_sq = st.total_sq;
    return r;
}

#pragma GCC visibility push(hidden)       // shared among the engine's files only: kept out of the library's dynamic symbols
// The release policy of the gradient buckets, on backward_impl's stack for one backward pass (engine_optim.hip): the transport (none,
// bucket callback, engine-issued RCCL), the wire format, where a bucket's AdamW runs (`early`: side stream, `dearly`: optimizer
// stream, or after backward), per-bucket or final Linear <G,W> dots, the early small bucket, the chunked last weight bucket.
struct GradRelease {
    sgv_engine* e; float fuse_lr;
    bool fuse = false, early = false, dearly = false, dots_per_bucket = false, last_chunked = false, lin_err = false;
    int last_b = -1, L0i = -1, bucket = 0;     // last weight bucket, the first encoder layer, the next weight bucket to release
    std::vector<hipEvent_t> chunk_done;
    const char* err = nullptr;                 // the first policy call that failed; a failure ends the work on its bucket, finish() reports it
    GradRelease(sgv_engine* e_, float lr) : e(e_), fuse_lr(lr) { e->release = this; }  ~GradRelease() { e->release = nullptr; }
    void failed(const char* what) { if (!err) err = what; }
    int begin(), gather_on(hipStream_t t);
    void fire(), fire_at(int b);               // release the next weight bucket / bucket b
    void flush_fin(bool affine), lin_dots(int b0, int b1);  // fixed-order partial sums; the Linear <G,W> dots of buckets [b0, b1)
    void release_small();                      // block_bwd: in front of the first encoder layer's weight-gradient GEMM
    int after_chunk(int c, int n_c, int co0, int co1);      // conv_bwd_dw: (chunk, chunks, first row, end row) after the chunk's GEMM is enqueued
    int before_first_block(), after_first_block(int br);    // around the first encoder block's backward: chunking on; off, the chunks' updates
    int finish();                              // the last weight bucket and the tail of the step; backward_impl returns it
};
// engine_build.hip
bool layer_fused_adam(const Layer& l);                                                       // conv weights that train: tiled AdamW
int build_layout(sgv_engine* e);                                                            // graph, arena layouts, table sizes
int build_bind(sgv_engine* e);                                                              // arenas allocated: pointers rebased, tables uploaded
// engine_optim.hip
bool grad_lp_active(const sgv_engine* e);
bool wire_lp_active(sgv_engine* e);
int lp_sync(sgv_engine* e);
int set_grad_bf16(sgv_engine* e, int value);
hipEvent_t next_event(sgv_engine* e);                                                       // engine_streams.hip: from the engine's pool (rewound by every backward)
#pragma GCC visibility pop

// ---- helpers that more than one translation unit calls, under the file that defines them: engine.hip ----
void sum_slabs(float* out, const float* partial, int splitk, long n, hipStream_t stream);   // out = sum of split-K slabs, fixed order
size_t entry_param_offset(const sgv_engine* e, const StateEntry& s);                         // float offset of a state entry in the parameter arena
size_t entry_grad_offset(const sgv_engine* e, const StateEntry& s);                          // ... in the gradient / Adam-moment arenas, NPOS if it gets no gradient
// engine_ckpt.hip
void ckpt_release(sgv_engine* e);                                                           // sgv_destroy: staging buffer, tables, copy stream
// engine_streams.hip
int stream_wait(sgv_engine* e, hipStream_t waiter, hipStream_t of);                         // waiter waits for what `of` holds so far
int join_side(sgv_engine* e);
bool streams_overlap(hipStream_t a, hipStream_t b);
hipError_t make_aux_stream(hipStream_t* out, const char* label, std::initializer_list<hipStream_t> avoid);
hipStream_t ensure_opt(sgv_engine* e);
hipStream_t ensure_comm_own(sgv_engine* e);
hipStream_t ensure_wire(sgv_engine* e);
// engine_input.hip
int aug_fire(sgv_engine* e);
int aug_join(sgv_engine* e);
void x_release(sgv_engine* e);
// engine_comm.hip
struct RcclApi {
    struct Id128 { char b[128]; };             // ncclUniqueId: 128 opaque bytes, passed by value
    void* h = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
extern RcclApi g_rccl;
constexpr int kNcclFloat32 = 7, kNcclBfloat16 = 9, kNcclAvg = 4;      // ncclDataType_t / ncclRedOp_t values of rccl.h (NCCL >= 2.10 ABI)
bool comm_is_single(void* comm);
int rccl_bucket(sgv_engine* e, void* comm, hipStream_t cs, int b, hipEvent_t done, bool split_dots = false);
