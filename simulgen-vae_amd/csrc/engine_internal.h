// Private to engine*.hip and test_hooks.hip: the engine's data model and the few helpers that more than one of those files calls.
// (What the surrogate output passes check and launch is in recon_tails.h.)
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
// engine.hip, for engine_surrogate.hip
struct ReconTail;                                                                           // recon_tails.h
int decode_begin(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, const char* who);   // checks, fresh copies, the caller's latents in place
int decoder_fwd(sgv_engine* e, int B, int train, int mode_fix, const ReconTail* tail = nullptr);        // the decoder, then the loss tail or `tail`
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
