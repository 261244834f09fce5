/*
 * sgvae.h -- C ABI of libsgvae.so: the MI355X-native (gfx950) engine for the SimulGen-VAE
 * training step.
 *
 * The reference (leesihun/SimulGen-VAE) has no FFI/plugin boundary for this path: it sits behind
 * Python classes.  Each entry point below names the reference interface it stands in for
 * (paths relative to the reference root).  The build's own host-side mirror
 * (simulgen-vae_amd/modules/, same names and argument meaning as the reference's
 * modules/ package) binds these symbols through ctypes; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions: every function returns 0 on success or a negative sgv_status; the message of the
 * last failure on the calling thread is sgv_last_error().  No C++ exception crosses the ABI.
 * The caller owns every buffer it passes; the engine owns parameters, optimizer state and
 * workspace.  All device work is enqueued on the hipStream_t given to sgv_create (pass the
 * stream PyTorch-ROCm is using so that it composes with torch tensors); nothing here
 * synchronises the stream except the explicitly host-returning calls (marked [sync]).
 * One engine per process/thread; an engine is not thread-safe.
 *
 * Layouts: "reference layout" means exactly what the reference's tensors hold:
 * activations [B, C, T] row-major fp32, parameters as in its state_dict.  Internally the engine
 * keeps activations channels-last [B, T, C] and weights [tap][Cout][Cin]; conversion happens
 * inside these calls.
 */
#ifndef SGVAE_H
#define SGVAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgv_engine sgv_engine;

typedef enum {
    SGV_OK = 0,
    SGV_ERR_ARG = -1,      /* bad argument / unsupported configuration */
    SGV_ERR_HIP = -2,      /* a HIP runtime call failed */
    SGV_ERR_STATE = -3,    /* call order (e.g. backward before forward) */
    SGV_ERR_NAME = -4,     /* unknown state_dict key */
    SGV_ERR_NOGPU = -5     /* no gfx950 device visible: there is no CPU fallback */
} sgv_status;

enum { SGV_DTYPE_F32 = 0, SGV_DTYPE_BF16 = 1 };
enum { SGV_LOSS_MSE = 0, SGV_LOSS_MAE = 1, SGV_LOSS_SMOOTHL1 = 2, SGV_LOSS_HUBER = 3 };
enum { SGV_MAX_LEVELS = 8 };
enum { SGV_SIDE_ABOVE = 0, SGV_SIDE_BELOW = 1 };   /* sgv_exceedance: a step exceeds its level when the value is above / below it (strict) */
enum { SGV_LAYOUT_TN = 0, SGV_LAYOUT_NT = 1 };   /* sgv_generate output: [B][T][N] (the data set's own order) or [B][N][T] (the reference's tensors) */

/* Mirrors the constructor arguments of modules.VAE_network.VAE (modules/VAE_network.py:60):
 * VAE(latent_dim, hierarchical_dim, num_filter_enc, num_filter_dec, num_node, num_time,
 *     lossfun, batch_size, small).  num_filter_dec is num_filter_enc reversed
 * (SimulGen-VAE.py:219) and is not passed separately. */
typedef struct {
    int32_t latent_dim;
    int32_t hierarchical_dim;
    int32_t n_levels;
    int32_t num_filter_enc[SGV_MAX_LEVELS];
    int32_t num_node;
    int32_t num_time;
    int32_t max_batch;        /* per-GPU batch the workspace is sized for */
    int32_t loss_type;        /* SGV_LOSS_* <- condition.txt Loss_type (SimulGen-VAE.py:208-215) */
    int32_t small;            /* 1 <=> --size small */
    int32_t compute_dtype;    /* SGV_DTYPE_*: storage/MFMA input type of activations and weight copies */
    int32_t flags;            /* bit0: TN GEMM uses scalar LDS fragment reads instead of ds_read_tr */
} sgv_config;

/* Scalars written by forward, in the order VAE.forward returns them (VAE_network.py:117):
 * [0] recon_loss (selected loss fn), [1] kl, [2] kl_2 stage 0, [3] kl_2 stage 1, ...,
 * [1+n_kl] recon_loss_MSE; n_kl = n_levels - 1. */
enum { SGV_MAX_SCALARS = 12 };

const char* sgv_last_error(void);

/* modules/VAE_network.py:60 VAE.__init__ (+ train.py:65,83 model creation / .to(device)). */
int sgv_create(const sgv_config* cfg, void* hip_stream, sgv_engine** out);
int sgv_destroy(sgv_engine* e);

/* nn.Module.state_dict() surface: key names/shapes of the reference (checkpoint row).
 * kind: 0 bias, 1 weight_orig, 2 weight_u, 3 weight_v, 4 GroupNorm weight, 5 GroupNorm bias. */
int sgv_param_count(const sgv_engine* e);
int sgv_param_info(const sgv_engine* e, int index, const char** name, int* ndim, int64_t shape[4],
                   int* kind, int* has_grad);
/* load_state_dict / state_dict(): host fp32 buffers in reference layout.  [sync] */
int sgv_load_state(sgv_engine* e, const char* name, const float* host, size_t count);
int sgv_export_state(sgv_engine* e, const char* name, float* host, size_t count);
/* p.grad of a parameter after sgv_backward (wrt weight_orig, i.e. with the spectral-norm chain
 * rule applied), reference layout; *is_none = 1 for parameters that never get a gradient
 * (train.py:157 `if p.grad is not None`).  The chain rule uses the current weight: read it before the AdamW step moves the
 * weight.  [sync] */
int sgv_export_grad(sgv_engine* e, const char* name, float* host, size_t count, int* is_none);
/* Adam exp_avg / exp_avg_sq of a parameter (torch.optim.AdamW state), reference layout. [sync] */
int sgv_export_adam(sgv_engine* e, const char* name, float* host_m, float* host_v, size_t count);
/* torch.optim.AdamW.load_state_dict for one parameter: the inverse of sgv_export_adam (reference layout in; either pointer may be
 * NULL).  SGV_ERR_NAME for an unknown key, SGV_ERR_ARG for a size mismatch or a parameter without optimizer state -- all three
 * before anything is launched or copied.  [sync] */
int sgv_load_adam(sgv_engine* e, const char* name, const float* host_m, const float* host_v, size_t count);
/* What a training run carries besides its tensors: state[0] = AdamW steps taken (torch's state["step"]; fixes the bias corrections
 * of the next step), state[1] = the noise seed (sgv_seed), state[2] = noise draws consumed (the Philox position of the engine's
 * own reparameterisation noise: every noise tensor the engine drew advanced it by one), state[3] = reserved, 0.  sgv_set_train_state puts all three back and,
 * unlike sgv_seed, keeps the draw position it is given; SGV_ERR_STATE while an AdamW step is open (after sgv_adamw_step_range
 * first=1 / sgv_adamw_bucket_async and before last=1), SGV_ERR_ARG if the reserved slot is not 0. */
int sgv_get_train_state(const sgv_engine* e, uint64_t state[4]);
int sgv_set_train_state(sgv_engine* e, const uint64_t state[4]);

/* Whole-state snapshot / restore for exact resume (the reference saves model.state_dict() once, after the last epoch,
 * modules/train.py:254; its optimizer state is never saved).  ONE flat fp32 buffer in reference layout holds, for every
 * sgv_param_info index in order, the value and then -- where the entry has a gradient -- exp_avg and exp_avg_sq.
 *  - sgv_snapshot_floats: the buffer's size; sgv_snapshot_slice: offset and count (floats) of (index, which), which = 0 value,
 *    1 exp_avg, 2 exp_avg_sq; count 0 for the moments of an entry without optimizer state.  The slice of a key holds exactly what
 *    sgv_export_state / sgv_export_adam return for it.
 *  - sgv_snapshot_begin: on the engine stream, table-driven permute kernels (csrc/engine_ckpt.hip) write the whole state in
 *    reference layout into a device staging buffer (allocated on first use, freed by sgv_destroy, not part of sgv_memory_info);
 *    one device-to-host copy into host_pinned follows on a copy stream the engine owns and has placed on another hardware queue
 *    than the engine stream.  Returns without synchronising: the engine stream may run the next step at once, the staging buffer
 *    holds the state as of this call.  host_pinned must be page-locked (hipHostMalloc / torch pin_memory) and must not be read
 *    before sgv_snapshot_wait.  SGV_ERR_ARG: wrong size or pageable memory; SGV_ERR_STATE: a snapshot is still in flight, or an
 *    AdamW step is open.
 *  - sgv_snapshot_wait: blocks until the copy stream is idle (the engine stream is not waited for).  No snapshot in flight: no-op.
 *  - sgv_restore: host buffer (pinned or not) -> staging -> inverse permute into the parameters and both moment arenas, then the
 *    compute-dtype copies are refreshed and the W^T u partials of the conv weights are rebuilt in the summation order of the tiled
 *    AdamW pass, so that the next training forward computes bit for bit what it computes after an optimizer step.  Pair it with
 *    sgv_set_train_state.  A backward needs a new forward afterwards.  SGV_ERR_STATE as above.  [sync] */
int sgv_snapshot_floats(sgv_engine* e, size_t* total_floats);
int sgv_snapshot_slice(sgv_engine* e, int index, int which, size_t* offset_floats, size_t* count_floats);
int sgv_snapshot_begin(sgv_engine* e, float* host_pinned, size_t floats);
int sgv_snapshot_wait(sgv_engine* e);
int sgv_restore(sgv_engine* e, const float* host, size_t floats);
/* The copy stream of the snapshots (created on first use, never on the engine stream's hardware queue), for a caller that moves
 * results of its own to the host beside the engine's work: order it behind the engine stream with an event, as sgv_snapshot_begin
 * does, and wait for its copies itself (an event or a stream
 * synchronise): sgv_snapshot_wait only waits when a snapshot is in flight.  sgv_destroy drains and destroys the stream. */
int sgv_copy_stream(sgv_engine* e, void** hip_stream);

/* Refresh the compute-dtype weight copies from the fp32 masters after sgv_load_state. */
int sgv_prepare(sgv_engine* e);

/* Batch input.  x_dev: device fp32 [batch, num_node, num_time] (the tensor train.py:142 hands to
 * model(image)); converted to the internal layout/dtype. */
int sgv_set_input(sgv_engine* e, const float* x_dev, int batch);
/* Reparameterisation noise (decoder.py:221 torch.randn_like), device fp32, reference layouts
 * [B,latent], [B,C,T]...; site 0 = top latent, 1.. = decoder stages.  If a site is never set the
 * engine draws it from its Philox stream (sgv_seed). */
int sgv_set_eps(sgv_engine* e, int site, const float* eps_dev, int batch);
int sgv_seed(sgv_engine* e, uint64_t seed);
/* Data-parallel noise ("Philox streams keyed by global sample index so results are world-size-invariant"): sample b
 * of this engine's batch is sample b * world + rank of the global batch (shards are r::world of the shuffled index list).  The
 * engine's own draws then take the Philox counters of that global row, so N ranks with the SAME seed and B / N samples each draw
 * exactly the noise one rank draws for B samples.  Default (0, 1). */
int sgv_set_shard(sgv_engine* e, int rank, int world);
/* Noise of a study that is cut into batches: with first_row = r, sample b of the following decoder passes that draw their noise
 * per call (sgv_generate, sgv_summarize, sgv_score, sgv_project, sgv_temporal, sgv_gram, sgv_exceedance, sgv_cycles) takes row r + b of the streams the call draws from instead of
 * row b.  sgv_forward and sgv_decode are not affected.  A caller that puts the draw position back in front of every batch (sgv_set_train_state) and sets
 * first_row to the index of the batch's first sample gives sample p of the study the noise one call over all samples would give
 * it, whatever the batch size; Surrogate.project does.  The passes that count members themselves (sgv_ensemble, sgv_sobol,
 * sgv_distribution, sgv_regress) ignore it, as do sites whose noise was set (sgv_set_eps).  first_row >= 0; default 0; sgv_seed leaves it alone. */
int sgv_set_draw_row(sgv_engine* e, long first_row);
/* Engine switches: "write_xhat" (materialise the reconstruction in training forwards; default 1),
 * "use_tr" (weight-gradient GEMM reads LDS with ds_read_b64_tr_b16; default 1), "dw_side_stream" (small weight-gradient
 * GEMMs on a second stream; default 1), "vendor_gemm" (removed in round 3: 0 is accepted, 1 is an error -- every GEMM
 * runs on the hand-written kernels; the hipBLASLt comparator lives in tests/micro/vendor, outside this library), "deterministic" (default 1: no
 * floating-point atomics anywhere in the step), "lanes" (second compute lane for the posterior branch of a decoder stage and
 * the xs heads; schedule only, results are bitwise the same; default 1), "fused_stages" (small Conv1d -> GroupNorm -> GELU
 * stages in one launch, csrc/convgn.hip; default 1, 0: GEMM + split-K combine + GroupNorm kernels),
 * "grad_bf16" (bf16 engines, single-GPU path; default 0, modules/train.py switches it on at world size 1: the weight gradients of
 * the layers whose weight-gradient GEMM is the 256 x 256 kernel reach the optimizer as bf16 -- rounded to nearest even in the
 * GEMM's epilogue, the rounding the data-parallel step's bf16 wire format applies to every weight gradient -- 4 bytes less written
 * and read per parameter; sgv_export_grad / sgv_grad_norm refresh the fp32 arena from the bf16 copy on demand; ignored while a
 * communicator or a bucket callback is registered.  Rule: after any call that exposes or changes the fp32 arena (sgv_scale_grads,
 * sgv_grad_buffer), in any order with sgv_grad_norm / sgv_export_grad, the next AdamW reads exactly the arena's values and
 * sgv_grad_norm / sgv_export_grad agree with them -- both calls refresh the arena first, and AdamW reads the fp32 arena for every
 * layer until the next backward). */
int sgv_set_option(sgv_engine* e, const char* key, int value);

/* VAE.forward (VAE_network.py:79-121) on the current input.  train != 0: spectral-norm power
 * iteration runs (model.train()); mode_fix != 0: Decoder.forward(mode="fix") (decoder.py:209-210).
 * scalars_host (may be NULL): SGV_MAX_SCALARS floats, filled after a stream sync.  [sync if given] */
int sgv_forward(sgv_engine* e, int train, int mode_fix, float* scalars_host);
/* Decoder.forward(z, xs, mode) from caller-supplied latents (utils.py:499, latent_conditioner_e2e.py:371,
 * reconstruction_evaluator.py:174): z_dev fp32 [B,latent], xs_dev fp32 [n_levels-1][B,hier] in the list
 * order Encoder.forward returns; eval-mode spectral norm.  Scalars as sgv_forward (the loss entries compare
 * against whatever input is current and are meaningless without one).  Result via sgv_get_xhat.  xs_dev == NULL is SGV_ERR_ARG
 * before anything is enqueued. */
int sgv_decode(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, float* scalars_host);
/* Decoder.forward(z, xs, mode) as sgv_decode, but the reconstruction leaves the engine as a physical-unit field:
 * out_dev fp32, layout SGV_LAYOUT_TN [B][T][N] or SGV_LAYOUT_NT [B][N][T]; scale_dev / min_dev fp32 [N] on the device
 * (MinMaxScaler.scale_ / .min_ of data_scaler).  No loss is computed, x_in is not read, x_hat is not stored.
 * One streaming kernel behind the recon head's convolution and statistics computes
 * (tanh(GroupNorm(y)) - min_n) / scale_n in fp32 and stores it straight into out_dev (16-byte aligned): no compute-dtype
 * rounding of the prediction on a bf16 engine.  Argument checks of sgv_decode, plus SGV_ERR_ARG for a NULL pointer or an unknown
 * layout, before anything is enqueued.  Synchronises nothing.  Afterwards there is no forward pass to read from:
 * sgv_get_xhat / sgv_get_activation / sgv_backward answer SGV_ERR_STATE until the next sgv_forward / sgv_decode. */
int sgv_generate(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix,
                 const float* scale_dev, const float* min_dev, int layout, float* out_dev);
/* Summaries of the field sgv_generate would write, without writing it.  Device pointers, each optional (NULL = not computed),
 * at least one required; node_* 16-byte aligned, frame_* 8-byte, probes 4-byte:
 *   node_stats  fp32  [B][3][N]  per sample and node: max over t, min over t, mean over t (fp32 sum, one division by T)
 *   node_when   int32 [B][2][N]  t of the max, t of the min; the smallest t on a tie
 *   frame_stats fp32  [B][T][2]  per sample and time step: max over the nodes, min over the nodes
 *   frame_where int32 [B][T][2]  node of the max, of the min; the smallest node on a tie
 *   probes      fp32  [B][T][K]  the field at the K nodes of sgv_set_probes
 * Every value compared is the descaled one, (tanh(GroupNorm(y)) - min_n) / scale_n, bit for bit what sgv_generate stores. */
typedef struct {
    float* node_stats;
    int32_t* node_when;
    float* frame_stats;
    int32_t* frame_where;
    float* probes;
} sgv_summary_out;
/* The probe nodes of sgv_summarize: count indices in [0, num_node) on the host, 0 <= count <= 4096 (0 clears the list;
 * duplicates allowed, order kept).  Checked here, SGV_ERR_ARG names the first offending position; the copy into the engine's
 * device buffer is enqueued on the engine stream from a copy of the list the engine keeps (nodes_host may be reused on return;
 * replacing an earlier list waits for the engine stream once, so that its upload has left that copy). */
int sgv_set_probes(sgv_engine* e, const int32_t* nodes_host, int count);
/* Decoder.forward(z, xs, mode) as sgv_generate (same arguments, same checks), followed by the summary pass in place of the
 * field: no atomics, every reduction in a fixed order, two calls on the same inputs are bitwise equal; the frame partials live
 * in the engine's workspace, nothing is allocated.  SGV_ERR_ARG before anything is enqueued: out NULL, all five outputs NULL,
 * probes asked for with no probe list set, a misaligned pointer.  Synchronises nothing.  Afterwards there is no forward pass to
 * read from, as after sgv_generate. */
int sgv_summarize(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix,
                  const float* scale_dev, const float* min_dev, const sgv_summary_out* out);
/* The error of the field sgv_generate would write against held-out fields, e[b][t][n] = field - truth, reduced by the pass that
 * would store the field; neither the field nor e is stored.  Device pointers, each optional (NULL = not computed), at least one
 * required; node_* 16-byte aligned, frame_* 4-byte:
 *   node_err    fp32  [B][3][N]  per sample and node: max over t of |e|, mean over t of e (the bias), mean over t of e^2
 *                                (fp32 sums, one division by T each)
 *   node_when   int32 [B][N]     t of the largest |e|; the smallest t on a tie
 *   frame_err   fp32  [B][T][3]  per sample and time step: max over the nodes of |e|, mean over the nodes of e^2, mean over the
 *                                nodes of truth^2 (fp32 sums inside a block of 512 nodes, combined in fp64, one division by N):
 *                                sqrt(sum_t [1] / sum_t [2]) is the relative L2 error, without reading the truth again
 *   frame_where int32 [B][T]     node of the largest |e|; the smallest node on a tie
 * e is one fp32 subtraction of the value sgv_generate stores: on the same inputs, the field minus the truth bit for bit. */
typedef struct {
    float* node_err;
    int32_t* node_when;
    float* frame_err;
    int32_t* frame_where;
} sgv_score_out;
/* Decoder.forward(z, xs, mode) as sgv_summarize (same arguments, same checks), followed by the error pass against truth_dev:
 * fp32 [B][T][N], dense, in physical units (the data set's own order, SGV_LAYOUT_TN of sgv_generate), 16-byte aligned.  truth
 * must be finite; it is not checked: a NaN poisons the sums it enters and loses every comparison, so a maximum may then be one
 * of the other elements.  No atomics, every reduction in a fixed order, two calls on the same inputs are bitwise equal; the
 * frame partials live in the engine's workspace, nothing is allocated.  SGV_ERR_ARG before anything is enqueued: e, z_dev,
 * scale_dev, min_dev, truth_dev or out NULL, all four outputs NULL, a misaligned pointer, the checks of sgv_decode.
 * Synchronises nothing.  Afterwards there is no forward pass to read from, as after sgv_generate. */
int sgv_score(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
              const float* min_dev, const float* truth_dev, const sgv_score_out* out);
/* Running statistics over many generated fields per (time step, node), the reduction along the batch axis: what a Monte-Carlo or
 * design-space study keeps of thousands of draws.  Device pointers, every array dense [T][N] and 16-byte aligned (limit: [N],
 * 4-byte aligned); three groups, each given completely or not at all (all NULL), at least one required:
 *   moments  mean, m2  fp32   Welford's running mean and sum of squared deviations: variance = m2 / count
 *   extrema  max, min  fp32   the envelope;  arg_max, arg_min int32: the index of the member that produced it, the earliest on a tie
 *   exceed   limit     fp32 [N] (input, physical units);  exceed int32: the number of members with field > limit[n] (strict)
 * The state belongs to the caller and persists across calls: the kernel reads, updates and writes it in place. */
typedef struct {
    float* mean;
    float* m2;
    float* max;
    float* min;
    int32_t* arg_max;
    int32_t* arg_min;
    const float* limit;
    int32_t* exceed;
} sgv_ensemble_state;
/* Decoder.forward(z, xs, mode) as sgv_summarize (same arguments, same checks), followed by the ensemble pass: sample b of the
 * batch is member count_before + b, and the value sgv_generate would store for it (SGV_LAYOUT_TN) is merged into *st, members in
 * ascending order, all in fp32 with every operation rounded on its own (k = index + 1, r = 1.0f / k, d = x - mean,
 * mean += d * r, m2 += d * (x - mean); strict comparisons for the extrema and the limit).  With count_before == 0 the state is
 * not read: it starts empty.  The result does not depend on where batch boundaries fall: any cut of the same members into calls
 * gives the same bits.  That holds for the noise too: where the caller has not set it (sgv_set_eps), the decoder's noise of a
 * member is a function of (seed, member index, site) alone -- the rows count_before + b of the streams the first call after
 * sgv_seed draws from, so a single call with count_before == 0 right after sgv_seed sees the noise sgv_generate would -- and the
 * engine's draw position is left where it is.  No atomics, no workspace, nothing allocated.  SGV_ERR_ARG before anything is enqueued: e, z_dev,
 * scale_dev, min_dev or st NULL, no group or half a group, a misaligned pointer, count_before < 0 or count_before + batch > 2^24,
 * the checks of sgv_decode.  Synchronises nothing.  Afterwards there is no forward pass to read from, as after sgv_generate. */
int sgv_ensemble(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                 const float* min_dev, long count_before, const sgv_ensemble_state* st);
/* The running sums of a variance-based sensitivity study (Sobol indices by Jansen's estimators) per (time step, node).  Device
 * pointers, 16-byte aligned, dense: mean, m2 fp32 [T][N] (Welford over the A and B members); first_sq, total_sq fp32 [d][T][N],
 * d = n_params (sums of squared differences per parameter).  mean and m2 are required and at least one of first_sq, total_sq.
 * The state belongs to the caller and persists across calls: the kernel reads, updates and writes it in place.  With n base
 * samples in it: var = m2 / (2 n), S_i = 1 - first_sq[i] / (2 n var), ST_i = total_sq[i] / (2 n var). */
typedef struct { float* mean; float* m2; float* first_sq; float* total_sq; } sgv_sobol_state;
/* Decoder.forward(z, xs, mode) as sgv_summarize (same arguments, same checks), followed by the Sobol pass.  The batch holds whole
 * blocks of n_params + 2 members in this order: A_j, B_j, AB_1_j .. AB_d_j, where AB_i_j is base sample A_j with the inputs of
 * parameter i taken from B_j; block j of the call is base sample blocks_before + j.  With x the value sgv_generate would store
 * (SGV_LAYOUT_TN), all in fp32 and every operation rounded on its own, j ascending: Welford's update of mean / m2 with A_j
 * (k = 2 j + 1) and then B_j (k = 2 j + 2), r = 1.0f / k, d = x - mean, mean += d * r, m2 += d * (x - mean); for every parameter
 * e = xB - xAB_i, first_sq[i] += e * e and e = xA - xAB_i, total_sq[i] += e * e.  With blocks_before == 0 the state is not read.
 * Any cut of the same blocks into calls gives the same bits, the decoder's noise included: it follows the member's index
 * blocks_before * (n_params + 2) + b by the mechanism of sgv_ensemble, and the draw position is left where it is.  No atomics, no
 * workspace, nothing allocated.  SGV_ERR_ARG before anything is enqueued: e, z_dev, scale_dev, min_dev or st NULL, mean or m2
 * missing, neither first_sq nor total_sq, a misaligned pointer, n_params outside [1, 30], batch no multiple of n_params + 2,
 * blocks_before < 0 or 2 (blocks_before + blocks) > 2^24, the checks of sgv_decode.  Synchronises nothing.  Afterwards there is no
 * forward pass to read from, as after sgv_generate. */
int sgv_sobol(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
              const float* min_dev, int n_params, long blocks_before, const sgv_sobol_state* st);
/* The empirical distribution of many generated fields per (time step, node): a histogram of K = bins uniform bins, 2 <= K <= 64,
 * between bounds the caller gives -- in a study, the envelope (min, max) an extrema pass of sgv_ensemble found over the same members.
 * Device pointers, dense, 16-byte aligned: lo, hi fp32 [T][N] (inputs, hi >= lo, finite: not checked); counts int32 [K + 2][T][N]:
 * row 0 counts the members below lo, rows 1 .. K are the bins, row K + 1 counts the members above hi.  The state belongs to the
 * caller and persists across calls: the kernel only ever adds to counts, so a new state must be zeroed by the caller. */
typedef struct { const float* lo; const float* hi; int32_t* counts; int bins; } sgv_distribution_state;
/* Decoder.forward(z, xs, mode) as sgv_summarize (same arguments, same checks), followed by the distribution pass: with x the value
 * sgv_generate would store for a sample (SGV_LAYOUT_TN), all in fp32 and every operation rounded on its own,
 *   invw = hi > lo ? (float)K / (hi - lo) : 0.0f
 *   row  = x < lo ? 0 : x > hi ? K + 1 : 1 + min((int)((x - lo) * invw), K - 1);    counts[row][t][n] += 1
 * so x == hi lands in the last bin and, where hi == lo, x == lo in bin 1; a NaN is counted in some row, which one is not specified.
 * The columns of counts sum to the number of members.  Integer counts do not depend on the order of the members: any cut of the same
 * members into calls gives the same bits.  Sample b of the batch is member count_before + b, which places it in the noise streams by
 * the mechanism of sgv_ensemble -- it is bit for bit the member sgv_ensemble saw at that index, so with lo / hi the extrema of an
 * ensemble pass over the same members nothing falls outside -- and leaves the draw position where it is; count_before does not
 * decide whether the state is read: it always is.  No atomics, no workspace, nothing allocated.  SGV_ERR_ARG before anything is
 * enqueued: e, z_dev, scale_dev, min_dev or st NULL, lo, hi or counts NULL, bins outside [2, 64], a misaligned pointer,
 * count_before < 0 or count_before + batch > 2^24, the checks of sgv_decode.  Synchronises nothing.  Afterwards there is no forward
 * pass to read from, as after sgv_generate. */
int sgv_distribution(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                     const float* min_dev, long count_before, const sgv_distribution_state* st);
/* The running state of a linear response surface of the field on K = n_cov covariates per member, 1 <= K <= 32, per (time step,
 * node).  Device pointers, dense, 16-byte aligned: mean, m2 fp32 [T][N] (Welford, exactly the moments of sgv_ensemble_state);
 * comoment fp32 [K][T][N]: sum over the members of (x - xbar)(y_i - ybar_i), x the field and y_i covariate i.  All three are
 * required.  The state belongs to the caller and persists across calls: the kernel reads, updates and writes it in place. */
typedef struct { float* mean; float* m2; float* comoment; } sgv_regress_state;
/* Decoder.forward(z, xs, mode) as sgv_summarize (same arguments, same checks), followed by the regression pass: sample b of the
 * batch is member m = count_before + b, k = m + 1, and with x the value sgv_generate would store for it (SGV_LAYOUT_TN), members
 * in ascending order, all in fp32 and every operation rounded on its own,
 *   d = x - mean;  mean = mean + d * (1.0f / (float)k);  m2 = m2 + d * (x - mean);  comoment[i] = comoment[i] + d * w[b][i]
 * for i = 0 .. n_cov - 1.  weights_dev, fp32 [batch][n_cov] on the device (4-byte aligned), are the centred covariates, which the
 * caller forms member by member in float64: ybar = ybar + (y_m - ybar) / k, w[b][:] = (float)(y_m - ybar), the running mean
 * including member m (the updating identity C_n = C_n-1 + (x_n - xbar_n-1)(y_n - ybar_n)).  With count_before == 0 the state is
 * not read: it starts empty.  Any cut of the same members into calls gives the same bits, the decoder's noise included: it follows
 * the member index by the mechanism of sgv_ensemble, and the draw position is left where it is.  No atomics, no workspace, nothing
 * allocated.  SGV_ERR_ARG before anything is enqueued: e, z_dev, scale_dev, min_dev, weights_dev or st NULL, mean, m2 or comoment
 * NULL, n_cov outside [1, 32], a misaligned pointer, count_before < 0 or count_before + batch > 2^24, the checks of sgv_decode.
 * Synchronises nothing.  Afterwards there is no forward pass to read from, as after sgv_generate. */
int sgv_regress(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                const float* min_dev, int n_cov, const float* weights_dev, long count_before, const sgv_regress_state* st);
/* Decoder.forward(z, xs, mode) as sgv_summarize (same arguments, same checks), followed by the project pass: n_func = R linear
 * functionals of the field, 1 <= R <= 32, the field itself never stored.  weights_dev fp32 [R][N] dense on the device, 16-byte
 * aligned; out_dev fp32 [batch][T][R] on the device, 4-byte aligned:
 *   out[b][t][r] = sum over n of weights[r][n] * x[b][t][n],  x the value sgv_generate would store (SGV_LAYOUT_TN).
 * fp32 fused multiply-adds in a fixed order inside a fixed share of the mesh, the shares combined in ascending order in fp64 and
 * rounded to fp32 once; no atomics.  out[b][t][r] depends on sample b, row t and weight row r alone, so any cut of the conditions
 * into batches, any R and any order of the rows give the same bits.  The partial sums lie in the engine's workspace (sized at
 * sgv_prepare); nothing is allocated.  SGV_ERR_ARG before anything is enqueued: e, z_dev, scale_dev, min_dev, weights_dev or
 * out_dev NULL, n_func outside [1, 32], a misaligned pointer, the checks of sgv_decode.  Synchronises nothing.  Afterwards there
 * is no forward pass to read from, as after sgv_generate. */
int sgv_project(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                const float* min_dev, const float* weights_dev, int n_func, float* out_dev);
/* Decoder.forward(z, xs, mode) as sgv_summarize (same arguments, same checks), followed by the temporal pass: n_func = R linear
 * functionals of the field over TIME, 1 <= R <= 32, the field itself never stored.  weights_dev fp32 [R][T] dense on the device,
 * 4-byte aligned; out_dev fp32 [batch][R][N] on the device, 16-byte aligned (its rows are written 32 bytes at a time):
 *   out[b][r][n] = sum over t of weights[r][t] * x[b][t][n],  x the value sgv_generate would store (SGV_LAYOUT_TN).
 * One fp32 fused multiply-add chain per output over t ascending, on the matrix cores; no partial sums, no atomics.  out[b][r][n]
 * depends on sample b, weight row r and node n alone, so any cut of the conditions into batches, any R and any order of the rows
 * give the same bits.  A transposed copy of the weights lies in the engine's workspace (sized at sgv_prepare); nothing is
 * allocated.  SGV_ERR_ARG before anything is enqueued: e, z_dev, scale_dev, min_dev, weights_dev or out_dev NULL, n_func outside
 * [1, 32], a misaligned pointer, the checks of sgv_decode.  Synchronises nothing.  Afterwards there is no forward pass to read
 * from, as after sgv_generate. */
int sgv_temporal(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                 const float* min_dev, const float* weights_dev, int n_func, float* out_dev);
/* Decoder.forward(z, xs, mode) as sgv_summarize (same arguments, same checks), followed by the Gram pass: the temporal Gram matrix of
 * the field per sample, the field itself never stored.  node_weights_dev_or_NULL = w and offset_dev_or_NULL = m fp32 [N] on the
 * device, 16-byte aligned, NULL for w = 1 / m = 0 (arrays of ones / zeros give the same bits); out_dev fp32 [batch][T][T] dense on the
 * device, 4-byte aligned:
 *   out[b][t][t'] = sum over n of w[n] * (x[b][t][n] - m[n]) * (x[b][t'][n] - m[n]),  x the value sgv_generate would store.
 * num_time <= 256 (SGV_MAX_GRAM_T).  x - m is rounded once to fp32 and is both operands of the matrix cores' fp32 multiply-add; for
 * t <= t' the element is the chain of fl(w[n] d[t][n]) * d[t'][n] (the smaller time index carries the weight) over blocks of 6144
 * nodes, the blocks added in ascending order in fp64 and rounded once, and (t', t) is its copy: out is bitwise symmetric, its
 * diagonal is >= 0 for w >= 0, and out[b] depends on sample b alone, so any cut of the conditions into batches gives the same bits.
 * The per-block partials lie in the engine's workspace (sized at sgv_create when num_time is within the limit); nothing is allocated,
 * no atomics.  The entries of w and m are not looked at: a negative weight is taken as it is.  SGV_ERR_ARG before anything is
 * enqueued: e, z_dev, scale_dev, min_dev or out_dev NULL, num_time > 256, a misaligned pointer, the checks of sgv_decode.
 * Synchronises nothing.  Afterwards there is no forward pass to read from, as after sgv_generate. */
int sgv_gram(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
             const float* min_dev, const float* node_weights_dev_or_NULL, const float* offset_dev_or_NULL, float* out_dev);
/* Decoder.forward(z, xs, mode) as sgv_summarize (same arguments, same checks), followed by the exceedance pass: the level-crossing
 * statistics of every node's time history against n_level = L levels per node, 1 <= L <= 4, the field itself never stored.
 * levels_dev fp32 [L][N] dense on the device, 4-byte aligned; side SGV_SIDE_ABOVE or SGV_SIDE_BELOW.  With x[t] the value
 * sgv_generate would store at (b, t, n) (SGV_LAYOUT_TN), lam = levels[l][n] and e[t] = (x[t] > lam) above, (x[t] < lam) below --
 * strict, on the descaled value, so negative scales are fine; a NaN exceeds nothing:
 *   stats[b][0][l][n] = count, the number of t with e[t];  [1] first, the smallest such t, -1 if none;  [2] last, the largest, -1 if
 *   none;  [3] longest, the length of the longest run of consecutive exceeding steps, 0 if none;  [4] runs, the number of t with
 *   e[t] and (t == 0 or not e[t - 1]), i.e. of maximal runs
 *   excess[b][l][n] = s after: s = +0.0; for t ascending, where e[t]: s = fl(s + d[t]) with d[t] = fl(x[t] - lam) above and
 *   fl(lam - x[t]) below, the difference of the stored value rounded on its own; exactly +0.0 where nothing exceeds
 * stats_dev_or_NULL int32 [batch][5][L][N] and excess_dev_or_NULL fp32 [batch][L][N] on the device, 16-byte aligned; either may be
 * NULL, not both.  num_time <= 65535.  Every output depends on its sample, its level row and its node alone, so any cut of the
 * conditions into batches, any L, any order of the levels and either output alone give the same bits.  No workspace, no atomics.
 * SGV_ERR_ARG before anything is enqueued: e, z_dev, scale_dev, min_dev or levels_dev NULL, both outputs NULL, n_level outside
 * [1, 4], an unknown side, num_time > 65535, a misaligned pointer, the checks of sgv_decode.  Synchronises nothing.  Afterwards
 * there is no forward pass to read from, as after sgv_generate. */
int sgv_exceedance(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                   const float* min_dev, const float* levels_dev, int n_level, int side, int32_t* stats_dev_or_NULL,
                   float* excess_dev_or_NULL);
/* The outputs of sgv_cycles, device pointers, 16-byte aligned, in two groups; a group is given whole or left NULL, at least one is
 * required.  x[t] is the value sgv_generate would store at (b, t, n) (SGV_LAYOUT_TN), h = gate[n] >= 0, m = exponent, fl() one fp32
 * rounding; every difference is formed from the stored value and rounded on its own, every product of the power and every
 * accumulation likewise (nothing is contracted into an fma); all comparisons are strict.
 * The turns -- ASTM E1049 simple-range counting behind a hysteresis gate, a machine of three states per node, dir in {0, +1, -1},
 * from dir = 0, hi = lo = x[0]; for t = 1 .. T - 1, x = x[t]:
 *   dir = 0:  fl(x - lo) > h: a valley is confirmed: last = lo, cand = x, dir = +1, reversals += 1; else fl(hi - x) > h: a peak:
 *             last = hi, cand = x, dir = -1, reversals += 1; else hi = max(hi, x), lo = min(lo, x).  The first turning point
 *             carries no range.
 *   dir = +1: x > cand: cand = x; else fl(cand - x) > h: a peak is confirmed: R = fl(cand - last) is counted, last = cand, cand = x,
 *             dir = -1, reversals += 1.
 *   dir = -1: x < cand: cand = x; else fl(x - cand) > h: a valley: R = fl(last - cand) is counted, last = cand, cand = x, dir = +1,
 *             reversals += 1.
 *   counted:  range_sum = fl(range_sum + R); range_max = R if R > range_max; damage = fl(damage + P) with P = R, then m - 1 times
 *             P = fl(P * R); all three from +0.0.
 *   open, the unfinished excursion: fl(hi - lo) at dir = 0, fl(cand - last) at +1, fl(last - cand) at -1.
 *   reversals int32 [B][N];  ranges fp32 [B][4][N] = range_sum, range_max, damage, open.  The counted ranges (half cycles) number
 *   max(reversals - 1, 0).  With h = 0 every strict local extremum of the history with its plateaus collapsed is a turning point; a
 *   constant history gives 0 and +0.0 throughout; a gate above the node's peak-to-peak gives reversals 0 and open = fl(max - min).
 * The rates -- for t = 1 .. T - 1, r[t] = fl(x[t] - x[t-1]):
 *   rate_when int32 [B][2][N] = rise_when, fall_when;  rates fp32 [B][3][N] = rise, fall, path: rise = max r[t], fall = min r[t],
 *   the steps those of each, the smallest on a tie (strict > / < updates starting from r[1]); path = s after s = +0.0;
 *   s = fl(s + |r[t]|), t ascending.  T = 1: rise = fall = path = +0.0 and both steps -1. */
typedef struct {
    int32_t* reversals;
    float* ranges;
    int32_t* rate_when;
    float* rates;
} sgv_cycles_out;
/* Decoder.forward(z, xs, mode) as sgv_summarize (same arguments, same checks), followed by the cycles pass: the load cycles and
 * the rates of every node's time history (sgv_cycles_out), the field itself never stored.  gate_dev fp32 [N] on the device, 4-byte
 * aligned, >= 0 (not checked: a negative or NaN gate is the caller's); exponent an integer in [1, 8].  num_time <= 65535.  Every
 * output depends on its sample and its node alone, so any cut of the conditions into batches and either group alone give the same
 * bits; the exponent shows in damage alone.  No workspace, no atomics.  SGV_ERR_ARG before anything is enqueued: e, z_dev,
 * scale_dev, min_dev, gate_dev or out NULL, no group, half a group, an exponent outside [1, 8], num_time > 65535, a misaligned
 * pointer, the checks of sgv_decode.  Synchronises nothing.  Afterwards there is no forward pass to read from, as after
 * sgv_generate. */
int sgv_cycles(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
               const float* min_dev, const float* gate_dev, int exponent, const sgv_cycles_out* out);
/* Encoder.forward only (utils.py:492): mu, log_var [B,latent], xs [n_levels-1][B,hier] to host. [sync] */
int sgv_encode(sgv_engine* e, float* mu_host, float* logvar_host, float* xs_host);
/* Reconstruction of the last forward, reference layout [B, num_node, num_time] fp32 on device. */
int sgv_get_xhat(sgv_engine* e, float* xhat_dev);
/* Named intermediate of the last forward as fp32 reference layout on host (parity tests):
 * "enc_h<i>", "dec_out<i>", "zmap<i>", "mu", "log_var", "z", "xs<i>", "x_hat"; "x_in" = the input batch as
 * held by the engine after sgv_set_input / sgv_augment_collate (readable before any forward).  [sync] */
int sgv_get_activation(sgv_engine* e, const char* name, float* host, size_t count);

/* loss = alpha*recon + beta*sum(kl); loss.backward() (train.py:144-153). */
int sgv_backward(sgv_engine* e, float alpha, float beta);
/* sgv_backward followed by sgv_adamw_step(lr) (train.py:153-168 without the logging in between), single-GPU path:
 * the AdamW pass of each conv-weight bucket is started on a second stream as soon as that bucket's gradients are
 * final and runs under the remaining backward kernels (HBM-bound optimizer next to MFMA-bound GEMMs).  Same
 * results as the two separate calls; gradients stay readable (sgv_export_grad) afterwards.  Not valid while a
 * bucket callback is registered. */
int sgv_backward_step(sgv_engine* e, float alpha, float beta, float lr);
/* Callback invoked from inside sgv_backward (host side, after the kernels producing a gradient
 * bucket have been enqueued) so the caller can overlap its all-reduce of
 * [sgv_grad_buffer + offset, +count) with the rest of backward.  Weight buckets arrive in
 * reverse-autograd order; the small last-numbered bucket (biases, GroupNorm affine, <G,W> scalars) is released
 * just before the first encoder layer's weight bucket, which is always the final callback. */
typedef void (*sgv_bucket_cb)(void* user, int bucket, size_t offset_elems, size_t count_elems);
int sgv_set_bucket_callback(sgv_engine* e, sgv_bucket_cb cb, void* user);
/* The flat fp32 gradient arena (device) of all parameters that receive gradients; what the
 * data-parallel all-reduce (RCCL via torch.distributed) operates on. */
int sgv_grad_buffer(sgv_engine* e, float** dev_ptr, size_t* count_elems);
int sgv_scale_grads(sgv_engine* e, float factor);

/* Native RCCL path (sgv_allreduce_grads(rcclComm_t); 8(e): one collective per step, overlapped with the
 * decoder backward).  RCCL is resolved at run time (dlopen of librccl.so.1, i.e. the copy already loaded in the process
 * if there is one), so the library has no link-time dependency on it.
 *  - sgv_rccl_unique_id / sgv_rccl_comm_init / sgv_rccl_comm_destroy: ncclGetUniqueId (128 bytes, rank 0; the caller
 *    broadcasts them), ncclCommInitRank, ncclCommDestroy -- so a host needs no RCCL binding of its own.
 *  - sgv_allreduce_grads: mean all-reduce (ncclAvg, fp32) of the whole gradient arena, bucket by bucket in backward
 *    order, on comm_stream after everything enqueued so far on the engine stream; the engine stream then waits for it.
 *  - sgv_set_rccl: register (comm, comm_stream) with the engine (NULL comm unregisters).  While registered,
 *    sgv_backward issues each bucket's all-reduce itself as soon as the kernels producing it are enqueued (no host
 *    callback), sgv_adamw_step / sgv_adamw_step_range make the engine stream wait for exactly the buckets they touch, and
 *    sgv_adamw_step updates every layer whose bucket has arrived while the last (first-encoder-layer) bucket is in flight;
 *    sgv_backward_step = sgv_backward + that sgv_adamw_step.  Mutually exclusive with sgv_set_bucket_callback. */
int sgv_rccl_unique_id(void* id128);
/* Local checks a host runs BEFORE it enters any collective step of the set-up, so that every rank can agree (through its own
 * process group) on the path it takes: sgv_rccl_probe resolves librccl and its entry points in this process (no communication);
 * sgv_rccl_comm_count = ncclCommCount of a communicator made by sgv_rccl_comm_init (what the bench line reports as rccl_nranks). */
int sgv_rccl_probe(void);
int sgv_rccl_comm_count(void* comm, int* nranks);
/* In-place mean all-reduce (ncclAvg) of `count` fp32 / bf16 elements on `stream`: the host's first collective on a new
 * communicator (a bounded self-test before the first training step), and a building block for hosts without an RCCL binding. */
int sgv_rccl_allreduce(void* comm, void* dev_buf, size_t count, int dtype, void* stream);
int sgv_rccl_comm_init(void** comm_out, int nranks, const void* id128, int rank);
int sgv_rccl_comm_destroy(void* comm);
int sgv_allreduce_grads(sgv_engine* e, void* rccl_comm, void* comm_stream);
int sgv_set_rccl(sgv_engine* e, void* rccl_comm, void* comm_stream);
/* A communication stream owned by the engine for sgv_set_rccl, chosen so that it shares its hardware queue with neither the engine
 * stream nor the engine's weight-gradient / second-lane streams (the HIP runtime maps streams onto four hardware queues; kernels of
 * two streams on one queue never overlap, and a collective on the engine stream's queue would serialise with backward). */
int sgv_comm_stream(sgv_engine* e, void** hip_stream);

/* Gradient 2-norm as train.py:156-161 computes it.  [sync] */
int sgv_grad_norm(sgv_engine* e, double* out);
/* torch.optim.AdamW(lr).step() with its defaults (train.py:92,168): betas (0.9, 0.999),
 * eps 1e-8, weight_decay 0.01; skips parameters without gradient.  Also refreshes the
 * compute-dtype weight copies. */
int sgv_adamw_step(sgv_engine* e, float lr);
/* The same step restricted to the parameters whose gradients live in buckets [bucket_lo, bucket_hi) (bucket
 * numbering of sgv_set_bucket_callback; the last bucket holds biases, GroupNorm affine and the spectral-norm
 * <G,W> scalars, which every conv weight's update needs).  Lets a data-parallel caller update the layers whose
 * all-reduce has finished while the last, largest bucket is still in flight.  first=1 on the first call of an
 * optimisation step, last=1 on the final one; every bucket must be covered exactly once per step. */
int sgv_adamw_step_range(sgv_engine* e, float lr, int bucket_lo, int bucket_hi, int first, int last);
int sgv_bucket_count(const sgv_engine* e);
/* Optimizer overlap for the data-parallel step (the reference's loop is optimizer.step() after backward, modules/train.py:153-168;
 * torch's DDP hides the all-reduce under backward, this also hides the update).  The <G,W> scalars of the conv layers of weight
 * bucket b sit together at the head of the small bucket's range: sgv_bucket_dots returns that sub-range, and they are final when
 * the bucket's callback fires.  A caller that averages [offset, +count) together with bucket b -- and leaves the union of those
 * sub-ranges (the first sum-of-counts elements of the small bucket) out of the small bucket's collective -- may then call
 * sgv_adamw_bucket_async(lr, b) as soon as it has made the optimizer stream (sgv_opt_stream) wait for both collectives: the
 * bucket's conv weights are updated on that stream under the rest of backward.  The sgv_adamw_step_range calls that close the
 * step (same bucket coverage as without the overlap) skip what was updated ahead, and last=1 joins the optimizer stream.
 * With sgv_set_rccl, sgv_backward_step does all of this by itself (option "ddp_early_adamw", default 1).  Linear-head weights,
 * biases and GroupNorm affine are updated by the closing calls: their <G,W> scalars are computed at the end of backward. */
int sgv_bucket_dots(const sgv_engine* e, int bucket, size_t* offset_elems, size_t* count_elems);
/* Where a released bucket is complete.  By default on the engine stream: before the callback the engine stream joins the
 * weight-gradient side stream and, for the bf16 wire format, runs the pack pass.  With sgv_set_option("wire_stream", 1) both
 * happen on the wire stream instead (sgv_wire_stream): the callback must issue its collective ordered after THAT stream, and
 * backward never waits for the side stream or the pack pass at a release point. */
int sgv_wire_stream(sgv_engine* e, void** hip_stream);
int sgv_opt_stream(sgv_engine* e, void** hip_stream);
int sgv_adamw_bucket_async(sgv_engine* e, float lr, int bucket);
/* Wire format of the data-parallel gradient exchange (the reference's DDP all-reduces fp32 gradients, modules/utils.py:209-238
 * sets the process group up and torch does the rest; this is the build's own choice for bf16 engines).  SGV_DTYPE_F32: the
 * buckets are ranges of the fp32 arena (default).  SGV_DTYPE_BF16: at its fire point every weight bucket is rounded (RNE) into a
 * bf16 copy at the same element offset of the payload buffer; the collective averages THAT range (the bucket callback receives
 * the same offset / count; with sgv_set_rccl the engine issues ncclAllReduce on it), and sgv_adamw_step / _range write it back
 * into the fp32 arena in front of the bucket's update.  The last (small) bucket -- biases, GroupNorm affine, <G,W> scalars --
 * always travels in fp32.  Halves the bytes on the xGMI links (0.80 of 1.61 GB per step for preset 1).
 * sgv_grad_payload_unpack writes back every bucket still packed (use before reading gradients with sgv_grad_norm / sgv_get_grad
 * when no optimiser step follows). */
int sgv_set_grad_payload(sgv_engine* e, int dtype);
int sgv_grad_payload_buffer(sgv_engine* e, void** dev_ptr, size_t* count_elems);
int sgv_grad_payload_unpack(sgv_engine* e);
/* Device memory held by the engine, bytes: out[0] fp32 master parameters, [1] gradient arena, [2] Adam moments, [3] compute-dtype
 * weight copies, [4] activations of forward + backward at max_batch (everything stays resident: the reference's
 * use_checkpointing flag is forced to False in its code, modules/VAE_network.py:68, and no recompute exists here either),
 * [5] split-K / reduction workspaces. */
int sgv_memory_info(const sgv_engine* e, size_t out[6]);
/* Measurement hook for BASELINE configs[3] ("+ grad-checkpoint"; the reference forces use_checkpointing to False,
 * modules/VAE_network.py:68).  With sgv_set_option("recompute_activations", 1) the backward pass regenerates every stage's
 * GroupNorm + GELU output from the stored pre-normalisation map right before the stage's backward (one extra streaming pass per
 * stage; same values, buffers stay allocated): it TIMES what recompute would cost; sgv_recompute_bytes returns the bytes of
 * the maps the last backward regenerated = what a recompute build would not keep resident. */
int sgv_recompute_bytes(const sgv_engine* e, size_t* bytes);
/* Gradient 2-norm accumulated by the AdamW pass(es) of the current step (same value sgv_grad_norm computes in a
 * separate pass).  [sync] */
int sgv_last_grad_norm(sgv_engine* e, double* out);
/* Epoch statistics without a host round trip per step (the reference's loop reads .item() scalars after every step,
 * modules/train.py:156-161,171-174).  sgv_scalars_accumulate: enqueue "add the scalars of the step that has just been
 * enqueued (forward + optimizer) to the device-side accumulator"; sgv_scalars_read: the accumulator, host16 =
 * [sum recon, sum kl, sum kl2_0.., ..., [8] sum mse, [9] sum of gradient norms, [10] steps]; reset != 0 clears it. */
int sgv_scalars_accumulate(sgv_engine* e);
int sgv_scalars_read(sgv_engine* e, double* host16, int reset);

/* AugmentedDataset.__getitem__ x batch + default collate (augmentation.py:43-124) on a dataset
 * resident in HBM in the engine's internal layout: builds the input batch directly.
 * dataset_dev: [P][num_time][num_node] in compute dtype (see sgv_dataset_convert).
 * idx[b]: sample index; noise_seed[b]: 0 = no noise else Philox key; scale[b]: 1.0 = none;
 * mix_idx[b]: -1 = none; lam[b]: mixup weight (already clipped to [0.1,0.9]). */
int sgv_augment_collate(sgv_engine* e, const void* dataset_dev, int batch, const int32_t* idx,
                        const uint64_t* noise_seed, const float* scale, const int32_t* mix_idx,
                        const float* lam);
/* The same batch construction, prefetched (the reference's DataLoader builds batch i + 1 in worker processes while step i
 * runs, modules/data_processing.py + torch DataLoader prefetch; here the GPU builds it beside the step):
 * sgv_augment_stage enqueues the augmentation of the NEXT batch into a second input buffer on a stream of its own -- its
 * kernels are launched from inside the next forward pass, behind the first encoder layer -- and returns at once;
 * sgv_augment_advance makes the staged batch the current input (what sgv_augment_collate does in one call).  Staging again
 * before advancing replaces the staged batch.  The current batch, its forward / backward and sgv_set_input are untouched by a
 * staged one.  sgv_augment_advance without a staged batch: SGV_ERR_STATE.  Same bytes as sgv_augment_collate for the same
 * arguments.  Loop:  stage(0); for i: advance(); stage(i + 1); forward; backward_step. */
int sgv_augment_stage(sgv_engine* e, const void* dataset_dev, int batch, const int32_t* idx,
                      const uint64_t* noise_seed, const float* scale, const int32_t* mix_idx,
                      const float* lam);
int sgv_augment_advance(sgv_engine* e);
/* utils.Dataset.__init__ with load_all (utils.py:41-43): device fp32 [count, num_node, num_time]
 * -> internal [count][num_time][num_node] in compute dtype at dst_dev. */
int sgv_dataset_convert(sgv_engine* e, const float* src_dev, void* dst_dev, int count);
size_t sgv_dataset_sample_bytes(const sgv_engine* e);

/* Input pipeline, stateless.  data_preprocess.data_scaler (data_preprocess.py:65-165) fits
 * sklearn.preprocessing.MinMaxScaler(feature_range=(-0.7, 0.7)) per node on a sample of [num_time x num_param]
 * rows and transforms the whole [P][T][N] array; SimulGen-VAE.py:282 then transposes it for Conv1d.
 * sgv_minmax_fit: per-node min / max (NaNs ignored) over n_rows device rows of n_node floats (accumulate=1 merges
 * into existing values, for chunked feeding) [sync]; sgv_minmax_coeffs: MinMaxScaler's scale_ / min_ (zero ranges
 * handled as sklearn does); sgv_scale_convert: x*scale_+min_ of raw rows written in the engine's resident
 * dataset layout [P][T][N] and compute dtype (raw [P][T][N] rows are already in that order). */
int sgv_minmax_fit(const float* rows_dev, long n_rows, int n_node, float* min_dev, float* max_dev, int accumulate,
                   void* stream);
int sgv_minmax_coeffs(const float* min_dev, const float* max_dev, int n_node, float lo, float hi, float* scale_dev,
                      float* offset_dev, void* stream);
int sgv_scale_convert(int dst_dtype, const float* src_dev, const float* scale_dev, const float* offset_dev,
                      void* dst_dev, long n_rows, int n_node, void* stream);

/* Profiling aid for bench.py: hipEvent-timed duration (total ms and number of launches since the
 * last reset) of a kernel class ("gemm_nt", "gemm_tn"), measured on the engine's own stream. [sync] */
int sgv_kernel_time(sgv_engine* e, const char* which, float* total_ms, int* calls);
int sgv_kernel_time_reset(sgv_engine* e, int enable);   /* 0 off, 1 per class, 2 per (class, layer, shape) */
/* Walk the timer tags recorded since the engine was created: index 0.. until the return value is
 * non-zero.  name receives "class" or "class|layer prefix|M=.. N=.. K=.. taps=.. splitk=..". [sync] */
int sgv_kernel_time_tag(sgv_engine* e, int index, char* name, size_t cap, float* total_ms, int* calls);

/* Low-level kernel entry points, exported for the unit parity tests (tests/test_kernels_gpu.py).
 * All pointers are device pointers; dtype is SGV_DTYPE_*.  [sync] */
int sgv_test_gemm_nt(int dtype, const void* A, const void* W, void* C, const float* bias, const float* scale,
                     const void* addend, int M, int N, int K, int taps, int Tlen, int splitk, int out_f32,
                     void* stream);
/* bf16 128x128 kernel with the GroupNorm-statistics epilogue: sums[(m / Tlen) * (N / Cg) + n / Cg][2] += (sum, sum of squares)
 * of the stored outputs; sums must be zeroed by the caller.  Rejected unless Tlen >= 128, Cg >= 128 and the shape runs on the
 * 128x128 kernel (fewer than 64 K-steps of 32, or N < 256). */
int sgv_test_gemm_nt_stats(const void* A, const void* W, void* C, const float* bias, const void* addend, int M, int N, int K,
                           int taps, int Tlen, int Cg, double* sums, void* stream);
/* Test hook: the fused small Conv1d + GroupNorm(G) + GELU (+ residual) forward kernel (csrc/convgn.hip) on caller-owned device
 * buffers: A [B*T][K] bf16, W [taps][N][K] bf16, y / out / res [B*T][N] bf16, sums [B*G][2] doubles.  Fails for shapes the kernel
 * does not take (T > 208, channels per group not in {16, 32, 64, 80, 128, 160}, K % 32 != 0). */
int sgv_test_conv_gn_fwd(const void* A, const void* W, const float* bias, const float* scale, const void* res, const float* gamma,
                         const float* beta, void* y, void* out, double* sums, int B, int T, int N, int K, int taps, int G, float rscale,
                         void* stream);
/* Test hook: its backward mirror -- input gradient of the upper convolution (A = its dY [B*T][K], W = its transposed tap-flipped
 * weight copy [taps][N][K], optional addend [B*T][N] bf16 added before rounding: the residual path; optional premul x [B*T][N]: the
 * gradient is multiplied by gelu'(x) and rounded again; optional da [B*T][N]: the input gradient itself is stored too) + GroupNorm / GELU backward
 * of the stage below (y, forward sums, gamma, beta, conv bias) in one
 * launch: dy [B*T][N] bf16, sums2 [B*G][2], ptot [B][3][N] (per-sample column totals), cdot_part [B*G]. */
int sgv_test_conv_gn_bwd(const void* A, const void* W, const float* scale, const void* addend, const void* premul, void* da, const void* y,
                         const double* sums, const float* gamma,
                         const float* beta, const float* cbias, void* dy, double* sums2, float* ptot, float* cdot_part, int B, int T,
                         int N, int K, int taps, int G, void* stream);
/* Test hook for the 256x256 persistent implicit-GEMM kernel (csrc/gemm256.hip; replaces the hipBLASLt dispatch of round 1 on
 * the reference call sites modules/decoder.py:117-121, modules/common.py:135-141, modules/encoder.py:34).  bf16 operands.
 * mode 0: the kernel itself with the given split-K; mode 1: the engine's kernel choice (gemm_nt_plan: 256x256 kernel, or
 * 256x256 over the first rows + the 128-row kernels over the rest, or the 128-row kernels alone); *plan_kind reports it.
 * sums != NULL: GroupNorm (sum, sum of squares) per (sample, group of Cg channels), [ceil(M/Tlen)][N/Cg][2] fp64, produced
 * deterministically by the epilogue + a fixed-order finalize.
 * Bits 8-15 of mode choose the work-item order of the 256x256 kernel (0: the launcher's choice, 1..254: row tiles in bands of
 * that many, 255: column-panel-major), bits 16-18 the cache policy of its streams (0: the launcher's choice, 7: default loads and
 * stores, else bit 0 = non-temporal weight loads, bit 1 = sc1 output stores), bits 19-20 its tile shape (0: 256 x 256 with mode 0 /
 * the plan's choice with mode 1, 1: 128 x 512, 2: the plan must not pick 128 x 512), bit 21 the split the engine runs on two
 * streams (M = 128 mod 256, bf16 output: the first M - 128 rows on the 256 x 256 kernel in `splitk` slices, the last 128 rows as a
 * launch of their own of the 128 x 512 tile shape on shifted row pointers; here one after the other on `stream`). */
int sgv_test_gemm_nt256(const void* A, const void* W, void* C, const float* bias, const float* scale, const void* addend, int M, int N,
                        int K, int taps, int Tlen, int splitk, int out_f32, int mode, int Cg, double* sums, int* plan_kind, void* stream);
/* Weight-gradient GEMM test hook.  use_tr: 0 plain LDS reads, 1 the launcher's choice, 2 force the 128x256 two-blocks-per-CU kernel,
 * 3 the same with its persistent walk, 4 force the persistent 256x256 kernel (csrc/gemm256tn.hip), 5 never that kernel, 6 that kernel
 * with its bf16 epilogue (dW is then a bf16 array; splitk 1), 7 that kernel in its work-stealing form (what a data-parallel backward
 * launches while a collective may hold CUs; results bitwise those of 4). */
int sgv_test_gemm_tn(int dtype, const void* A, const void* Bm, float* dW, int M, int N1, int N2, int taps,
                     int Tlen, int splitk, int use_tr, void* stream);
/* Test hook for the stream placement: *overlaps = 1 if kernels of the engine's auxiliary stream `which` (0 second lane, 1 weight-
 * gradient side stream, 2 optimizer stream, 3 the engine's communication stream; 2 and 3 are created by the call if need be) can run
 * while a kernel of the engine stream is running, i.e. the two do not share a hardware queue; -1 if the engine has no such stream. */
int sgv_test_stream_overlap(sgv_engine* e, int which, int* overlaps);
/* Test hook: `blocks` workgroups of `threads` threads and `lds_bytes` of LDS spin for `ticks` of the 100 MHz clock (<= 10 ms) on
 * `stream` -- a stand-in for a collective's resident channel workgroups when measuring how the persistent GEMMs cope. */
int sgv_test_occupy(void* stream, int blocks, int threads, int lds_bytes, long long ticks);
/* Test double for the collective of the engine-issued data-parallel step (sgv_set_rccl with any non-null communicator handle):
 * k != 0 replaces ncclAllReduce by "multiply the range in place by k on the given stream" (fp32 and bf16 ranges; no RCCL is
 * loaded or called), k == 0 restores the library.  With k a power of two a step through the double must leave bitwise the
 * state of a plain step at (k alpha, k beta) if and only if every gradient element and every <G,W> slot went through exactly
 * one collective.  *calls / *elems return (and reset) the number of collectives and of elements since the last call. */
int sgv_test_fake_collective(float k, long* calls, long* elems);

/* Test hooks for the non-GEMM kernels of the step (csrc/ew.hip, csrc/recon_out.hip; tests/test_ew_kernels_gpu.py): caller-owned device buffers in, the
 * launcher the engine calls, then a stream sync.  Maps are channels-last [B*T][ld] of `dtype` (ld >= C, ld % 8 == 0), C % 8 == 0,
 * 1 <= G <= 32, C % G == 0; gamma / beta / dgamma / dbeta / dbias / cbias are [C] fp32, sums / sums2 [B*G][2] fp64.  `work` is a
 * scratch array of work_floats >= sgv_test_gn_workspace_floats(B, T, C) floats.  Bad arguments return SGV_ERR_ARG before any
 * launch.  Optional pointers may be NULL.  Nothing persistent is allocated. */
size_t sgv_test_gn_workspace_floats(int B, int T, int C);
/* out = [res + rscale *] act(GroupNorm(y)), act: 0 none, 1 GELU (erf), 2 tanh, 3 ReLU; sums (written) = (sum, sum of squares)
 * per (sample, group).  *path: 1 = the one-launch slab kernel ran, 0 = statistics + apply. */
int sgv_test_gn_fwd(int dtype, int act, const void* y, long ldy, const void* res, long ldres, float rscale, void* out, long ldout,
                    const float* gamma, const float* beta, double* sums, float* work, size_t work_floats, int B, int T, int C, int G,
                    int* path, void* stream);
/* Backward of out = act(GroupNorm(y)), act in {0, 1, 3}, immediate mode.  With dz = dout * rscale * act'(z) (z the normalised
 * and affine value, xhat the normalised one): dgamma (+)= sum dz xhat, dbeta (+)= sum dz, sums2 = (sum gamma dz, sum gamma dz xhat) per
 * (sample, group), dy = gscale * dL/dy, dbias (+)= column sums of dy, cdot[0] = sum dy * (y - cbias).  accum_affine: += into
 * dgamma / dbeta / dbias instead of =.  *path as above. */
int sgv_test_gn_bwd(int dtype, int act, const void* y, long ldy, const void* dout, long lddout, float rscale, float gscale,
                    const float* gamma, const float* beta, const double* sums, void* dy, long lddy, double* sums2, float* dgamma,
                    float* dbeta, float* dbias, float* cdot, const float* cbias, int accum_affine, float* work, size_t work_floats,
                    int B, int T, int C, int G, int* path, void* stream);
/* Recon head as the engine runs it: statistics of y, then xhat = tanh(GroupNorm(y)) against the target x with loss kind
 * SGV_LOSS_*: loss_sums[2] = (selected loss sum, squared-error sum), xhat optional.  train != 0 also: sums2, the unit-weight
 * unit[3][C] = (dgamma, dbeta, dbias), and the second pass dy = gscale * dL/dy with cdot[0] = sum dy * (y - cbias). */
int sgv_test_recon_loss(int dtype, int train, int loss_type, const void* y, long ldy, const void* x, long ldx, void* xhat, long ldxhat,
                        const float* gamma, const float* beta, double* sums, double* loss_sums, double* sums2, float* unit, float gscale,
                        void* dy, long lddy, float* cdot, const float* cbias, float* work, size_t work_floats, int B, int T, int C,
                        int G, void* stream);
/* The kernel of sgv_generate on caller-owned buffers: statistics of y (ew_gn_stats, groups by the model's rule
 * G = min(8, max(1, C / 4))), then out = (tanh(GroupNorm(y)) - min) / scale as fp32, layout SGV_LAYOUT_TN [B][T][C] or
 * SGV_LAYOUT_NT [B][C][T], dense and 16-byte aligned; sums [B*G][2] fp64 (written), scale / min [C] fp32. */
int sgv_test_recon_physical(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                            const float* scale, const float* min, int layout, float* out, int B, int T, int C, void* stream);
/* The kernels of sgv_summarize on caller-owned buffers: inputs as sgv_test_recon_physical, then the statistics of y and the summary
 * pass into the outputs of `out` (shapes of sgv_summary_out with N = C).  probes_host: n_probes node indices on the host, checked
 * as sgv_set_probes checks them (needed when out->probes is given).  SGV_ERR_ARG, nothing launched: a NULL input, out NULL or
 * all of its outputs NULL, probes without a list, an index outside [0, C), a misaligned pointer. */
int sgv_test_recon_summary(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                           const float* scale, const float* min, const sgv_summary_out* out, const int32_t* probes_host,
                           int n_probes, int B, int T, int C, void* stream);
/* The kernels of sgv_score on caller-owned buffers: inputs as sgv_test_recon_physical plus truth fp32 [B][T][C] (dense, 16-byte
 * aligned), then the statistics of y and the error pass into the outputs of `out` (shapes of sgv_score_out with N = C); the frame
 * workspace is allocated and freed here.  SGV_ERR_ARG, nothing launched: a NULL input (truth included), out NULL or all of its
 * outputs NULL, B or T < 1, C < 8 or C % 8 != 0, a bad row stride, a misaligned pointer (y, truth, node_* 16 bytes; frame_* 4). */
int sgv_test_recon_score(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                         const float* scale, const float* min, const float* truth, const sgv_score_out* out, int B, int T, int C,
                         void* stream);
/* The kernel of sgv_ensemble on caller-owned buffers: inputs as sgv_test_recon_physical, then the statistics of y and the ensemble
 * pass into *st (shapes of sgv_ensemble_state with N = C).  SGV_ERR_ARG, nothing launched: a NULL input, st NULL, no group or half
 * a group, B or T < 1, C < 8 or C % 8 != 0, a bad row stride, a misaligned pointer (y and the state arrays 16 bytes; limit 4),
 * count_before < 0 or count_before + B > 2^24. */
int sgv_test_recon_ensemble(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                            const float* scale, const float* min, long count_before, const sgv_ensemble_state* st, int B, int T,
                            int C, void* stream);
/* The kernel of sgv_sobol on caller-owned buffers: inputs as sgv_test_recon_physical, B = whole blocks of n_params + 2 members,
 * then the statistics of y and the Sobol pass into *st (shapes of sgv_sobol_state with N = C).  SGV_ERR_ARG, nothing launched: a
 * NULL input, st NULL, mean or m2 missing, neither first_sq nor total_sq, B or T < 1, C < 8 or C % 8 != 0, a bad row stride, a
 * misaligned pointer (y and the state arrays 16 bytes), n_params outside [1, 30], B no multiple of n_params + 2,
 * blocks_before < 0 or 2 (blocks_before + blocks) > 2^24. */
int sgv_test_recon_sobol(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                         const float* scale, const float* min, int n_params, long blocks_before, const sgv_sobol_state* st, int B,
                         int T, int C, void* stream);
/* The kernel of sgv_distribution on caller-owned buffers: inputs as sgv_test_recon_physical, then the statistics of y and the
 * distribution pass into *st (shapes of sgv_distribution_state with N = C).  SGV_ERR_ARG, nothing launched: a NULL input, st NULL,
 * lo, hi or counts NULL, bins outside [2, 64], B or T < 1, C < 8 or C % 8 != 0, a bad row stride, a misaligned pointer (y, lo, hi
 * and counts 16 bytes), count_before < 0 or count_before + B > 2^24. */
int sgv_test_recon_distribution(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                                const float* scale, const float* min, long count_before, const sgv_distribution_state* st, int B,
                                int T, int C, void* stream);
/* The kernel of sgv_regress on caller-owned buffers: inputs as sgv_test_recon_physical, weights fp32 [B][n_cov] on the device, then
 * the statistics of y and the regression pass into *st (shapes of sgv_regress_state with N = C).  SGV_ERR_ARG, nothing launched: a
 * NULL input (weights included), st NULL, mean, m2 or comoment NULL, n_cov outside [1, 32], B or T < 1, C < 8 or C % 8 != 0, a bad
 * row stride, a misaligned pointer (y and the state arrays 16 bytes; weights 4), count_before < 0 or count_before + B > 2^24. */
int sgv_test_recon_regress(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                           const float* scale, const float* min, int n_cov, const float* weights, long count_before,
                           const sgv_regress_state* st, int B, int T, int C, void* stream);
/* The kernel of sgv_project on caller-owned buffers: inputs as sgv_test_recon_physical, weights fp32 [n_func][C] and out fp32
 * [B][T][n_func] on the device, then the statistics of y and the project pass with a workspace of its own.  SGV_ERR_ARG, nothing
 * launched: a NULL input (weights included), out NULL, n_func outside [1, 32], B or T < 1, C < 8 or C % 8 != 0, a bad row stride, a
 * misaligned pointer (y and weights 16 bytes; out 4). */
int sgv_test_recon_project(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                           const float* scale, const float* min, const float* weights, int n_func, float* out, int B, int T, int C,
                           void* stream);
/* The kernel of sgv_temporal on caller-owned buffers: inputs as sgv_test_recon_physical, weights fp32 [n_func][T] and out fp32
 * [B][n_func][C] on the device, then the statistics of y and the temporal pass with a workspace of its own.  SGV_ERR_ARG, nothing
 * launched: a NULL input (weights included), out NULL, n_func outside [1, 32], B or T < 1, C < 8 or C % 8 != 0, a bad row stride, a
 * misaligned pointer (y and out 16 bytes; weights 4). */
int sgv_test_recon_temporal(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                            const float* scale, const float* min, const float* weights, int n_func, float* out, int B, int T, int C,
                            void* stream);
/* The kernel of sgv_gram on caller-owned buffers: inputs as sgv_test_recon_physical, node_weights and offset fp32 [C] on the device
 * or NULL, out fp32 [B][T][T] on the device, then the statistics of y and the Gram pass with a workspace of its own.  SGV_ERR_ARG,
 * nothing launched: a NULL input, out NULL, B or T < 1, T > 256, C < 8 or C % 8 != 0, a bad row stride, a misaligned pointer (y,
 * node_weights and offset 16 bytes; out 4). */
int sgv_test_recon_gram(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta, const float* scale,
                        const float* min, const float* node_weights, const float* offset, float* out, int B, int T, int C, void* stream);
/* The kernel of sgv_exceedance on caller-owned buffers: inputs as sgv_test_recon_physical, levels fp32 [n_level][C], stats int32
 * [B][5][n_level][C] or NULL and excess fp32 [B][n_level][C] or NULL on the device, then the statistics of y and the exceedance
 * pass.  SGV_ERR_ARG, nothing launched: a NULL input (levels included), both outputs NULL, n_level outside [1, 4], an unknown
 * side, B or T < 1, T > 65535, C < 8 or C % 8 != 0, a bad row stride, a misaligned pointer (y, stats and excess 16 bytes; levels 4). */
int sgv_test_recon_exceedance(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta,
                              const float* scale, const float* min, const float* levels, int n_level, int side, int32_t* stats,
                              float* excess, int B, int T, int C, void* stream);
/* The kernel of sgv_cycles on caller-owned buffers: inputs as sgv_test_recon_physical, gate fp32 [C] and the outputs of out
 * ([B][C], [B][4][C], [B][2][C], [B][3][C]) on the device, then the statistics of y and the cycles pass.  SGV_ERR_ARG, nothing
 * launched: a NULL input (gate and out included), no group, half a group, an exponent outside [1, 8], B or T < 1, T > 65535,
 * C < 8 or C % 8 != 0, a bad row stride, a misaligned pointer (y and the outputs 16 bytes; gate 4). */
int sgv_test_recon_cycles(int dtype, const void* y, long ldy, double* sums, const float* gamma, const float* beta, const float* scale,
                          const float* min, const float* gate, int exponent, const sgv_cycles_out* out, int B, int T, int C, void* stream);
/* GELU without GroupNorm.  mode 0: out = gelu(y).  mode 1: out = dout * rscale * gelu'(y), dbias = column sums of out,
 * cdot[0] = sum out * (y - cbias).  mode 2: y holds a gradient dY: dbias = its column sums, cdot[0] = sum dY * (yf32 - cbias)
 * (yf32 [B*T][ldyf] fp32; cdot needs it). */
int sgv_test_act(int dtype, int mode, const void* y, long ldy, const void* dout, long lddout, float rscale, void* out, long ldout,
                 float* dbias, float* cdot, const float* cbias, const float* yf32, long ldyf, float* work, size_t work_floats, int B,
                 int T, int C, void* stream);
/* Latent reparameterisation + KL: last [B][2Z] = [mu | logvar], eps / z / dz [B][Z], dlast [B][2Z], all fp32.  z and kl given:
 * forward (kl[0] = batch mean).  dz and dlast given: backward of sum dz z + coef * B * kl. */
int sgv_test_latent(const float* last, const float* eps, float* z, double* kl, const float* dz, float* dlast, float coef, int B, int Z,
                    void* stream);
/* Decoder stage: pz = [mu | lv], qz = [dmu | dlv] fp32 [M][2C], eps fp32 [M][C].  zs_next given: forward, zs_next = dec_out + z
 * (dtype maps), zmap (fp32 [M][C], optional) = z, kl[0] = inv_b * sum of the KL terms; kl_part: scratch of 2048 doubles.
 * dzs given: backward (std_scale 1) of sum dzs z + coef * (sum of the KL terms): g_p / g_q [M][2C] of dtype. */
int sgv_test_stage(int dtype, const float* pz, const float* qz, const float* eps, const void* dec_out, long ldd, void* zs_next,
                   long ldz, float* zmap, float std_scale, float inv_b, double* kl, double* kl_part, const void* dzs, long lddzs,
                   void* g_p, void* g_q, float coef, int M, int C, void* stream);
/* Linear "head" (K large, O small; K % 8 == 0): Y given: Y [B][O] fp32 = scale[0] * X W^T + bias, X [B][K] of xdtype, W [O][K]
 * fp32, part: scratch of part_floats >= 128 * B * O floats.  dY given: dX (xdtype, optional) = scale[0] * dY W (+ addend),
 * dW (optional) = dY^T X, db (optional, with dW) = column sums of dY. */
int sgv_test_linear_head(int xdtype, const void* X, const float* W, const float* bias, const float* scale, float* Y, float* part,
                         size_t part_floats, const float* dY, const void* addend, void* dX, float* dW, float* db, int B, int K, int O,
                         void* stream);
/* Linear "expand" (K small, O large): Y given: Y [B][O] of dtype = scale[0] * X W^T + bias (X [B][K], W [O][K], bias fp32).
 * dY given (dtype): dW, db (both required), dX (optional) = scale[0] * dY W. */
int sgv_test_linear_expand(int dtype, const float* X, const float* W, const float* bias, const float* scale, void* Y, const void* dY,
                           float* dX, float* dW, float* db, int B, int K, int O, void* stream);

/* Test hook for the multi-tensor optimizer / spectral-norm passes (csrc/optim.hip; tests/test_optim_kernels_gpu.py): an opaque
 * object over a list of caller-owned device tensors.  Creation builds the descriptor and work-item tables with the same host
 * helpers (csrc/sgv_ew.h) the engine and the parameter-set object size theirs with; every call runs the launcher the engine
 * calls and synchronises `stream`.  Weights are fp32 [taps][rows][cols] (cols contiguous), u [rows], v_sn [taps*cols] in
 * (tap, col) order, sigma [2] = (sigma, 1/sigma), dot [32] = the <G, W_eff> slots (the update adds them up).  rows = 0: a plain
 * tensor of n elements (bias / affine), no spectral norm.  wc / wct: compute-dtype copies [taps][rows][cols] and the transposed,
 * tap-flipped [taps][cols][rows], each optional; g_bf16: optional bf16 mirror of g.  tiled != 0: updated by the 64 x 64-tile
 * pass (the engine's conv weights: that pass also writes wc / wct and the W^T u partials a following power iteration may
 * reuse), otherwise by the flat pass.  active = 0: the power iteration leaves the entry alone.  Bias corrections follow from
 * `step` (1-based); betas (0.9, 0.999) and eps 1e-8 are the engine's.  Scratch belongs to the object and starts as NaN.
 * Creation rejects what the engine's layout never produces: n or cols not a multiple of 4, p / g / m / v not 16-byte aligned,
 * tiled without spectral norm, taps * rows * cols != n. */
typedef struct {
    float* p; float* g; float* m; float* v;
    long n;
    int32_t taps, rows, cols;
    float* u; float* v_sn; float* sigma; float* dot;
    void* wc; void* wct;
    const void* g_bf16;
    int32_t tiled;
    int32_t active;
} sgv_optset_entry;
typedef struct sgv_optset sgv_optset;
int sgv_test_optset_create(int dtype, const sgv_optset_entry* entries, int n, sgv_optset** out);
int sgv_test_optset_destroy(sgv_optset* os);
/* train != 0: v <- norm(W^T u), u <- norm(W v), sigma = u.(W v); else sigma only.  The W v pass reads wc instead of W for bf16
 * objects when wc is given and cols % 8 == 0.  reuse_tpart != 0 (training): the first pass skips the tiled entries, whose
 * partials the last tiled update left behind. */
int sgv_test_optset_power_iteration(sgv_optset* os, int train, int reuse_tpart, void* stream);
/* dot[0] = <g, p> / sigma for the non-tiled spectrally-normalised entries (the conv kernels produce it for the tiled ones: the
 * caller writes their slot itself); slots 1.. are left alone. */
int sgv_test_optset_grad_dot(sgv_optset* os, void* stream);
/* Sum of squares of the gradients wrt the original weights (chain rule applied), over all entries, from the fp32 gradients. */
int sgv_test_optset_grad_norm(sgv_optset* os, double* gnorm_sq_out, void* stream);
/* One AdamW step: flat pass over the non-tiled entries (gscale_dev: optional device scalar multiplied into the gradient after
 * the norm is taken), tiled pass over the others.  grad_source selects what the tiled pass reads: 0 the fp32 g, 1 the entry's
 * g_bf16 where given, 2 the bf16 wire copy g_wire of the fp32 arena starting at g_base (g_wire_elems elements: element k of
 * g_wire mirrors g_base[k]).  gnorm_sq_out (optional): the squared gradient norm the two passes accumulated. */
int sgv_test_optset_adamw(sgv_optset* os, float lr, float wd, int step, const float* gscale_dev, int grad_source, const float* g_base,
                          const void* g_wire, size_t g_wire_elems, double* gnorm_sq_out, void* stream);
/* wc / wct of every entry that has one, from the fp32 p. */
int sgv_test_optset_make_copies(sgv_optset* os, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGVAE_H */
