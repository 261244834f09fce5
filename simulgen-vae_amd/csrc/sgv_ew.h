// Host-callable launchers of the elementwise / normalisation / optimizer kernels (ew.hip, recon_out.hip, optim.hip).
#pragma once
#include "sgv_common.h"
#include <vector>

struct GNParams {
    const void* y = nullptr;    long ldy = 0;      // conv output (pre-norm) [B*T][C]
    const void* res = nullptr;  long ldres = 0;    // optional residual base
    void* out = nullptr;        long ldout = 0;    // result
    const void* dout = nullptr; long lddout = 0;   // incoming gradient, or loss target (FROM_LOSS)
    const float* gamma = nullptr;
    const float* beta = nullptr;
    float* dgamma = nullptr;
    float* dbeta = nullptr;
    float* dbias = nullptr;                        // bias gradient of the producing conv
    float* part = nullptr;                         // workspace for per-block column sums (ew_gn_part_floats)
    float* cdot = nullptr;                         // <G, W_eff> = sum dY*(y - cbias) of the producing conv (slot 0 of its dot slots)
    float* cdot_part = nullptr;                    // deferred mode: one partial per block of the dY-producing launch goes here and the
    int* cdot_blocks = nullptr;                    //   caller sums them later (ew_fin_dots); *cdot_blocks (host) = how many were written.
                                                   //   null: the launcher sums them into cdot[0] itself (workspace: p.part)
    float* ptot = nullptr;                         // deferred mode: [B][3][C] per-sample column totals (sum dz, sum dz*xhat, bias-gradient
                                                   //   term) for ew_fin_affine; null: the launcher finalises dbeta / dgamma / dbias itself
    const float* cbias = nullptr;                  // that conv's bias
    const float* yf32 = nullptr; long ldyf = 0;    // act mode 2: the conv output (fp32) paired with dY in `y`
    double* sums = nullptr;                        // [B*G][2] sum, sum of squares
    double* sums2 = nullptr;                       // [B*G][2] backward group sums
    double* loss_sums = nullptr;                   // [2]
    int accum_affine = 0;                          // immediate mode: dbeta / dgamma / dbias += instead of =
    int defer_colsum = 0;                          // ew_act modes 1 / 2: leave the per-block column sums in `part` ([ew_act_part_rows][C]); the caller sums them later (ew_fin_affine, arrays = 1)
    float* lpart = nullptr;                        // recon loss: per-block (selected, squared) partial sums (workspace)
    int B = 0, T = 0, C = 0, G = 1, Cg = 1, CV = 1;
    float rscale = 1.f;                            // residual / incoming-gradient scale
    float gscale = 1.f;                            // output gradient scale (loss weight)
    int loss_type = 0;
};

// second operand of ew_gn_tail: out = relu(A + gn(y)), A = gn2(y2) (gamma2 / beta2 / sums2) or y2 * cscale[b][c] (cscale != null)
struct GNTail {
    const void* y2 = nullptr; long ldy2 = 0;
    const float* gamma2 = nullptr;
    const float* beta2 = nullptr;
    double* sums2 = nullptr;            // [B*G][2] statistics of y2 (same groups as y)
    const float* cscale = nullptr;      // [B][C]
};

constexpr int SGV_GN_MAX_GROUPS = 32;
// convgn.hip: fused small convolution + GroupNorm + GELU (+ residual) forward, one workgroup per (group, sample)
struct ConvGN {
    const void* A; long lda;            // input [B*T][lda] bf16, K columns used
    const void* W; long ldw;            // weights [taps][N][ldw] bf16 (K contiguous)
    long w_tap_stride;
    const float* bias;                  // [N]
    const float* scale;                 // device scalar 1/sigma, or null
    void* y; long ldy;                  // pre-norm conv output [B*T][ldy] bf16 (stored)
    void* out; long ldout;              // result
    const void* res; long ldres;        // optional residual base
    float rscale;
    const float* gamma; const float* beta;
    double* sums;                       // [B*G][2] sum, sum of squares (stored)
    int B, T, N, K, taps, pad, G, Cg;
};
// backward mirror: input gradient of the UPPER convolution + GroupNorm / GELU backward of the stage below it in one launch
// (the gradient wrt the lower stage's activated output is never stored)
struct ConvGNBwd {
    const void* A; long lda;            // dY of the upper stage [B*T][lda] bf16, K = its output channels
    const void* W; long ldw;            // its transposed, tap-flipped weight copy [taps][N][ldw] bf16
    long w_tap_stride;
    const float* scale;                 // 1/sigma of the upper convolution, or null
    const void* addend; long ldadd;     // optional [B*T][ldadd] bf16 added to the input gradient before it is rounded (residual path)
    const void* premul; long ldpre;     // optional [B*T][ldpre] bf16 x: the (rounded) input gradient is multiplied by gelu'(x) and rounded
                                        //   again (the upper convolution reads GELU(x): modules/decoder.py condition blocks)
    const void* y; long ldy;            // pre-norm output of the lower stage [B*T][ldy] bf16
    const double* sums;                 // its forward statistics [B*G][2]
    const float* gamma; const float* beta;
    const float* cbias;                 // bias of the lower convolution (for <G, W_eff>), or null
    void* dy; long lddy;                // out: gradient wrt y [B*T][lddy] bf16
    void* da; long ldda;                // optional out: the input gradient itself [B*T][ldda] bf16 (a residual block below needs it again)
    double* sums2;                      // out [B*G][2]
    float* ptot;                        // out [B][3][C]: per-sample column totals (sum dz, sum dz*xhat, bias-gradient term)
    float* cdot_part;                   // out [B*G]: partials of <G, W_eff> = sum dY * (y - cbias), or null
    float rscale, gscale;
    int B, T, N, K, taps, pad, G, Cg;
};
bool conv_gn_bwd_eligible(int dtype, const ConvGNBwd& p);
int launch_conv_gn_bwd(const ConvGNBwd& p, hipStream_t s);
bool conv_gn_fused_eligible(int dtype, const ConvGN& p);
int launch_conv_gn_fwd(const ConvGN& p, hipStream_t s);
// Deterministic reductions: no kernel of the step accumulates floating-point values with atomics.  Block partials go to
// workspaces and are summed in a fixed order, either by the launcher itself or, for quantities nobody needs before the
// optimizer (GroupNorm affine / bias gradients, <G, W_eff>), by two table-driven passes the engine runs once per bucket.
struct FinDot { const float* src; float* dst; int count; int pad; };                      // dst[0] = sum src[0..count)
struct FinAffine { const float* ptot; float* dbeta; float* dgamma; float* dbias; int C; int B; int accum; int arrays; };   // d*[c] (+)= sum_b ptot[b][k][c]; arrays = k range (0 -> 3; 1: ptot is [B][C], dbeta only)
int ew_fin_dots(const FinDot* items_host, int n, hipStream_t s);
int ew_fin_affine(const FinAffine* items_host, int n, hipStream_t s);
// out[b*n + j] = scale * sum_{r<R} part[(b*R + r)*n + j] in a fixed order (out_f or out_d, the other null)
int ew_rowsum(const float* part, int batches, int R, int n, float* out_f, double* out_d, double scale, hipStream_t s);
int ew_rowsum_d(const double* part, int R, int n, double* out_d, double scale, hipStream_t s);
int ew_gn_stats(int dtype, GNParams p, hipStream_t s);
// whole GroupNorm passes: one fused launch when a (sample, group) slab is small, else the multi-kernel path
int ew_gn_fwd(int dtype, int act, GNParams p, hipStream_t s);   // stats (p.sums is written, not accumulated) + apply
int ew_gn_bwd(int dtype, int act, GNParams p, hipStream_t s);   // reduce + finalize + dY; act in {0, 1 gelu, 3 relu}
bool gn_fused_ok(const GNParams& p);       // ew_gn_fwd takes the one-launch slab kernel (B, T, C, G, Cg set)
bool gn_fused_bwd_ok(const GNParams& p);   // ew_gn_bwd does
int ew_gn_bwd_reduce_act(int dtype, int act, GNParams p, hipStream_t s);   // act: 0 none, 1 gelu, 3 relu
int ew_gn_bwd_apply_act(int dtype, int act, GNParams p, hipStream_t s);
int ew_gn_apply(int dtype, int act, GNParams p, hipStream_t s);
int ew_gn_tail(int dtype, GNParams p, GNTail t, hipStream_t s);    // p: y / gamma / beta / sums (given) / out; see GNTail
size_t ew_gn_part_floats(int B, int T, int C);
int ew_gn_max_blocks(int B, int T, int C);
int ew_act_part_rows(int B, int T, int C);         // rows of per-block column sums an ew_act launch with dbias writes          // upper bound of the per-block <G,W_eff> partials one launch writes
int ew_recon_loss(int dtype, int train, GNParams p, hipStream_t s);
int ew_recon_bwd_apply(int dtype, GNParams p, hipStream_t s);
// ---- the recon tails (recon_out.hip): passes that replace the loss tail of the recon head ----
// recon head -> physical-unit fp32 field: out = (tanh(GroupNorm(y)) - mn) / scale per channel; layout 0 [B][T][C], 1 [B][C][T] (dense).
// Non-zero (nothing launched): -1 null pointer, -2 unknown layout, -3 bad shape, -4 y or out not 16-byte aligned
int ew_recon_physical(int dtype, GNParams p, const float* scale, const float* mn, int layout, float* out, hipStream_t s);
// recon head -> summaries of the physical field, the field itself never stored (same p, scale, mn as ew_recon_physical).  Any subset of
// the outputs, null = not computed: node_stats fp32 [B][3][C] (max, min, mean over t), node_when int32 [B][2][C] (t of max, of
// min; smallest t on a tie), frame_stats fp32 [B][T][2] (max, min over the channels), frame_where int32 [B][T][2] (their
// channel; smallest on a tie), probes fp32 [B][T][n_probes] (the field at probe_nodes[k], device int32, each in [0, C): the
// caller has checked them).  work: ew_recon_summary_work_floats floats, 16-byte aligned, needed for a frame output.
struct ReconSummary {
    float* node_stats = nullptr; int* node_when = nullptr; float* frame_stats = nullptr; int* frame_where = nullptr; float* probes = nullptr;
    const int* probe_nodes = nullptr; int n_probes = 0;
    float* work = nullptr;
};
size_t ew_recon_summary_work_floats(int B, int T, int C);
int ew_recon_summary(int dtype, GNParams p, const float* scale, const float* mn, const ReconSummary& o, hipStream_t s);
// recon head -> the error of the physical field against truth (fp32 dense [B][T][C], physical units, 16-byte aligned, finite: not
// checked), neither stored: e = val - truth, val as ew_recon_physical stores it.  Any subset of the outputs, null = not computed:
// node_err fp32 [B][3][C] (max_t |e|, mean_t e, mean_t e^2), node_when int32 [B][C] (t of max |e|; smallest t on a tie), frame_err
// fp32 [B][T][3] (max_n |e|, mean_n e^2, mean_n truth^2), frame_where int32 [B][T] (node of max |e|; smallest on a tie).
// work: ew_recon_summary_work_floats floats, 16-byte aligned, needed for a frame output.
struct ReconScore {
    float* node_err = nullptr; int* node_when = nullptr; float* frame_err = nullptr; int* frame_where = nullptr;
    float* work = nullptr;
};
int ew_recon_score(int dtype, GNParams p, const float* scale, const float* mn, const float* truth, const ReconScore& o, hipStream_t s);
// recon head -> running statistics over the members of a batch (and of the batches before it) per (t, channel), the field never
// stored: the values ew_recon_physical would store (layout [B][T][C]) are merged member after member, in fp32, into a state that
// persists across launches.  Three groups, any subset, each complete; every array dense [T][C], 16-byte aligned:
//   moments  mean, m2 fp32: Welford, k = index + 1, r = 1.0f / k, d = x - mean, mean += d * r, m2 += d * (x - mean), each rounded
//   extrema  vmax, vmin fp32 and imax, imin int32: strict comparisons, so the earliest member keeps a tie; the index of the member
//   exceed   limit fp32 [C] (input) and exceed int32: the count of members with x > limit[channel]
// Member b has index count_before + b.  With count_before == 0 the state is not read (mean = m2 = 0, extrema -inf / +inf, indices
// and counts 0).  Any cut of the same members into launches gives the same bits.
struct ReconEnsemble {
    float* mean = nullptr; float* m2 = nullptr;
    float* vmax = nullptr; float* vmin = nullptr; int* imax = nullptr; int* imin = nullptr;
    const float* limit = nullptr; int* exceed = nullptr;
};
int ew_recon_ensemble(int dtype, GNParams p, const float* scale, const float* mn, long count_before, const ReconEnsemble& o, hipStream_t s);
// recon head -> the running sums of a Sobol sensitivity study per (t, channel), the field never stored.  The batch holds whole blocks
// of n_params + 2 members, A_j, B_j, AB_1_j .. AB_d_j (AB_i_j: A_j with the columns of parameter i from B_j); x is the value
// ew_recon_physical would store, everything fp32 with one rounding per operation, j ascending from blocks_before:
//   mean, m2      [T][C]     Welford over A_0, B_0, A_1, B_1, .. (k = 2 j + 1 for A_j, 2 j + 2 for B_j), as ReconEnsemble's moments
//   first_sq      [d][T][C]  first_sq[i] += (xB - xAB_i)^2    (Jansen's first-order form: S_i = 1 - first_sq[i] / (2 n var))
//   total_sq      [d][T][C]  total_sq[i] += (xA - xAB_i)^2    (Jansen's total form: ST_i = total_sq[i] / (2 n var))
// mean and m2 are required, and at least one of first_sq, total_sq; every array dense and 16-byte aligned.  With blocks_before == 0
// the state is not read.  Any cut of the same blocks into launches gives the same bits.
struct ReconSobol {
    float* mean = nullptr; float* m2 = nullptr;
    float* first_sq = nullptr; float* total_sq = nullptr;
};
int ew_recon_sobol(int dtype, GNParams p, const float* scale, const float* mn, int n_params, long blocks_before, const ReconSobol& o, hipStream_t s);
// recon head -> a histogram over the members of a batch (and of the batches before it) per (t, channel), the field never stored.  x is
// the value ew_recon_physical would store (layout [B][T][C]), K = bins in [2, 64], lo and hi fp32 [T][C] (inputs), counts int32
// [K + 2][T][C]: row 0 underflow, rows 1 .. K the bins, row K + 1 overflow; every array dense and 16-byte aligned.  All fp32, every
// operation rounded on its own:
//   invw = hi > lo ? (float)K / (hi - lo) : 0.0f
//   row  = x < lo ? 0 : x > hi ? K + 1 : 1 + min((int)((x - lo) * invw), K - 1);   counts[row][t][c] += 1
// The pass only adds to counts (there is no "state not read" mode: the caller zeroes a new state), so any cut of the same members
// into launches gives the same bits; count_before only bounds the size of the study.
struct ReconDistribution {
    const float* lo = nullptr; const float* hi = nullptr; int* counts = nullptr; int bins = 0;
};
int ew_recon_distribution(int dtype, GNParams p, const float* scale, const float* mn, long count_before, const ReconDistribution& o, hipStream_t s);
// recon head -> the running co-moments of the field with n_cov = K covariates per member, 1 <= K <= 32, per (t, channel), the field never
// stored.  x is the value ew_recon_physical would store (layout [B][T][C]); w fp32 [B][K] (input, 4-byte aligned) holds the centred
// covariates of the batch's members, w[b][i] = y_b,i - ybar_i with ybar the running mean including that member (formed by the caller);
// mean, m2 fp32 [T][C] and co fp32 [K][T][C], dense and 16-byte aligned.  Member b has k = count_before + b + 1; all fp32, every
// operation rounded on its own, members in ascending order:
//   d = x - mean;  mean = mean + d * (1.0f / (float)k);  m2 = m2 + d * (x - mean);  co[i] = co[i] + d * w[b][i]
// mean and m2 are ReconEnsemble's moments bit for bit.  With count_before == 0 the state is not read.  Any cut of the same members into
// launches gives the same bits.
struct ReconRegress {
    float* mean = nullptr; float* m2 = nullptr; float* co = nullptr; const float* w = nullptr;
};
int ew_recon_regress(int dtype, GNParams p, const float* scale, const float* mn, int n_cov, long count_before, const ReconRegress& o, hipStream_t s);
// recon head -> n_func = R linear functionals of the physical field, 1 <= R <= SGV_MAX_FUNCTIONALS, the field never stored:
//   out[b][t][r] = sum over n of weights[r][n] * x[b][t][n],  x the value ew_recon_physical would store (layout [B][T][C]).
// weights fp32 [R][C] dense, 16-byte aligned (input); out fp32 [B][T][R], 4-byte aligned; work: ew_recon_project_work_floats floats,
// 16-byte aligned.  fp32 fused multiply-adds in ascending n inside a fixed share of the channels, the shares combined in ascending
// order in fp64 and rounded to fp32 once: out[b][t][r] depends on sample b, row t and weight row r alone -- not on B, on the
// sample's place in the batch, on R or on the other rows -- and two launches are bitwise equal.  No atomics.
// Non-zero (nothing launched): -1 null input (weights included), -2 no output, -3 bad shape or R outside [1, 32], -4 y, weights or
// work not 16-byte aligned or out not 4-byte aligned, -6 no workspace
constexpr int SGV_MAX_FUNCTIONALS = 32;
struct ReconProject {
    const float* weights = nullptr; int n_func = 0; float* out = nullptr;
    float* work = nullptr;
};
size_t ew_recon_project_work_floats(int B, int T, int C, int R);
int ew_recon_project(int dtype, GNParams p, const float* scale, const float* mn, const ReconProject& o, hipStream_t s);
// recon head -> n_func = R linear functionals over TIME of the physical field, 1 <= R <= SGV_MAX_TEMPORAL, the field never stored:
//   out[b][r][n] = sum over t of weights[r][t] * x[b][t][n],  x the value ew_recon_physical would store (layout [B][T][C]).
// weights fp32 [R][T] dense, 4-byte aligned (input; read once by a kernel that writes the transposed, zero-padded copy the pass
// reads); out fp32 [B][R][C], 16-byte aligned (its rows are written 32 bytes at a time, and C % 8 == 0 keeps every row aligned);
// work: ew_recon_temporal_work_floats floats, that copy.  One fp32 fused multiply-add chain per output over t ascending, from 0,
// nothing else: out[b][r][n] depends on sample b, weight row r and channel n alone -- a row gives alone the bits it gives among
// 32, in any order of the rows; a sample gives the bits it gives in any batch and at any place in it -- and two launches are
// bitwise equal.  No atomics, no partial sums.
// Non-zero (nothing launched): -1 null input (weights included), -2 no output, -3 bad shape or R outside [1, 32], -4 y or out not
// 16-byte aligned or weights or work not 4-byte aligned, -6 no workspace
constexpr int SGV_MAX_TEMPORAL = 32;
struct ReconTemporal {
    const float* weights = nullptr; int n_func = 0; float* out = nullptr;
    float* work = nullptr;
};
size_t ew_recon_temporal_work_floats(int T);
int ew_recon_temporal(int dtype, GNParams p, const float* scale, const float* mn, const ReconTemporal& o, hipStream_t s);
// recon head -> the temporal Gram matrix of the physical field per sample, the field never stored:
//   out[b][t][t'] = sum over n of w[n] * (x[b][t][n] - m[n]) * (x[b][t'][n] - m[n]),  x the value ew_recon_physical would store
// (layout [B][T][C]), T <= SGV_MAX_GRAM_T.  node_weights = w [C] and offset = m [C] fp32, 16-byte aligned, either may be null (w = 1,
// m = 0; arrays of ones / zeros give the same bits); out fp32 [B][T][T] dense, 4-byte aligned; work: ew_recon_gram_work_floats
// floats, 16-byte aligned.  d = fl(x - m) is rounded once and is both operands; for t <= t' the element is one fp32 fused
// multiply-add chain of fl(w[n] d[t][n]) * d[t'][n] -- the SMALLER time index carries the weight -- over the channels of a block of
// 6144 in the kernel's order, from 0; the blocks' partials are added in ascending order in fp64 and rounded once; (t', t) is the
// copy of (t, t'), so out is bitwise symmetric and its diagonal is >= 0 for w >= 0.  out[b] depends on sample b alone -- a sample
// gives the bits it gives in any batch and at any place in it -- and two launches are bitwise equal.  No atomics.
// Non-zero (nothing launched): -1 null input, -2 no output, -3 bad shape or T > SGV_MAX_GRAM_T, -4 y, node_weights, offset or work not
// 16-byte aligned or out not 4-byte aligned, -6 no workspace
constexpr int SGV_MAX_GRAM_T = 256;
struct ReconGram {
    const float* node_weights = nullptr; const float* offset = nullptr; float* out = nullptr;
    float* work = nullptr;
};
size_t ew_recon_gram_work_floats(int B, int T, int C);
int ew_recon_gram(int dtype, GNParams p, const float* scale, const float* mn, const ReconGram& o, hipStream_t s);
// recon head -> the level-crossing statistics over TIME of the physical field against n_level = L levels per channel,
// 1 <= L <= SGV_MAX_EXCEED_LEVELS, the field never stored.  With x[t] the value ew_recon_physical would store at (b, t, n) (layout
// [B][T][C]), lam = levels[l][n] and e[t] = (x[t] > lam) for above, (x[t] < lam) otherwise (strict; a NaN exceeds nothing):
//   stats[b][0][l][n] = count:   the number of t with e[t]
//   stats[b][1][l][n] = first:   the smallest t with e[t], -1 if none
//   stats[b][2][l][n] = last:    the largest t with e[t], -1 if none
//   stats[b][3][l][n] = longest: the length of the longest run of consecutive t with e[t], 0 if none
//   stats[b][4][l][n] = runs:    the number of t with e[t] and (t == 0 or not e[t - 1])
//   excess[b][l][n]   = s after: s = +0.0; for t ascending, where e[t]: s = fl(s + d[t]), d[t] = fl(x[t] - lam) (fl(lam - x[t])
//                       below) -- the difference of the stored value, rounded on its own.  Exactly +0.0 where nothing exceeds.
// levels fp32 [L][C] dense, 4-byte aligned (input); stats int32 [B][5][L][C] and excess fp32 [B][L][C], 16-byte aligned, either may
// be null, not both.  T <= 65535 (the kernel packs its counters into 16-bit halves).  An output depends on sample b, level row l
// and channel n alone -- a level gives alone the bits it gives among 4, in any order; a sample the bits it gives in any batch; an
// output the bits it gives with or without the other -- and two launches are bitwise equal.  No atomics, no workspace.
// Non-zero (nothing launched): -1 null input (levels included), -2 no output, -3 bad shape, L outside [1, SGV_MAX_EXCEED_LEVELS] or
// T > 65535, -4 y, stats or excess not 16-byte aligned or levels not 4-byte aligned
constexpr int SGV_MAX_EXCEED_LEVELS = 4;          // (SGV_MAX_LEVELS of include/sgvae.h is the depth of the hierarchy, another thing)
struct ReconExceed {
    const float* levels = nullptr; int n_level = 0; bool above = true;
    int* stats = nullptr; float* excess = nullptr;
};
int ew_recon_exceedance(int dtype, GNParams p, const float* scale, const float* mn, const ReconExceed& o, hipStream_t s);
// recon head -> the load cycles and the rates of every channel's time history, the field never stored: ASTM E1049 simple-range
// counting behind a hysteresis gate (peak-valley filtering) and the statistics of the first differences.  x[t] is the value
// ew_recon_physical would store at (b, t, n) (layout [B][T][C]), h = gate[n] >= 0, m = exponent in [1, SGV_MAX_CYCLES_EXPONENT], fl()
// one fp32 rounding.  Every difference is formed from the stored value and rounded on its own, every product of the power and every
// accumulation likewise: nothing is contracted into an fma.  All comparisons are strict.
// Rates, t = 1 .. T - 1, r[t] = fl(x[t] - x[t-1]):
//   rates[b][0][n] = rise = max r[t], rates[b][1][n] = fall = min r[t]; rate_when[b][0][n], [1][n] = the step t of each, the smallest on
//   a tie (strict > / < updates starting from r[1]); rates[b][2][n] = path = s after s = +0.0; s = fl(s + |r[t]|), t ascending.
//   T = 1: rise = fall = path = +0.0, both steps -1.
// Turns, a machine of three states per channel, dir in {0, +1, -1}, from dir = 0, hi = lo = x[0]; for t = 1 .. T - 1, x = x[t]:
//   dir = 0:  fl(x - lo) > h: a valley is confirmed, last = lo, cand = x, dir = +1, reversals += 1; else fl(hi - x) > h: a peak,
//             last = hi, cand = x, dir = -1, reversals += 1; else hi = max(hi, x), lo = min(lo, x).  (Both cannot hold for h >= 0; the
//             order is the definition.)  The first turning point carries no range.
//   dir = +1: x > cand: cand = x; else fl(cand - x) > h: a peak is confirmed, R = fl(cand - last) is counted, last = cand, cand = x,
//             dir = -1, reversals += 1.
//   dir = -1: x < cand: cand = x; else fl(x - cand) > h: a valley, R = fl(last - cand) is counted, last = cand, cand = x, dir = +1,
//             reversals += 1.
//   counted: range_sum = fl(range_sum + R); range_max = R if R > range_max; damage = fl(damage + P), P = R, then m - 1 times
//            P = fl(P * R); all three from +0.0.
//   open, the unfinished excursion at the end: fl(hi - lo) at dir = 0, fl(cand - last) at +1, fl(last - cand) at -1.
//   reversals[b][n]; ranges[b][0..3][n] = range_sum, range_max, damage, open.  The counted ranges (half cycles) number
//   max(reversals - 1, 0); a constant history gives 0 and +0.0 throughout; a gate above the peak-to-peak gives reversals 0 and
//   open = fl(max - min).
// gate fp32 [C], 4-byte aligned (input); reversals int32 [B][C] with ranges fp32 [B][4][C] (the turns), rate_when int32 [B][2][C] with
// rates fp32 [B][3][C] (the rates), 16-byte aligned; a group may be absent, not both, and not half of one.  T <= 65535 (the kernel packs
// its counters and steps into 16-bit halves).  An output depends on sample b and channel n alone -- a sample gives the bits it gives in
// any batch, a group the bits it gives with or without the other, the exponent shows in damage alone -- and two launches are bitwise
// equal.  No atomics, no workspace.
// Non-zero (nothing launched): -1 null input (gate included), -2 no group or half a group, -3 bad shape, exponent outside
// [1, SGV_MAX_CYCLES_EXPONENT] or T > 65535, -4 y or an output not 16-byte aligned or gate not 4-byte aligned
constexpr int SGV_MAX_CYCLES_EXPONENT = 8;
struct ReconCycles {
    const float* gate = nullptr; int exponent = 0;
    int* reversals = nullptr; float* ranges = nullptr;          // the turns
    int* rate_when = nullptr; float* rates = nullptr;           // the rates
};
int ew_recon_cycles(int dtype, GNParams p, const float* scale, const float* mn, const ReconCycles& o, hipStream_t s);
int ew_act(int dtype, int mode, GNParams p, hipStream_t s);
int ew_add3(int dtype, const void* a, long lda, const void* b, long ldb, const void* c, long ldc, void* out, long ldo,
            int rows, int C, hipStream_t s);
int ew_transpose(int src_dtype, int dst_dtype, const void* src, void* dst, int Bn, int I, int J, long lds_, long ldd,
                 long sbatch, long dbatch, hipStream_t s);
int ew_randn(float* out, long n, uint64_t seed, uint64_t stream, hipStream_t s, long per_row = 0, int world = 1, int rank = 0, long row0 = 0);
int ew_latent_fwd(const float* last, const float* eps, float* z, int B, int Z, double* kl_sum, hipStream_t s);
int ew_latent_bwd(const float* last, const float* eps, const float* dz, float* dlast, int B, int Z, float coef, hipStream_t s);
int ew_stage_fwd(int dtype, const float* pz, const float* qz, const float* eps, const void* dec_out, long ldd,
                 void* zs_next, long ldz, float* zmap, int M, int C, float std_scale, double* kl_sum, float inv_b,
                 double* kl_part, hipStream_t s);      // kl_part: workspace of >= 2048 doubles (per-block partials)
int ew_stage_bwd(int dtype, const float* pz, const float* qz, const float* eps, const void* dzs, long ldd, void* g_p,
                 void* g_q, int M, int C, float coef, hipStream_t s);
int ew_linear_head_fwd(int xdtype, const void* X, const float* W, const float* bias, const float* scale, float* Y, int B,
                       int K, int O, float* part, hipStream_t s);   // part: workspace of >= 128 * B * O floats (K-slice partials)
int ew_linear_head_bwd(int xdtype, const float* dY, const void* X, const float* W, const float* scale, const void* addend,
                       void* dX, float* dW, float* db, int B, int K, int O, hipStream_t s);
int ew_linear_expand_fwd(int dtype, const float* X, const float* W, const float* bias, const float* scale, void* Y, int B,
                         int K, int O, hipStream_t s);
int ew_linear_expand_bwd(int dtype, const void* dY, const float* X, const float* W, const float* scale, float* dX, float* dW,
                         float* db, int B, int K, int O, hipStream_t s);
int ew_augment(int dtype, const void* data, void* out, long sample_elems, int batch, const int* idx,
               const unsigned long long* noise_seed, const float* scale, const int* mix_idx, const float* lam, hipStream_t s);
int ew_pack_bf16(const float* src, void* dst_bf16, long n, hipStream_t s);     // data-parallel gradient payload: fp32 -> bf16 (RNE)
int ew_unpack_bf16(const void* src_bf16, float* dst, long n, hipStream_t s);
int ew_axpy(float* y, const float* x, float a, long n, hipStream_t s);
int ew_scale3(float* d0, float* d1, float* d2, const float* x, float a, long n, hipStream_t s);   // d_k = a * x[k*n .. (k+1)*n)
int ew_fill_from_scalar(float* dst, const float* src_scalar, long n, hipStream_t s);   // dst[i] = *src_scalar
int ew_scale(float* y, float a, long n, hipStream_t s);
// input pipeline
constexpr int SGV_MINMAX_ROWSPLIT = 64;
int ew_minmax_fit(const float* rows, long n_rows, int N, float* mn, float* mx, float* partial, int RS, int accumulate, hipStream_t s);
int ew_minmax_coeffs(const float* mn, const float* mx, int N, float lo, float hi, float* scale, float* offset, hipStream_t s);
int ew_scale_convert(int dtype, const float* src, const float* scale, const float* offset, void* dst, long n_rows, int N, hipStream_t s);
int ew_cast_rows(int dtype, const float* src, long lds_, void* dst, long ldd, int rows, int C, hipStream_t s);

// ---------------- optimizer / spectral norm (optim.hip) ----------------
// One descriptor per spectrally-normalised weight, internal layout [taps][rows][cols] fp32.
struct SNDesc {
    float* W;          // master weight
    float* u;          // [rows]
    float* v;          // [taps*cols], internal order (tap, col)
    float* tmp_t;      // [taps*cols] scratch: W^T u
    float* tmp_s;      // [rows]      scratch: W v
    float* tpart;      // [ceil(rows/64)][taps*cols] partials of W^T u per 64-row block (summed in block order by sn_tsum_kernel)
    float* spart;      // [taps*ceil(cols/1024)][rows] partials of W v per (tap, 1024-column block) (summed by sn_ssum_kernel)
    float* sigma;      // [2]: sigma, 1/sigma
    float* dot;        // [SGV_DOT_SLOTS] partial <G, W_eff> (lives in the gradient arena's small zone: all-reduced with it)
    const float* G;    // gradient wrt W_eff (null if the layer gets no gradient)
    const void* wc;    // bf16 copy of W in the same [taps][rows][cols] order (bf16 engines), or null: W v reads it instead of W
    int taps, rows, cols;
    int active;        // participates in this forward
};
// One descriptor per trainable tensor for the fused AdamW pass.
struct AdamDesc {
    float* p; float* g; float* m; float* v;
    long n;
    int sn;            // index into the SNDesc table, or -1 (bias / GroupNorm affine)
    int rows, cols;    // SN geometry for the rank-1 correction (taps*rows*cols == n)
    void* wc; void* wct;  // compute-dtype copies [taps][rows][cols] and [taps'][cols][rows] (tap-flipped), or null
    int taps;
    const unsigned short* glp;   // bf16 mirror of g (same element order) or null: read instead of g when the launch says so (desc_lp)
};
struct WorkItem { int desc; int chunk; };
// <G,W_eff> of a layer lives in this many slots of the gradient arena's small zone; the AdamW pass adds them up.  The
// fixed-order finalize (ew_fin_dots) writes the whole value to slot 0, the other slots stay at their initial zero -- the slot count is the arena
// layout round 1's atomic accumulation chose, kept so that checkpoints and the all-reduced arena keep their offsets.
constexpr int SGV_DOT_SLOTS = 32;

// items_ts / items_ss: (desc, 64-element chunk of taps*cols / 64-row chunk) for the fixed-order sums of tpart / spart
int opt_sn_power_iteration(const SNDesc* descs_dev, const WorkItem* items1, int n1, const WorkItem* items3, int n3,
                           const WorkItem* items_ts, int n_ts, const WorkItem* items_ss, int n_ss, int ndesc, int train, hipStream_t s);
// dot_part[i] = <G, W> / sigma of work item i (summed per layer by ew_fin_dots)
int opt_sn_grad_dot(const SNDesc* descs_dev, const WorkItem* items, int n, float* dot_part, hipStream_t s);
int opt_adamw(const AdamDesc* adam_dev, const SNDesc* sn_dev, const WorkItem* items, int n, float lr, float b1, float b2,
              float eps, float wd, float bc1, float bc2sqrt, double* gnorm_part, int compute_dtype, hipStream_t s, const float* gscale = nullptr);
// gnorm_part: one double per work item (the block's sum of squared gradients), written at gnorm_part[blockIdx.x]: pass the
// table base + the offset of `items` in the table; the caller sums the whole table in index order (ew_rowsum_d)
// 64x64-tile AdamW for spectrally-normalised conv weights; also writes wc/wct and the per-64-row-block partials of W_new^T u into tpart
int opt_adamw_sn(const AdamDesc* adam_dev, const SNDesc* sn_dev, const WorkItem* items, int n, float lr, float b1, float b2,
                 float eps, float wd, float bc1, float bc2sqrt, double* gnorm_sq, int compute_dtype, hipStream_t s,
                 const float* g_base = nullptr, const void* g_lp = nullptr, int desc_lp = 0);      // g_lp: gradients from the bf16 wire copy (offsets relative to g_base)
// tpart of the tiled entries rebuilt from the current weights and u, bit for bit what opt_adamw_sn leaves behind (same items table)
int opt_sn_tpart_tiles(const AdamDesc* adam_dev, const SNDesc* sn_dev, const WorkItem* items, int n, hipStream_t s);
int opt_grad_norm(const AdamDesc* adam_dev, const SNDesc* sn_dev, const WorkItem* items, int n, double* gnorm_sq,
                  hipStream_t s);
int opt_make_copies(const AdamDesc* adam_dev, const WorkItem* items, int n, int compute_dtype, hipStream_t s);
constexpr int OPT_CHUNK = 8192;      // elements per work item in the flat passes
constexpr int SN_ROWS_PER_ITEM = 64; // rows per work item in the GEMV passes
constexpr int SN_COLS_PER_ITEM = 1024;
constexpr int SN_SUM_CHUNK = 64;     // elements of taps*cols (sn_tsum_kernel) / rows (sn_ssum_kernel) per work item of the partial sums
constexpr int OPT_TILE = 64;         // tile edge of the tiled AdamW pass
constexpr int COPY_TILE = 32;        // tile edge of opt_make_copies
// Per-tensor geometry of the work-item tables and scratch buffers, [taps][rows][cols] weights.  OptTables (below) is the one host-side
// builder of those tables: the engine, the parameter set (pset.hip) and the sgv_test_optset hook all go through it; the kernels decode
// the same chunk numbering.
inline int sn_row_blocks(int rows) { return (rows + SN_ROWS_PER_ITEM - 1) / SN_ROWS_PER_ITEM; }
inline int sn_col_blocks(int cols) { return (cols + SN_COLS_PER_ITEM - 1) / SN_COLS_PER_ITEM; }
inline int sn_gemv_items(int taps, int rows, int cols) { return taps * sn_row_blocks(rows) * sn_col_blocks(cols); }   // items1 / items3 of the power iteration
inline int sn_tsum_items(int taps, int cols) { return (taps * cols + SN_SUM_CHUNK - 1) / SN_SUM_CHUNK; }               // items_ts
inline int sn_ssum_items(int rows) { return (rows + SN_SUM_CHUNK - 1) / SN_SUM_CHUNK; }                                // items_ss
inline long opt_flat_items(long n) { return (n + OPT_CHUNK - 1) / OPT_CHUNK; }                                         // <G,W>, flat AdamW, gradient norm
inline int opt_tile_items(int taps, int rows, int cols) { return taps * ((rows + OPT_TILE - 1) / OPT_TILE) * ((cols + OPT_TILE - 1) / OPT_TILE); }
inline int opt_copy_items(int taps, int rows, int cols) { return taps * ((rows + COPY_TILE - 1) / COPY_TILE) * ((cols + COPY_TILE - 1) / COPY_TILE); }
inline size_t sn_tpart_floats(int taps, int rows, int cols) { return (size_t)sn_row_blocks(rows) * taps * cols; }
inline size_t sn_spart_floats(int taps, int rows, int cols) { return (size_t)taps * sn_col_blocks(cols) * rows; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
#pragma GCC visibility push(hidden)      // host-side table building, shared among the library's files only: kept out of its dynamic symbols
// Scratch of one spectrally-normalised weight: four consecutive 16-byte aligned blocks (tmp_t, tmp_s, tpart, spart)
inline size_t sn_scratch_floats(int taps, int rows, int cols) {
    return align_up((size_t)taps * cols, 4) + align_up((size_t)rows, 4) + align_up(sn_tpart_floats(taps, rows, cols), 4) + align_up(sn_spart_floats(taps, rows, cols), 4);
}
inline void sn_scratch_carve(SNDesc& d, float*& cursor) {      // d.taps / rows / cols set; cursor moves on by sn_scratch_floats
    d.tmp_t = cursor; cursor += align_up((size_t)d.taps * d.cols, 4);
    d.tmp_s = cursor; cursor += align_up((size_t)d.rows, 4);
    d.tpart = cursor; cursor += align_up(sn_tpart_floats(d.taps, d.rows, d.cols), 4);
    d.spart = cursor; cursor += align_up(sn_spart_floats(d.taps, d.rows, d.cols), 4);
}
// SNDesc::wc: W v reads the bf16 copy instead of the master weight where its 16-byte loads fit (bf16 engine, copy present, cols % 8 == 0)
inline const void* sn_compute_copy(bool bf16, const void* copy, int cols) { return bf16 && copy && cols % 8 == 0 ? copy : nullptr; }
// `v` in a fresh device allocation (*dst = null for an empty vector); false: hipMalloc or the copy failed
bool upload_bytes(const void* src, size_t bytes, void** dst);
template <typename T> bool upload_vec(const std::vector<T>& v, T** dst) { return upload_bytes(v.data(), sizeof(T) * v.size(), (void**)dst); }
// The descriptor and work-item tables of the kernels above (opt_tables.hip).  Construction is plain host code: add_sn / add_adam /
// add_copy in any order, then finish(); upload() makes the device copies and the per-item partial buffers, release() frees them.
// Items keep insertion order, except that finish() stable-sorts the DOT, FLAT and TILE lists and the FinDot entries by `group` (the
// engine's gradient buckets: a bucket's share of a pass is one range of its list).  dot_part / gnorm_part are summed in index order, so
// the order of the lists is visible bit for bit in <G,W> and in the gradient norm.
struct OptTables {
    enum List { SN, SN_UNF, TSUM, SSUM, DOT, ADAM, FLAT, TILE, COPY, N_LISTS };
    std::vector<SNDesc> sn;                  // host copies: callers may edit them and copy them to sn_dev / adam_dev again
    std::vector<AdamDesc> adam;
    std::vector<WorkItem> items[N_LISTS];    // SN: power iteration, SN_UNF: without the entries the reuse pass skips; TSUM / SSUM: its partial sums;
                                             // DOT: <G,W>; ADAM: every trainable tensor (gradient norm, untiled AdamW); FLAT / TILE: the two AdamW passes; COPY
    std::vector<FinDot> fin;                 // one per add_sn(.., flat_dot): its DOT items' partials -> SNDesc::dot; src is an index into dot_part until upload()
    std::vector<int> dot_off, fin_off, flat_off, tile_off;   // after finish(): [group] -> first DOT item / fin entry / FLAT item / TILE item, [n_groups] = size
    SNDesc* sn_dev = nullptr; AdamDesc* adam_dev = nullptr;
    WorkItem* dev[N_LISTS] = {};
    float* dot_part = nullptr;               // one float per DOT item
    double* gnorm_part = nullptr;            // one double per AdamW item of a pass: max(FLAT + TILE, ADAM), the tiles' share after the flat items'
    int n(List l) const { return (int)items[l].size(); }
    // d complete (pointers, geometry, active).  Inactive: no SN / TSUM / SSUM items.  skip_in_reuse: its tpart comes from the tiled AdamW, so
    // it stays out of SN_UNF.  flat_dot: <G,W> by the flat pass (DOT items + a FinDot).  Returns the descriptor's index.
    int add_sn(const SNDesc& d, bool skip_in_reuse, bool flat_dot, int group = 0);
    // ADAM items and, by `tiled`, FLAT or TILE items; none for a descriptor without gradient (a.g null: it only carries copies).  Returns its id.
    int add_adam(const AdamDesc& a, bool tiled, int group = 0);
    void add_copy(int adam_id);
    void finish(int n_groups = 1);
    bool upload(int part_fill_byte);         // false: an allocation or copy failed (release() what was made)
    void release();
private:
    std::vector<int> dot_group, fin_group, flat_group, tile_group;     // per element, until finish()
};
#pragma GCC visibility pop
// torch.optim.AdamW defaults and the bias corrections of step `step` (1-based): bc1 = 1 - b1^step, bc2s = sqrt(1 - b2^step)
struct AdamCoef { float b1, b2, bc1, bc2s; };
inline AdamCoef adam_coef(long step) {
    const double b1 = 0.9, b2 = 0.999;
    return {(float)b1, (float)b2, (float)(1.0 - pow(b1, (double)step)), (float)sqrt(1.0 - pow(b2, (double)step))};
}
