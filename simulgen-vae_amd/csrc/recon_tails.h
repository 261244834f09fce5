// Private to engine.hip, engine_surrogate.hip and test_hooks.hip: the recon tails (recon_out.hip), the passes that replace the loss tail
// of the recon head in a surrogate pass, each described once.  A ReconTail is all that the engine (decoder_fwd) and a kernel hook
// (recon_hook_run) know about a tail; tail_<pass> checks the pass's own arguments and fills one, for the public entry point
// (engine_surrogate.hip) and for the hook (test_hooks.hip) alike.  Nothing else fills a Recon* struct of sgv_ew.h.
#pragma once
#include <functional>

#include "engine_internal.h"

struct ReconTail {
    const char* tag = nullptr;          // kernel-time tag of the pass
    const char* rejected = nullptr;     // the engine's message when the launcher returns non-zero: a format with one %d
    // >= 0: sample b of the batch is member members_before + b of its study and the decoder's noise follows that index (ensemble,
    // Sobol, distribution, regress); < 0: the noise is drawn per call, from row e->draw_row on
    long members_before = -1;
    // floats of workspace the pass needs behind the statistics; empty: none.  (Set from lambdas, whose handlers are local to the
    // translation unit: a plain function pointer would add std::function's handler for it to the library's dynamic symbols)
    std::function<size_t(int B, int T, int C)> work;
    // the pass's launcher on the recon head's map and statistics in p, with `work` placed where the pass wants it; the launcher's code.
    // Holds the caller's pointers by value and owns nothing.  A pass with a workspace keeps its Recon* struct as the closure's own copy
    // (a mutable lambda) and writes `work` into that copy at each call; std::function's call operator is const, so a const tail runs it
    std::function<int(int dtype, const GNParams& p, float* work, hipStream_t s)> run;
    size_t work_floats(int B, int T, int C) const { return work ? work(B, T, C) : 0; }
};

// ---- limits of the passes, and the checks that more than one caller shares ----
constexpr int SGV_MAX_PROBES = 4096;
constexpr int SGV_DISTRIBUTION_MIN_BINS = 2, SGV_DISTRIBUTION_MAX_BINS = 64;      // HI_MIN_BINS, HI_MAX_BINS of recon_out.hip: the block's byte histogram fits the LDS
constexpr int SGV_REGRESS_MAX_COVARIATES = 32;      // RG_MAX_K of recon_out.hip: the launch's weights fit the block's LDS table
constexpr int SGV_SOBOL_MAX_PARAMS = 30;            // SB_MAX_D of recon_out.hip: a block of n_params + 2 members fits the kernel's member table
// position of the first probe node outside [0, N), -1 if none (sgv_set_probes, sgv_test_recon_summary)
static inline int first_bad_probe(const int32_t* nodes, int count, int N) {
    for (int i = 0; i < count; ++i) if (nodes[i] < 0 || nodes[i] >= N) return i;
    return -1;
}
// members count_before .. count_before + batch - 1 of a study lie in [0, 2^24): ensemble, distribution, regress
static inline int member_range_ok(const char* who, const char* batch_name, long count_before, int batch) {
    if (count_before < 0 || batch < 1 || count_before + batch > (1L << 24))
        return fail(SGV_ERR_ARG, "%s: count_before = %ld with %s = %d is outside [0, 2^24]", who, count_before, batch_name, batch);
    return 0;
}
// on its own because the hook reads the outputs in its probe checks and uploads the probes in front of tail_summary
static inline int summary_out_ok(const char* who, const char* noun, const sgv_summary_out* o) {
    if (!o) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!o->node_stats && !o->node_when && !o->frame_stats && !o->frame_where && !o->probes) return fail(SGV_ERR_ARG, "%s: all five outputs are NULL", who);
    if ((((uintptr_t)o->node_stats | (uintptr_t)o->node_when) & 15) || (((uintptr_t)o->frame_stats | (uintptr_t)o->frame_where) & 7) || ((uintptr_t)o->probes & 3))
        return fail(SGV_ERR_ARG, "%s: misaligned %s (node_stats / node_when 16 bytes, frame_stats / frame_where 8, probes 4)", who, noun);
    return 0;
}

// ---- one builder per pass: 0 and `tail` filled, or SGV_ERR_ARG with the message set.  `who` is the caller's name, the prefix of the
// message, and a second string (out_name, noun, truth_name, batch_name) the one word in which the texts of an entry point and of its
// hook differ.  scale, mn: the caller has checked them, as it has the map; `batch` is the number of samples the pass will see. ----
static inline int tail_field(const char* who, const char* out_name, const float* scale, const float* mn, int layout, float* out, ReconTail& tail) {
    if (!out) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (layout != SGV_LAYOUT_TN && layout != SGV_LAYOUT_NT) return fail(SGV_ERR_ARG, "%s: unknown layout %d", who, layout);
    if ((uintptr_t)out & 15) return fail(SGV_ERR_ARG, "%s: %s must be 16-byte aligned", who, out_name);
    tail.tag = "recon_phys";
    tail.rejected = "sgv_generate: the output pass rejected its arguments (%d: out_dev must be 16-byte aligned)";
    tail.run = [=](int dtype, const GNParams& p, float*, hipStream_t s) { return ew_recon_physical(dtype, p, scale, mn, layout, out, s); };
    return 0;
}
// probe_nodes: n_probes checked node indices on the device; that there are some if o->probes is given is the caller's check
static inline int tail_summary(const char* who, const char* noun, const float* scale, const float* mn, const sgv_summary_out* o, const int* probe_nodes,
                               int n_probes, ReconTail& tail) {
    CHK(summary_out_ok(who, noun, o));
    ReconSummary r;
    r.node_stats = o->node_stats; r.node_when = o->node_when; r.frame_stats = o->frame_stats; r.frame_where = o->frame_where;
    r.probes = o->probes; r.probe_nodes = probe_nodes; r.n_probes = n_probes;
    tail.tag = "recon_summary";
    tail.rejected = "sgv_summarize: the summary pass rejected its arguments (%d)";
    tail.work = [](int B, int T, int C) { return ew_recon_summary_work_floats(B, T, C); };
    tail.run = [=](int dtype, const GNParams& p, float* work, hipStream_t s) mutable { r.work = work; return ew_recon_summary(dtype, p, scale, mn, r, s); };
    return 0;
}
static inline int tail_score(const char* who, const char* truth_name, const float* scale, const float* mn, const float* truth, const sgv_score_out* o,
                             ReconTail& tail) {
    if (!truth || !o) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!o->node_err && !o->node_when && !o->frame_err && !o->frame_where) return fail(SGV_ERR_ARG, "%s: all four outputs are NULL", who);
    if ((((uintptr_t)truth | (uintptr_t)o->node_err | (uintptr_t)o->node_when) & 15) || (((uintptr_t)o->frame_err | (uintptr_t)o->frame_where) & 3))
        return fail(SGV_ERR_ARG, "%s: misaligned pointer (%s, node_err / node_when 16 bytes, frame_err / frame_where 4)", who, truth_name);
    ReconScore r;
    r.node_err = o->node_err; r.node_when = o->node_when; r.frame_err = o->frame_err; r.frame_where = o->frame_where;
    tail.tag = "recon_score";
    tail.rejected = "sgv_score: the error pass rejected its arguments (%d)";
    tail.work = [](int B, int T, int C) { return ew_recon_summary_work_floats(B, T, C); };
    tail.run = [=](int dtype, const GNParams& p, float* work, hipStream_t s) mutable { r.work = work; return ew_recon_score(dtype, p, scale, mn, truth, r, s); };
    return 0;
}
static inline int tail_ensemble(const char* who, const char* batch_name, const float* scale, const float* mn, long count_before, const sgv_ensemble_state* st,
                                int batch, ReconTail& tail) {
    if (!st) return fail(SGV_ERR_ARG, "%s: null argument", who);
    const bool mo = st->mean || st->m2, ex = st->max || st->min || st->arg_max || st->arg_min, ec = st->exceed || st->limit;
    if (!mo && !ex && !ec) return fail(SGV_ERR_ARG, "%s: no group of the state is given", who);
    if ((mo && !(st->mean && st->m2)) || (ex && !(st->max && st->min && st->arg_max && st->arg_min)) || (ec && !(st->exceed && st->limit)))
        return fail(SGV_ERR_ARG, "%s: half a group (mean + m2, max + min + arg_max + arg_min, limit + exceed go together)", who);
    if ((((uintptr_t)st->mean | (uintptr_t)st->m2 | (uintptr_t)st->max | (uintptr_t)st->min | (uintptr_t)st->arg_max | (uintptr_t)st->arg_min |
          (uintptr_t)st->exceed) & 15) || ((uintptr_t)st->limit & 3))
        return fail(SGV_ERR_ARG, "%s: misaligned pointer (the state arrays 16 bytes, limit 4)", who);
    CHK(member_range_ok(who, batch_name, count_before, batch));
    ReconEnsemble r;
    r.mean = st->mean; r.m2 = st->m2; r.vmax = st->max; r.vmin = st->min; r.imax = st->arg_max; r.imin = st->arg_min;
    r.limit = st->limit; r.exceed = st->exceed;
    tail.tag = "recon_ensemble";
    tail.rejected = "sgv_ensemble: the ensemble pass rejected its arguments (%d)";
    tail.members_before = count_before;
    tail.run = [=](int dtype, const GNParams& p, float*, hipStream_t s) { return ew_recon_ensemble(dtype, p, scale, mn, count_before, r, s); };
    return 0;
}
static inline int tail_sobol(const char* who, const char* batch_name, const float* scale, const float* mn, int n_params, long blocks_before,
                             const sgv_sobol_state* st, int batch, ReconTail& tail) {
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
    ReconSobol r;
    r.mean = st->mean; r.m2 = st->m2; r.first_sq = st->first_sq; r.total_sq = st->total_sq;
    tail.tag = "recon_sobol";
    tail.rejected = "sgv_sobol: the Sobol pass rejected its arguments (%d)";
    tail.members_before = blocks_before * (n_params + 2);
    tail.run = [=](int dtype, const GNParams& p, float*, hipStream_t s) { return ew_recon_sobol(dtype, p, scale, mn, n_params, blocks_before, r, s); };
    return 0;
}
static inline int tail_distribution(const char* who, const char* batch_name, const float* scale, const float* mn, long count_before,
                                    const sgv_distribution_state* st, int batch, ReconTail& tail) {
    if (!st) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!st->lo || !st->hi || !st->counts) return fail(SGV_ERR_ARG, "%s: lo, hi and counts are all required", who);
    if (st->bins < SGV_DISTRIBUTION_MIN_BINS || st->bins > SGV_DISTRIBUTION_MAX_BINS)
        return fail(SGV_ERR_ARG, "%s: bins = %d is outside [%d, %d]", who, st->bins, SGV_DISTRIBUTION_MIN_BINS, SGV_DISTRIBUTION_MAX_BINS);
    if (((uintptr_t)st->lo | (uintptr_t)st->hi | (uintptr_t)st->counts) & 15) return fail(SGV_ERR_ARG, "%s: misaligned pointer (lo, hi and counts 16 bytes)", who);
    CHK(member_range_ok(who, batch_name, count_before, batch));
    ReconDistribution r;
    r.lo = st->lo; r.hi = st->hi; r.counts = st->counts; r.bins = st->bins;
    tail.tag = "recon_hist";
    tail.rejected = "sgv_distribution: the distribution pass rejected its arguments (%d)";
    tail.members_before = count_before;
    tail.run = [=](int dtype, const GNParams& p, float*, hipStream_t s) { return ew_recon_distribution(dtype, p, scale, mn, count_before, r, s); };
    return 0;
}
static inline int tail_regress(const char* who, const char* batch_name, const float* scale, const float* mn, int n_cov, const float* weights,
                               long count_before, const sgv_regress_state* st, int batch, ReconTail& tail) {
    if (!st || !weights) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!st->mean || !st->m2 || !st->comoment) return fail(SGV_ERR_ARG, "%s: mean, m2 and comoment are all required", who);
    if (n_cov < 1 || n_cov > SGV_REGRESS_MAX_COVARIATES) return fail(SGV_ERR_ARG, "%s: n_cov = %d is outside [1, %d]", who, n_cov, SGV_REGRESS_MAX_COVARIATES);
    if ((((uintptr_t)st->mean | (uintptr_t)st->m2 | (uintptr_t)st->comoment) & 15) || ((uintptr_t)weights & 3))
        return fail(SGV_ERR_ARG, "%s: misaligned pointer (the state arrays 16 bytes, weights 4)", who);
    CHK(member_range_ok(who, batch_name, count_before, batch));
    ReconRegress r;
    r.mean = st->mean; r.m2 = st->m2; r.co = st->comoment; r.w = weights;
    tail.tag = "recon_regress";
    tail.rejected = "sgv_regress: the regression pass rejected its arguments (%d)";
    tail.members_before = count_before;
    tail.run = [=](int dtype, const GNParams& p, float*, hipStream_t s) { return ew_recon_regress(dtype, p, scale, mn, n_cov, count_before, r, s); };
    return 0;
}
// SGV_MAX_FUNCTIONALS (sgv_ew.h) weight rows at most
static inline int tail_project(const char* who, const float* scale, const float* mn, const float* weights, int n_func, float* out, ReconTail& tail) {
    if (!weights || !out) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (n_func < 1 || n_func > SGV_MAX_FUNCTIONALS) return fail(SGV_ERR_ARG, "%s: n_func = %d is outside [1, %d]", who, n_func, SGV_MAX_FUNCTIONALS);
    if (((uintptr_t)weights & 15) || ((uintptr_t)out & 3)) return fail(SGV_ERR_ARG, "%s: misaligned pointer (weights 16 bytes, out 4)", who);
    ReconProject r;
    r.weights = weights; r.n_func = n_func; r.out = out;
    tail.tag = "recon_project";
    tail.rejected = "sgv_project: the project pass rejected its arguments (%d)";
    tail.work = [=](int B, int T, int C) { return ew_recon_project_work_floats(B, T, C, n_func); };
    tail.run = [=](int dtype, const GNParams& p, float* work, hipStream_t s) mutable { r.work = work; return ew_recon_project(dtype, p, scale, mn, r, s); };
    return 0;
}
// SGV_MAX_TEMPORAL (sgv_ew.h) weight rows at most; the rows of out are written 32 bytes at a time
static inline int tail_temporal(const char* who, const float* scale, const float* mn, const float* weights, int n_func, float* out, ReconTail& tail) {
    if (!weights || !out) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (n_func < 1 || n_func > SGV_MAX_TEMPORAL) return fail(SGV_ERR_ARG, "%s: n_func = %d is outside [1, %d]", who, n_func, SGV_MAX_TEMPORAL);
    if (((uintptr_t)weights & 3) || ((uintptr_t)out & 15)) return fail(SGV_ERR_ARG, "%s: misaligned pointer (weights 4 bytes, out 16)", who);
    ReconTemporal r;
    r.weights = weights; r.n_func = n_func; r.out = out;
    tail.tag = "recon_temporal";
    tail.rejected = "sgv_temporal: the temporal pass rejected its arguments (%d)";
    tail.work = [](int, int T, int) { return ew_recon_temporal_work_floats(T); };
    tail.run = [=](int dtype, const GNParams& p, float* work, hipStream_t s) mutable { r.work = work; return ew_recon_temporal(dtype, p, scale, mn, r, s); };
    return 0;
}
// T <= SGV_MAX_GRAM_T (sgv_ew.h) row tiles fit the kernel's accumulators; the weights and the offset may be null
static inline int tail_gram(const char* who, const float* scale, const float* mn, int T, const float* node_weights, const float* offset, float* out,
                            ReconTail& tail) {
    if (!out) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (T > SGV_MAX_GRAM_T) return fail(SGV_ERR_ARG, "%s: T = %d is beyond the limit of %d time steps", who, T, SGV_MAX_GRAM_T);
    if ((((uintptr_t)node_weights | (uintptr_t)offset) & 15) || ((uintptr_t)out & 3)) return fail(SGV_ERR_ARG, "%s: misaligned pointer (node_weights and offset 16 bytes, out 4)", who);
    ReconGram r;
    r.node_weights = node_weights; r.offset = offset; r.out = out;
    tail.tag = "recon_gram";
    tail.rejected = "sgv_gram: the Gram pass rejected its arguments (%d)";
    tail.work = [](int B, int T, int C) { return ew_recon_gram_work_floats(B, T, C); };
    tail.run = [=](int dtype, const GNParams& p, float* work, hipStream_t s) mutable { r.work = work; return ew_recon_gram(dtype, p, scale, mn, r, s); };
    return 0;
}
// SGV_MAX_EXCEED_LEVELS (sgv_ew.h) levels at most, T within the kernel's packed 16-bit counters; the rows of both outputs are written
// 32 bytes at a time
static inline int tail_exceedance(const char* who, const float* scale, const float* mn, int T, const float* levels, int n_level, int side, int32_t* stats,
                                  float* excess, ReconTail& tail) {
    if (!levels) return fail(SGV_ERR_ARG, "%s: null argument", who);
    if (!stats && !excess) return fail(SGV_ERR_ARG, "%s: no output (stats and excess are both null)", who);
    if (n_level < 1 || n_level > SGV_MAX_EXCEED_LEVELS) return fail(SGV_ERR_ARG, "%s: n_level = %d is outside [1, %d]", who, n_level, SGV_MAX_EXCEED_LEVELS);
    if (side != SGV_SIDE_ABOVE && side != SGV_SIDE_BELOW) return fail(SGV_ERR_ARG, "%s: unknown side %d", who, side);
    if (T > 65535) return fail(SGV_ERR_ARG, "%s: T = %d is beyond the limit of 65535 time steps", who, T);
    if (((uintptr_t)levels & 3) || (((uintptr_t)stats | (uintptr_t)excess) & 15)) return fail(SGV_ERR_ARG, "%s: misaligned pointer (levels 4 bytes, stats and excess 16)", who);
    ReconExceed r;
    r.levels = levels; r.n_level = n_level; r.above = side == SGV_SIDE_ABOVE; r.stats = stats; r.excess = excess;
    tail.tag = "recon_exceed";
    tail.rejected = "sgv_exceedance: the exceedance pass rejected its arguments (%d)";
    tail.run = [=](int dtype, const GNParams& p, float*, hipStream_t s) { return ew_recon_exceedance(dtype, p, scale, mn, r, s); };
    return 0;
}
// exponent within [1, SGV_MAX_CYCLES_EXPONENT] (sgv_ew.h), T within the kernel's packed 16-bit counters; a group of outputs whole or not
// at all; the rows of the outputs are written 32 bytes at a time
static inline int tail_cycles(const char* who, const float* scale, const float* mn, int T, const float* gate, int exponent, const sgv_cycles_out* o,
                              ReconTail& tail) {
    if (!gate || !o) return fail(SGV_ERR_ARG, "%s: null argument", who);
    const bool turns = o->reversals || o->ranges, rates = o->rate_when || o->rates;
    if (!turns && !rates) return fail(SGV_ERR_ARG, "%s: no group of the outputs is given", who);
    if ((turns && !(o->reversals && o->ranges)) || (rates && !(o->rate_when && o->rates)))
        return fail(SGV_ERR_ARG, "%s: half a group (reversals + ranges, rate_when + rates go together)", who);
    if (exponent < 1 || exponent > SGV_MAX_CYCLES_EXPONENT) return fail(SGV_ERR_ARG, "%s: exponent = %d is outside [1, %d]", who, exponent, SGV_MAX_CYCLES_EXPONENT);
    if (T > 65535) return fail(SGV_ERR_ARG, "%s: T = %d is beyond the limit of 65535 time steps", who, T);
    if (((uintptr_t)gate & 3) || (((uintptr_t)o->reversals | (uintptr_t)o->ranges | (uintptr_t)o->rate_when | (uintptr_t)o->rates) & 15))
        return fail(SGV_ERR_ARG, "%s: misaligned pointer (gate 4 bytes, the outputs 16)", who);
    ReconCycles r;
    r.gate = gate; r.exponent = exponent; r.reversals = o->reversals; r.ranges = o->ranges; r.rate_when = o->rate_when; r.rates = o->rates;
    tail.tag = "recon_cycles";
    tail.rejected = "sgv_cycles: the cycles pass rejected its arguments (%d)";
    tail.run = [=](int dtype, const GNParams& p, float*, hipStream_t s) { return ew_recon_cycles(dtype, p, scale, mn, r, s); };
    return 0;
}
