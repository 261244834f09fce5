// The surrogate entry points of include/sgvae.h: the decoder from the caller's latents with a recon tail (recon_tails.h) in place of the
// loss tail.  Each is three steps: the null check of what they all take, the tail's builder with the pass's own checks, surrogate_pass
// -- so a bad argument is reported in that order, in front of decode_begin's batch and xs checks.
#include "engine_internal.h"
#include "recon_tails.h"

static int common_ok(const char* who, const sgv_engine* e, const float* z_dev, const float* scale_dev, const float* min_dev) {
    return !e || !z_dev || !scale_dev || !min_dev ? fail(SGV_ERR_ARG, "%s: null argument", who) : 0;
}
// what the entry points share behind their argument checks: decode_begin, no forward left to read (the maps of an earlier forward are
// overwritten from here on, and these passes leave no x_hat behind), the decoder with `tail` as its tail
static int surrogate_pass(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const char* who, const ReconTail& tail) {
    CHK(decode_begin(e, z_dev, xs_dev, batch, who));
    e->have_fwd = false;
    e->fwd_train = false;
    CHK(decoder_fwd(e, batch, 0, mode_fix, &tail));
    for (int s = 0; s < e->n_st; ++s) e->eps_set[s] = 0;
    return SGV_OK;
}

extern "C" {
int sgv_generate(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                 const float* min_dev, int layout, float* out_dev) {
    const char* me = "sgv_generate";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_field(me, "out_dev", scale_dev, min_dev, layout, out_dev, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_set_probes(sgv_engine* e, const int32_t* nodes_host, int count) {
    if (!e) return fail(SGV_ERR_ARG, "sgv_set_probes: null engine");
    if (count < 0 || count > SGV_MAX_PROBES) return fail(SGV_ERR_ARG, "sgv_set_probes: count %d outside [0, %d]", count, SGV_MAX_PROBES);
    if (count > 0 && !nodes_host) return fail(SGV_ERR_ARG, "sgv_set_probes: null node list");
    const int bad = first_bad_probe(nodes_host, count, e->N);
    if (bad >= 0) return fail(SGV_ERR_ARG, "sgv_set_probes: nodes[%d] = %d is outside [0, %d)", bad, (int)nodes_host[bad], e->N);
    if (count > 0) {
        if (!e->probes_dev) HIPCHK(hipMalloc((void**)&e->probes_dev, sizeof(int32_t) * SGV_MAX_PROBES));
        // an upload still in flight reads the old vector: let it finish before the storage changes
        if (!e->probes_host.empty()) HIPCHK(hipStreamSynchronize(e->stream));
        e->probes_host.assign(nodes_host, nodes_host + count);
        HIPCHK(hipMemcpyAsync(e->probes_dev, e->probes_host.data(), sizeof(int32_t) * count, hipMemcpyHostToDevice, e->stream));
    }
    e->n_probes = count;
    return SGV_OK;
}

int sgv_summarize(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                  const float* min_dev, const sgv_summary_out* out) {
    const char* me = "sgv_summarize";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_summary(me, "output", scale_dev, min_dev, out, e->probes_dev, e->n_probes, tail));
    if (out->probes && e->n_probes < 1) return fail(SGV_ERR_ARG, "sgv_summarize: probes asked for, but no probe nodes are set (sgv_set_probes)");
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_score(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
              const float* min_dev, const float* truth_dev, const sgv_score_out* out) {
    const char* me = "sgv_score";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_score(me, "truth_dev", scale_dev, min_dev, truth_dev, out, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_ensemble(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                 const float* min_dev, long count_before, const sgv_ensemble_state* st) {
    const char* me = "sgv_ensemble";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_ensemble(me, "batch", scale_dev, min_dev, count_before, st, batch, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_sobol(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
              const float* min_dev, int n_params, long blocks_before, const sgv_sobol_state* st) {
    const char* me = "sgv_sobol";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_sobol(me, "batch", scale_dev, min_dev, n_params, blocks_before, st, batch, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_distribution(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                     const float* min_dev, long count_before, const sgv_distribution_state* st) {
    const char* me = "sgv_distribution";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_distribution(me, "batch", scale_dev, min_dev, count_before, st, batch, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_regress(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                const float* min_dev, int n_cov, const float* weights_dev, long count_before, const sgv_regress_state* st) {
    const char* me = "sgv_regress";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_regress(me, "batch", scale_dev, min_dev, n_cov, weights_dev, count_before, st, batch, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_project(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                const float* min_dev, const float* weights_dev, int n_func, float* out_dev) {
    const char* me = "sgv_project";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_project(me, scale_dev, min_dev, weights_dev, n_func, out_dev, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_temporal(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                 const float* min_dev, const float* weights_dev, int n_func, float* out_dev) {
    const char* me = "sgv_temporal";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_temporal(me, scale_dev, min_dev, weights_dev, n_func, out_dev, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_gram(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
             const float* min_dev, const float* node_weights_dev_or_NULL, const float* offset_dev_or_NULL, float* out_dev) {
    const char* me = "sgv_gram";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_gram(me, scale_dev, min_dev, e->T, node_weights_dev_or_NULL, offset_dev_or_NULL, out_dev, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_exceedance(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
                   const float* min_dev, const float* levels_dev, int n_level, int side, int32_t* stats_dev_or_NULL,
                   float* excess_dev_or_NULL) {
    const char* me = "sgv_exceedance";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_exceedance(me, scale_dev, min_dev, e->T, levels_dev, n_level, side, stats_dev_or_NULL, excess_dev_or_NULL, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}

int sgv_cycles(sgv_engine* e, const float* z_dev, const float* xs_dev, int batch, int mode_fix, const float* scale_dev,
               const float* min_dev, const float* gate_dev, int exponent, const sgv_cycles_out* out) {
    const char* me = "sgv_cycles";
    ReconTail tail;
    CHK(common_ok(me, e, z_dev, scale_dev, min_dev));
    CHK(tail_cycles(me, scale_dev, min_dev, e->T, gate_dev, exponent, out, tail));
    return surrogate_pass(e, z_dev, xs_dev, batch, mode_fix, me, tail);
}
}  // extern "C"
