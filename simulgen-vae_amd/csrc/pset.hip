// Parameter-set object of the operator-level ABI (include/sgvae_ops.h): the multi-tensor passes of optim.hip (legacy
// spectral-norm power iteration, <G,W> dots, gradient 2-norm, AdamW with the spectral-norm chain rule) over an arbitrary
// list of caller-owned fp32 tensors, so a host-side model (the latent conditioner mirror) spends 8 launches per step on
// its parameters instead of ~5 per tensor.  torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW semantics
// (reference modules/latent_conditioner.py:195-211,304,314).
#include "../../include/sgvae_ops.h"
#include "sgv_ew.h"

#include <math.h>
#include <string.h>
#include <vector>

struct sgv_pset {
    OptTables tab;                                // one group, nothing tiled: every spectral-norm entry gets its <G,W> from the flat pass
    std::vector<int> sn_of_entry;                 // entry -> index into tab.sn, or -1
    float *mv = nullptr, *sigma = nullptr, *dots = nullptr, *tmp = nullptr, *coef = nullptr;
    double* gnorm = nullptr;
    size_t n_tmp = 0, n_dots = 0;
    int step = 0;
};

__global__ void pset_clip_coef_kernel(const double* sumsq, float max_norm, float* out) {
    const float tn = (float)sqrt(sumsq[0]);
    out[0] = max_norm > 0.f ? fminf(1.f, max_norm / (tn + 1e-6f)) : 1.f;
    out[1] = tn;
}

extern "C" {

int sgv_pset_destroy(sgv_pset* ps) {
    if (!ps) return 0;
    void* ptrs[] = {ps->mv, ps->sigma, ps->dots, ps->tmp, ps->coef, ps->gnorm};
    for (void* p : ptrs) if (p) hipFree(p);
    ps->tab.release();
    delete ps;
    return 0;
}

int sgv_pset_create(const sgv_pset_entry* entries, int n, sgv_pset** out) {
    if (!entries || n <= 0 || !out) return sgv_set_error(-1, "sgv_pset_create: bad argument");
    sgv_pset* ps = new sgv_pset();
    size_t total = 0, n_sn = 0, n_tmp = 0;
    for (int i = 0; i < n; ++i) {
        const sgv_pset_entry& e = entries[i];
        if (!e.p || !e.g || e.n <= 0 || e.n % 4 || ((uintptr_t)e.p & 15) || ((uintptr_t)e.g & 15)) {
            delete ps;
            return sgv_set_error(-1, "sgv_pset_create: entry %d needs 16-byte aligned p/g and a multiple of 4 elements (n=%ld)", i, e.n);
        }
        if (e.rows > 0) {
            if ((long)e.rows * e.cols != e.n || e.cols % 4 || !e.u || !e.v) {
                delete ps;
                return sgv_set_error(-1, "sgv_pset_create: spectral-norm entry %d needs rows*cols == n, cols %% 4 == 0 and u, v", i);
            }
            ++n_sn;
            n_tmp += sn_scratch_floats(1, e.rows, e.cols);
        }
        total += align_up((size_t)e.n, 4);
    }
#define PS_ALLOC(ptr, bytes)                                                                   \
    do {                                                                                       \
        if (hipMalloc((void**)&(ptr), (bytes) ? (bytes) : 256) != hipSuccess || hipMemset((ptr), 0, (bytes) ? (bytes) : 256) != hipSuccess) { \
            sgv_pset_destroy(ps);                                                              \
            return sgv_set_error(-2, "sgv_pset_create: allocation of %zu bytes failed", (size_t)(bytes)); \
        }                                                                                      \
    } while (0)
    PS_ALLOC(ps->mv, total * 2 * sizeof(float));
    PS_ALLOC(ps->sigma, (n_sn ? n_sn : 1) * 2 * sizeof(float));
    ps->n_dots = (n_sn ? n_sn : 1) * SGV_DOT_SLOTS;
    PS_ALLOC(ps->dots, ps->n_dots * sizeof(float));
    ps->n_tmp = n_tmp;
    PS_ALLOC(ps->tmp, n_tmp * sizeof(float));
    PS_ALLOC(ps->coef, 2 * sizeof(float));
    PS_ALLOC(ps->gnorm, sizeof(double));
    OptTables& t = ps->tab;
    size_t off = 0;
    float* scratch = ps->tmp;
    ps->sn_of_entry.assign(n, -1);
    for (int i = 0; i < n; ++i) {
        const sgv_pset_entry& e = entries[i];
        AdamDesc a; memset(&a, 0, sizeof(a));
        a.p = e.p; a.g = e.g; a.m = ps->mv + off; a.v = ps->mv + total + off; a.n = e.n; a.sn = -1; a.rows = 1; a.cols = (int)e.n; a.taps = 1;
        off += align_up((size_t)e.n, 4);
        if (e.rows > 0) {
            SNDesc d; memset(&d, 0, sizeof(d));
            const int si = (int)t.sn.size();
            d.W = e.p; d.u = e.u; d.v = e.v;
            d.taps = 1; d.rows = e.rows; d.cols = e.cols; d.active = 1;
            sn_scratch_carve(d, scratch);
            d.sigma = ps->sigma + 2 * si; d.dot = ps->dots + (size_t)si * SGV_DOT_SLOTS; d.G = e.g;
            ps->sn_of_entry[i] = t.add_sn(d, false, true);
            a.sn = si; a.rows = e.rows; a.cols = e.cols;
        }
        t.add_adam(a, false);
    }
    t.finish();
    if (!t.upload(0)) {
        sgv_pset_destroy(ps);
        return sgv_set_error(-2, "sgv_pset_create: table upload failed");
    }
    *out = ps;
    return 0;
}

int sgv_pset_power_iteration(sgv_pset* ps, int train, void* stream) {
    if (!ps) return sgv_set_error(-1, "null parameter set");
    const OptTables& t = ps->tab;
    if (t.sn.empty()) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (opt_sn_power_iteration(t.sn_dev, t.dev[OptTables::SN], t.n(OptTables::SN), t.dev[OptTables::SN], t.n(OptTables::SN), t.dev[OptTables::TSUM],
                               t.n(OptTables::TSUM), t.dev[OptTables::SSUM], t.n(OptTables::SSUM), (int)t.sn.size(), train, s))
        return sgv_set_error(-2, "power-iteration launch failed");
    return 0;
}

const float* sgv_pset_sigma(const sgv_pset* ps, int entry) {
    if (!ps || entry < 0 || entry >= (int)ps->sn_of_entry.size() || ps->sn_of_entry[entry] < 0) return nullptr;
    return ps->sigma + 2 * ps->sn_of_entry[entry];
}

int sgv_pset_step(sgv_pset* ps, float lr, float weight_decay, float max_norm, float* total_norm_host, void* stream) {
    if (!ps) return sgv_set_error(-1, "null parameter set");
    hipStream_t s = (hipStream_t)stream;
    ps->step += 1;
    const AdamCoef c = adam_coef(ps->step);
    // <G,W>/sigma per spectrally-normalised tensor and the gradient norm: per-work-item partials, summed in a fixed order
    const OptTables& t = ps->tab;
    const WorkItem* items_adam = t.dev[OptTables::ADAM];
    const int n_adam = t.n(OptTables::ADAM);
    if (opt_sn_grad_dot(t.sn_dev, t.dev[OptTables::DOT], t.n(OptTables::DOT), t.dot_part, s)) return sgv_set_error(-2, "grad-dot launch failed");
    if (!t.fin.empty() && ew_fin_dots(t.fin.data(), (int)t.fin.size(), s)) return sgv_set_error(-2, "grad-dot sum launch failed");
    if (opt_grad_norm(t.adam_dev, t.sn_dev, items_adam, n_adam, t.gnorm_part, s)) return sgv_set_error(-2, "grad-norm launch failed");
    if (ew_rowsum_d(t.gnorm_part, n_adam, 1, ps->gnorm, 1.0, s)) return sgv_set_error(-2, "grad-norm sum launch failed");
    hipLaunchKernelGGL(pset_clip_coef_kernel, dim3(1), dim3(1), 0, s, ps->gnorm, max_norm, ps->coef);
    if (opt_adamw(t.adam_dev, t.sn_dev, items_adam, n_adam, lr, c.b1, c.b2, 1e-8f, weight_decay, c.bc1, c.bc2s, t.gnorm_part, 0, s, ps->coef))
        return sgv_set_error(-2, "adamw launch failed");
    if (total_norm_host) {
        float h[2] = {0.f, 0.f};
        if (hipMemcpyAsync(h, ps->coef, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return sgv_set_error(-2, "norm read-back failed");
        *total_norm_host = h[1];
    }
    return 0;
}

}  // extern "C"
