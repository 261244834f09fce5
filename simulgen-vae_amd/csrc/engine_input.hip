// Input pipeline: min-max fit and scaling of a raw dataset (no engine), dataset conversion, the augmentation collate and its prefetched form.
#include "engine_internal.h"

// ---- prefetched augmentation (see the members) ----
static constexpr size_t AUG_CTL = 8192;
static bool ensure_aug(sgv_engine* e) {
    if (e->aug_stream) return true;
    if (make_aux_stream(&e->aug_stream, "augmentation", {e->stream, e->side, e->lane2}) != hipSuccess) { e->aug_stream = nullptr; return false; }
    bool ok = hipEventCreateWithFlags(&e->aug_done, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&e->aug_gate, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i) ok = hipEventCreateWithFlags(&e->x_free[i], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMalloc((void**)&e->aug_ctl, AUG_CTL) == hipSuccess;
    if (!ok) { hipStreamDestroy(e->aug_stream); e->aug_stream = nullptr; }
    return ok;
}
// Enqueue the staged batch's kernels, ordered after the current position of the stream the caller enqueues on.  A few samples per
// launch: one launch of 8192 small workgroups would refill every CU as slots free and keep the forward pass's big-LDS workgroups
// (fused Conv+GroupNorm stages, 128-row GEMMs) off the chip until it ends (AdamW slices).
int aug_fire(sgv_engine* e) {
    if (!e->aug_staged || e->aug_fired) return SGV_OK;
    constexpr int per = 2;             // samples per launch
    const int nb = 1 - e->x_cur, batch = e->aug_next_batch;
    char* scratch = e->aug_ctl;
    int* d_idx = (int*)scratch; int* d_mix = d_idx + batch;
    float* d_scale = (float*)(d_mix + batch); float* d_lam = d_scale + batch;
    unsigned long long* d_seed = (unsigned long long*)(scratch + align_up((size_t)batch * 16, 8));
    HIPCHK(hipEventRecord(e->aug_gate, e->stream));
    HIPCHK(hipStreamWaitEvent(e->aug_stream, e->aug_gate, 0));
    const long se = (long)e->N * e->T;
    for (int b0 = 0; b0 < batch; b0 += per) {
        const int nbt = std::min(per, batch - b0);
        ew_augment(e->dt, e->aug_data, (char*)e->x_bufs[nb].p + (size_t)b0 * se * e->esz, se, nbt, d_idx + b0, d_seed + b0, d_scale + b0, d_mix + b0, d_lam + b0, e->aug_stream);
    }
    HIPCHK(hipEventRecord(e->aug_done, e->aug_stream));
    if (e->timing) HIPCHK(hipStreamWaitEvent(e->stream, e->aug_done, 0));      // kernel-timing passes keep the step on one stream
    e->aug_fired = true;
    return SGV_OK;
}
// the main stream takes the batch whose prefetch kernels may still be running
int aug_join(sgv_engine* e) {
    if (e->aug_pending) { HIPCHK(hipStreamWaitEvent(e->stream, e->aug_done, 0)); e->aug_pending = false; }
    return SGV_OK;
}
// the main stream is done reading the current input buffer (end of a forward pass, end of backward)
void x_release(sgv_engine* e) {
    if (!e->aug_stream) return;
    if (hipEventRecord(e->x_free[e->x_cur], e->stream) == hipSuccess) e->x_free_set[e->x_cur] = true;
}

// ---- input pipeline (stateless: no engine needed) ----------------------------------------------------
int sgv_minmax_fit(const float* rows_dev, long n_rows, int n_node, float* min_dev, float* max_dev, int accumulate, void* stream) {
    if (!rows_dev || !min_dev || !max_dev) return fail(SGV_ERR_ARG, "null argument");
    if (n_rows <= 0 || n_node <= 0 || n_node % 4) return fail(SGV_ERR_ARG, "sgv_minmax_fit: n_rows > 0 and n_node %% 4 == 0 required");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SGV_ERR_NOGPU, "no HIP device visible: libsgvae has no CPU fallback");
    float* partial = nullptr;
    HIPCHK(hipMalloc((void**)&partial, sizeof(float) * 2 * (size_t)n_node * SGV_MINMAX_ROWSPLIT));
    int r = ew_minmax_fit(rows_dev, n_rows, n_node, min_dev, max_dev, partial, SGV_MINMAX_ROWSPLIT, accumulate, (hipStream_t)stream);
    hipError_t se = hipStreamSynchronize((hipStream_t)stream);
    hipFree(partial);
    if (r || se != hipSuccess) return fail(SGV_ERR_HIP, "minmax_fit failed");
    return SGV_OK;
}
int sgv_minmax_coeffs(const float* min_dev, const float* max_dev, int n_node, float lo, float hi, float* scale_dev, float* offset_dev, void* stream) {
    if (!min_dev || !max_dev || !scale_dev || !offset_dev || n_node <= 0) return fail(SGV_ERR_ARG, "bad argument");
    if (ew_minmax_coeffs(min_dev, max_dev, n_node, lo, hi, scale_dev, offset_dev, (hipStream_t)stream)) return fail(SGV_ERR_HIP, "minmax_coeffs launch failed");
    return SGV_OK;
}
int sgv_scale_convert(int dst_dtype, const float* src_dev, const float* scale_dev, const float* offset_dev, void* dst_dev, long n_rows, int n_node, void* stream) {
    if (!src_dev || !scale_dev || !offset_dev || !dst_dev) return fail(SGV_ERR_ARG, "null argument");
    if (n_node <= 0 || n_node % 8) return fail(SGV_ERR_ARG, "sgv_scale_convert: n_node %% 8 == 0 required");
    if (dst_dtype != SGV_DTYPE_F32 && dst_dtype != SGV_DTYPE_BF16) return fail(SGV_ERR_ARG, "bad dtype");
    if (ew_scale_convert(dst_dtype, src_dev, scale_dev, offset_dev, dst_dev, n_rows, n_node, (hipStream_t)stream)) return fail(SGV_ERR_HIP, "scale_convert launch failed");
    return SGV_OK;
}

size_t sgv_dataset_sample_bytes(const sgv_engine* e) { return e ? (size_t)e->N * e->T * e->esz : 0; }

int sgv_dataset_convert(sgv_engine* e, const float* src_dev, void* dst_dev, int count) {
    if (!e || !src_dev || !dst_dev) return fail(SGV_ERR_ARG, "null argument");
    ew_transpose(0, e->dt, src_dev, dst_dev, count, e->N, e->T, e->T, e->N, (long)e->N * e->T, (long)e->T * e->N, e->stream);
    return SGV_OK;
}

// The control arrays of a batch in the device layout (idx | mix_idx | scale | lam, then the 8-byte seeds), packed into one of the engine's host
// staging buffers for a single host->device copy (pageable source: staged before the call returns; a buffer is reused four calls later).
static const std::vector<char>& aug_ctl_pack(sgv_engine* e, int batch, const int32_t* idx, const uint64_t* noise_seed, const float* scale,
                                             const int32_t* mix_idx, const float* lam) {
    const size_t seed_off = align_up((size_t)batch * 16, 8);
    std::vector<char>& hb = e->aug_host[e->aug_turn++ & 3];
    hb.resize(seed_off + (size_t)batch * 8);
    char* h = hb.data();
    memcpy(h, idx, batch * 4); memcpy(h + batch * 4, mix_idx, batch * 4);
    memcpy(h + batch * 8, scale, batch * 4); memcpy(h + batch * 12, lam, batch * 4);
    memcpy(h + seed_off, noise_seed, batch * 8);
    return hb;
}

int sgv_augment_collate(sgv_engine* e, const void* dataset_dev, int batch, const int32_t* idx, const uint64_t* noise_seed,
                        const float* scale, const int32_t* mix_idx, const float* lam) {
    if (!e || !dataset_dev || !idx || !noise_seed || !scale || !mix_idx || !lam) return fail(SGV_ERR_ARG, "null argument");
    if (batch < 1 || batch > e->maxB) return fail(SGV_ERR_ARG, "batch %d outside [1,%d]", batch, e->maxB);
    CHK(aug_join(e));
    // small per-sample control arrays go through a device scratch at the head of xpose_tmp
    char* scratch = (char*)e->xpose_tmp;
    int* d_idx = (int*)scratch; int* d_mix = d_idx + batch;
    float* d_scale = (float*)(d_mix + batch); float* d_lam = d_scale + batch;
    unsigned long long* d_seed = (unsigned long long*)(scratch + align_up((size_t)batch * 16, 8));
    const std::vector<char>& hb = aug_ctl_pack(e, batch, idx, noise_seed, scale, mix_idx, lam);
    HIPCHK(hipMemcpyAsync(scratch, hb.data(), hb.size(), hipMemcpyHostToDevice, e->stream));
    ew_augment(e->dt, dataset_dev, e->x_in.p, (long)e->N * e->T, batch, d_idx, d_seed, d_scale, d_mix, d_lam, e->stream);
    x_release(e);
    e->batch = batch;
    e->have_fwd = false;
    return SGV_OK;
}

int sgv_augment_stage(sgv_engine* e, const void* dataset_dev, int batch, const int32_t* idx, const uint64_t* noise_seed,
                      const float* scale, const int32_t* mix_idx, const float* lam) {
    if (!e || !dataset_dev || !idx || !noise_seed || !scale || !mix_idx || !lam) return fail(SGV_ERR_ARG, "null argument");
    if (batch < 1 || batch > e->maxB) return fail(SGV_ERR_ARG, "batch %d outside [1,%d]", batch, e->maxB);
    if (align_up((size_t)batch * 16, 8) + (size_t)batch * 8 > AUG_CTL) return fail(SGV_ERR_ARG, "batch %d: control arrays exceed the staging scratch", batch);
    if (!ensure_aug(e)) return fail(SGV_ERR_HIP, "could not create the augmentation stream");
    // the spare buffer's last reader (the backward pass two steps back, or a pass on a batch that was staged over) has ended;
    // a batch staged before and never advanced to is replaced: same stream, so its kernels precede this copy
    const int nb = 1 - e->x_cur;
    if (e->x_free_set[nb]) HIPCHK(hipStreamWaitEvent(e->aug_stream, e->x_free[nb], 0));
    const std::vector<char>& hb = aug_ctl_pack(e, batch, idx, noise_seed, scale, mix_idx, lam);
    HIPCHK(hipMemcpyAsync(e->aug_ctl, hb.data(), hb.size(), hipMemcpyHostToDevice, e->aug_stream));
    e->aug_data = dataset_dev; e->aug_next_batch = batch;
    e->aug_staged = true; e->aug_fired = false;
    return SGV_OK;
}
int sgv_augment_advance(sgv_engine* e) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (!e->aug_staged) return fail(SGV_ERR_STATE, "sgv_augment_advance: no batch staged (sgv_augment_stage)");
    CHK(aug_fire(e));                        // no training forward since the stage call: the kernels go out now
    e->x_cur = 1 - e->x_cur; e->x_in = e->x_bufs[e->x_cur];
    e->batch = e->aug_next_batch;
    e->have_fwd = false;
    e->aug_staged = false; e->aug_fired = false;
    e->aug_pending = true;                   // the next reader of the batch waits for aug_done
    return SGV_OK;
}
