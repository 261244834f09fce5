// Gradients after they exist: the bf16 gradient mirror, the AdamW scheduling, the release policy of the gradient buckets during
// backward (GradRelease), and the entry points of the C ABI that are only about gradients and the optimizer.
#include "engine_internal.h"

// ---- bf16 weight gradients straight from the 256 x 256 kernel (see the grad_bf16 member) ----
// which layers: those whose weight-gradient GEMM takes that kernel, unsplit, at the engine's full batch, and whose mirror range the
// launcher accepts as its bf16 output (alignment, offset ranges: a refused launch must never be left to write the mirror) -- fixed
// once: the AdamW table points the layer at the mirror arena
static void classify_lp(sgv_engine* e) {
    if (e->lp_classified) return;
    const long M = (long)e->maxB * e->T;
    for (auto& l : e->layers) {
        l.lp = false;
        if (!layer_fused_adam(l) || e->dt != SGV_DTYPE_BF16 || !e->use_tr) continue;
        GemmTN q; memset(&q, 0, sizeof(q));
        q.M = (int)M; q.N1 = l.cout; q.N2 = l.cin; q.taps = l.k; q.pad = (l.k - 1) / 2; q.Tlen = e->T; q.lda = l.cout; q.ldb = l.cin; q.ldo = l.cin; q.use_tr = 1; q.splitk = 1;
        q.out = reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(e->grads_lp) + l.gw); q.out_bf16 = 1;
        l.lp = gemm_tn_uses_t256(e->dt, q) && gemm_tn256_accepts(q) && gemm_tn_pick_splitk(q.M, q.N1, q.N2, q.taps, e->dt, e->T) == 1;
    }
    e->bucket_lp_layers.assign(e->buckets.size(), {});
    for (size_t b = 0; b + 1 < e->buckets.size(); ++b) {
        std::vector<std::pair<size_t, int>> v;
        for (size_t i = 0; i < e->layers.size(); ++i) {
            const Layer& l = e->layers[i];
            if (l.lp && l.gw >= e->buckets[b].first && l.gw < e->buckets[b].first + e->buckets[b].second) v.push_back({l.gw, (int)i});
        }
        std::sort(v.begin(), v.end());
        for (auto& x : v) e->bucket_lp_layers[b].push_back(x.second);
    }
    e->lp_classified = true;
}
static int ensure_lp_mirror(sgv_engine* e) {
    if (!e->grads_lp) HIPCHK(hipMalloc(&e->grads_lp, e->n_grads * 2));
    classify_lp(e);
    return 0;
}
// single-GPU option: no communicator, no bucket callback
bool grad_lp_active(const sgv_engine* e) { return e->grad_bf16 && e->grads_lp && !e->comm && !e->cb; }
// data-parallel step with the bf16 wire format (the condition under which fire_at packs a bucket)
bool wire_lp_active(sgv_engine* e) {
    const char* off = getenv("SGV_WIRE_DIRECT");           // read per call: a test compares both forms in one process
    if (off && atoi(off) == 0) return false;
    return e->payload_bf16 && e->grads_lp && e->lp_classified && (e->comm ? !comm_is_single(e->comm) : e->cb != nullptr);
}
// the fp32 arena of the layers whose last gradient was stored as bf16: refreshed for the calls that read it.  (After a
// data-parallel step the mirror holds the averaged gradient of those layers.)
int lp_sync(sgv_engine* e) {
    for (size_t i = 0; i < e->layers.size(); ++i) {
        if (!e->lp_dirty[i]) continue;
        const Layer& l = e->layers[i];
        ew_unpack_bf16((const char*)e->grads_lp + 2 * l.gw, e->grads + l.gw, l.nw(), e->stream);
        e->lp_dirty[i] = 0;
    }
    return 0;
}
// a bucket's fp32 gradients -> the bf16 wire copy, except the layers whose GEMM wrote the copy itself
static void pack_bucket(sgv_engine* e, int b, hipStream_t st) {
    size_t cur = e->buckets[b].first;
    const size_t end = cur + e->buckets[b].second;
    if (e->lp_classified && b < (int)e->bucket_lp_layers.size())
        for (int li : e->bucket_lp_layers[b]) {
            const Layer& l = e->layers[li];
            if (!e->lp_dirty[li]) continue;
            if (l.gw > cur) ew_pack_bf16(e->grads + cur, (char*)e->grads_lp + 2 * cur, (long)(l.gw - cur), st);
            cur = l.gw + align_up((size_t)l.nw(), 4);
        }
    if (end > cur) ew_pack_bf16(e->grads + cur, (char*)e->grads_lp + 2 * cur, (long)(end - cur), st);
}
// option "grad_bf16" (see the member)
int set_grad_bf16(sgv_engine* e, int value) {
    if (value && (e->dt != SGV_DTYPE_BF16)) return fail(SGV_ERR_ARG, "grad_bf16 needs a bf16 engine");
    CHK(lp_sync(e));
    if (value) {
        CHK(ensure_lp_mirror(e));
        // point the optimizer's table at the mirror for the classified layers (the kernel follows the pointer only when the launch
        // says so: adamw_tiles)
        bool changed = false;
        for (auto& a : e->tab.adam) {
            if (a.sn < 0 || a.sn >= (int)e->layers.size()) continue;
            const Layer& l = e->layers[a.sn];
            if (!l.lp || a.g != e->grads + l.gw || a.glp) continue;
            a.glp = reinterpret_cast<const unsigned short*>(e->grads_lp) + l.gw; changed = true;
        }
        if (changed) { HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipMemcpy(e->tab.adam_dev, e->tab.adam.data(), sizeof(AdamDesc) * e->tab.adam.size(), hipMemcpyHostToDevice)); }
    }
    e->grad_bf16 = value != 0;
    return 0;
}

// which: 1 = conv-weight tiles, 2 = flat items (biases, GroupNorm affine, Linear heads), 3 = both
static int adamw_begin(sgv_engine* e) {
    if (e->adam_open) return 0;          // a bucket of this step was updated ahead of the caller's first=1 call
    e->step += 1;
    e->copies_fresh = false;
    e->wtu_fresh = false;
    e->adam_open = true;
    e->bucket_updated.assign(e->buckets.size(), 0);
    return 0;
}
// end of an optimisation step: whatever ran on the optimizer stream joins the engine stream, gradient norm^2 in a fixed order
static int adamw_finish(sgv_engine* e) {
    if (e->opt_dirty) {
        CHK(stream_wait(e, e->stream, e->opt));
        e->opt_dirty = false;
    }
    e->copies_fresh = true;
    e->wtu_fresh = true;
    e->adam_open = false;
    ew_rowsum_d(e->tab.gnorm_part, e->tab.n(OptTables::FLAT) + e->tab.n(OptTables::TILE), 1, e->scal + 15, 1.0, e->stream);
    return 0;
}
static int adamw_tiles(sgv_engine* e, float lr, int t0, int t1, hipStream_t st, bool from_lp) {
    if (t1 <= t0) return 0;
    const AdamCoef c = adam_coef(e->step);
    // Beside the backward pass (any stream but the main one) the pass goes out in slices of 3072 64 x 64 tiles: its
    // workgroups are small and short-lived, so while one launch lasts they refill every CU the moment a slot frees, and a kernel of
    // the main stream whose workgroup needs most of a CU's LDS (the 128-row GEMM tails, the fused Conv+GroupNorm stages) is not
    // placed until the launch ends -- a kernel trace showed a 60 us tail taking 816 us beside a 1.3 ms AdamW launch.  At a launch
    // boundary the chip drains, and the waiting workgroups get their CUs.
    constexpr int ADAM_SLICE = 3072;    // re-tuned on the final build: 2048 / 2560 / 3072 / 3584 = 11.16 / 11.11 / 11.10 / 11.11 ms
    const int slice = st != e->stream ? ADAM_SLICE : t1 - t0;
    for (int a = t0; a < t1; a += slice) {
        const int b = std::min(t1, a + slice);
        if (opt_adamw_sn(e->tab.adam_dev, e->tab.sn_dev, e->tab.dev[OptTables::TILE] + a, b - a, lr, c.b1, c.b2, 1e-8f, 0.01f, c.bc1, c.bc2s, e->tab.gnorm_part + e->tab.n(OptTables::FLAT) + a, e->dt, st,
                         e->grads, from_lp ? e->grads_lp : nullptr, (!from_lp && grad_lp_active(e) && !e->lp_fp32) ? 1 : 0))
            return fail(SGV_ERR_HIP, "adamw launch failed");
    }
    return 0;
}
// what the flat pass reads of a packed weight bucket (Linear heads)
static void unpack_bucket_flat(sgv_engine* e, int b, hipStream_t st) {
    for (auto& r : e->bucket_flat_w[b]) ew_unpack_bf16((const char*)e->grads_lp + 2 * r.first, e->grads + r.first, (long)r.second, st);
    e->bucket_packed[b] &= ~2;
}
static int adamw_range(sgv_engine* e, float lr, int bucket_lo, int bucket_hi, int which, hipStream_t st) {
    // native RCCL path: the all-reduce of every bucket touched here must have landed, and so must the small bucket's
    // (last index): it carries the <G,W> scalars every conv weight's update reads
    const int n_pend = (int)e->bucket_pending.size();
    for (int b = bucket_lo; b < n_pend; b = (b + 1 < bucket_hi ? b + 1 : (b < n_pend - 1 ? n_pend - 1 : n_pend)))
        if (e->bucket_pending[b]) {
            HIPCHK(hipStreamWaitEvent(st, e->bucket_done[b], 0));
            e->bucket_pending[b] = 0;
        }
    // the averaged bf16 wire copy: the tiled pass reads it in place, the flat pass gets its few weights unpacked
    const int np = (int)e->bucket_packed.size();
    for (int b = bucket_lo; b < bucket_hi && b < np; ++b)
        if ((which & 2) && (e->bucket_packed[b] & 2)) unpack_bucket_flat(e, b, st);
    // biases, GroupNorm affine and the Linear heads: flat pass.  Conv weights: tiled pass that also writes both
    // compute copies and W_new^T u for the next forward's power iteration; buckets updated ahead (adamw_bucket_async) are skipped.
    const AdamCoef c = adam_coef(e->step);
    const int f0 = e->tab.flat_off[bucket_lo], f1 = e->tab.flat_off[bucket_hi];
    if ((which & 2) && opt_adamw(e->tab.adam_dev, e->tab.sn_dev, e->tab.dev[OptTables::FLAT] + f0, f1 - f0, lr, c.b1, c.b2, 1e-8f, 0.01f, c.bc1, c.bc2s, e->tab.gnorm_part + f0, e->dt, st))
        return fail(SGV_ERR_HIP, "adamw launch failed");
    if (which & 1) {
        const int nu = (int)e->bucket_updated.size();
        auto skip = [&](int b) { return b < nu && e->bucket_updated[b]; };
        auto lp = [&](int b) { return b < np && (e->bucket_packed[b] & 1); };
        for (int b = bucket_lo; b < bucket_hi;) {
            if (skip(b)) { ++b; continue; }
            int h = b + 1;
            while (h < bucket_hi && !skip(h) && lp(h) == lp(b)) ++h;          // runs of buckets read from the same place
            CHK(adamw_tiles(e, lr, e->tab.tile_off[b], e->tab.tile_off[h], st, lp(b)));
            for (int k = b; k < h; ++k) if (k < np) e->bucket_packed[k] &= ~1;
            b = h;
        }
    }
    return 0;
}
// conv-weight AdamW of ONE weight bucket on `st`, ahead of the rest of the step: the caller has made `st` wait for the bucket's
// gradients (and their all-reduce) and for the <G,W> slots of its layers (bucket_dots)
static int adamw_bucket_async(sgv_engine* e, float lr, int b, hipStream_t st) {
    CHK(adamw_begin(e));
    const bool packed = b < (int)e->bucket_packed.size() && e->bucket_packed[b];
    const bool from_lp = packed && (e->bucket_packed[b] & 1);
    CHK(adamw_tiles(e, lr, e->tab.tile_off[b], e->tab.tile_off[b + 1], st, from_lp));
    if (from_lp) e->bucket_packed[b] &= ~1;
    e->bucket_updated[b] = 1;
    if (st != e->stream) e->opt_dirty = e->opt_dirty || st == e->opt;
    return 0;
}

// ---- GradRelease (engine_internal.h): when a gradient bucket is complete and what happens to it then ----
// fuse_lr >= 0: also run the optimizer, and start the AdamW of every conv-weight bucket on the side stream as soon as
// that bucket's gradients are final, under the rest of backward (single-GPU path: no bucket callback registered)
int GradRelease::begin() {
    fuse = fuse_lr >= 0.f;
    early = fuse && !e->cb && !e->comm && e->side && e->use_side && !e->timing;
    // engine-issued collectives with the learning rate in hand (sgv_backward_step on a registered communicator): every weight
    // bucket's <G,W> slots are averaged with the bucket and its conv-weight AdamW starts on the optimizer stream as soon as both
    // have landed, under the rest of backward -- the data-parallel mirror of `early`
    dearly = e->ddp_early && fuse && e->comm && !comm_is_single(e->comm) && !e->timing && ensure_opt(e);
    if (early || dearly) CHK(adamw_begin(e));
    // chunked exchange of the last weight bucket: it must be exactly the first encoder layer's tiled weight
    last_b = (int)e->buckets.size() - 2;
    L0i = e->encA[0].st[0].layer;
    if (dearly && e->ddp_last_chunks > 1 && last_b >= 0) {
        const Layer& L0 = e->layers[L0i];
        const int rt6 = (L0.cout + 63) / 64, ct6 = (L0.cin + 63) / 64;
        last_chunked = e->encA[0].st.size() == 1 && L0.k == 1 && L0.has_grad && layer_fused_adam(L0) && L0.cout % (128 * e->ddp_last_chunks) == 0 &&
                       e->buckets[last_b].first == L0.gw && e->buckets[last_b].second == align_up((size_t)L0.nw(), 4) &&
                       e->tab.tile_off[last_b + 1] - e->tab.tile_off[last_b] == rt6 * ct6 && e->tab.flat_off[last_b + 1] == e->tab.flat_off[last_b] &&
                       2.0e-9 * (double)((long)e->batch * e->T) * L0.cout * L0.cin > e->ddp_chunk_min_gf;      // the big-GEMM regime: main stream, split-K 1
    }
    // <G,W_eff> of the Linear layers is computed from G itself: in one launch at the end of backward -- unless a collective may
    // already be reducing a released bucket's gradients in place by then (fp32 wire format): with a callback or a communicator
    // every bucket's Linear layers get theirs at the bucket's fire point.  Same per-item partials, same fixed-order sums.
    dots_per_bucket = e->cb || e->comm;
    return 0;
}
// the inputs of a bucket's collective are what the main stream and the side stream hold so far.  They are gathered on the
// stream the collective is issued from (the communicator's stream; with a callback the wire stream, option "wire_stream"), and
// the bf16 wire copy is packed THERE: the main stream neither waits for the side stream's weight-gradient GEMMs nor runs the
// pack pass (0.45 ms per step at preset 1).  Without a wire stream (a caller that orders itself after the engine stream) the
// main stream joins the side stream and packs, as before.
int GradRelease::gather_on(hipStream_t t) {
    CHK(stream_wait(e, t, e->stream));
    if (e->side_dirty) CHK(stream_wait(e, t, e->side));
    return 0;
}
void GradRelease::fire_at(int b) {
    if (b < 0 || b >= (int)e->buckets.size()) return;
    if (e->cb || (e->comm && !comm_is_single(e->comm))) e->coll_inflight = true;
    if (e->comm || e->cb) {
        const hipStream_t ws = e->comm ? e->comm_stream : (e->use_wire ? e->wire : nullptr);
        if (ws ? gather_on(ws) : join_side(e)) { failed(ws ? "gathering a bucket on its wire stream" : "joining the side stream"); return; }
        if (e->payload_bf16 && b != (int)e->buckets.size() - 1 && !(e->comm && comm_is_single(e->comm))) {
            pack_bucket(e, b, ws ? ws : e->stream);
            e->bucket_packed[b] = 3;
        }
    }
    if (e->comm) {
        if (rccl_bucket(e, e->comm, e->comm_stream, b, e->bucket_done[b], dearly)) { failed("a bucket's all-reduce"); return; }
        e->bucket_pending[b] = 1;
        if (dearly && b < (int)e->buckets.size() - 2) {
            if (hipStreamWaitEvent(e->opt, e->bucket_done[b], 0) != hipSuccess) { failed("the optimizer stream's wait for a bucket"); return; }
            e->bucket_pending[b] = 0;
            if (adamw_bucket_async(e, fuse_lr, b, e->opt)) failed("a bucket's AdamW on the optimizer stream");
        }
    } else if (e->cb) {
        e->cb(e->cb_user, b, e->buckets[b].first, e->buckets[b].second);
    } else if (early && b < (int)e->buckets.size() - 2) {
        // the bucket's weight gradients (and the <G,W> slots of its conv layers) are final once everything enqueued
        // so far has run: AdamW of its conv weights goes to the side stream, under the remaining backward
        if (stream_wait(e, e->side, e->stream)) { failed("the side stream's wait for a bucket"); return; }
        if (adamw_range(e, fuse_lr, b, b + 1, 1, e->side)) failed("a bucket's AdamW on the side stream");
        e->side_dirty = true;
    }
}
// fixed-order sums of the partials collected so far: the <G,W_eff> scalars of the layers whose dY kernels have been enqueued
// (every fire point: the bucket's AdamW / all-reduce reads them), the GroupNorm affine and bias gradients (small bucket)
void GradRelease::flush_fin(bool affine) {
    if (!e->fin_dots.empty()) { ew_fin_dots(e->fin_dots.data(), (int)e->fin_dots.size(), e->stream); e->fin_dots.clear(); }
    if (affine && !e->fin_affine.empty()) { ew_fin_affine(e->fin_affine.data(), (int)e->fin_affine.size(), e->stream); e->fin_affine.clear(); }
}
void GradRelease::lin_dots(int b0, int b1) {
    const int d0 = e->tab.dot_off[b0], d1 = e->tab.dot_off[b1];
    if (d1 > d0 && opt_sn_grad_dot(e->tab.sn_dev, e->tab.dev[OptTables::DOT] + d0, d1 - d0, e->tab.dot_part + d0, e->stream)) lin_err = true;
    e->fin_dots.insert(e->fin_dots.end(), e->tab.fin.begin() + e->tab.fin_off[b0], e->tab.fin.begin() + e->tab.fin_off[b1]);
}
void GradRelease::fire() { if (dots_per_bucket) lin_dots(bucket, bucket + 1); flush_fin(false); fire_at(bucket); ++bucket; }
// the small zone (biases, GroupNorm affine, <G,W_eff> scalars) is complete once the first conv's dY exists:
// release it BEFORE the first-layer weight-gradient GEMM so that its all-reduce (and, with it, the AdamW
// of every other layer) does not queue behind the 390 MB first-layer bucket
void GradRelease::release_small() { flush_fin(true); fire_at((int)e->buckets.size() - 1); }
// in front of the first encoder block's backward: everything but that block's weight gradients is now enqueued
int GradRelease::before_first_block() {
    fire();
    // <G,W_eff> of the (small) Linear layers from their weights; conv layers accumulated theirs in the dY kernels
    if (!dots_per_bucket) lin_dots(0, (int)e->buckets.size());
    if (lin_err) return fail(SGV_ERR_HIP, "grad-dot launch failed");
    if (last_chunked) { e->dw_chunks = e->ddp_last_chunks; e->dw_chunk_layer = L0i; }
    return 0;
}
// after GEMM chunk c of n_c (rows co0..co1 of the first layer's weight gradient) is enqueued: its exchange, on the communicator's stream
int GradRelease::after_chunk(int c, int n_c, int co0, int co1) {
    const Layer& L0 = e->layers[L0i];
    const size_t off = L0.gw + (size_t)co0 * L0.cin, cnt = (size_t)(co1 - co0) * L0.cin;
    const hipStream_t cs = e->comm_stream;
    if (gather_on(cs)) return 1;                                  // the chunk's GEMM (main stream)
    const bool lp = e->payload_bf16 != 0;
    void* w = lp ? (void*)((char*)e->grads_lp + 2 * off) : (void*)(e->grads + off);
    if (lp && !e->dw_chunk_direct) ew_pack_bf16(e->grads + off, w, (long)cnt, cs);
    if (g_rccl.AllReduce(w, w, cnt, lp ? kNcclBfloat16 : kNcclFloat32, kNcclAvg, e->comm, cs)) return 1;
    if (c == 0 && e->bucket_dots[last_b].second) {
        float* d = e->grads + e->bucket_dots[last_b].first;
        if (g_rccl.AllReduce(d, d, e->bucket_dots[last_b].second, kNcclFloat32, kNcclAvg, e->comm, cs)) return 1;
    }
    hipEvent_t ev = c == n_c - 1 ? e->bucket_done[last_b] : next_event(e);
    if (!ev || hipEventRecord(ev, cs) != hipSuccess) return 1;
    chunk_done.push_back(ev);
    return 0;
}
int GradRelease::after_first_block(int br) {
    e->dw_chunks = 1; e->dw_chunk_layer = -1;
    CHK(br);
    if (last_chunked && (int)chunk_done.size() == e->ddp_last_chunks) {
        // the chunks' updates go to the MAIN stream, behind the last GEMM chunk: it has nothing else left to do, and chunk c's
        // AdamW then runs beside chunk c + 1's exchange instead of in front of it on the communication stream's queue
        const Layer& L0 = e->layers[L0i];
        const int n_c = e->ddp_last_chunks, rows = L0.cout / n_c, ct6 = (L0.cin + 63) / 64;
        const bool lp = e->payload_bf16 != 0;
        for (int c = 0; c < n_c; ++c) {
            HIPCHK(hipStreamWaitEvent(e->stream, chunk_done[c], 0));
            CHK(adamw_tiles(e, fuse_lr, e->tab.tile_off[last_b] + (c * rows / 64) * ct6, e->tab.tile_off[last_b] + ((c + 1) * rows / 64) * ct6, e->stream, lp));
        }
        e->bucket_updated[last_b] = 1;
    }
    return 0;
}
// the first encoder block's weights, then what is left of the step
int GradRelease::finish() {
    if (last_chunked && e->bucket_updated[last_b]) ++bucket;      // exchanged and updated chunk by chunk above
    else fire();
    if (err) return fail(SGV_ERR_HIP, "gradient bucket release: %s failed", err);
    const int nbk = (int)e->buckets.size();
    CHK(join_side(e));                                                // side-stream dW GEMMs of the last bucket
    if (early) {
        CHK(adamw_range(e, fuse_lr, nbk - 2, nbk - 1, 1, e->stream)); // first encoder block's conv weights
        CHK(adamw_range(e, fuse_lr, 0, nbk, 2, e->stream));           // every flat item
        e->side_dirty = true;                                          // AdamW launches may still run on the side stream
        CHK(join_side(e));
        CHK(adamw_finish(e));
    } else if (fuse && !e->cb) {
        CHK(sgv_adamw_step(e, fuse_lr));
    }
    return SGV_OK;
}

extern "C" {
int sgv_grad_buffer(sgv_engine* e, float** dev_ptr, size_t* count_elems) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    // grad_bf16: the caller may read or write the arena from here on -- it gets the gradients of the last backward, and what it
    // leaves there is what the next AdamW reads (the refresh is finished before the pointer is handed out)
    if (std::find(e->lp_dirty.begin(), e->lp_dirty.end(), 1) != e->lp_dirty.end()) {
        CHK(lp_sync(e));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    e->lp_fp32 = true;
    if (dev_ptr) *dev_ptr = e->grads;
    if (count_elems) *count_elems = e->n_grads;
    return SGV_OK;
}
int sgv_scale_grads(sgv_engine* e, float factor) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    CHK(lp_sync(e));                     // grad_bf16: the gradient of the mirrored layers into the fp32 arena, scaled there with the rest
    e->lp_fp32 = true;
    ew_scale(e->grads, factor, (long)e->n_grads, e->stream);
    return SGV_OK;
}
int sgv_grad_norm(sgv_engine* e, double* out) {
    if (!e || !out) return fail(SGV_ERR_ARG, "null argument");
    CHK(lp_sync(e));
    if (opt_grad_norm(e->tab.adam_dev, e->tab.sn_dev, e->tab.dev[OptTables::ADAM], e->tab.n(OptTables::ADAM), e->tab.gnorm_part, e->stream)) return fail(SGV_ERR_HIP, "grad-norm launch failed");
    ew_rowsum_d(e->tab.gnorm_part, e->tab.n(OptTables::ADAM), 1, e->scal + 15, 1.0, e->stream);
    double h = 0.0;
    HIPCHK(hipMemcpyAsync(&h, e->scal + 15, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    *out = sqrt(h);
    return SGV_OK;
}
int sgv_bucket_dots(const sgv_engine* e, int bucket, size_t* offset_elems, size_t* count_elems) {
    if (!e || !offset_elems || !count_elems) return fail(SGV_ERR_ARG, "null argument");
    if (bucket < 0 || bucket >= (int)e->bucket_dots.size()) return fail(SGV_ERR_ARG, "bucket %d is not a weight bucket [0,%d)", bucket, (int)e->bucket_dots.size());
    *offset_elems = e->bucket_dots[bucket].first; *count_elems = e->bucket_dots[bucket].second;
    return SGV_OK;
}
int sgv_adamw_bucket_async(sgv_engine* e, float lr, int bucket) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (lr < 0.f) return fail(SGV_ERR_ARG, "negative learning rate");
    if (!ensure_opt(e)) return fail(SGV_ERR_HIP, "the engine has no optimizer stream");
    if (bucket < 0 || bucket >= (int)e->buckets.size() - 1) return fail(SGV_ERR_ARG, "bucket %d is not a weight bucket [0,%d)", bucket, (int)e->buckets.size() - 1);
    if (e->adam_open && e->bucket_updated[bucket]) return fail(SGV_ERR_STATE, "bucket %d was already updated in this step", bucket);
    return adamw_bucket_async(e, lr, bucket, e->opt);
}
int sgv_adamw_step_range(sgv_engine* e, float lr, int bucket_lo, int bucket_hi, int first, int last) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    const int nbk = (int)e->buckets.size();
    if (bucket_lo < 0 || bucket_hi > nbk || bucket_lo > bucket_hi) return fail(SGV_ERR_ARG, "bucket range [%d,%d) outside [0,%d)", bucket_lo, bucket_hi, nbk);
    if (first) CHK(adamw_begin(e));
    if (e->step < 1 || !e->adam_open) return fail(SGV_ERR_STATE, "sgv_adamw_step_range: the first call of a step must pass first=1");
    CHK(adamw_range(e, lr, bucket_lo, bucket_hi, 3, e->stream));
    if (last) CHK(adamw_finish(e));
    return SGV_OK;
}
int sgv_adamw_step(sgv_engine* e, float lr) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    const int nbk = (int)e->buckets.size();
    if (e->comm && nbk >= 3) {
        // every layer whose bucket has arrived, then the small bucket's tensors, while the last weight bucket (first
        // encoder layer, index nbk - 2) is still in flight; that layer last
        CHK(sgv_adamw_step_range(e, lr, 0, nbk - 2, 1, 0));
        CHK(sgv_adamw_step_range(e, lr, nbk - 1, nbk, 0, 0));
        return sgv_adamw_step_range(e, lr, nbk - 2, nbk - 1, 0, 1);
    }
    return sgv_adamw_step_range(e, lr, 0, nbk, 1, 1);
}
int sgv_bucket_count(const sgv_engine* e) { return e ? (int)e->buckets.size() : 0; }
int sgv_set_grad_payload(sgv_engine* e, int dtype) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    if (dtype != SGV_DTYPE_F32 && dtype != SGV_DTYPE_BF16) return fail(SGV_ERR_ARG, "gradient payload must be f32 or bf16");
    for (char c : e->bucket_packed) if (c) return fail(SGV_ERR_STATE, "a packed bucket is in flight: change the payload between steps");
    if (dtype == SGV_DTYPE_BF16) CHK(ensure_lp_mirror(e));
    e->payload_bf16 = dtype == SGV_DTYPE_BF16;
    e->bucket_packed.assign(e->buckets.size(), 0);
    return SGV_OK;
}
int sgv_grad_payload_buffer(sgv_engine* e, void** ptr, size_t* count) {
    if (!e || !ptr || !count) return fail(SGV_ERR_ARG, "null argument");
    if (!e->payload_bf16) return fail(SGV_ERR_STATE, "the gradient payload is the fp32 arena (sgv_grad_buffer)");
    *ptr = e->grads_lp; *count = e->n_grads;
    return SGV_OK;
}
int sgv_grad_payload_unpack(sgv_engine* e) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    for (int b = 0; b < (int)e->bucket_packed.size(); ++b)
        if (e->bucket_packed[b]) {
            if (b < (int)e->bucket_pending.size() && e->bucket_pending[b]) { HIPCHK(hipStreamWaitEvent(e->stream, e->bucket_done[b], 0)); e->bucket_pending[b] = 0; }
            ew_unpack_bf16((const char*)e->grads_lp + 2 * e->buckets[b].first, e->grads + e->buckets[b].first, (long)e->buckets[b].second, e->stream);
            e->bucket_packed[b] = 0;
        }
    return SGV_OK;
}
int sgv_last_grad_norm(sgv_engine* e, double* out) {
    if (!e || !out) return fail(SGV_ERR_ARG, "null argument");
    double h = 0.0;
    HIPCHK(hipMemcpyAsync(&h, e->scal + 15, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    *out = sqrt(h);
    return SGV_OK;
}
}  // extern "C"
