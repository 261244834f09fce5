// Whole-state snapshot and restore: parameters, spectral-norm u / v and both Adam moments as ONE flat fp32 buffer in reference
// layout, permuted on the device (what permute_entry of engine.hip does on one host thread, tensor by tensor) and moved with one
// copy.  The snapshot goes through a device staging buffer and a copy stream of the engine's own, so the caller's next step does
// not wait for the 3 x 400 M floats of a preset-1 model to cross PCIe.
#include <algorithm>

#include "engine_internal.h"

// ---- permute kernels ---------------------------------------------------------------------------------------------------------
// Every case of permute_entry is one of two shapes.
//  * tile: a tensor indexed (b, p, q) whose internal layout is contiguous in p and whose reference layout is contiguous in q:
//        internal = ioff + b * ib + p + q * iq          reference = b * rb + p * rp + q
//      Conv1d weight   (b, p, q) = (co, ci, tap): internal [tap][Cout][Cin], reference [Cout][Cin][tap] -- the tap interleave
//      ConvTranspose1d (co, ci, tap): internal [taps-1-tap][Cout][Cin] (iq < 0, ioff = the last tap), reference [Cin][Cout][tap]
//      Linear head     (o, c, t): internal columns (t, c), reference columns (c, t)
//      v of those three and the bias / u of a Linear expand layer: the same with one b.
//    A work item moves TB x 64 x TQ elements (TB * TQ <= 64) through an LDS tile of TB * TQ rows of 64 p-values: the internal side
//    is touched in rows of 64 consecutive floats (one 256-byte request per wave), the reference side in the order its layout is
//    contiguous in -- (b, p, q) for mode 0, where p and q together form the reference row (Cin * taps floats of a conv weight),
//    (p, b, q) for mode 1 (ConvTranspose1d: b and q do).  The row pitch of the tile is odd and close to 64 + 32 / TQ: ds_read_b32 /
//    ds_write_b32 bank on (address / 4) mod 32 within each half wave, the internal side walks p (consecutive banks), the reference
//    side walks q first, then p: rows q * pitch + p of a half wave then fall on different banks.
//  * copy: reference index (x, y, z) contiguous, internal = x * ix + y * iy + z * iz: the plain copies (bias, u, GroupNorm affine,
//    1-tap Conv1d weights) and the row permutation of a Linear expand weight, whose rows are contiguous on both sides.
// Pure data movement: 4-byte loads and stores, no arithmetic, no atomics; results are exact.
struct CkptTile {
    float* base;            // internal tensor (parameter arena or a moment arena)
    long ref_off;           // float offset of the slice in the flat buffer
    long ib, iq, ioff;
    long rb, rp;
    int Bn, P, Q;
    int TB, TQ, pitch, mode;
};
struct CkptCopy {
    float* base;
    long ref_off;
    long n;                 // X * Y * Z
    long ix, iy, iz;
    int Y, Z;
};
constexpr int CKPT_TP = 64;              // p-values per tile row
constexpr int CKPT_ROWS = 64;            // (b, q) rows per tile
constexpr int CKPT_MAX_PITCH = 64 + 33;
constexpr int CKPT_COPY_CHUNK = 4096;    // elements per work item of the copy kernel

// TO_REF: internal -> flat reference buffer (snapshot); else the inverse (restore)
template <bool TO_REF>
__global__ __launch_bounds__(256) void ckpt_tile_kernel(const CkptTile* descs, const WorkItem* items, float* flat) {
    __shared__ float tile[CKPT_ROWS * CKPT_MAX_PITCH];
    const WorkItem it = items[blockIdx.x];
    const CkptTile d = descs[it.desc];
    const int npt = (d.P + CKPT_TP - 1) / CKPT_TP, nqt = (d.Q + d.TQ - 1) / d.TQ;
    int c = it.chunk;
    const int qt = c % nqt; c /= nqt;
    const int pt = c % npt;
    const int bt = c / npt;
    const int b0 = bt * d.TB, p0 = pt * CKPT_TP, q0 = qt * d.TQ;
    const int nb = min(d.TB, d.Bn - b0), np = min(CKPT_TP, d.P - p0), nq = min(d.TQ, d.Q - q0);
    if (nb <= 0 || np <= 0 || nq <= 0) return;
    const int rows = nb * nq;
    float* ref = flat + d.ref_off;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int total = rows * np;
    if (TO_REF) {
        if (lane < np)
            for (int r = w; r < rows; r += 4) {
                const int b = r / nq, q = r - b * nq;
                tile[r * d.pitch + lane] = d.base[d.ioff + (long)(b0 + b) * d.ib + (p0 + lane) + (long)(q0 + q) * d.iq];
            }
        __syncthreads();
    }
    for (int f = threadIdx.x; f < total; f += 256) {
        const int q = f % nq, t = f / nq;
        int b, p;
        if (d.mode == 0) { p = t % np; b = t / np; } else { b = t % nb; p = t / nb; }
        float* g = ref + (long)(b0 + b) * d.rb + (long)(p0 + p) * d.rp + (q0 + q);
        float* l = tile + (b * nq + q) * d.pitch + p;
        if (TO_REF) *g = *l; else *l = *g;
    }
    if (!TO_REF) {
        __syncthreads();
        if (lane < np)
            for (int r = w; r < rows; r += 4) {
                const int b = r / nq, q = r - b * nq;
                d.base[d.ioff + (long)(b0 + b) * d.ib + (p0 + lane) + (long)(q0 + q) * d.iq] = tile[r * d.pitch + lane];
            }
    }
}
template <bool TO_REF>
__global__ __launch_bounds__(256) void ckpt_copy_kernel(const CkptCopy* descs, const WorkItem* items, float* flat) {
    const WorkItem it = items[blockIdx.x];
    const CkptCopy d = descs[it.desc];
    const long lo = (long)it.chunk * CKPT_COPY_CHUNK, hi = min(d.n, lo + CKPT_COPY_CHUNK);
    float* ref = flat + d.ref_off;
    for (long f = lo + threadIdx.x; f < hi; f += 256) {
        const long t = f / d.Z;
        const int z = (int)(f - t * d.Z);
        const long x = t / d.Y;
        const int y = (int)(t - x * d.Y);
        float* in = d.base + x * d.ix + (long)y * d.iy + (long)z * d.iz;
        if (TO_REF) ref[f] = *in; else *in = ref[f];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct CkptSlice { size_t off = 0, count = 0; };
struct CkptState {
    size_t total = 0;                               // floats of the flat buffer
    std::vector<CkptSlice> slices;                  // [entry * 3 + which], which: 0 value, 1 exp_avg, 2 exp_avg_sq (count 0: no such slice)
    float* staging = nullptr;                       // device copy of the flat buffer
    CkptTile* tiles_dev = nullptr; CkptCopy* copies_dev = nullptr;
    WorkItem* items_tile = nullptr; WorkItem* items_copy = nullptr;
    int n_items_tile = 0, n_items_copy = 0;
    hipStream_t stream = nullptr;                   // the copy stream
    hipEvent_t ready = nullptr;                     // staging buffer complete on the engine stream
    bool pending = false;                           // a snapshot's copy has been enqueued and not yet waited for
};

static CkptState* ckpt_layout(sgv_engine* e) {
    if (e->ckpt) return e->ckpt;
    CkptState* c = new CkptState();
    c->slices.resize(e->entries.size() * 3);
    size_t off = 0;
    for (size_t i = 0; i < e->entries.size(); ++i) {
        const StateEntry& s = e->entries[i];
        const int nw = entry_grad_offset(e, s) != NPOS ? 3 : 1;
        for (int w = 0; w < nw; ++w) { c->slices[i * 3 + w].off = off; c->slices[i * 3 + w].count = (size_t)s.count(); off += (size_t)s.count(); }
    }
    c->total = off;
    e->ckpt = c;
    return c;
}

// the geometry of one state entry: fills `t` and returns true for a tile permutation, else fills `cp`
static bool ckpt_geometry(const sgv_engine* e, const StateEntry& s, CkptTile& t, CkptCopy& cp) {
    memset(&t, 0, sizeof(t)); memset(&cp, 0, sizeof(cp));
    const long cnt = s.count();
    auto plain = [&]() { cp.n = cnt; cp.Y = 1; cp.Z = 1; cp.ix = 1; cp.iy = 0; cp.iz = 0; return false; };
    auto tile = [&](int Bn, int P, int Q, long ib, long iq, long ioff, long rb, long rp, int mode) {
        t.Bn = Bn; t.P = P; t.Q = Q; t.ib = ib; t.iq = iq; t.ioff = ioff; t.rb = rb; t.rp = rp; t.mode = mode;
        t.TQ = std::min(Q, 32); t.TB = std::max(1, std::min(Bn, CKPT_ROWS / t.TQ));
        t.pitch = 64 + std::max(1, (32 / t.TQ) | 1);
        return true;
    };
    if (s.gn >= 0) return plain();
    const Layer& l = e->layers[s.layer];
    const int T = e->T, C = l.lin_C;
    const long cc = (long)l.cout * l.cin;
    if (s.kind == 1) {
        if (l.op == OP_CONV) return l.k == 1 ? plain() : tile(l.cout, l.cin, l.k, l.cin, cc, 0, (long)l.cin * l.k, l.k, 0);
        if (l.op == OP_CONVT) return tile(l.cout, l.cin, l.k, l.cin, -cc, (long)(l.k - 1) * cc, l.k, (long)l.cout * l.k, 1);
        if (l.lin_kind == LIN_HEAD) return tile(l.cout, C, T, l.cin, C, 0, l.cin, T, 0);
        // LIN_EXPAND: reference rows (c, t), internal rows (t, c), cin floats each
        cp.n = cnt; cp.Y = T; cp.Z = l.cin; cp.ix = l.cin; cp.iy = (long)C * l.cin; cp.iz = 1;
        return false;
    }
    if (s.kind == 3) {
        if (l.op == OP_CONV) return l.k == 1 ? plain() : tile(1, l.cin, l.k, 0, l.cin, 0, 0, l.k, 0);
        if (l.op == OP_CONVT) return tile(1, l.cin, l.k, 0, -(long)l.cin, (long)(l.k - 1) * l.cin, 0, l.k, 0);
        if (l.lin_kind == LIN_HEAD) return tile(1, C, T, 0, C, 0, 0, T, 0);
        return plain();
    }
    if (l.op == OP_LINEAR && l.lin_kind == LIN_EXPAND) return tile(1, C, T, 0, C, 0, 0, T, 0);
    return plain();
}

// the copy stream, made on first use: never on the main stream's hardware queue (nor on the side / second-lane streams'), so that a
// copy runs beside the next step
static hipStream_t ckpt_copy_stream(sgv_engine* e) {
    CkptState* c = ckpt_layout(e);
    if (!c->stream) make_aux_stream(&c->stream, "snapshot copy", {e->stream, e->side, e->lane2});
    return c->stream;
}

static int ckpt_prepare(sgv_engine* e) {
    CkptState* c = ckpt_layout(e);
    if (c->staging) return 0;
    std::vector<CkptTile> tiles; std::vector<CkptCopy> copies;
    std::vector<WorkItem> it_tile, it_copy;
    for (size_t i = 0; i < e->entries.size(); ++i) {
        const StateEntry& s = e->entries[i];
        CkptTile t; CkptCopy cp;
        const bool is_tile = ckpt_geometry(e, s, t, cp);
        // every element of the slice is covered exactly once, and nothing outside it
        if (is_tile ? (long)t.Bn * t.P * t.Q != s.count() : cp.n != s.count() || (cp.n % ((long)cp.Y * cp.Z)) != 0)
            return fail(SGV_ERR_STATE, "snapshot geometry of '%s' does not match its size", s.name.c_str());
        const size_t po = entry_param_offset(e, s), go = entry_grad_offset(e, s);
        for (int w = 0; w < 3; ++w) {
            const CkptSlice& sl = c->slices[i * 3 + w];
            if (!sl.count) continue;
            float* base = w == 0 ? e->params + po : (w == 1 ? e->adam_m : e->adam_v) + go;
            if (is_tile) {
                t.base = base; t.ref_off = (long)sl.off;
                const int id = (int)tiles.size();
                tiles.push_back(t);
                const int n = ((t.Bn + t.TB - 1) / t.TB) * ((t.P + CKPT_TP - 1) / CKPT_TP) * ((t.Q + t.TQ - 1) / t.TQ);
                for (int k = 0; k < n; ++k) it_tile.push_back({id, k});
            } else {
                cp.base = base; cp.ref_off = (long)sl.off;
                const int id = (int)copies.size();
                copies.push_back(cp);
                const long n = (cp.n + CKPT_COPY_CHUNK - 1) / CKPT_COPY_CHUNK;
                for (long k = 0; k < n; ++k) it_copy.push_back({id, (int)k});
            }
        }
    }
    if (!upload_vec(tiles, &c->tiles_dev) || !upload_vec(copies, &c->copies_dev) || !upload_vec(it_tile, &c->items_tile) || !upload_vec(it_copy, &c->items_copy))
        return fail(SGV_ERR_HIP, "snapshot table upload failed");
    c->n_items_tile = (int)it_tile.size(); c->n_items_copy = (int)it_copy.size();
    HIPCHK(hipEventCreateWithFlags(&c->ready, hipEventDisableTiming));
    if (!ckpt_copy_stream(e)) return fail(SGV_ERR_HIP, "snapshot copy stream creation failed");
    HIPCHK(hipMalloc((void**)&c->staging, std::max<size_t>(c->total, 1) * sizeof(float)));
    return 0;
}

template <bool TO_REF>
static int ckpt_permute(sgv_engine* e) {
    CkptState* c = e->ckpt;
    if (c->n_items_tile > 0) hipLaunchKernelGGL(ckpt_tile_kernel<TO_REF>, dim3(c->n_items_tile), dim3(256), 0, e->stream, c->tiles_dev, c->items_tile, c->staging);
    if (c->n_items_copy > 0) hipLaunchKernelGGL(ckpt_copy_kernel<TO_REF>, dim3(c->n_items_copy), dim3(256), 0, e->stream, c->copies_dev, c->items_copy, c->staging);
    return hipGetLastError() == hipSuccess ? 0 : fail(SGV_ERR_HIP, "snapshot permute launch failed");
}

void ckpt_release(sgv_engine* e) {
    CkptState* c = e->ckpt;
    if (!c) return;
    if (c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
    if (c->ready) hipEventDestroy(c->ready);
    void* ptrs[] = {c->staging, c->tiles_dev, c->copies_dev, c->items_tile, c->items_copy};
    for (void* p : ptrs) if (p) hipFree(p);
    delete c;
    e->ckpt = nullptr;
}

extern "C" {

int sgv_snapshot_floats(sgv_engine* e, size_t* total_floats) {
    if (!e || !total_floats) return fail(SGV_ERR_ARG, "null argument");
    *total_floats = ckpt_layout(e)->total;
    return SGV_OK;
}

int sgv_snapshot_slice(sgv_engine* e, int index, int which, size_t* offset_floats, size_t* count_floats) {
    if (!e || !offset_floats || !count_floats) return fail(SGV_ERR_ARG, "null argument");
    if (index < 0 || index >= (int)e->entries.size() || which < 0 || which > 2) return fail(SGV_ERR_ARG, "bad (index, which) = (%d, %d)", index, which);
    const CkptSlice& sl = ckpt_layout(e)->slices[(size_t)index * 3 + which];
    *offset_floats = sl.off; *count_floats = sl.count;
    return SGV_OK;
}

int sgv_snapshot_begin(sgv_engine* e, float* host_pinned, size_t floats) {
    if (!e || !host_pinned) return fail(SGV_ERR_ARG, "null argument");
    CkptState* c = ckpt_layout(e);
    if (floats != c->total) return fail(SGV_ERR_ARG, "snapshot buffer holds %zu floats, the state has %zu", floats, c->total);
    if (c->pending) return fail(SGV_ERR_STATE, "sgv_snapshot_begin: the previous snapshot has not been waited for");
    if (e->adam_open) return fail(SGV_ERR_STATE, "sgv_snapshot_begin: an AdamW step is open");
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, host_pinned) != hipSuccess || at.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return fail(SGV_ERR_ARG, "sgv_snapshot_begin: the host buffer is not pinned (page-locked) memory");
    }
    CHK(ckpt_prepare(e));
    CHK(ckpt_permute<true>(e));
    HIPCHK(hipEventRecord(c->ready, e->stream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ready, 0));
    HIPCHK(hipMemcpyAsync(host_pinned, c->staging, c->total * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    c->pending = true;
    return SGV_OK;
}

int sgv_snapshot_wait(sgv_engine* e) {
    if (!e) return fail(SGV_ERR_ARG, "null engine");
    CkptState* c = e->ckpt;
    if (!c || !c->pending) return SGV_OK;
    c->pending = false;
    HIPCHK(hipStreamSynchronize(c->stream));
    return SGV_OK;
}

int sgv_copy_stream(sgv_engine* e, void** hip_stream) {
    if (!e || !hip_stream) return fail(SGV_ERR_ARG, "null argument");
    hipStream_t s = ckpt_copy_stream(e);
    if (!s) return fail(SGV_ERR_HIP, "copy stream creation failed");
    *hip_stream = (void*)s;
    return SGV_OK;
}

int sgv_restore(sgv_engine* e, const float* host, size_t floats) {
    if (!e || !host) return fail(SGV_ERR_ARG, "null argument");
    CkptState* c = ckpt_layout(e);
    if (floats != c->total) return fail(SGV_ERR_ARG, "restore buffer holds %zu floats, the state has %zu", floats, c->total);
    if (c->pending) return fail(SGV_ERR_STATE, "sgv_restore: a snapshot is in flight (sgv_snapshot_wait first)");
    if (e->adam_open) return fail(SGV_ERR_STATE, "sgv_restore: an AdamW step is open");
    CHK(ckpt_prepare(e));
    HIPCHK(hipMemcpyAsync(c->staging, host, c->total * sizeof(float), hipMemcpyHostToDevice, e->stream));
    CHK(ckpt_permute<false>(e));
    // as sgv_load_state: everything that caches a function of the weights is stale.  The gradient arena, its bf16 mirror and the
    // mirror's per-layer valid flags describe the last backward, not the weights, and stay; bucket_updated only has a meaning
    // while a step is open, which is refused above; the activations of a forward run with the old weights must not feed a backward
    e->copies_fresh = false;
    e->wtu_fresh = false;
    e->have_fwd = false;
    CHK(sgv_prepare(e));
    // an uninterrupted run enters its next training forward with the W^T u partials of the last tiled AdamW pass; the full
    // power-iteration pass sums the same 64-row blocks in another order, so those partials are rebuilt here in the tiled pass's order
    if (opt_sn_tpart_tiles(e->tab.adam_dev, e->tab.sn_dev, e->tab.dev[OptTables::TILE], e->tab.n(OptTables::TILE), e->stream)) return fail(SGV_ERR_HIP, "W^T u partial launch failed");
    e->wtu_fresh = true;
    HIPCHK(hipStreamSynchronize(e->stream));
    return SGV_OK;
}

}  // extern "C"
