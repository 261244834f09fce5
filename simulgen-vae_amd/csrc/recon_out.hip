// The recon tails (gfx950): passes that replace the loss tail of the recon head in surrogate use -- the physical-unit field
// (sgv_generate), its summaries (sgv_summarize), its error against held-out fields (sgv_score), the running statistics over the
// members of an ensemble (sgv_ensemble), the running sums of a Sobol sensitivity study (sgv_sobol), the histogram of the members
// between given bounds (sgv_distribution), the co-moments of the members with their covariates (sgv_regress), weighted sums over the
// mesh (sgv_project) or over time (sgv_temporal), the temporal Gram matrix (sgv_gram), the level-crossing statistics over time
// (sgv_exceedance) and the load cycles and rates of the time histories (sgv_cycles).  All of them stream y = the recon head's convolution output once, form the same value per
// element (recon_phys_val) and differ in what they do with it; DESIGN.md, "the recon tails", describes the shared pieces below.
#include <algorithm>
#include <type_traits>
#include "sgv_gn_dev.h"

// ------------------------------------------------------------------------------------------
// Surrogate prediction: recon head -> physical-unit field in one pass (sgv_generate).
//   out = (tanh(gamma * (y - mean) * rstd + beta) - min_n) / scale_n      (MinMaxScaler.inverse_transform per node)
// fp32 from the load of y to the fp32 store: no loss, no target read, no compute-dtype x_hat in between.  mean / rstd come from
// p.sums exactly as in the eval loss pass (gn_consts; the normalised value is formed as (y - mean) * rstd first, as there).
// ------------------------------------------------------------------------------------------
struct ReconPhys { const float* scale; const float* mn; float* out; };
// One element of the physical field and the reciprocal of its scale: the only place either is written down.  Every kernel of this
// file calls these, so a summary, a score or an ensemble state is a reduction of bit-identical values.
__device__ __forceinline__ float recon_phys_val(float y, float mean, float rstd, float gam, float bet, float mn, float inv) {
    const float xh = (y - mean) * rstd;
    return (tanh_f(xh * gam + bet) - mn) * inv;
}
__device__ __forceinline__ float recon_phys_inv(float scale) { return 1.0f / scale; }      // correctly rounded reciprocal, once per thread
// the constants of channel ch, (gamma, beta, min, 1 / scale); !ok (a thread past C in the kernels whose shuffles and barriers need every
// thread) loads nothing and gets 0.  By value, and the 8-wide loop that fills gam / bet / mn / inv stays in the kernels: handing their
// arrays to a helper cost registers ("the recon tails").
__device__ __forceinline__ float4 recon_channel(const GNParams& p, const ReconPhys& q, int ch, bool ok) {
    return ok ? make_float4(p.gamma[ch], p.beta[ch], q.mn[ch], recon_phys_inv(q.scale[ch])) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// [B][T][N]: the geometry of gn_apply_kernel, 16-byte loads of y and two 16-byte stores per thread and row
template <typename T>
__global__ __launch_bounds__(256) void recon_phys_tn_kernel(const GNParams p, const ReconPhys q) {
    const GNCtx c = gn_ctx(p);
    float mean[8], rstd[8];
    gn_consts(p, c, mean, rstd);
    if (!c.col_ok) return;
    float gam[8], bet[8], mn[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float4 k = recon_channel(p, q, c.c0 + e, c.col_ok); gam[e] = k.x; bet[e] = k.y; mn[e] = k.z; inv[e] = k.w; }
    const T* y = reinterpret_cast<const T*>(p.y);
    for (int t = c.t_lo + c.ty; t < c.t_hi; t += 2 * c.RL) {      // two rows per round, loads first
        const bool two = t + c.RL < c.t_hi;
        const long m0 = (long)c.b * p.T + t, m1 = two ? m0 + c.RL : m0;
        Raw8<T> r0, r1;
        raw_load(y + m0 * p.ldy + c.c0, r0);
        raw_load(y + m1 * p.ldy + c.c0, r1);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u == 1 && !two) break;
            float v[8];
            raw_unpack(u ? r1 : r0, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = recon_phys_val(v[e], mean[e], rstd[e], gam[e], bet[e], mn[e], inv[e]);
            store8(q.out + (u ? m1 : m0) * p.C + c.c0, v);
        }
    }
}

// [B][N][T] (the reference's tensor layout): a tile of 32 rows (t) x 64 channels goes through LDS transposed; every thread loads
// 8 channels of one row (16 / 32 bytes), the stores run along T.  blockIdx = (channel tile, row tile, sample).
constexpr int RP_TT = 32, RP_TN = 64;
template <typename T>
__global__ __launch_bounds__(256) void recon_phys_nt_kernel(const GNParams p, const ReconPhys q) {
    __shared__ float tile[RP_TN][RP_TT + 1];
    __shared__ float cst[6][RP_TN];          // per channel of the tile: mean, rstd, gamma, beta, min, 1 / scale
    const int b = blockIdx.z, n0 = blockIdx.x * RP_TN, t0 = blockIdx.y * RP_TT;
    const int tid = threadIdx.x;
    if (tid < RP_TN && n0 + tid < p.C) {
        const int ch = n0 + tid, g = min(ch / p.Cg, p.G - 1);
        gn_mean_rstd(p, b, g, cst[0][tid], cst[1][tid]);
        cst[2][tid] = p.gamma[ch]; cst[3][tid] = p.beta[ch]; cst[4][tid] = q.mn[ch]; cst[5][tid] = recon_phys_inv(q.scale[ch]);
    }
    __syncthreads();
    const int r = tid >> 3, cx = (tid & 7) * 8;          // row of the tile, first of this thread's 8 channels
    const int t = t0 + r;
    if (t < p.T && n0 + cx < p.C) {
        float v[8];
        load8(reinterpret_cast<const T*>(p.y) + ((long)b * p.T + t) * p.ldy + n0 + cx, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = cx + e;
            tile[j][r] = recon_phys_val(v[e], cst[0][j], cst[1][j], cst[2][j], cst[3][j], cst[4][j], cst[5][j]);
        }
    }
    __syncthreads();
    const int tx = tid & 31;
    if (t0 + tx < p.T) {
        for (int j = tid >> 5; j < RP_TN; j += 8) {
            if (n0 + j >= p.C) break;
            q.out[((long)b * p.C + n0 + j) * p.T + t0 + tx] = tile[j][tx];
        }
    }
}

// ------------------------------------------------------------------------------------------
// What the launchers share: the checks on p, the setup of the kernels' arguments, the choice of an instantiation.
// ------------------------------------------------------------------------------------------
constexpr int RS_MAX_CV = 64;
struct RSGeom { int CV, colblocks; };
static RSGeom rs_geom(int C) {
    const int nv = C / 8;
    int cv = 1;
    while (cv < nv && cv < RS_MAX_CV) cv <<= 1;
    return {cv, cdiv_i(nv, cv)};
}
size_t ew_recon_summary_work_floats(int B, int T, int C) { return (size_t)B * T * rs_geom(C).colblocks * 4; }

// the inputs every tail has: -1 a null pointer, -3 a bad shape, 0 fine
static int recon_args_ok(const GNParams& p, const float* scale, const float* mn) {
    if (!p.y || !p.sums || !p.gamma || !p.beta || !scale || !mn) return -1;
    if (p.B < 1 || p.T < 1 || p.C < 8 || p.C % 8 || p.ldy < p.C || p.ldy % 8 || p.G < 1 || p.G > SGV_GN_MAX_GROUPS || p.C % p.G) return -3;
    return 0;
}
// Cg and the column geometry of the summary / score / ensemble kernels (CV = 64 column lanes, fewer for C < 512; GN_LAUNCH sets its own)
static ReconPhys recon_setup(GNParams& p, const float* scale, const float* mn, float* out = nullptr) {
    p.Cg = p.C / p.G;
    p.CV = rs_geom(p.C).CV;
    return {scale, mn, out};
}
// f(Elem<T>, std::bool_constant<flag>...) for the element type of `dtype` and up to three run-time flags; the combination with every
// flag false is never called, so a kernel template is instantiated for exactly the combinations its launcher can ask for
template <typename T> struct Elem { using type = T; };
template <bool... Bs, typename F>
static void recon_dispatch(F& f, int dtype) {
    if constexpr ((Bs || ...)) {
        if (dtype == 1) f(Elem<bf16_t>{}, std::bool_constant<Bs>{}...);
        else f(Elem<float>{}, std::bool_constant<Bs>{}...);
    }
}
template <bool... Bs, typename F, typename... Rest>
static void recon_dispatch(F& f, int dtype, bool b, Rest... rest) {
    if (b) recon_dispatch<Bs..., true>(f, dtype, rest...);
    else recon_dispatch<Bs..., false>(f, dtype, rest...);
}

// p: y / ldy / gamma / beta / sums (given) / B, T, C, G, Cg; scale, mn [C] fp32; out fp32, dense: layout 0 [B][T][C], 1 [B][C][T]
int ew_recon_physical(int dtype, GNParams p, const float* scale, const float* mn, int layout, float* out, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    if (!out) return -1;
    if (layout != 0 && layout != 1) return -2;
    if (((uintptr_t)p.y | (uintptr_t)out) & 15) return -4;          // 16-byte vector accesses
    const ReconPhys q = recon_setup(p, scale, mn, out);
    if (layout == 0) {
        if (dtype == 1) GN_LAUNCH((recon_phys_tn_kernel<bf16_t>), p, s, q);
        else GN_LAUNCH((recon_phys_tn_kernel<float>), p, s, q);
    } else {
        const dim3 grid(cdiv_i(p.C, RP_TN), cdiv_i(p.T, RP_TT), p.B);
        if (dtype == 1) hipLaunchKernelGGL((recon_phys_nt_kernel<bf16_t>), grid, dim3(256), 0, s, p, q);
        else hipLaunchKernelGGL((recon_phys_nt_kernel<float>), grid, dim3(256), 0, s, p, q);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// The pieces the summary and the score pass are built from.  No atomics: a block owns 8 * CV channels of one sample for ALL rows (no
// row split), so a node's time axis lies in one block -- its RL row lanes are combined through LDS in lane order; a row's reduction
// over the block's channels happens inside the wave, over the CV lanes of that row, and goes to a partials workspace
// [B*T][column blocks] of float4, which recon_frames_kernel combines.  (value, index) pairs are ordered by value, then by the
// smaller index, so the result does not depend on the shape of any tree: ties go to the smallest t / n and two launches are bitwise
// equal.  Geometry: CV = 64 column lanes (one wave per row; fewer for C < 512), RL = 256 / CV row lanes, grid (ceil(C / (8 CV)), 1, B).
// ------------------------------------------------------------------------------------------
// b replaces a when it is the larger (MAX) / smaller value, or the same value at a smaller index
template <bool MAX>
__device__ __forceinline__ void ext_take(float& av, int& ai, float bv, int bi) {
    const bool better = MAX ? bv > av : bv < av;
    if (better || (bv == av && bi < ai)) { av = bv; ai = bi; }
}
constexpr int RS_NO_INDEX = 0x7fffffff;       // index of the neutral element: loses every tie
// In-wave reduction over the CV lanes of a row (neighbours inside a wave, aligned to CV) with DPP operands -- VALU instructions,
// no trip through the LDS crossbar: pairs within quads, quads within 8 and 8s within 16 lanes by mirrored exchanges (every lane
// of a DPP row of 16 then holds that row's result), then lane 15 of each DPP row into the next row and lane 31 into the upper
// half.  Lanes of DPP rows outside the row mask get their own value back.  The LAST lane of the CV ends up with the result.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int dpp_i(int v);
template <int CTRL, int ROW_MASK> __device__ __forceinline__ float dpp_f(float v) { return __int_as_float(dpp_i<CTRL, ROW_MASK>(__float_as_int(v))); }
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int dpp_i(int v) {
    // every lane has a source in the unmasked exchanges: with bound_ctrl set the compiler may fold the move into the instruction that uses it
    if constexpr (ROW_MASK == 0xF) return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
    else return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xF, false);
}
#define RS_LANE_REDUCE(NAME, TYPE, OP, DPP)                                                      \
    __device__ __forceinline__ TYPE NAME(TYPE v, int cv) {                                       \
        if (cv > 1) v = OP(v, DPP<0xB1, 0xF>(v));  /* quad_perm [1, 0, 3, 2] */                  \
        if (cv > 2) v = OP(v, DPP<0x4E, 0xF>(v));  /* quad_perm [2, 3, 0, 1] */                  \
        if (cv > 4) v = OP(v, DPP<0x141, 0xF>(v)); /* row_half_mirror */                         \
        if (cv > 8) v = OP(v, DPP<0x140, 0xF>(v)); /* row_mirror */                              \
        if (cv > 16) v = OP(v, DPP<0x142, 0xA>(v)); /* row_bcast:15 into rows 1 and 3 */         \
        if (cv > 32) v = OP(v, DPP<0x143, 0xC>(v)); /* row_bcast:31 into rows 2 and 3 */         \
        return v;                                                                                \
    }
RS_LANE_REDUCE(lane_max_f, float, fmaxf, dpp_f)
RS_LANE_REDUCE(lane_min_f, float, fminf, dpp_f)
RS_LANE_REDUCE(lane_min_i, int, min, dpp_i)
// the sum over a row's lanes in the same fixed tree (the score pass); lanes of DPP rows outside a row mask end up with twice their
// value, which nobody reads: as above, only the LAST lane of the CV holds the result
__device__ __forceinline__ float rs_add_f(float a, float b) { return a + b; }
RS_LANE_REDUCE(lane_sum_f, float, rs_add_f, dpp_f)
#undef RS_LANE_REDUCE

// The frame reduction: the maximum (MAX) or minimum of v over the CV lanes of this thread's row and the smallest index among the lanes
// that hold it -- i is the smallest index at which this lane saw v.  The passes are VALU-bound, not HBM-bound:
// reducing (value, index) pairs through the DPP tree, 4 moves + 12 compare / select per step, cost more than the element arithmetic;
// so the values are reduced alone, the winner is handed back from the last lane to the row's lanes, and the index is reduced as an
// integer minimum.  The pair is complete in the LAST lane of the CV.
struct ValIdx { float v; int i; };
template <bool MAX>
__device__ __forceinline__ ValIdx row_extremum(float v, int i, int cv) {
    const int last = ((int)threadIdx.x & 63) | (cv - 1);
    const float r = __shfl(MAX ? lane_max_f(v, cv) : lane_min_f(v, cv), last, 64);
    return {r, lane_min_i(v == r ? i : RS_NO_INDEX, cv)};
}

// The row-lane combines: the RL row lanes of a block hold partial results for the same 8 channels; they meet through LDS (2048
// entries per array: 256 threads x 8) and row lane 0 (`owner`) takes the others in lane order, so it ends up with the result.
// All 256 threads call; a barrier separates the owner's reads from whatever is written to the arrays next.
__device__ __forceinline__ int rowlane_slot(const GNParams& p, int ty, int tx) { return (ty * p.CV + tx) * 8; }
template <bool MAX>
__device__ __forceinline__ void rowlane_extremum(const GNParams& p, const GNCtx& c, bool owner, float* smv, int* smi, float v[8], int i[8]) {
    const int slot = rowlane_slot(p, c.ty, c.tx);
#pragma unroll
    for (int e = 0; e < 8; ++e) { smv[slot + e] = v[e]; smi[slot + e] = i[e]; }
    __syncthreads();
    if (owner) {
        for (int r = 1; r < c.RL; ++r)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = rowlane_slot(p, r, c.tx) + e;
                ext_take<MAX>(v[e], i[e], smv[j], smi[j]);
            }
    }
    __syncthreads();
}
// plain sums of one array, or of two side by side (smb / b given); the last use of the arrays: no barrier behind the owner's reads
__device__ __forceinline__ void rowlane_sum(const GNParams& p, const GNCtx& c, bool owner, float* sma, float a[8], float* smb = nullptr,
                                            float* b = nullptr) {
    const int slot = rowlane_slot(p, c.ty, c.tx);
#pragma unroll
    for (int e = 0; e < 8; ++e) { sma[slot + e] = a[e]; if (smb) smb[slot + e] = b[e]; }
    __syncthreads();
    if (owner) {
        for (int r = 1; r < c.RL; ++r)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = rowlane_slot(p, r, c.tx) + e;
                a[e] += sma[j];
                if (smb) b[e] += smb[j];
            }
    }
}

// ------------------------------------------------------------------------------------------
// Surrogate field summaries (sgv_summarize): the same pass as recon_phys_tn_kernel with the stores replaced by reductions of the
// values it would have stored -- per (sample, node) max / min / mean over t and the t of both extrema, per (sample, t) max / min
// over the nodes and the node of both, and the time histories at a list of probe nodes.  Every comparison is made on the descaled
// value (scale_n may be negative).  Frame partial: (max, node, min, node).
// ------------------------------------------------------------------------------------------
// 4 waves / SIMD asked for: with every output the bf16 kernel sits at 128 VGPRs without scratch (131 and 3 waves unasked; the fp32 one
// then keeps a few dwords in scratch)
template <typename T, bool NODE, bool FRAME>
__global__ __launch_bounds__(256, 4) void recon_summary_kernel(const GNParams p, const ReconPhys q, const ReconSummary o) {
    const GNCtx c = gn_ctx(p);          // gridDim.y == 1: t_lo = 0, t_hi = T
    float mean[8], rstd[8];
    gn_consts(p, c, mean, rstd);
    // no early return for the lanes past C: the shuffles and barriers below need every thread; such lanes load nothing and
    // carry the neutral element
    float gam[8], bet[8], mn[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float4 k = recon_channel(p, q, c.c0 + e, c.col_ok); gam[e] = k.x; bet[e] = k.y; mn[e] = k.z; inv[e] = k.w; }
    float vmax[8], vmin[8], vsum[8];
    int tmax[8], tmin[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { vmax[e] = -INFINITY; vmin[e] = INFINITY; vsum[e] = 0.f; tmax[e] = RS_NO_INDEX; tmin[e] = RS_NO_INDEX; }
    const T* y = reinterpret_cast<const T*>(p.y);
    float4* const fpart = reinterpret_cast<float4*>(o.work);
    for (int t0 = 0; t0 < p.T; t0 += 2 * c.RL) {          // block-uniform trip count; two rows per round, loads first
        const int ta = t0 + c.ty, tb = ta + c.RL;
        const bool oka = c.col_ok && ta < p.T, okb = c.col_ok && tb < p.T;
        const long m0 = (long)c.b * p.T + ta, m1 = m0 + c.RL;
        Raw8<T> r0, r1;
        raw_zero(r0); raw_zero(r1);
        if (oka) raw_load(y + m0 * p.ldy + c.c0, r0);
        if (okb) raw_load(y + m1 * p.ldy + c.c0, r1);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool ok = u ? okb : oka;
            const int t = u ? tb : ta;
            float fmx = -INFINITY, fmn = INFINITY;
            int imx = RS_NO_INDEX, imn = RS_NO_INDEX;
            if (ok) {
                float v[8];
                raw_unpack(u ? r1 : r0, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float x = recon_phys_val(v[e], mean[e], rstd[e], gam[e], bet[e], mn[e], inv[e]);
                    if constexpr (NODE) {          // this thread's rows come in ascending t: a strict comparison keeps the first
                        if (x > vmax[e]) { vmax[e] = x; tmax[e] = t; }
                        if (x < vmin[e]) { vmin[e] = x; tmin[e] = t; }
                        vsum[e] += x;
                    }
                    if constexpr (FRAME) {         // ascending n
                        if (x > fmx) { fmx = x; imx = c.c0 + e; }
                        if (x < fmn) { fmn = x; imn = c.c0 + e; }
                    }
                }
            }
            if constexpr (FRAME) {
                const ValIdx rmx = row_extremum<true>(fmx, imx, p.CV), rmn = row_extremum<false>(fmn, imn, p.CV);
                if (c.tx == p.CV - 1 && t < p.T)
                    fpart[((long)c.b * p.T + t) * gridDim.x + blockIdx.x] = make_float4(rmx.v, __int_as_float(rmx.i), rmn.v, __int_as_float(rmn.i));
            }
        }
    }
    if constexpr (NODE) {
        __shared__ float smv[2048];
        __shared__ int smi[2048];
        const bool owner = c.ty == 0 && c.col_ok;
        rowlane_extremum<true>(p, c, owner, smv, smi, vmax, tmax);
        rowlane_extremum<false>(p, c, owner, smv, smi, vmin, tmin);
        rowlane_sum(p, c, owner, smv, vsum);
        if (owner) {
            const float ft = (float)p.T;
#pragma unroll
            for (int e = 0; e < 8; ++e) vsum[e] = vsum[e] / ft;          // the one division of the mean
            if (o.node_stats) {
                float* d = o.node_stats + (long)c.b * 3 * p.C + c.c0;
                store8(d, vmax); store8(d + p.C, vmin); store8(d + 2L * p.C, vsum);
            }
            if (o.node_when) {
                int* d = o.node_when + (long)c.b * 2 * p.C + c.c0;
                store8(d, tmax); store8(d + p.C, tmin);
            }
        }
    }
}

// Frame partials [rows = B*T][nblk] -> the frame outputs; one wave per row, every lane takes its partials in ascending block order
// and the lanes meet in a fixed xor tree.  Summary (!SCORE): (max, node, min, node) -> stats [rows][2], where [rows][2].  Score:
// (max |e|, node, sum e^2, sum truth^2) -> stats [rows][3] (max |e|, mean e^2, mean truth^2), where [rows]; the sums in fp64 (a + b
// is commutative: every lane of the tree holds the same bits), one division by C, rounded to fp32 once.
template <bool MAX>
__device__ __forceinline__ void wave_extremum(float& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        ext_take<MAX>(v, i, ov, oi);
    }
}
template <bool SCORE>
__global__ __launch_bounds__(256) void recon_frames_kernel(const float4* part, int rows, int nblk, int C, float* stats, int* where) {
    const int row = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    float fmx = -INFINITY, fmn = INFINITY;
    int imx = RS_NO_INDEX, imn = RS_NO_INDEX;
    double se = 0.0, st = 0.0;
    if (row < rows) {          // wave-uniform
        for (int j = lane; j < nblk; j += 64) {
            const float4 v = part[(long)row * nblk + j];
            ext_take<true>(fmx, imx, v.x, __float_as_int(v.y));
            if constexpr (SCORE) { se += (double)v.z; st += (double)v.w; }
            else ext_take<false>(fmn, imn, v.z, __float_as_int(v.w));
        }
    }
    wave_extremum<true>(fmx, imx);
    if constexpr (SCORE) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { se += __shfl_xor(se, off, 64); st += __shfl_xor(st, off, 64); }
    } else wave_extremum<false>(fmn, imn);
    if (row < rows && lane == 0) {
        if constexpr (SCORE) {
            if (stats) { stats[3L * row] = fmx; stats[3L * row + 1] = (float)(se / (double)C); stats[3L * row + 2] = (float)(st / (double)C); }
            if (where) where[row] = imx;
        } else {
            if (stats) { stats[2L * row] = fmx; stats[2L * row + 1] = fmn; }
            if (where) { where[2L * row] = imx; where[2L * row + 1] = imn; }
        }
    }
}
template <bool SCORE>
static void recon_frames(const GNParams& p, const float* work, float* stats, int* where, hipStream_t s) {
    hipLaunchKernelGGL(recon_frames_kernel<SCORE>, dim3(cdiv_i((long)p.B * p.T, 4)), dim3(256), 0, s, reinterpret_cast<const float4*>(work),
                       p.B * p.T, rs_geom(p.C).colblocks, p.C, stats, where);
}

// probes[b][t][k] = the field at node nodes[k] (checked on the host: 0 <= node < C): 64 probes x 4 rows per block, the
// per-probe constants once per thread.  mean / rstd go through gn_mean_rstd as in gn_consts, so the values are those of the
// full pass bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void recon_probe_kernel(const GNParams p, const ReconPhys q, const int* nodes, int K, float* out) {
    const int k = blockIdx.x * 64 + ((int)threadIdx.x & 63), ty = (int)threadIdx.x >> 6, b = blockIdx.z;
    if (k >= K) return;
    const int n = nodes[k];
    float mean, rstd;
    gn_mean_rstd(p, b, min(n / p.Cg, p.G - 1), mean, rstd);
    const float4 ch = recon_channel(p, q, n, true);
    const T* y = reinterpret_cast<const T*>(p.y);
    for (int t = blockIdx.y * 4 + ty; t < p.T; t += gridDim.y * 4) {
        const long m = (long)b * p.T + t;
        out[m * K + k] = recon_phys_val(to_f32(y[m * p.ldy + n]), mean, rstd, ch.x, ch.y, ch.z, ch.w);
    }
}

// p as for ew_recon_physical; o: any subset of the five outputs (ReconSummary, sgv_ew.h), o.work = ew_recon_summary_work_floats
// floats when a frame output is asked for.  Non-zero (nothing launched): -1 null input, -2 no output, -3 bad shape, -4 a pointer
// not 16-byte aligned (probes, frame outputs: 4 / 8 bytes), -5 probes without a node list, -6 frame output without workspace
int ew_recon_summary(int dtype, GNParams p, const float* scale, const float* mn, const ReconSummary& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    const bool node = o.node_stats || o.node_when, frame = o.frame_stats || o.frame_where;
    if (!node && !frame && !o.probes) return -2;
    if (((uintptr_t)p.y | (uintptr_t)o.node_stats | (uintptr_t)o.node_when | (uintptr_t)o.work) & 15) return -4;
    if (((uintptr_t)o.frame_stats | (uintptr_t)o.frame_where) & 7) return -4;
    if ((uintptr_t)o.probes & 3) return -4;
    if (o.probes && (!o.probe_nodes || o.n_probes < 1)) return -5;
    if (frame && !o.work) return -6;
    const ReconPhys q = recon_setup(p, scale, mn);
    if (node || frame) {
        const dim3 grid(rs_geom(p.C).colblocks, 1, p.B);
        auto launch = [&](auto el, auto node_c, auto frame_c) {
            hipLaunchKernelGGL((recon_summary_kernel<typename decltype(el)::type, decltype(node_c)::value, decltype(frame_c)::value>), grid, dim3(256), 0, s,
                               p, q, o);
        };
        recon_dispatch(launch, dtype, node, frame);
        if (frame) recon_frames<false>(p, o.work, o.frame_stats, o.frame_where, s);
    }
    if (o.probes) {
        const dim3 grid(cdiv_i(o.n_probes, 64), std::min(cdiv_i(p.T, 4), 64), p.B);
        if (dtype == 1) hipLaunchKernelGGL((recon_probe_kernel<bf16_t>), grid, dim3(256), 0, s, p, q, o.probe_nodes, o.n_probes, o.probes);
        else hipLaunchKernelGGL((recon_probe_kernel<float>), grid, dim3(256), 0, s, p, q, o.probe_nodes, o.n_probes, o.probes);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// Surrogate scoring (sgv_score): the summary pass with one more input stream.  e[b, t, n] = val[b, t, n] - truth[b, t, n], val the
// value recon_phys_tn_kernel would store, truth fp32 dense [B][T][C] in physical units; reduced to, per (sample, node), max_t |e|,
// the t of it, mean_t e and mean_t e^2, and per (sample, t), max_n |e|, its node, mean_n e^2 and mean_n truth^2 (what a relative
// L2 error needs, so the truth is read once).  The two frame sums go through the same fixed DPP tree as the maximum.
// Frame partial: (max |e|, node, sum e^2, sum truth^2).
// ------------------------------------------------------------------------------------------
// the error of one element: exactly one fp32 subtraction of the stored value (never contracted with the multiplication by
// 1 / scale inside recon_phys_val: F - truth formed from the stored field F has the same bits)
__device__ __forceinline__ float recon_score_err(float val, float truth) {
#pragma clang fp contract(off)
    return val - truth;
}

// No occupancy asked for, unlike recon_summary_kernel: 8 x (max, t, sum e, sum e^2) per thread plus the truth of two rows in flight take
// 138 VGPRs (bf16; fp32 143) with all outputs, 3 waves / SIMD, no scratch; held to 128 the kernel spilled 44 bytes per lane and was
// slower (0.537 against 0.464 ms).  Node or frame outputs alone stay under 128 and run at 4 waves.
template <typename T, bool NODE, bool FRAME>
__global__ __launch_bounds__(256) void recon_score_kernel(const GNParams p, const ReconPhys q, const float* __restrict__ truth, const ReconScore o) {
    const GNCtx c = gn_ctx(p);          // gridDim.y == 1: t_lo = 0, t_hi = T
    float mean[8], rstd[8];
    gn_consts(p, c, mean, rstd);
    // no early return for the lanes past C (see recon_summary_kernel): they load neither y nor truth and carry the neutral element
    float gam[8], bet[8], mn[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float4 k = recon_channel(p, q, c.c0 + e, c.col_ok); gam[e] = k.x; bet[e] = k.y; mn[e] = k.z; inv[e] = k.w; }
    float vmax[8], vsum[8], vsq[8];
    int tmax[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { vmax[e] = -INFINITY; tmax[e] = RS_NO_INDEX; vsum[e] = 0.f; vsq[e] = 0.f; }
    const T* y = reinterpret_cast<const T*>(p.y);
    float4* const fpart = reinterpret_cast<float4*>(o.work);
    for (int t0 = 0; t0 < p.T; t0 += 2 * c.RL) {          // block-uniform trip count; two rows per round, loads first
        const int ta = t0 + c.ty, tb = ta + c.RL;
        const bool oka = c.col_ok && ta < p.T, okb = c.col_ok && tb < p.T;
        const long m0 = (long)c.b * p.T + ta, m1 = m0 + c.RL;
        Raw8<T> r0, r1;
        Raw8<float> w0, w1;
        raw_zero(r0); raw_zero(r1); raw_zero(w0); raw_zero(w1);
        if (oka) { raw_load(y + m0 * p.ldy + c.c0, r0); raw_load(truth + m0 * p.C + c.c0, w0); }
        if (okb) { raw_load(y + m1 * p.ldy + c.c0, r1); raw_load(truth + m1 * p.C + c.c0, w1); }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool ok = u ? okb : oka;
            const int t = u ? tb : ta;
            float fmx = -INFINITY, fse = 0.f, fst = 0.f;
            int imx = RS_NO_INDEX;
            if (ok) {
                float v[8], w[8];
                raw_unpack(u ? r1 : r0, v);
                raw_unpack(u ? w1 : w0, w);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // squares rounded once and then added (no fused multiply-add, which the compiler would form in some instantiations
                    // and not in others): every subset of the outputs gives the same bits
#pragma clang fp contract(off)
                    const float d = recon_score_err(recon_phys_val(v[e], mean[e], rstd[e], gam[e], bet[e], mn[e], inv[e]), w[e]);
                    const float a = fabsf(d);
                    if constexpr (NODE) {          // this thread's rows come in ascending t: a strict comparison keeps the first
                        if (a > vmax[e]) { vmax[e] = a; tmax[e] = t; }
                        vsum[e] += d;
                        vsq[e] += d * d;
                    }
                    if constexpr (FRAME) {         // ascending n
                        if (a > fmx) { fmx = a; imx = c.c0 + e; }
                        fse += d * d;
                        fst += w[e] * w[e];
                    }
                }
            }
            if constexpr (FRAME) {
                const ValIdx rmx = row_extremum<true>(fmx, imx, p.CV);
                const float rse = lane_sum_f(fse, p.CV), rst = lane_sum_f(fst, p.CV);
                if (c.tx == p.CV - 1 && t < p.T)
                    fpart[((long)c.b * p.T + t) * gridDim.x + blockIdx.x] = make_float4(rmx.v, __int_as_float(rmx.i), rse, rst);
            }
        }
    }
    if constexpr (NODE) {
        __shared__ float smv[2048];
        __shared__ int smi[2048];
        const bool owner = c.ty == 0 && c.col_ok;
        rowlane_extremum<true>(p, c, owner, smv, smi, vmax, tmax);
        rowlane_sum(p, c, owner, smv, vsum, reinterpret_cast<float*>(smi), vsq);          // the two sums side by side
        if (owner) {
            const float ft = (float)p.T;
#pragma unroll
            for (int e = 0; e < 8; ++e) { vsum[e] = vsum[e] / ft; vsq[e] = vsq[e] / ft; }          // the one division of each mean
            if (o.node_err) {
                float* d = o.node_err + (long)c.b * 3 * p.C + c.c0;
                store8(d, vmax); store8(d + p.C, vsum); store8(d + 2L * p.C, vsq);
            }
            if (o.node_when) store8(o.node_when + (long)c.b * p.C + c.c0, tmax);
        }
    }
}

// p as for ew_recon_physical; truth fp32 dense [B][T][C]; o: any subset of the four outputs (ReconScore, sgv_ew.h), o.work =
// ew_recon_summary_work_floats floats when a frame output is asked for.  Non-zero (nothing launched): -1 null input, -2 no output,
// -3 bad shape, -4 y / truth / a node output / work not 16-byte aligned or a frame output not 4-byte aligned, -5 frame output
// without workspace
int ew_recon_score(int dtype, GNParams p, const float* scale, const float* mn, const float* truth, const ReconScore& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    if (!truth) return -1;
    const bool node = o.node_err || o.node_when, frame = o.frame_err || o.frame_where;
    if (!node && !frame) return -2;
    if (((uintptr_t)p.y | (uintptr_t)truth | (uintptr_t)o.node_err | (uintptr_t)o.node_when | (uintptr_t)o.work) & 15) return -4;
    if (((uintptr_t)o.frame_err | (uintptr_t)o.frame_where) & 3) return -4;
    if (frame && !o.work) return -5;
    const ReconPhys q = recon_setup(p, scale, mn);
    const dim3 grid(rs_geom(p.C).colblocks, 1, p.B);
    auto launch = [&](auto el, auto node_c, auto frame_c) {
        hipLaunchKernelGGL((recon_score_kernel<typename decltype(el)::type, decltype(node_c)::value, decltype(frame_c)::value>), grid, dim3(256), 0, s,
                           p, q, truth, o);
    };
    recon_dispatch(launch, dtype, node, frame);
    if (frame) recon_frames<true>(p, o.work, o.frame_err, o.frame_where, s);
    return 0;
}

// ------------------------------------------------------------------------------------------
// Surrogate ensemble statistics (sgv_ensemble): the reduction along the batch axis.  For every (t, n) the values the members of
// a launch would store are merged, one member after the other in ascending order, into a running state [T][C] that outlives the
// launch: Welford mean / M2, maximum / minimum with the index of the member that produced each, and the count of members above a
// per-node limit.  Member b of a launch has index m = count_before + b; every update is sequential in m and the state is stored
// in the types it is held in, so any cut of the same members into launches gives the same bits.
// Geometry: the columns of rs_geom (CV = 64 column lanes x 4 row lanes for C >= 512, 8 channels per thread), grid (column blocks,
// row chunks over T).  A thread owns its (t, octet) for all members: no reduction across threads, no LDS traffic besides the
// block's table of (mean, rstd) per (member, group) -- members have different GroupNorm statistics -- which is filled once per
// block through gn_mean_rstd, and 1 / k per member.  With count_before == 0 the state is not read.
// ------------------------------------------------------------------------------------------
constexpr int EN_MAX_B = 32;          // members per launch (the table); ew_recon_ensemble cuts a larger batch into several launches
constexpr int EN_FLIGHT = 4;          // members whose y loads are issued before the first is used

// The member table and the octet's group lookup of the kernels that take several members per launch, as functions: what
// recon_ensemble_kernel does in line (moved into these helpers its register allocation changed: 12 -> 36 bytes of scratch per lane in
// the bf16 kernel with all groups, so it keeps its own copy) and recon_sobol_kernel calls.  The block's table of (mean, rstd) per
// (member, group), filled through gn_mean_rstd by all 256 threads (the caller's barrier follows) ...
__device__ __forceinline__ void member_table_fill(const GNParams& p, float2 (*tab)[SGV_GN_MAX_GROUPS]) {
    for (int i = threadIdx.x; i < p.B * p.G; i += 256) {
        float m, r;
        gn_mean_rstd(p, i / p.G, i % p.G, m, r);
        tab[i / p.G][i % p.G] = make_float2(m, r);
    }
}
// ... and the octet's group lookup: the group of each of a thread's 8 channels, one byte each; with Cg >= 8 (block-uniform) the octet
// lies in at most two groups, lo and hi, and two table reads per member do
struct OctetGroups { unsigned long long idx; int lo, hi; bool two; };
__device__ __forceinline__ OctetGroups octet_groups(const GNParams& p, int c0) {
    OctetGroups og;
    og.idx = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) og.idx |= (unsigned long long)min((c0 + e) / p.Cg, p.G - 1) << (8 * e);
    og.lo = (int)(og.idx & 0xff); og.hi = (int)(og.idx >> 56);
    og.two = p.Cg >= 8;
    return og;
}
__device__ __forceinline__ void octet_mean_rstd(const float2 (*tab)[SGV_GN_MAX_GROUPS], int b, const OctetGroups& og, float gm[8], float gr[8]) {
    if (og.two) {
        const float2 lo = tab[b][og.lo], hi = tab[b][og.hi];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool up = (int)((og.idx >> (8 * e)) & 0xff) != og.lo;
            gm[e] = up ? hi.x : lo.x; gr[e] = up ? hi.y : lo.y;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float2 w = tab[b][(int)((og.idx >> (8 * e)) & 0xff)];
            gm[e] = w.x; gr[e] = w.y;
        }
    }
}

// 3 waves / SIMD asked for: unasked, the kernel with all groups takes 176 VGPRs (bf16; fp32 192) and runs at 2 waves;
// held to 168 it keeps 12 bytes per lane in scratch (fp32 68) and is faster, 0.339 against 0.365 ms in one job -- the pass is bound by memory
// and the third wave hides more latency than the three spilled dwords cost.  Every other instantiation is below 168 anyway.
template <typename T, bool MOMENTS, bool EXTREMA, bool EXCEED>
__global__ __launch_bounds__(256, 3) void recon_ensemble_kernel(const GNParams p, const ReconPhys q, const ReconEnsemble o, const int count_before) {
    __shared__ float2 tab[EN_MAX_B][SGV_GN_MAX_GROUPS];          // (mean, rstd) of group g of member b
    __shared__ float rk[EN_MAX_B];                               // 1 / k, k = count_before + b + 1: one correctly rounded division per member
    for (int i = threadIdx.x; i < p.B * p.G; i += 256) {
        float m, r;
        gn_mean_rstd(p, i / p.G, i % p.G, m, r);
        tab[i / p.G][i % p.G] = make_float2(m, r);
    }
    if ((int)threadIdx.x < p.B) rk[threadIdx.x] = 1.0f / (float)(count_before + (int)threadIdx.x + 1);
    __syncthreads();
    const GNCtx c = gn_ctx(p);          // blockIdx.z == 0; c.b is not a member here
    if (!c.col_ok) return;              // no barrier below: lanes past C touch nothing
    float lim[8];
    float gam[8], bet[8], mn[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float4 k = recon_channel(p, q, c.c0 + e, c.col_ok); gam[e] = k.x; bet[e] = k.y; mn[e] = k.z; inv[e] = k.w; }
    unsigned long long gidx = 0;        // the group of each of the 8 channels, one byte each
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        lim[e] = EXCEED ? o.limit[c.c0 + e] : 0.f;
        gidx |= (unsigned long long)min((c.c0 + e) / p.Cg, p.G - 1) << (8 * e);
    }
    const int g_lo = (int)(gidx & 0xff), g_hi = (int)(gidx >> 56);
    const bool two = p.Cg >= 8;          // block-uniform: the octet lies in at most two groups, g_lo and g_hi
    const T* y = reinterpret_cast<const T*>(p.y);
    const bool fresh = count_before == 0;
    for (int t = c.t_lo + c.ty; t < c.t_hi; t += c.RL) {
        const long at = (long)t * p.C + c.c0;
        float mean[8], m2[8], vmax[8], vmin[8];
        int imax[8], imin[8], exc[8];
        if (fresh) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { mean[e] = 0.f; m2[e] = 0.f; vmax[e] = -INFINITY; vmin[e] = INFINITY; imax[e] = 0; imin[e] = 0; exc[e] = 0; }
        } else {
            if constexpr (MOMENTS) { load8(o.mean + at, mean); load8(o.m2 + at, m2); }
            if constexpr (EXTREMA) { load8(o.vmax + at, vmax); load8(o.vmin + at, vmin); load8(o.imax + at, imax); load8(o.imin + at, imin); }
            if constexpr (EXCEED) load8(o.exceed + at, exc);
        }
        for (int b0 = 0; b0 < p.B; b0 += EN_FLIGHT) {          // EN_FLIGHT members per round, loads first
            Raw8<T> r[EN_FLIGHT];
#pragma unroll
            for (int u = 0; u < EN_FLIGHT; ++u)                  // past the last member: its row again, loaded and not used
                raw_load(y + ((long)min(b0 + u, p.B - 1) * p.T + t) * p.ldy + c.c0, r[u]);
#pragma unroll
            for (int u = 0; u < EN_FLIGHT; ++u) {
                const int b = b0 + u;
                if (b >= p.B) break;
                const int m = count_before + b;
                const float rkb = rk[b];
                float v[8], gm[8], gr[8];
                raw_unpack(r[u], v);
                if (two) {
                    const float2 lo = tab[b][g_lo], hi = tab[b][g_hi];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const bool up = (int)((gidx >> (8 * e)) & 0xff) != g_lo;
                        gm[e] = up ? hi.x : lo.x; gr[e] = up ? hi.y : lo.y;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float2 w = tab[b][(int)((gidx >> (8 * e)) & 0xff)];
                        gm[e] = w.x; gr[e] = w.y;
                    }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // every product and sum below rounds on its own (no fused multiply-add, which the compiler would form in some
                    // instantiations and not in others), and x is the stored value before it meets the state
#pragma clang fp contract(off)
                    const float x = recon_phys_val(v[e], gm[e], gr[e], gam[e], bet[e], mn[e], inv[e]);
                    if constexpr (MOMENTS) {          // Welford, one member at a time
                        const float d = x - mean[e];
                        mean[e] = mean[e] + d * rkb;
                        m2[e] = m2[e] + d * (x - mean[e]);
                    }
                    if constexpr (EXTREMA) {          // ascending m: a strict comparison keeps the earliest member
                        if (x > vmax[e]) { vmax[e] = x; imax[e] = m; }
                        if (x < vmin[e]) { vmin[e] = x; imin[e] = m; }
                    }
                    if constexpr (EXCEED) exc[e] += x > lim[e] ? 1 : 0;
                }
            }
        }
        if constexpr (MOMENTS) { store8(o.mean + at, mean); store8(o.m2 + at, m2); }
        if constexpr (EXTREMA) { store8(o.vmax + at, vmax); store8(o.vmin + at, vmin); store8(o.imax + at, imax); store8(o.imin + at, imin); }
        if constexpr (EXCEED) store8(o.exceed + at, exc);
    }
}

// p as for ew_recon_physical (layout [B][T][C] only); o: any of the three groups of ReconEnsemble (sgv_ew.h), each complete;
// count_before members are already in the state (0: the state is not read).  A batch of more than EN_MAX_B members goes out as
// several launches with count_before advanced, which is bitwise the same.  Non-zero (nothing launched): -1 null input, -2 no
// group or half a group, -3 bad shape, -4 y or a state array not 16-byte aligned (limit 4), -5 count_before < 0 or
// count_before + B > 2^24 (beyond that (float)k is not exact)
int ew_recon_ensemble(int dtype, GNParams p, const float* scale, const float* mn, long count_before, const ReconEnsemble& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    const bool mo = o.mean || o.m2, ex = o.vmax || o.vmin || o.imax || o.imin, ec = o.exceed || o.limit;
    if (!mo && !ex && !ec) return -2;
    if ((mo && !(o.mean && o.m2)) || (ex && !(o.vmax && o.vmin && o.imax && o.imin)) || (ec && !(o.exceed && o.limit))) return -2;
    if (((uintptr_t)p.y | (uintptr_t)o.mean | (uintptr_t)o.m2 | (uintptr_t)o.vmax | (uintptr_t)o.vmin | (uintptr_t)o.imax | (uintptr_t)o.imin |
         (uintptr_t)o.exceed) & 15) return -4;
    if ((uintptr_t)o.limit & 3) return -4;
    if (count_before < 0 || count_before + p.B > (1L << 24)) return -5;
    const ReconPhys q = recon_setup(p, scale, mn);
    const RSGeom g = rs_geom(p.C);
    const int RL = 256 / g.CV;
    const int rowchunks = std::max(1, std::min(cdiv_i(p.T, RL), cdiv_i(2048, g.colblocks)));      // >= ~2048 blocks, at least one row per row lane
    const dim3 grid(g.colblocks, rowchunks, 1);
    const int B = p.B;
    const size_t esz = dtype == 1 ? 2 : 4;
    for (int b0 = 0; b0 < B; b0 += EN_MAX_B) {
        GNParams ps = p;
        ps.B = std::min(EN_MAX_B, B - b0);
        ps.y = (const char*)p.y + (size_t)b0 * p.T * p.ldy * esz;
        ps.sums = p.sums + (size_t)b0 * p.G * 2;
        const int cb = (int)count_before + b0;
        auto launch = [&](auto el, auto mo_c, auto ex_c, auto ec_c) {
            hipLaunchKernelGGL((recon_ensemble_kernel<typename decltype(el)::type, decltype(mo_c)::value, decltype(ex_c)::value, decltype(ec_c)::value>), grid,
                               dim3(256), 0, s, ps, q, o, cb);
        };
        recon_dispatch(launch, dtype, mo, ex, ec);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// Sobol sensitivity indices (sgv_sobol): the first tail that combines the members of a launch with each other.  A launch holds whole
// blocks of d + 2 members, in this order: A_j, B_j, AB_1_j .. AB_d_j (AB_i_j: the condition A_j with the columns of parameter i taken
// from B_j).  Per (t, n), with x the value recon_phys_val gives for a member, all fp32, every operation rounded on its own:
//   mean, m2       Welford over A_0, B_0, A_1, B_1, ..: A_j has k = 2 j + 1, B_j k = 2 j + 2, the arithmetic of recon_ensemble_kernel
//   first_sq[i]    e = xB - xAB_i;  first_sq[i] = first_sq[i] + e * e      (Jansen's first-order form), ascending j
//   total_sq[i]    e = xA - xAB_i;  total_sq[i] = total_sq[i] + e * e      (Jansen's total form), ascending j
// j counts from blocks_before; every update is sequential in j and the state is stored as it is held, so any cut of the same blocks
// into launches gives the same bits.  With blocks_before == 0 the state is not read.
// Geometry, ownership, the member table and the group lookup are recon_ensemble_kernel's: a thread owns its (t, octet) for all members,
// no reduction across threads, no atomics, no workspace.  Loop order: the A and B values of the launch's blocks stay in registers
// (16 floats per block); then parameter i's two state arrays are streamed through once per launch -- load, update over the blocks,
// store -- while the y rows of parameter i + 1 are already on their way.
// ------------------------------------------------------------------------------------------
constexpr int SB_MAX_D = EN_MAX_B - 2;          // parameters (column groups): one block must fit the member table
// blocks per launch: 16 VGPRs of A / B values each, and a row in flight for this parameter and one for the next (4 / 8 VGPRs each).  Four
// blocks keep the bf16 kernel out of scratch (a batch of 16 is then one launch for every d); the fp32 kernel kept 72 bytes per lane
// in scratch with four and none with three
template <typename T> constexpr int sb_max_blk() { return sizeof(T) == 2 ? 4 : 3; }

// 2 waves / SIMD asked for; the compiler's numbers (gfx950) stand there: no instantiation uses scratch.
template <typename T, bool FIRST, bool TOTAL>
__global__ __launch_bounds__(256, 2) void recon_sobol_kernel(const GNParams p, const ReconPhys q, const ReconSobol o, const int d, const int nbl,
                                                             const int blocks_before) {
    __shared__ float2 tab[EN_MAX_B][SGV_GN_MAX_GROUPS];          // (mean, rstd) of group g of member b; p.B = nbl * (d + 2) <= EN_MAX_B
    constexpr int NB = sb_max_blk<T>();
    __shared__ float rk[2 * NB];                         // 1 / k of A_j (2 j) and B_j (2 j + 1), k = 2 (blocks_before + j) + 1, + 2
    member_table_fill(p, tab);
    if ((int)threadIdx.x < 2 * nbl) rk[threadIdx.x] = 1.0f / (float)(2 * blocks_before + (int)threadIdx.x + 1);
    __syncthreads();
    const GNCtx c = gn_ctx(p);          // blockIdx.z == 0; c.b is not a member here
    if (!c.col_ok) return;              // no barrier below: lanes past C touch nothing
    float gam[8], bet[8], mn[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float4 k = recon_channel(p, q, c.c0 + e, c.col_ok); gam[e] = k.x; bet[e] = k.y; mn[e] = k.z; inv[e] = k.w; }
    const OctetGroups og = octet_groups(p, c.c0);
    const T* y = reinterpret_cast<const T*>(p.y);
    const bool fresh = blocks_before == 0;
    const int S = d + 2;
    const long TC = (long)p.T * p.C;
    // x[8] of member b from its loaded row: the value the output pass would store
    auto value = [&](const Raw8<T>& r, int b, float x[8]) {
        float v[8], gm[8], gr[8];
        raw_unpack(r, v);
        octet_mean_rstd(tab, b, og, gm, gr);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = recon_phys_val(v[e], gm[e], gr[e], gam[e], bet[e], mn[e], inv[e]);
    };
    for (int t = c.t_lo + c.ty; t < c.t_hi; t += c.RL) {
        const long at = (long)t * p.C + c.c0;
        // row t of member j * S + m; past the launch's last block: that block's row again, loaded and not used
        auto row = [&](int j, int m) { return y + ((long)(min(j, nbl - 1) * S + m) * p.T + t) * p.ldy + c.c0; };
        float xa[NB][8], xb[NB][8];
        Raw8<T> cur[NB];          // the rows of AB_i_j, parameter i
        {
            float mean[8], m2[8];
            if (fresh) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { mean[e] = 0.f; m2[e] = 0.f; }
            } else { load8(o.mean + at, mean); load8(o.m2 + at, m2); }
#pragma unroll
            for (int j0 = 0; j0 < NB; j0 += 2) {          // two blocks per round: EN_FLIGHT rows, loads first
                if (j0 >= nbl) break;
                Raw8<T> ra[2], rb[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) { raw_load(row(j0 + u, 0), ra[u]); raw_load(row(j0 + u, 1), rb[u]); }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int j = j0 + u;
                    if (j >= NB || j >= nbl) break;
                    value(ra[u], j * S, xa[j]);
                    value(rb[u], j * S + 1, xb[j]);
                    const float ra_k = rk[2 * j], rb_k = rk[2 * j + 1];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        // Welford, A_j then B_j; no fused multiply-add anywhere (see recon_ensemble_kernel)
#pragma clang fp contract(off)
                        float dl = xa[j][e] - mean[e];
                        mean[e] = mean[e] + dl * ra_k;
                        m2[e] = m2[e] + dl * (xa[j][e] - mean[e]);
                        dl = xb[j][e] - mean[e];
                        mean[e] = mean[e] + dl * rb_k;
                        m2[e] = m2[e] + dl * (xb[j][e] - mean[e]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) raw_load(row(j, 2), cur[j]);          // parameter 0, on its way while the moments go out
            store8(o.mean + at, mean); store8(o.m2 + at, m2);
        }
        for (int i = 0; i < d; ++i) {
            const long ai = (long)i * TC + at;
            float fs[8], ts[8];
            if (fresh) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { fs[e] = 0.f; ts[e] = 0.f; }
            } else {
                if constexpr (FIRST) load8(o.first_sq + ai, fs);
                if constexpr (TOTAL) load8(o.total_sq + ai, ts);
            }
            Raw8<T> nxt[NB];          // parameter i + 1 (after the last one: its rows again, loaded and not used)
            const int in = min(i + 1, d - 1);
#pragma unroll
            for (int j = 0; j < NB; ++j) raw_load(row(j, 2 + in), nxt[j]);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (j >= nbl) break;
                float x[8];
                value(cur[j], j * S + 2 + i, x);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // the difference, its square and the sum round one after the other
#pragma clang fp contract(off)
                    if constexpr (FIRST) { const float df = xb[j][e] - x[e]; fs[e] = fs[e] + df * df; }
                    if constexpr (TOTAL) { const float dt = xa[j][e] - x[e]; ts[e] = ts[e] + dt * dt; }
                }
            }
            if constexpr (FIRST) store8(o.first_sq + ai, fs);
            if constexpr (TOTAL) store8(o.total_sq + ai, ts);
#pragma unroll
            for (int j = 0; j < NB; ++j) cur[j] = nxt[j];
        }
    }
}

// p as for ew_recon_physical (layout [B][T][C] only), p.B = whole blocks of n_params + 2 members; o: ReconSobol (sgv_ew.h), mean and m2
// and at least one of first_sq, total_sq; blocks_before blocks are already in the state (0: the state is not read).  More blocks than a
// launch holds (sb_max_blk, and EN_MAX_B members) go out as several launches cut at block boundaries with blocks_before advanced,
// which is bitwise the same.  Non-zero (nothing launched): -1 null input, -2 neither first_sq nor total_sq, or mean / m2 missing,
// -3 bad shape, n_params outside [1, SB_MAX_D] or B no multiple of n_params + 2, -4 y or a state array not 16-byte aligned,
// -5 blocks_before < 0 or 2 (blocks_before + blocks) > 2^24 (beyond that (float)k is not exact)
int ew_recon_sobol(int dtype, GNParams p, const float* scale, const float* mn, int n_params, long blocks_before, const ReconSobol& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    if ((!o.first_sq && !o.total_sq) || !o.mean || !o.m2) return -2;
    if (n_params < 1 || n_params > SB_MAX_D || p.B % (n_params + 2)) return -3;
    if (((uintptr_t)p.y | (uintptr_t)o.mean | (uintptr_t)o.m2 | (uintptr_t)o.first_sq | (uintptr_t)o.total_sq) & 15) return -4;
    const int S = n_params + 2, blocks = p.B / S;
    if (blocks_before < 0 || blocks_before > (1L << 23) || 2 * (blocks_before + blocks) > (1L << 24)) return -5;
    const ReconPhys q = recon_setup(p, scale, mn);
    const RSGeom g = rs_geom(p.C);
    const int RL = 256 / g.CV;
    const int rowchunks = std::max(1, std::min(cdiv_i(p.T, RL), cdiv_i(2048, g.colblocks)));      // as ew_recon_ensemble
    const dim3 grid(g.colblocks, rowchunks, 1);
    const int per = std::min(dtype == 1 ? sb_max_blk<bf16_t>() : sb_max_blk<float>(), EN_MAX_B / S);          // >= 1: S <= EN_MAX_B
    const size_t esz = dtype == 1 ? 2 : 4;
    for (int j0 = 0; j0 < blocks; j0 += per) {
        GNParams ps = p;
        const int nbl = std::min(per, blocks - j0);
        ps.B = nbl * S;
        ps.y = (const char*)p.y + (size_t)j0 * S * p.T * p.ldy * esz;
        ps.sums = p.sums + (size_t)j0 * S * p.G * 2;
        const int bb = (int)blocks_before + j0;
        auto launch = [&](auto el, auto fi_c, auto to_c) {
            hipLaunchKernelGGL((recon_sobol_kernel<typename decltype(el)::type, decltype(fi_c)::value, decltype(to_c)::value>), grid, dim3(256), 0, s,
                               ps, q, o, n_params, nbl, bb);
        };
        recon_dispatch(launch, dtype, o.first_sq != nullptr, o.total_sq != nullptr);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// Surrogate distributions (sgv_distribution): the histogram of the members per (t, n), between bounds lo / hi [T][C] the caller gives
// (the envelope an extrema pass of sgv_ensemble found over the same members).  With x the value recon_phys_val gives for a member and
// K bins, all fp32 and every operation rounded on its own:
//   invw = hi > lo ? (float)K / (hi - lo) : 0.0f              (one subtraction, one correctly rounded division)
//   row  = x < lo ? 0 : x > hi ? K + 1 : 1 + min((int)((x - lo) * invw), K - 1)
//   counts[row][t][n] += 1                                    (int32 [K + 2][T][C]: underflow, the K bins, overflow)
// The pass only adds: integer counts are exact and independent of order, so any cut of the members into launches gives the same bits
// and there is no "state not read" mode -- a new state is zeroed by the caller.
// Geometry, ownership, the member table and the group lookup are recon_ensemble_kernel's: a thread owns its (t, octet) for all members,
// no reduction across threads, no atomics, no workspace.  The bin index depends on the data, so counters in registers would be indexed
// dynamically and end in scratch; they live in LDS instead, one byte per (row, thread, channel) -- a launch holds at most EN_MAX_B = 32
// members.  Layout [K + 2][2][256] dwords: dword (row, h, tid) holds the bytes of channels 4 h .. 4 h + 3 of thread tid, so the 32
// lanes the LDS serves per cycle touch 32 different banks whatever their rows are (a row is 512 dwords).  With the 8 bytes of a thread
// side by side, lanes l and l + 16 of every such group would share a bank.  (K + 2) * 2 KiB of dynamic LDS per block: 68 KiB at K = 32
// (two blocks per CU), 132 KiB at K = 64 (one).
// Per row t: the launch's members are counted into the thread's own bytes -- the 8 bytes of a member are read, then written, and the
// LDS serves a wave's operations in order, so the next member sees them -- then the rows of the state are flushed HI_FLIGHT at a
// time: the thread's two dwords of each are read, and where one is not zero the 32-byte octet of counts is loaded, the bytes are added,
// the octet is stored and the dwords are zeroed again.  Rows without an increment cost no global traffic.
// ------------------------------------------------------------------------------------------
constexpr int HI_MIN_BINS = 2, HI_MAX_BINS = 64;
constexpr int HI_FLIGHT = 4;          // rows of the state whose octets are loaded before the first is used
constexpr int HI_ROW_DWORDS = 512;    // one row of the block's byte histogram: [2][256] dwords
static size_t hist_lds_bytes(int bins) { return (size_t)(bins + 2) * HI_ROW_DWORDS * 4; }

template <typename T>
__global__ __launch_bounds__(256) void recon_hist_kernel(const GNParams p, const ReconPhys q, const ReconDistribution o) {
    extern __shared__ unsigned int hist_lds[];                   // [K + 2][2][256]
    __shared__ float2 tab[EN_MAX_B][SGV_GN_MAX_GROUPS];          // (mean, rstd) of group g of member b
    const int K = o.bins, tid = threadIdx.x;
    member_table_fill(p, tab);
    for (int r = 0; r < K + 2; ++r) { hist_lds[r * HI_ROW_DWORDS + tid] = 0u; hist_lds[r * HI_ROW_DWORDS + 256 + tid] = 0u; }
    __syncthreads();
    const GNCtx c = gn_ctx(p);          // blockIdx.z == 0; c.b is not a member here
    if (!c.col_ok) return;              // no barrier below: lanes past C touch nothing
    float gam[8], bet[8], mn[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float4 k = recon_channel(p, q, c.c0 + e, c.col_ok); gam[e] = k.x; bet[e] = k.y; mn[e] = k.z; inv[e] = k.w; }
    const OctetGroups og = octet_groups(p, c.c0);
    const T* y = reinterpret_cast<const T*>(p.y);
    unsigned int* const mine = hist_lds + tid;                                        // dword (row, h): mine[row * HI_ROW_DWORDS + 256 h]
    unsigned char* const mine_b = reinterpret_cast<unsigned char*>(mine);             // byte of channel e in row 0: mine_b[1024 (e / 4) + e % 4]
    const long TC = (long)p.T * p.C;
    const float fK = (float)K, fKm1 = (float)(K - 1);
    for (int t = c.t_lo + c.ty; t < c.t_hi; t += c.RL) {
        const long at = (long)t * p.C + c.c0;
        float lo[8], hi[8], invw[8];
        load8(o.lo + at, lo); load8(o.hi + at, hi);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
#pragma clang fp contract(off)
            invw[e] = hi[e] > lo[e] ? fK / (hi[e] - lo[e]) : 0.0f;
        }
        for (int b0 = 0; b0 < p.B; b0 += EN_FLIGHT) {          // EN_FLIGHT members per round, loads first
            Raw8<T> r[EN_FLIGHT];
#pragma unroll
            for (int u = 0; u < EN_FLIGHT; ++u)                  // past the last member: its row again, loaded and not used
                raw_load(y + ((long)min(b0 + u, p.B - 1) * p.T + t) * p.ldy + c.c0, r[u]);
#pragma unroll
            for (int u = 0; u < EN_FLIGHT; ++u) {
                const int b = b0 + u;
                if (b >= p.B) break;
                float v[8], gm[8], gr[8];
                raw_unpack(r[u], v);
                octet_mean_rstd(tab, b, og, gm, gr);
                int off[8];          // the byte of (row, channel e), from mine_b
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // x is the stored value; the difference and the product round one after the other (no fused multiply-add)
#pragma clang fp contract(off)
                    const float x = recon_phys_val(v[e], gm[e], gr[e], gam[e], bet[e], mn[e], inv[e]);
                    const float s = (x - lo[e]) * invw[e];
                    // s >= 0 wherever the rule is defined, and there min((int)s, K - 1) == (int)min(s, K - 1); clamped as a float, a NaN
                    // or a range turned round still gives a row of the block's histogram
                    const int j = (int)fminf(fmaxf(s, 0.0f), fKm1);
                    const int row = x < lo[e] ? 0 : x > hi[e] ? K + 1 : 1 + j;
                    off[e] = row * (HI_ROW_DWORDS * 4) + (e >> 2) * 1024 + (e & 3);
                }
                unsigned char n[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) n[e] = mine_b[off[e]];          // 8 different bytes: channel e has its own
#pragma unroll
                for (int e = 0; e < 8; ++e) mine_b[off[e]] = (unsigned char)(n[e] + 1);
            }
        }
        for (int r0 = 0; r0 < K + 2; r0 += HI_FLIGHT) {          // HI_FLIGHT rows of the state per round, loads first
            unsigned int w0[HI_FLIGHT], w1[HI_FLIGHT];
            int cnt[HI_FLIGHT][8];
#pragma unroll
            for (int u = 0; u < HI_FLIGHT; ++u) {
                const bool in = r0 + u < K + 2;
                w0[u] = in ? mine[(r0 + u) * HI_ROW_DWORDS] : 0u;
                w1[u] = in ? mine[(r0 + u) * HI_ROW_DWORDS + 256] : 0u;
            }
#pragma unroll
            for (int u = 0; u < HI_FLIGHT; ++u)
                if (w0[u] | w1[u]) load8(o.counts + (long)(r0 + u) * TC + at, cnt[u]);
#pragma unroll
            for (int u = 0; u < HI_FLIGHT; ++u) {
                if (!(w0[u] | w1[u])) continue;
#pragma unroll
                for (int e = 0; e < 8; ++e) cnt[u][e] += (int)(((e < 4 ? w0[u] : w1[u]) >> (8 * (e & 3))) & 0xffu);
                store8(o.counts + (long)(r0 + u) * TC + at, cnt[u]);
                mine[(r0 + u) * HI_ROW_DWORDS] = 0u;
                mine[(r0 + u) * HI_ROW_DWORDS + 256] = 0u;
            }
        }
    }
}

// p as for ew_recon_physical (layout [B][T][C] only); o: ReconDistribution (sgv_ew.h), all of lo, hi, counts; count_before members are
// already in the state, which bounds the study and nothing else.  A batch of more than EN_MAX_B members goes out as several launches
// (a counter of a launch fits a byte), which is bitwise the same.  Non-zero (nothing launched): -1 null input, -2 lo, hi or counts
// missing, -3 bad shape or bins outside [2, 64], -4 y, lo, hi or counts not 16-byte aligned, -5 count_before < 0 or
// count_before + B > 2^24, -6 the kernel's dynamic LDS limit could not be raised
int ew_recon_distribution(int dtype, GNParams p, const float* scale, const float* mn, long count_before, const ReconDistribution& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    if (!o.lo || !o.hi || !o.counts) return -2;
    if (o.bins < HI_MIN_BINS || o.bins > HI_MAX_BINS) return -3;
    if (((uintptr_t)p.y | (uintptr_t)o.lo | (uintptr_t)o.hi | (uintptr_t)o.counts) & 15) return -4;
    if (count_before < 0 || count_before + p.B > (1L << 24)) return -5;
    // more than 64 KiB of dynamic LDS has to be asked for, once per kernel
    static bool raised[2] = {false, false};
    if (!raised[dtype == 1]) {
        const void* fn = dtype == 1 ? reinterpret_cast<const void*>(&recon_hist_kernel<bf16_t>) : reinterpret_cast<const void*>(&recon_hist_kernel<float>);
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_lds_bytes(HI_MAX_BINS)) != hipSuccess) return -6;
        raised[dtype == 1] = true;
    }
    const ReconPhys q = recon_setup(p, scale, mn);
    const RSGeom g = rs_geom(p.C);
    const int RL = 256 / g.CV;
    const int rowchunks = std::max(1, std::min(cdiv_i(p.T, RL), cdiv_i(2048, g.colblocks)));      // as ew_recon_ensemble
    const dim3 grid(g.colblocks, rowchunks, 1);
    const int B = p.B;
    const size_t esz = dtype == 1 ? 2 : 4, lds = hist_lds_bytes(o.bins);
    for (int b0 = 0; b0 < B; b0 += EN_MAX_B) {
        GNParams ps = p;
        ps.B = std::min(EN_MAX_B, B - b0);
        ps.y = (const char*)p.y + (size_t)b0 * p.T * p.ldy * esz;
        ps.sums = p.sums + (size_t)b0 * p.G * 2;
        auto launch = [&](auto el, auto) { hipLaunchKernelGGL((recon_hist_kernel<typename decltype(el)::type>), grid, dim3(256), lds, s, ps, q, o); };
        recon_dispatch(launch, dtype, true);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// Surrogate response surfaces (sgv_regress): the co-moments of the field with K covariates the caller has per member (the inputs of a
// design study, or any scalar per draw), beside the moments of the ensemble pass.  The host centres the covariates -- w[m][i] =
// float32(y_m,i - ybar_i), ybar the running mean including member m, in float64 -- and per (t, n), with x the value recon_phys_val gives
// for member m, k = m + 1, all fp32 and every operation rounded on its own, members in ascending order:
//   d = x - mean;  mean = mean + d * (1.0f / (float)k);  m2 = m2 + d * (x - mean)          (recon_ensemble_kernel's moments, bit for bit)
//   co[i] = co[i] + d * w[m][i]      for i = 0 .. K - 1                                       (C_n = C_n-1 + (x_n - xbar_n-1)(y_n - ybar_n))
// m counts from count_before; every update is sequential in m and the state is stored as it is held, so any cut of the same members
// into launches gives the same bits.  With count_before == 0 the state is not read.
// Geometry, ownership, the member table and the group lookup are recon_ensemble_kernel's: a thread owns its (t, octet) for all members,
// no reduction across threads, no atomics, no workspace.  Loop order (recon_sobol_kernel's): Welford over the launch's members first,
// each member's d[8] staying in registers, then covariate i's state row is streamed through once per launch -- load, update over the
// members, store -- while the row of covariate i + 1 is already on its way.  The launch's weights [members][K] lie in LDS beside the
// member table; every thread of the block reads the same word, a broadcast.
// ------------------------------------------------------------------------------------------
constexpr int RG_MAX_K = 32;          // covariates
// members per launch: 8 VGPRs of d each.  Fewer members mean more passes over the (2 + K) state arrays per batch, more cost occupancy;
// 16 measured faster than 8 in bf16, and fp32 takes the larger candidate without scratch
template <typename T> constexpr int rg_members() { return sizeof(T) == 2 ? 16 : 8; }

// f(integral_constant<b0>) for b0 = B0, B0 + STEP, .. while b0 < min(n, NM): the members of recon_regress_kernel, or rounds of them
template <int B0, int NM, int STEP, typename F>
__device__ __forceinline__ void rg_rounds(int n, F&& f) {
    if constexpr (B0 < NM) {
        if (B0 < n) {
            f(std::integral_constant<int, B0>{});
            rg_rounds<B0 + STEP, NM, STEP>(n, f);
        }
    }
}

// 2 waves / SIMD asked for: 243 VGPRs for bf16 with 16 members, 190 for fp32 with 8, neither with scratch.  bf16 with 8 members and 3 waves
// asked for kept 28 bytes per lane in scratch and was slower.
template <typename T, int NM>
__global__ __launch_bounds__(256, 2) void recon_regress_kernel(const GNParams p, const ReconPhys q, const ReconRegress o, const int K, const int count_before) {
    __shared__ float2 tab[NM][SGV_GN_MAX_GROUPS];          // (mean, rstd) of group g of member b; p.B <= NM
    __shared__ float rk[NM];                               // 1 / k, k = count_before + b + 1: one correctly rounded division per member
    __shared__ float wl[NM * RG_MAX_K];                    // w[b][i] at wl[b * K + i]
    member_table_fill(p, tab);
    if ((int)threadIdx.x < p.B) rk[threadIdx.x] = 1.0f / (float)(count_before + (int)threadIdx.x + 1);
    for (int i = threadIdx.x; i < p.B * K; i += 256) wl[i] = o.w[i];
    __syncthreads();
    const GNCtx c = gn_ctx(p);          // blockIdx.z == 0; c.b is not a member here
    if (!c.col_ok) return;              // no barrier below: lanes past C touch nothing
    float gam[8], bet[8], mn[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float4 k = recon_channel(p, q, c.c0 + e, c.col_ok); gam[e] = k.x; bet[e] = k.y; mn[e] = k.z; inv[e] = k.w; }
    const OctetGroups og = octet_groups(p, c.c0);
    const T* y = reinterpret_cast<const T*>(p.y);
    const bool fresh = count_before == 0;
    const long TC = (long)p.T * p.C;
    for (int t = c.t_lo + c.ty; t < c.t_hi; t += c.RL) {
        const long at = (long)t * p.C + c.c0;
        float d[NM][8];          // x - mean before the member entered the mean
        Raw8<float> cur;         // co[i] of this (t, octet)
        raw_zero(cur);
        {
            float mean[8], m2[8];
            if (fresh) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { mean[e] = 0.f; m2[e] = 0.f; }
            } else { load8(o.mean + at, mean); load8(o.m2 + at, m2); }
            // EN_FLIGHT members per round, loads first; the rounds are written out at compile time (rg_rounds), so that every index into d
            // is a constant whatever the unroller decides: d must never be addressed dynamically
            rg_rounds<0, NM, EN_FLIGHT>(p.B, [&](auto b0c) {
                constexpr int b0 = decltype(b0c)::value;
                Raw8<T> r[EN_FLIGHT];
#pragma unroll
                for (int u = 0; u < EN_FLIGHT; ++u)                  // past the last member: its row again, loaded and not used
                    raw_load(y + ((long)min(b0 + u, p.B - 1) * p.T + t) * p.ldy + c.c0, r[u]);
#pragma unroll
                for (int u = 0; u < EN_FLIGHT; ++u) {
                    if (b0 + u >= p.B) break;
                    const float rkb = rk[b0 + u];
                    float v[8], gm[8], gr[8];
                    raw_unpack(r[u], v);
                    octet_mean_rstd(tab, b0 + u, og, gm, gr);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        // Welford, one member at a time; no fused multiply-add anywhere (see recon_ensemble_kernel)
#pragma clang fp contract(off)
                        const float x = recon_phys_val(v[e], gm[e], gr[e], gam[e], bet[e], mn[e], inv[e]);
                        d[b0 + u][e] = x - mean[e];
                        mean[e] = mean[e] + d[b0 + u][e] * rkb;
                        m2[e] = m2[e] + d[b0 + u][e] * (x - mean[e]);
                    }
                }
            });
            if (!fresh) raw_load(o.co + at, cur);          // covariate 0, on its way while the moments go out
            store8(o.mean + at, mean); store8(o.m2 + at, m2);
        }
        for (int i = 0; i < K; ++i) {
            const long ai = (long)i * TC + at;
            Raw8<float> nxt;         // covariate i + 1 (after the last one: its row again, loaded and not used)
            raw_zero(nxt);
            if (!fresh) raw_load(o.co + (long)min(i + 1, K - 1) * TC + at, nxt);
            float co[8];
            raw_unpack(cur, co);
            rg_rounds<0, NM, 1>(p.B, [&](auto bc) {
                constexpr int b = decltype(bc)::value;
                const float w = wl[b * K + i];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // the product and the sum round one after the other
#pragma clang fp contract(off)
                    co[e] = co[e] + d[b][e] * w;
                }
            });
            store8(o.co + ai, co);
            cur = nxt;
        }
    }
}

// p as for ew_recon_physical (layout [B][T][C] only); o: ReconRegress (sgv_ew.h), all of mean, m2, co and w; n_cov = K covariates;
// count_before members are already in the state (0: the state is not read).  A batch of more than rg_members members goes out as
// several launches with count_before advanced, which is bitwise the same.  Non-zero (nothing launched): -1 null input, -2 mean, m2,
// co or w missing, -3 bad shape or n_cov outside [1, 32], -4 y or a state array not 16-byte aligned or w not 4-byte aligned,
// -5 count_before < 0 or count_before + B > 2^24 (beyond that (float)k is not exact)
int ew_recon_regress(int dtype, GNParams p, const float* scale, const float* mn, int n_cov, long count_before, const ReconRegress& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    if (!o.mean || !o.m2 || !o.co || !o.w) return -2;
    if (n_cov < 1 || n_cov > RG_MAX_K) return -3;
    if (((uintptr_t)p.y | (uintptr_t)o.mean | (uintptr_t)o.m2 | (uintptr_t)o.co) & 15) return -4;
    if ((uintptr_t)o.w & 3) return -4;
    if (count_before < 0 || count_before + p.B > (1L << 24)) return -5;
    const ReconPhys q = recon_setup(p, scale, mn);
    const RSGeom g = rs_geom(p.C);
    const int RL = 256 / g.CV;
    const int rowchunks = std::max(1, std::min(cdiv_i(p.T, RL), cdiv_i(2048, g.colblocks)));      // as ew_recon_ensemble
    const dim3 grid(g.colblocks, rowchunks, 1);
    const int B = p.B, per = dtype == 1 ? rg_members<bf16_t>() : rg_members<float>();
    const size_t esz = dtype == 1 ? 2 : 4;
    for (int b0 = 0; b0 < B; b0 += per) {
        GNParams ps = p;
        ps.B = std::min(per, B - b0);
        ps.y = (const char*)p.y + (size_t)b0 * p.T * p.ldy * esz;
        ps.sums = p.sums + (size_t)b0 * p.G * 2;
        ReconRegress os = o;
        os.w = o.w + (size_t)b0 * n_cov;
        const int cb = (int)count_before + b0;
        auto launch = [&](auto el, auto) {
            using T = typename decltype(el)::type;
            hipLaunchKernelGGL((recon_regress_kernel<T, rg_members<T>()>), grid, dim3(256), 0, s, ps, q, os, n_cov, cb);
        };
        recon_dispatch(launch, dtype, true);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// Surrogate linear functionals (sgv_project): R weighted sums over the mesh per (sample, t), out[b][t][r] = sum_n W[r][n] x[b][t][n] with
// x the value recon_phys_val gives -- the first tail shaped like a GEMM, [B*T] x [C] x [R <= 32], and the first on the matrix cores:
// v_mfma_f32_32x32x2_f32 with the 32 columns the functionals (rows of W past R are zeros), exact fp32 products and one fused
// multiply-add chain per output, ascending in k.
// Geometry: the rows m = b * T + t are taken flat, PJ_M tiles of 32 per block; a tile may span samples, so every lane keeps the sample
// of each of its rows and takes (mean, rstd) from a block table [row's sample][group] filled through gn_mean_rstd.  The MFMA's A operand
// wants lane l to hold row l & 31 and k = l >> 5, so the load geometry is the operand's: lane l loads 8 channels (16 / 32 bytes) of
// row l & 31 at channel cb + 8 (l >> 5), and MFMA e = 0..7 of the step takes channels cb + e (k = 0) and cb + 8 + e (k = 1); the B
// operand is 8 consecutive weights of row l & 31 at the same channels, and the channel constants are those channels'.  The weights and
// constants of a step serve all PJ_M row tiles.
// Shares: a block owns PJ_CHUNK channels, its four waves PJ_WAVE_COLS contiguous ones each.  A wave's chain runs over its channels in
// the order above; the four waves meet through LDS and are added in wave order in fp32; the per-block partials [B*T][chunks][R] go
// to the workspace and recon_project_finish_kernel adds them in ascending chunk order in fp64 and rounds once.  The shares depend on C alone,
// and an output element of the MFMA depends on its own row of A and column of B alone: hence the invariances of sgv_ew.h.  Lanes past C
// carry zeros on both operands and load nothing there; rows past B*T load the last row again and are not written.
// ------------------------------------------------------------------------------------------
constexpr int PJ_ROWS = 32;                         // rows of an MFMA tile
constexpr int PJ_M = 2;                             // row tiles per block: what one load of weights and constants serves
constexpr int PJ_WAVE_COLS = 1024;                  // channels of a wave's chain (a multiple of 16)
constexpr int PJ_CHUNK = 4 * PJ_WAVE_COLS;          // channels per block, per partial
static int pj_chunks(int C) { return cdiv_i(C, PJ_CHUNK); }
size_t ew_recon_project_work_floats(int B, int T, int C, int R) { return ((size_t)B * T * pj_chunks(C) * R + 3) & ~(size_t)3; }

template <typename T>
__global__ __launch_bounds__(256) void recon_project_kernel(const GNParams p, const ReconPhys q, const ReconProject o) {
    __shared__ float2 tab[PJ_M * PJ_ROWS][SGV_GN_MAX_GROUPS];          // (mean, rstd) of group g of the block's i-th sample
    __shared__ float red[4][PJ_M * PJ_ROWS * 32];                      // the waves' accumulators: [wave][tile][row][r]
    const long rows = (long)p.B * p.T, row0 = (long)blockIdx.y * (PJ_M * PJ_ROWS);
    const int b_first = (int)(row0 / p.T), b_last = (int)(min(rows - 1, row0 + PJ_M * PJ_ROWS - 1) / p.T);
    for (int i = threadIdx.x; i < (b_last - b_first + 1) * p.G; i += 256) {
        float m, r;
        gn_mean_rstd(p, b_first + i / p.G, i % p.G, m, r);
        tab[i / p.G][i % p.G] = make_float2(m, r);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 31, h = lane >> 5;
    const T* yrow[PJ_M];
    int bi[PJ_M];
#pragma unroll
    for (int m = 0; m < PJ_M; ++m) {
        const long row = min(row0 + m * PJ_ROWS + lr, rows - 1);
        yrow[m] = reinterpret_cast<const T*>(p.y) + row * p.ldy;
        bi[m] = (int)(row / p.T) - b_first;
    }
    const bool r_ok = lr < o.n_func;
    const float* const wrow = o.weights + (long)(r_ok ? lr : 0) * p.C;
    const int c_lo = blockIdx.x * PJ_CHUNK + wv * PJ_WAVE_COLS, c_hi = min(p.C, c_lo + PJ_WAVE_COLS);
    f32x16 acc[PJ_M];
#pragma unroll
    for (int m = 0; m < PJ_M; ++m)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[m][v] = 0.f;
    for (int cb = c_lo; cb < c_hi; cb += 16) {          // wave-uniform; c_hi is a multiple of 8: only the upper half of the last step can be past it
        const bool ok = cb + 8 * h < c_hi;
        const int c0 = ok ? cb + 8 * h : cb;            // a half past the end loads the lower half's addresses and uses nothing
        Raw8<T> ry[PJ_M];
#pragma unroll
        for (int m = 0; m < PJ_M; ++m) raw_load(yrow[m] + c0, ry[m]);
        float w[8], gam[8], bet[8], mn[8], inv[8];
        load8(wrow + c0, w);
        load8(p.gamma + c0, gam); load8(p.beta + c0, bet); load8(q.mn + c0, mn); load8(q.scale + c0, inv);
        const bool w_ok = ok && r_ok;
#pragma unroll
        for (int e = 0; e < 8; ++e) { w[e] = w_ok ? w[e] : 0.f; inv[e] = recon_phys_inv(inv[e]); }
        // the groups of the octet: with Cg >= 8 (block-uniform) at most two, the first n_lo channels in g_lo
        const int g0 = c0 / p.Cg, n_lo = p.Cg - (c0 - g0 * p.Cg);
        const int g_lo = min(g0, p.G - 1), g_hi = min(g0 + 1, p.G - 1);
        float x[PJ_M][8];
#pragma unroll
        for (int m = 0; m < PJ_M; ++m) {
            float v[8], gm[8], gr[8];
            raw_unpack(ry[m], v);
            if (p.Cg >= 8) {
                const float2 lo = tab[bi[m]][g_lo], hi = tab[bi[m]][g_hi];
#pragma unroll
                for (int e = 0; e < 8; ++e) { gm[e] = e < n_lo ? lo.x : hi.x; gr[e] = e < n_lo ? lo.y : hi.y; }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float2 k = tab[bi[m]][min((c0 + e) / p.Cg, p.G - 1)];
                    gm[e] = k.x; gr[e] = k.y;
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float val = recon_phys_val(v[e], gm[e], gr[e], gam[e], bet[e], mn[e], inv[e]);
                x[m][e] = ok ? val : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int m = 0; m < PJ_M; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[m][e], w[e], acc[m], 0, 0, 0);
    }
    // C / D map of the 32x32 forms: register v of lane l holds row (v & 3) + 8 (v >> 2) + 4 (l >> 5), column l & 31
#pragma unroll
    for (int m = 0; m < PJ_M; ++m)
#pragma unroll
        for (int v = 0; v < 16; ++v) red[wv][(m * PJ_ROWS + (v & 3) + 8 * (v >> 2) + 4 * h) * 32 + lr] = acc[m][v];
    __syncthreads();
    const int nchunk = gridDim.x;
    for (int i = threadIdx.x; i < PJ_M * PJ_ROWS * 32; i += 256) {
        const long row = row0 + (i >> 5);
        const int r = i & 31;
        if (row < rows && r < o.n_func)
            o.work[(row * nchunk + blockIdx.x) * o.n_func + r] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];          // wave order
    }
}

// partials [rows][nchunk][R] -> out [rows][R]: one thread per output, its partials in ascending chunk order in fp64, rounded once
__global__ __launch_bounds__(256) void recon_project_finish_kernel(const float* __restrict__ part, long n_out, int nchunk, int R, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    const long row = i / R;
    const int r = (int)(i - row * R);
    double s = 0.0;
    for (int j = 0; j < nchunk; ++j) s += (double)part[(row * nchunk + j) * R + r];
    out[i] = (float)s;
}

// p as for ew_recon_physical (layout [B][T][C] only); o: ReconProject (sgv_ew.h), o.work = ew_recon_project_work_floats floats.  Non-zero
// (nothing launched): -1 null input, -2 no output, -3 bad shape or n_func outside [1, 32], -4 y, weights or work not 16-byte aligned
// or out not 4-byte aligned, -6 no workspace
int ew_recon_project(int dtype, GNParams p, const float* scale, const float* mn, const ReconProject& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    if (!o.weights) return -1;
    if (!o.out) return -2;
    if (o.n_func < 1 || o.n_func > SGV_MAX_FUNCTIONALS) return -3;
    if (((uintptr_t)p.y | (uintptr_t)o.weights | (uintptr_t)o.work) & 15) return -4;
    if ((uintptr_t)o.out & 3) return -4;
    if (!o.work) return -6;
    const ReconPhys q = recon_setup(p, scale, mn);
    const long rows = (long)p.B * p.T;
    const int nchunk = pj_chunks(p.C);
    const dim3 grid(nchunk, cdiv_i(rows, PJ_M * PJ_ROWS), 1);
    if (dtype == 1) hipLaunchKernelGGL((recon_project_kernel<bf16_t>), grid, dim3(256), 0, s, p, q, o);
    else hipLaunchKernelGGL((recon_project_kernel<float>), grid, dim3(256), 0, s, p, q, o);
    hipLaunchKernelGGL(recon_project_finish_kernel, dim3(cdiv_i(rows * o.n_func, 256)), dim3(256), 0, s, o.work, rows * o.n_func, nchunk, o.n_func, o.out);
    return 0;
}

// ------------------------------------------------------------------------------------------
// Surrogate temporal functionals (sgv_temporal): R weighted sums over time per (sample, node), out[b][r][n] = sum_t W[r][t] x[b][t][n]
// with x the value recon_phys_val gives -- the dual of sgv_project and the second tail on the matrix cores, v_mfma_f32_32x32x2_f32 again:
// exact fp32 products and one fused multiply-add chain per output, ascending in t.
// Geometry: the contraction index t is the MFMA's k, two time rows per step.  The weights are the A operand: lane l holds
// W[r = l & 31][t0 + (l >> 5)], rows past R zeros; the kernel reads them from a transposed, zero-padded copy wt [T_pad][32] (T_pad = T
// rounded up to 2) that recon_temporal_weights_kernel writes in front of it, one coalesced dword per lane and step.  The field is the B
// operand: lane l loads 8 channels (16 / 32 bytes) of row t0 + (l >> 5) at channel c0 = c_w + 8 (l & 31), and MFMA e = 0..7 of the step
// takes the lane's channel e, so a wave reads two contiguous rows of TP_WAVE_COLS = 256 channels per step and owns 8 accumulator tiles
// of 32 functionals x 32 channels.  In the C / D map register v of lane l is functional (v & 3) + 8 (v >> 2) + 4 (l >> 5) at the lane's
// own column, i.e. at its 8 consecutive channels over the 8 tiles: the stores to out[b][r][c0 .. c0 + 7] are 32 bytes per lane and
// 1 KiB contiguous per half-wave, straight from the registers.  The channel constants and the sample's (mean, rstd) of the lane's 8
// channels are loaded once for all T.
// Shares: a block is one sample and TP_BLOCK_COLS channels, its four waves TP_WAVE_COLS contiguous ones each; they never meet: no
// reduction across threads, no LDS besides gn_consts' table, no workspace besides wt, no finish kernel, no atomics.  An output's chain
// runs over t alone and an output element of the MFMA depends on its own row of A and column of B alone: hence the invariances of
// sgv_ew.h.  For odd T the upper half of the last step carries zeros on both operands and loads row T - 1 again; lanes past C load
// the wave's first octet again, carry zeros on B (and their weight on A) and store nothing.  The y rows (and the weights) of
// tp_flight() steps are in flight: a register ring, the loads of step s + tp_flight() are issued as soon as step s is unpacked.
// ------------------------------------------------------------------------------------------
constexpr int TP_WAVE_COLS = 256;                   // channels of a wave: 32 lanes x 8
constexpr int TP_BLOCK_COLS = 4 * TP_WAVE_COLS;     // channels of a block
template <typename T> constexpr int tp_flight() { return sizeof(T) == 2 ? 8 : 4; }          // steps in flight: 8 KiB of y per wave and 32 registers per lane in either dtype
static int tp_tpad(int T) { return (T + 1) & ~1; }
size_t ew_recon_temporal_work_floats(int T) { return (size_t)tp_tpad(T) * SGV_MAX_TEMPORAL; }

// weights [R][T] -> wt [T_pad][32], zeros at r >= R and t >= T: one thread per element of wt
__global__ __launch_bounds__(256) void recon_temporal_weights_kernel(const float* __restrict__ w, int R, int T, int n, float* __restrict__ wt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int t = i >> 5, r = i & 31;
    wt[i] = r < R && t < T ? w[(long)r * T + t] : 0.f;
}

template <typename T>
__global__ __launch_bounds__(256, 2) void recon_temporal_kernel(const GNParams p, const ReconPhys q, const ReconTemporal o) {
    constexpr int F = tp_flight<T>();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 31, h = lane >> 5;
    const int c_w = blockIdx.x * TP_BLOCK_COLS + wv * TP_WAVE_COLS;
    GNCtx c;
    c.b = blockIdx.z;
    c.c0 = c_w + 8 * lr;
    c.col_ok = c.c0 < p.C;
    float mean[8], rstd[8];
    gn_consts(p, c, mean, rstd);          // all 256 threads
    if (c_w >= p.C) return;               // a whole wave past C; no barrier below
    // An MFMA reads the registers of every lane whatever EXEC says, and a lane's A operand (its weight) goes into its functional at
    // ALL columns: the lanes past C stay in the loop and carry their weights.  Their B operand reaches their own columns only; it is
    // zero, their y loads are the wave's first octet again and nothing of theirs is stored.
    float gam[8], bet[8], mn[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float4 k = recon_channel(p, q, c.c0 + e, c.col_ok); gam[e] = k.x; bet[e] = k.y; mn[e] = k.z; inv[e] = k.w; }
    const T* const y = reinterpret_cast<const T*>(p.y) + (long)c.b * p.T * p.ldy + (c.col_ok ? c.c0 : c_w);
    const float* const wt = o.work + lr;
    const int nsteps = (p.T + 1) >> 1;
    f32x16 acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[e][v] = 0.f;
    // step s: rows 2 s + h.  A row past T - 1 (the upper half of the last step of an odd T, or a step past the last) is row T - 1 again,
    // loaded and not used; wt is read inside [0, T_pad) only
    Raw8<T> ry[F];
    float a[F];
#pragma unroll
    for (int u = 0; u < F; ++u) {
        const int t = 2 * min(u, nsteps - 1) + h;
        raw_load(y + (long)min(t, p.T - 1) * p.ldy, ry[u]);
        a[u] = wt[t * 32];
    }
    for (int s0 = 0; s0 < nsteps; s0 += F) {
#pragma unroll
        for (int u = 0; u < F; ++u) {
            const int s = s0 + u;
            if (s >= nsteps) break;          // wave-uniform
            float v[8];
            raw_unpack(ry[u], v);
            const float au = a[u];
            const bool t_ok = c.col_ok && 2 * s + h < p.T;
            {
                const int t = 2 * min(s + F, nsteps - 1) + h;
                raw_load(y + (long)min(t, p.T - 1) * p.ldy, ry[u]);
                a[u] = wt[t * 32];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float x = recon_phys_val(v[e], mean[e], rstd[e], gam[e], bet[e], mn[e], inv[e]);
                acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(au, t_ok ? x : 0.f, acc[e], 0, 0, 0);
            }
        }
    }
    // C / D map of the 32x32 forms: register v of lane l holds row (v & 3) + 8 (v >> 2) + 4 (l >> 5), column l & 31
    float* const out = o.out + (long)c.b * o.n_func * p.C + c.c0;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int r = (v & 3) + 8 * (v >> 2) + 4 * h;
        if (c.col_ok && r < o.n_func) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = acc[e][v];
            store8(out + (long)r * p.C, x);
        }
    }
}

// p as for ew_recon_physical (layout [B][T][C] only); o: ReconTemporal (sgv_ew.h), o.work = ew_recon_temporal_work_floats floats.  Non-zero
// (nothing launched): -1 null input (weights included), -2 no output, -3 bad shape or n_func outside [1, 32], -4 y or out not 16-byte
// aligned or weights or work not 4-byte aligned, -6 no workspace
int ew_recon_temporal(int dtype, GNParams p, const float* scale, const float* mn, const ReconTemporal& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    if (!o.weights) return -1;
    if (!o.out) return -2;
    if (o.n_func < 1 || o.n_func > SGV_MAX_TEMPORAL) return -3;
    if (((uintptr_t)p.y | (uintptr_t)o.out) & 15) return -4;
    if (((uintptr_t)o.weights | (uintptr_t)o.work) & 3) return -4;
    if (!o.work) return -6;
    const ReconPhys q = recon_setup(p, scale, mn);
    const int n = tp_tpad(p.T) * SGV_MAX_TEMPORAL;
    hipLaunchKernelGGL(recon_temporal_weights_kernel, dim3(cdiv_i(n, 256)), dim3(256), 0, s, o.weights, o.n_func, p.T, n, o.work);
    const dim3 grid(cdiv_i(p.C, TP_BLOCK_COLS), 1, p.B);
    if (dtype == 1) hipLaunchKernelGGL((recon_temporal_kernel<bf16_t>), grid, dim3(256), 0, s, p, q, o);
    else hipLaunchKernelGGL((recon_temporal_kernel<float>), grid, dim3(256), 0, s, p, q, o);
    return 0;
}

// ------------------------------------------------------------------------------------------
// Surrogate Gram matrices (sgv_gram): the temporal Gram matrix per sample, G[b][t][t'] = sum_n w[n] (x[b][t][n] - m[n]) (x[b][t'][n] - m[n])
// with x the value recon_phys_val gives -- the first tail that is quadratic in the field, the first with the field on BOTH sides of
// the MFMA (v_mfma_f32_32x32x2_f32 again: exact fp32 products, one fused multiply-add chain per output) and the first that stages its
// values through LDS: tanh makes every tail VALU-bound, so a value d = fl(x - m) is formed ONCE per block and read by every tile pair
// that needs it.
// Geometry: the T rows are cut into NT = ceil(T / 32) row tiles, the channels of the block into steps of GR_STEP = 16.  The fragment of
// tile ti in a step at channel cb is recon_project_kernel's: lane l holds d[32 ti + (l & 31)][cb + 8 (l >> 5) + e], e = 0..7.  Wave
// wv forms the fragments of tiles wv and wv + 4 and writes them to LDS in operand order, frag[buffer][tile][e][lane] -- a lane's own
// position, conflict-free on both sides.  The tile pairs ti <= tj (NT (NT + 1) / 2 of them, 28 at T = 200, 36 at the limit) are dealt
// to the four waves round robin, pair id = wv + 4 j for the wave's j-th accumulator; MFMA e of a step is
//   acc[ti][tj] += A(fl(w d_ti[e])) * B(d_tj[e])        k = 0: channel cb + e, k = 1: channel cb + 8 + e,
// so THE ROW INDEX t (the smaller tile) CARRIES THE WEIGHT: the element kept for t <= t' is the chain of fma(fl(w[n] d[t][n]),
// d[t'][n], .) and (t', t) is its copy.  In a diagonal tile both (t, t') and (t', t) are computed; the one with row <= column is
// kept.  w d is rounded once, by the consuming wave (w of the lane's 8 channels is the same for every tile); w == nullptr is w = 1
// and m == nullptr is m = 0, which give the same bits as arrays of ones and zeros since 1 * d and x - 0 are exact.
// The LDS is double-buffered, one barrier per step: in step s the waves form step s + 1 into the other buffer (from y and channel
// constants loaded a step earlier), then multiply step s.  Rows past T carry zeros and load row T - 1 again, the upper half of a
// last step past the chunk's end carries zeros and loads the lower half's addresses; an MFMA reads every lane's registers whatever
// EXEC says, and here every lane's operands come from LDS words that were written.  Tiles past NT are neither written nor read.
// Shares: a block is one sample and GR_CHUNK channels (C alone decides), all T rows.  An output's chain runs over the block's channels
// in the order above, from 0; the per-block partials go to the workspace as [B][chunks][pairs * 1024] in the C / D register order
// (v * 64 + lane) and recon_gram_finish_kernel adds them in ascending chunk order in fp64, rounds once and writes (t, t') and (t', t).
// No atomics; neither the batch nor the grid shows in the bits.
// ------------------------------------------------------------------------------------------
constexpr int GR_STEP = 16;                         // channels of a step: 8 MFMAs of k = 2 per tile pair
constexpr int GR_CHUNK = 6144;                      // channels per block, per partial (a multiple of GR_STEP)
constexpr int GR_MAX_TILES = SGV_MAX_GRAM_T / 32;   // 8
static int gr_chunks(int C) { return cdiv_i(C, GR_CHUNK); }
static int gr_tiles(int T) { return cdiv_i(T, 32); }
static int gr_pairs(int T) { return gr_tiles(T) * (gr_tiles(T) + 1) / 2; }
size_t ew_recon_gram_work_floats(int B, int T, int C) { return (size_t)B * gr_chunks(C) * gr_pairs(T) * 1024; }
// pair id -> (ti, tj), ti <= tj, row by row: (0,0) (0,1) .. (0,NT-1) (1,1) ..
__device__ __forceinline__ void gr_pair(int pid, int nt, int& ti, int& tj) {
    int i = 0, rem = pid;
    while (rem >= nt - i) { rem -= nt - i; ++i; }
    ti = i; tj = i + rem;
}

// d = fl(x - m): x rounded as ew_recon_physical would store it, then the difference, rounded on its own.  Without the pragma the
// subtraction is contracted into recon_phys_val's multiply by 1 / scale (one rounding instead of two) and d is no longer the difference of
// the stored value; __fsub_rn is a plain x - y in the compiler's headers and is contracted all the same.
__device__ __forceinline__ float gr_diff(float x, float m) {
#pragma clang fp contract(off)
    return x - m;
}
// NJ: accumulator tiles per wave, 7 up to 7 row tiles (T <= 224) and 9 at 8
template <typename T, int NJ>
__global__ __launch_bounds__(256) void recon_gram_kernel(const GNParams p, const ReconPhys q, const ReconGram o) {
    __shared__ float frag[2][GR_MAX_TILES][8][64];          // d in operand order, double-buffered: 32 KiB
    __shared__ float2 tab[SGV_GN_MAX_GROUPS];               // (mean, rstd) of the sample's groups
    const int b = blockIdx.z;
    if ((int)threadIdx.x < p.G) {
        float m, r;
        gn_mean_rstd(p, b, threadIdx.x, m, r);
        tab[threadIdx.x] = make_float2(m, r);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 31, h = lane >> 5;
    const int nt = (p.T + 31) >> 5, npairs = nt * (nt + 1) / 2;
    const int c_lo = blockIdx.x * GR_CHUNK, c_hi = min(p.C, c_lo + GR_CHUNK);
    const int nsteps = (c_hi - c_lo + GR_STEP - 1) / GR_STEP;
    // the rows this lane forms: tiles wv and wv + 4
    const T* yrow[2];
    bool row_ok[2], tile_ok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int t = 32 * (wv + 4 * u) + lr;
        tile_ok[u] = wv + 4 * u < nt;
        row_ok[u] = t < p.T;
        yrow[u] = reinterpret_cast<const T*>(p.y) + ((long)b * p.T + min(t, p.T - 1)) * p.ldy;
    }
    // the tile pairs this wave multiplies
    int pa[NJ], pb[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        int ti = 0, tj = 0;
        if (wv + 4 * j < npairs) gr_pair(wv + 4 * j, nt, ti, tj);
        pa[j] = ti * 512 + lane; pb[j] = tj * 512 + lane;
    }
    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;

    // what a step needs from memory: y of the lane's two rows, the constants, offset and weight of its 8 channels
    Raw8<T> ry[2];
    float gam[8], bet[8], mn[8], inv[8], off[8], wgt[8];
    auto fetch = [&](int s) {          // s < nsteps
        const int cb = c_lo + s * GR_STEP;
        const int c0 = cb + 8 * h < c_hi ? cb + 8 * h : cb;
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (tile_ok[u]) raw_load(yrow[u] + c0, ry[u]);
        load8(p.gamma + c0, gam); load8(p.beta + c0, bet); load8(q.mn + c0, mn); load8(q.scale + c0, inv);
        if (o.offset) load8(o.offset + c0, off);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) off[e] = 0.f;
        }
    };
    auto fetch_w = [&](int s) {
        const int cb = c_lo + s * GR_STEP;
        const int c0 = cb + 8 * h < c_hi ? cb + 8 * h : cb;
        if (o.node_weights) load8(o.node_weights + c0, wgt);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) wgt[e] = 1.f;
        }
    };
    // forms step s from what fetch(s) loaded and writes it to buffer s & 1
    auto produce = [&](int s) {
        const int cb = c_lo + s * GR_STEP;
        const bool ok = cb + 8 * h < c_hi;
        const int c0 = ok ? cb + 8 * h : cb;
        // the groups of the octet: with Cg >= 8 (block-uniform) at most two, the first n_lo channels in g_lo
        const int g0 = c0 / p.Cg, n_lo = p.Cg - (c0 - g0 * p.Cg);
        float gm[8], gr[8];
        if (p.Cg >= 8) {
            const float2 lo = tab[min(g0, p.G - 1)], hi = tab[min(g0 + 1, p.G - 1)];
#pragma unroll
            for (int e = 0; e < 8; ++e) { gm[e] = e < n_lo ? lo.x : hi.x; gr[e] = e < n_lo ? lo.y : hi.y; }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float2 k = tab[min((c0 + e) / p.Cg, p.G - 1)];
                gm[e] = k.x; gr[e] = k.y;
            }
        }
        float iv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) iv[e] = recon_phys_inv(inv[e]);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!tile_ok[u]) continue;          // wave-uniform
            float v[8];
            raw_unpack(ry[u], v);
            float* const dst = &frag[s & 1][wv + 4 * u][0][lane];
            const bool use = ok && row_ok[u];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float x = recon_phys_val(v[e], gm[e], gr[e], gam[e], bet[e], mn[e], iv[e]);
                dst[e * 64] = use ? gr_diff(x, off[e]) : 0.f;
            }
        }
    };

    fetch(0);
    produce(0);
    fetch(min(1, nsteps - 1));
    fetch_w(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        if (s + 1 < nsteps) {
            produce(s + 1);
            fetch(min(s + 2, nsteps - 1));
        }
        const float* const src = &frag[s & 1][0][0][0];
        float w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = wgt[e];
        fetch_w(min(s + 1, nsteps - 1));
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (wv + 4 * j >= npairs) break;          // wave-uniform
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = w[e] * src[pa[j] + e * 64], bb = src[pb[j] + e * 64];
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // the partials, in the C / D register order: element v * 64 + lane of the pair
    float* const part = o.work + ((long)b * gridDim.x + blockIdx.x) * npairs * 1024 + lane;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (wv + 4 * j >= npairs) break;
#pragma unroll
        for (int v = 0; v < 16; ++v) part[(long)(wv + 4 * j) * 1024 + v * 64] = acc[j][v];
    }
}

// partials [B][nchunk][npairs * 1024] -> out [B][T][T]: one thread per element of a pair's tile, its partials in ascending chunk order in
// fp64, rounded once.  C / D map of the 32x32 forms: register v of lane l holds row (v & 3) + 8 (v >> 2) + 4 (l >> 5), column l & 31.  An
// element with t <= t' < T is written to (t, t') and (t', t); the lower triangle of a diagonal tile and what lies past T is dropped.
__global__ __launch_bounds__(256) void recon_gram_finish_kernel(const float* __restrict__ part, int B, int T, int nchunk, float* __restrict__ out) {
    const int nt = (T + 31) >> 5, npairs = nt * (nt + 1) / 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * npairs * 1024) return;
    const int b = (int)(i / (npairs * 1024)), k = (int)(i - (long)b * npairs * 1024);
    const int pid = k >> 10, v = (k >> 6) & 15, l = k & 63;
    int ti, tj;
    gr_pair(pid, nt, ti, tj);
    const int t = 32 * ti + (v & 3) + 8 * (v >> 2) + 4 * (l >> 5), u = 32 * tj + (l & 31);
    if (t > u || u >= T) return;
    double s = 0.0;
    for (int j = 0; j < nchunk; ++j) s += (double)part[((long)b * nchunk + j) * npairs * 1024 + k];
    const float g = (float)s;
    out[((long)b * T + t) * T + u] = g;
    out[((long)b * T + u) * T + t] = g;
}

// p as for ew_recon_physical (layout [B][T][C] only); o: ReconGram (sgv_ew.h), o.work = ew_recon_gram_work_floats floats.  Non-zero
// (nothing launched): -1 null input, -2 no output, -3 bad shape or T beyond SGV_MAX_GRAM_T, -4 y, node_weights, offset or work not
// 16-byte aligned or out not 4-byte aligned, -6 no workspace
int ew_recon_gram(int dtype, GNParams p, const float* scale, const float* mn, const ReconGram& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    if (!o.out) return -2;
    if (p.T > SGV_MAX_GRAM_T) return -3;
    if (((uintptr_t)p.y | (uintptr_t)o.node_weights | (uintptr_t)o.offset | (uintptr_t)o.work) & 15) return -4;
    if ((uintptr_t)o.out & 3) return -4;
    if (!o.work) return -6;
    const ReconPhys q = recon_setup(p, scale, mn);
    const int nchunk = gr_chunks(p.C);
    const dim3 grid(nchunk, 1, p.B);
    auto launch = [&](auto el, auto) {
        using T = typename decltype(el)::type;
        if (gr_tiles(p.T) <= 7) hipLaunchKernelGGL((recon_gram_kernel<T, 7>), grid, dim3(256), 0, s, p, q, o);
        else hipLaunchKernelGGL((recon_gram_kernel<T, 9>), grid, dim3(256), 0, s, p, q, o);
    };
    recon_dispatch(launch, dtype, true);
    const long n = (long)p.B * gr_pairs(p.T) * 1024;
    hipLaunchKernelGGL(recon_gram_finish_kernel, dim3(cdiv_i(n, 256)), dim3(256), 0, s, o.work, p.B, p.T, nchunk, o.out);
    return 0;
}

// ------------------------------------------------------------------------------------------
// Surrogate exceedance durations (sgv_exceedance): the level-crossing statistics of every node's time history against L levels per
// node, e_t = (x_t > level) or (x_t < level), strict, x the value recon_phys_val gives: how many steps exceed, the first and the last of
// them, the number of maximal runs of consecutive exceeding steps, the longest run, and the fp32 sum of the excess fl(x_t - level)
// (fl(level - x_t) below) over the exceeding steps, t ascending from +0.0.  The first tail whose result depends on the ORDER of the
// time steps.
// Geometry: a thread owns its 8 channels of one sample for all T, t ascending -- the ownership of recon_temporal_kernel without the
// MFMA: thread i of a block has channels 8 i .. 8 i + 7 of the block's XC_BLOCK_COLS, so a wave reads XC_WAVE_COLS contiguous channels
// of a row per step, 16 bytes (bf16) or 32 bytes (fp32) per lane.  The channel constants, the sample's (mean, rstd) and the lane's
// L x 8 levels are loaded once; the y rows of xc_flight() steps are in flight in a register ring, the load of step t + xc_flight() issued as
// soon as step t is unpacked.  No reduction across threads, no LDS besides gn_consts' table, no workspace, no finish kernel, no
// atomics: an output depends on its sample, its level and its channel alone.
// State, 4 words per (channel, level), 128 registers at L = 4 (unpacked it would be 7 words): count | current run << 16;
// runs | longest << 16; first | (0xffff - last) << 16, both halves kept by one packed 16-bit minimum; the sum.  Every half stays below
// 2^16 while T < 65536 (t <= 65534, so 0xffff is free as "none"); the launcher refuses a longer T.  The levels are a run-time count
// 1 <= L <= SGV_MAX_EXCEED_LEVELS behind wave-uniform branches of the unrolled loop; the state of the levels past L is dead.
// ------------------------------------------------------------------------------------------
constexpr int XC_WAVE_COLS = 512;                   // channels of a wave: 64 lanes x 8
constexpr int XC_BLOCK_COLS = 4 * XC_WAVE_COLS;     // channels of a block
template <typename T> constexpr int xc_flight() { return sizeof(T) == 2 ? 4 : 2; }          // steps in flight: 4 KiB of y per wave and 16 registers per lane in either dtype
constexpr int XC_MAX_T = 65535;                     // the packed 16-bit halves of the state

typedef unsigned short xc_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned xc_pk_min(unsigned a, unsigned b) {          // v_pk_min_u16
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(xc_u16x2, a), __builtin_bit_cast(xc_u16x2, b)));
}

template <typename T, bool ABOVE, bool STEPS, bool EXCESS>
__global__ __launch_bounds__(256, 2) void recon_exceed_kernel(const GNParams p, const ReconPhys q, const ReconExceed o) {
    constexpr int F = xc_flight<T>(), LM = SGV_MAX_EXCEED_LEVELS;
    GNCtx c;
    c.b = blockIdx.z;
    c.c0 = blockIdx.x * XC_BLOCK_COLS + threadIdx.x * 8;
    c.col_ok = c.c0 < p.C;
    float mean[8], rstd[8];
    gn_consts(p, c, mean, rstd);          // all 256 threads
    if (!c.col_ok) return;                // no barrier, no shuffle below
    float gam[8], bet[8], mn[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float4 k = recon_channel(p, q, c.c0 + e, true); gam[e] = k.x; bet[e] = k.y; mn[e] = k.z; inv[e] = k.w; }
    const int L = o.n_level;
    float lev[LM][8], sum[LM][8];
    unsigned cc[LM][8], rl[LM][8], fl[LM][8];          // count | current << 16; runs | longest << 16; first | (0xffff - last) << 16
#pragma unroll
    for (int l = 0; l < LM; ++l)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            lev[l][e] = l < L ? o.levels[(long)l * p.C + c.c0 + e] : 0.f;
            sum[l][e] = 0.f; cc[l][e] = 0u; rl[l][e] = 0u; fl[l][e] = 0xffffffffu;
        }
    const T* const y = reinterpret_cast<const T*>(p.y) + (long)c.b * p.T * p.ldy + c.c0;
    // a row past T - 1 is row T - 1 again, loaded and not used
    Raw8<T> ry[F];
#pragma unroll
    for (int u = 0; u < F; ++u) raw_load(y + (long)min(u, p.T - 1) * p.ldy, ry[u]);
    for (int t0 = 0; t0 < p.T; t0 += F) {
#pragma unroll
        for (int u = 0; u < F; ++u) {
            const int t = t0 + u;
            if (t >= p.T) break;          // uniform
            float x[8];
            raw_unpack(ry[u], x);
            raw_load(y + (long)min(t + F, p.T - 1) * p.ldy, ry[u]);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = recon_phys_val(x[e], mean[e], rstd[e], gam[e], bet[e], mn[e], inv[e]);
            const unsigned here = (unsigned)t | (0xffffu - (unsigned)t) << 16;
#pragma unroll
            for (int l = 0; l < LM; ++l) {
                if (l >= L) break;          // uniform
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bool ex = ABOVE ? x[e] > lev[l][e] : x[e] < lev[l][e];
                    if constexpr (STEPS) {
                        const unsigned start = ex && cc[l][e] < 0x10000u ? 1u : 0u;
                        cc[l][e] = ex ? cc[l][e] + 0x10001u : cc[l][e] & 0xffffu;
                        const unsigned r = rl[l][e] + start;
                        rl[l][e] = max(r, (cc[l][e] & 0xffff0000u) | (r & 0xffffu));
                        fl[l][e] = xc_pk_min(fl[l][e], ex ? here : 0xffffffffu);
                    }
                    if constexpr (EXCESS) {
                        // the difference of the stored value, rounded on its own (gr_diff), then one add
                        const float d = ABOVE ? gr_diff(x[e], lev[l][e]) : gr_diff(lev[l][e], x[e]);
                        sum[l][e] = ex ? sum[l][e] + d : sum[l][e];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int l = 0; l < LM; ++l) {
        if (l >= L) break;
        if constexpr (STEPS) {
            int* const st = o.stats + ((long)c.b * 5 * L + l) * p.C + c.c0;          // [B][5][L][C]: count, first, last, longest, runs
            const long plane = (long)L * p.C;
            int v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (int)(cc[l][e] & 0xffffu);
            store8(st, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = cc[l][e] & 0xffffu ? (int)(fl[l][e] & 0xffffu) : -1;
            store8(st + plane, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = cc[l][e] & 0xffffu ? (int)(0xffffu - (fl[l][e] >> 16)) : -1;
            store8(st + 2 * plane, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (int)(rl[l][e] >> 16);
            store8(st + 3 * plane, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (int)(rl[l][e] & 0xffffu);
            store8(st + 4 * plane, v);
        }
        if constexpr (EXCESS) store8(o.excess + ((long)c.b * L + l) * p.C + c.c0, sum[l]);
    }
}

// p as for ew_recon_physical (layout [B][T][C] only); o: ReconExceed (sgv_ew.h).  Non-zero (nothing launched): -1 null input (levels
// included), -2 no output, -3 bad shape, n_level outside [1, SGV_MAX_EXCEED_LEVELS] or T > 65535 (the packed state), -4 y, stats or excess
// not 16-byte aligned or levels not 4-byte aligned
int ew_recon_exceedance(int dtype, GNParams p, const float* scale, const float* mn, const ReconExceed& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    if (!o.levels) return -1;
    if (!o.stats && !o.excess) return -2;
    if (o.n_level < 1 || o.n_level > SGV_MAX_EXCEED_LEVELS || p.T > XC_MAX_T) return -3;
    if (((uintptr_t)p.y | (uintptr_t)o.stats | (uintptr_t)o.excess) & 15) return -4;
    if ((uintptr_t)o.levels & 3) return -4;
    const ReconPhys q = recon_setup(p, scale, mn);
    const dim3 grid(cdiv_i(p.C, XC_BLOCK_COLS), 1, p.B);
    auto launch = [&](auto el, auto ab, auto st, auto ex) {
        if constexpr (decltype(st)::value || decltype(ex)::value)
            hipLaunchKernelGGL((recon_exceed_kernel<typename decltype(el)::type, decltype(ab)::value, decltype(st)::value, decltype(ex)::value>), grid, dim3(256), 0, s,
                               p, q, o);
    };
    // recon_dispatch leaves out the combination with every flag false only; the launcher above never instantiates the kernel without an output
    if (o.above) recon_dispatch<true>(launch, dtype, o.stats != nullptr, o.excess != nullptr);
    else recon_dispatch<false>(launch, dtype, o.stats != nullptr, o.excess != nullptr);
    return 0;
}

// ------------------------------------------------------------------------------------------
// Surrogate load cycles and rates (sgv_cycles): per channel, the turning points of its time history behind a hysteresis gate -- ASTM
// E1049 simple-range counting, the ranges between successive confirmed reversals, their number, sum, maximum and damage sum
// sum R^m, the unfinished excursion at the end -- and the statistics of the first differences: the largest rise and fall, their
// steps, the path length.  The contract, to the rounding, is in sgv_ew.h (ReconCycles); x is the value recon_phys_val gives.
// Geometry: recon_exceed_kernel's.  A thread owns its 8 channels of one sample for all T, t ascending, the rows of xc_flight() steps in
// flight in a register ring, a row past T - 1 being row T - 1 again; no reduction across threads, no LDS besides gn_consts' table, no
// workspace, no finish kernel, no atomics.  Step 0 only sets the state (hi = lo = the previous x = x[0]); it is loaded beside the ring,
// which starts at step 1, so the loop over t has one body: with the step-0 case inside it the fp32 kernel took 256 registers and
// 36 bytes of scratch.
// State, 11 words per channel: a = hi (dir 0) or cand; b = lo (dir 0) or last; st = reversals | (dir != 0) << 16 | (dir == -1) << 31;
// range_sum, range_max, damage; the previous x; rise, fall, rise_when | fall_when << 16 (0xffff: none yet), path.  Every half stays
// below 2^16 while T < 65536; the launcher refuses a longer T.  The two directions share one code path through the sign bit:
// fl(a - b) = fl((-b) - (-a)) exactly.  Differences go through gr_diff, the power and the sums through cy_count, so that nothing is
// contracted with recon_phys_val's multiply by 1 / scale or with each other.  The power is a run-time loop, the same for every lane;
// a channel that confirms nothing at a step counts R = +0.0, which leaves its three sums as they are (s + 0 = s, 0 > max never), so
// the step has no divergent branch.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void cy_count(const float R[8], int m, float rsum[8], float rmax[8], float dmg[8]) {
#pragma clang fp contract(off)
    float P[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) P[e] = R[e];
    for (int k = 1; k < m; ++k)           // uniform
#pragma unroll
        for (int e = 0; e < 8; ++e) P[e] = P[e] * R[e];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        rsum[e] = rsum[e] + R[e];
        rmax[e] = R[e] > rmax[e] ? R[e] : rmax[e];
        dmg[e] = dmg[e] + P[e];
    }
}
__device__ __forceinline__ float cy_flip(float v, unsigned sign) { return __uint_as_float(__float_as_uint(v) ^ sign); }

template <typename T, bool TURNS, bool RATES>
__global__ __launch_bounds__(256, 2) void recon_cycles_kernel(const GNParams p, const ReconPhys q, const ReconCycles o) {
    constexpr int F = xc_flight<T>();
    GNCtx c;
    c.b = blockIdx.z;
    c.c0 = blockIdx.x * XC_BLOCK_COLS + threadIdx.x * 8;
    c.col_ok = c.c0 < p.C;
    float mean[8], rstd[8];
    gn_consts(p, c, mean, rstd);          // all 256 threads
    if (!c.col_ok) return;                // no barrier, no shuffle below
    float gam[8], bet[8], mn[8], inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float4 k = recon_channel(p, q, c.c0 + e, true); gam[e] = k.x; bet[e] = k.y; mn[e] = k.z; inv[e] = k.w; }
    const int m = o.exponent;
    float gate[8], a[8], b[8], rsum[8], rmax[8], dmg[8];          // the turns
    unsigned st[8];
    float prev[8], rise[8], fall[8], path[8];                      // the rates
    unsigned wh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        gate[e] = TURNS ? o.gate[c.c0 + e] : 0.f;
        a[e] = b[e] = rsum[e] = rmax[e] = dmg[e] = 0.f; st[e] = 0u;
        prev[e] = rise[e] = fall[e] = path[e] = 0.f; wh[e] = 0xffffffffu;
    }
    const T* const y = reinterpret_cast<const T*>(p.y) + (long)c.b * p.T * p.ldy + c.c0;
    // the ring holds steps 1 .. F, slot u of a round the step t0 + u; a row past T - 1 is row T - 1 again, loaded and not used
    Raw8<T> ry[F], r0;
#pragma unroll
    for (int u = 0; u < F; ++u) raw_load(y + (long)min(1 + u, p.T - 1) * p.ldy, ry[u]);
    raw_load(y, r0);
    {          // step 0: hi = lo = x[0], no difference yet
        float x[8];
        raw_unpack(r0, x);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = b[e] = prev[e] = recon_phys_val(x[e], mean[e], rstd[e], gam[e], bet[e], mn[e], inv[e]);
    }
    for (int t0 = 1; t0 < p.T; t0 += F) {
#pragma unroll
        for (int u = 0; u < F; ++u) {
            const int t = t0 + u;
            if (t >= p.T) break;          // uniform
            float x[8];
            raw_unpack(ry[u], x);
            raw_load(y + (long)min(t + F, p.T - 1) * p.ldy, ry[u]);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = recon_phys_val(x[e], mean[e], rstd[e], gam[e], bet[e], mn[e], inv[e]);
            if constexpr (RATES) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xx = x[e];
                    const float r = gr_diff(xx, prev[e]);
                    const bool first = t == 1, up = first || r > rise[e], dn = first || r < fall[e];
                    rise[e] = up ? r : rise[e];
                    fall[e] = dn ? r : fall[e];
                    wh[e] = up ? (wh[e] & 0xffff0000u) | (unsigned)t : wh[e];
                    wh[e] = dn ? (wh[e] & 0xffffu) | (unsigned)t << 16 : wh[e];
                    path[e] = path[e] + fabsf(r);
                    prev[e] = xx;
                }
            }
            if constexpr (TURNS) {
                float R[8];               // the range confirmed at this step, +0.0 where none is
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xx = x[e];
                    const unsigned sg = st[e] & 0x80000000u;          // dir = -1: the rising direction of the negated history
                    const bool idle = !(st[e] & 0x10000u);            // dir = 0
                    const float A = a[e], Bv = b[e], h = gate[e];
                    const float xs = cy_flip(xx, sg), As = cy_flip(A, sg);
                    // one difference serves dir = 0 (hi - x, the peak), +1 (cand - x) and -1 (x - cand); dir = 0 tries the valley first
                    const bool ext = xs > As, up0 = idle && gr_diff(xx, Bv) > h;
                    const bool rev = gr_diff(As, xs) > h && !(idle ? up0 : ext);
                    R[e] = rev && !idle ? gr_diff(As, cy_flip(Bv, sg)) : 0.f;
                    b[e] = rev ? A : idle && !up0 && xx < Bv ? xx : Bv;
                    a[e] = up0 || rev || ext ? xx : A;
                    st[e] = ((st[e] + (up0 || rev ? 0x1u : 0u)) | (up0 || rev ? 0x10000u : 0u)) ^ (rev ? 0x80000000u : 0u);
                }
                cy_count(R, m, rsum, rmax, dmg);
            }
        }
    }
    if constexpr (TURNS) {
        int v[8];
        float w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (int)(st[e] & 0xffffu);
        store8(o.reversals + (long)c.b * p.C + c.c0, v);
        float* const rg = o.ranges + (long)c.b * 4 * p.C + c.c0;          // [B][4][C]: range_sum, range_max, damage, open
        store8(rg, rsum);
        store8(rg + p.C, rmax);
        store8(rg + 2L * p.C, dmg);
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = st[e] & 0x80000000u ? gr_diff(b[e], a[e]) : gr_diff(a[e], b[e]);
        store8(rg + 3L * p.C, w);
    }
    if constexpr (RATES) {
        int* const rw = o.rate_when + (long)c.b * 2 * p.C + c.c0;          // [B][2][C]: rise_when, fall_when
        int v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (wh[e] & 0xffffu) == 0xffffu ? -1 : (int)(wh[e] & 0xffffu);
        store8(rw, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = wh[e] >> 16 == 0xffffu ? -1 : (int)(wh[e] >> 16);
        store8(rw + p.C, v);
        float* const rt = o.rates + (long)c.b * 3 * p.C + c.c0;            // [B][3][C]: rise, fall, path
        store8(rt, rise);
        store8(rt + p.C, fall);
        store8(rt + 2L * p.C, path);
    }
}

// p as for ew_recon_physical (layout [B][T][C] only); o: ReconCycles (sgv_ew.h).  Non-zero (nothing launched): -1 null input (gate
// included), -2 no group or half a group, -3 bad shape, exponent outside [1, SGV_MAX_CYCLES_EXPONENT] or T > 65535 (the packed state),
// -4 y or an output not 16-byte aligned or gate not 4-byte aligned
int ew_recon_cycles(int dtype, GNParams p, const float* scale, const float* mn, const ReconCycles& o, hipStream_t s) {
    if (const int r = recon_args_ok(p, scale, mn)) return r;
    if (!o.gate) return -1;
    const bool turns = o.reversals || o.ranges, rates = o.rate_when || o.rates;
    if (!turns && !rates) return -2;
    if ((turns && !(o.reversals && o.ranges)) || (rates && !(o.rate_when && o.rates))) return -2;
    if (o.exponent < 1 || o.exponent > SGV_MAX_CYCLES_EXPONENT || p.T > XC_MAX_T) return -3;
    if (((uintptr_t)p.y | (uintptr_t)o.reversals | (uintptr_t)o.ranges | (uintptr_t)o.rate_when | (uintptr_t)o.rates) & 15) return -4;
    if ((uintptr_t)o.gate & 3) return -4;
    const ReconPhys q = recon_setup(p, scale, mn);
    const dim3 grid(cdiv_i(p.C, XC_BLOCK_COLS), 1, p.B);
    auto launch = [&](auto el, auto tu, auto ra) {
        hipLaunchKernelGGL((recon_cycles_kernel<typename decltype(el)::type, decltype(tu)::value, decltype(ra)::value>), grid, dim3(256), 0, s, p, q, o);
    };
    recon_dispatch(launch, dtype, turns, rates);
    return 0;
}
