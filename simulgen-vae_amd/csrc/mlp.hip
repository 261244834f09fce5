// Fused fp32 dense layers of the parametric (CSV) latent conditioner (reference modules/latent_conditioner_model_parametric.py:25-213):
// Linear -> LayerNorm -> GELU -> Dropout stacks, ResidualBlocks and two Tanh heads over row-major [B][features] activations.
//
// At the configured sizes (batch 64, widths 32..1024) a step is bound by launches and the dependent boundaries between
// them, not by FLOPs, so each dense layer is two launches forward and two backward:
//   mlp_gemm_fwd   Z = X.W^T + b (+ tanh) for up to two independent problems (linear2 + the skip Linear of a residual block,
//                  the first Linear of both heads) on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation);
//   mlp_rows_fwd   per row: LayerNorm(Za) [+ LayerNorm(Zb) | + R] -> GELU -> [LayerNorm] -> dropout mask * scale, the row
//                  statistics saved for the backward (which recomputes every other intermediate from Z);
//   mlp_rows_bwd   the same chain backwards: dZa, dZb (or dR), and per-row partials of every dgamma / dbeta;
//   mlp_gemm_bwd   dX = sum_p dZ_p.W_p (+ addend), dW = dZ^T.X, db, and the batch reduction of the LayerNorm partials.
// Every reduction runs in a fixed order (no floating-point atomics, no grid-wide barriers): results replay bitwise.
// Edge tiles are masked, so any B, K, O is accepted.
#include "../../include/sgvae_ops.h"
#include "sgv_common.h"

#include <math.h>

#define MLP_THREADS 256
#define MLP_MAX_PROBS 2
#define MLP_MAX_SUMS 12

__host__ __device__ static inline int cdiv_i(long a, long b) { return (int)((a + b - 1) / b); }

// ---- block-wide helpers ----------------------------------------------------------------------------------------------
// Sum over the block of NV values per thread, in a fixed order: xor butterfly inside each wave (lane 0's result is
// broadcast, so every lane sees the same bits), then the four wave totals in index order.
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float t = v[i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
        v[i] = __shfl(t, 0, 64);
    }
    __syncthreads();                              // earlier readers of sh are done
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) sh[w * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = ((sh[i] + sh[NV + i]) + sh[2 * NV + i]) + sh[3 * NV + i];
}

// One 16x16 output tile D[i][j] = sum_k A(i, k) * B(k, j) by the four waves of the block: wave w takes the k-steps
// 4w, 4w + 16, ... into two alternating accumulators (the 16x16x4 MFMA has a 40-cycle dependent latency), and the wave
// partials are added in wave order through LDS.  Lane l of wave 0 returns rows 4(l>>4) .. 4(l>>4)+3, column l & 15.
template <class LA, class LB>
__device__ __forceinline__ void tile_accumulate(LA la, LB lb, int nk, f32x4& acc0, f32x4& acc1) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = lane & 15, kq = lane >> 4;
    int step = 0;
    for (int k0 = 4 * w; k0 < nk; k0 += 16, ++step) {
        const int k = k0 + kq;
        const float a = la(i, k), b = lb(k, i);
        if (step & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc1, 0, 0, 0);
        else          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc0, 0, 0, 0);
    }
}
__device__ __forceinline__ f32x4 tile_reduce(f32x4 acc0, f32x4 acc1, float* sh /* 4*64*4 floats */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const f32x4 s = acc0 + acc1;
#pragma unroll
    for (int r = 0; r < 4; ++r) sh[(w * 64 + lane) * 4 + r] = s[r];
    __syncthreads();
    f32x4 out;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        out[r] = ((sh[(0 * 64 + lane) * 4 + r] + sh[(1 * 64 + lane) * 4 + r]) + sh[(2 * 64 + lane) * 4 + r]) + sh[(3 * 64 + lane) * 4 + r];
    return out;
}

// exact erf form (nn.GELU default); libm erff, not the polynomial of sgv_common.h
__device__ __forceinline__ float mlp_gelu(float s) { return 0.5f * s * (1.f + erff(s * 0.70710678118654752f)); }
__device__ __forceinline__ float mlp_gelu_grad(float s) {
    return 0.5f * (1.f + erff(s * 0.70710678118654752f)) + s * 0.39894228040143268f * expf(-0.5f * s * s);
}

// ---- forward GEMM --------------------------------------------------------------------------------------------------------
struct GemmFwdArgs {
    sgv_mlp_gemm p[MLP_MAX_PROBS];
    int tiles0, B, tanh_out;
};

__global__ __launch_bounds__(MLP_THREADS) void mlp_gemm_fwd_kernel(GemmFwdArgs a) {
    __shared__ float sh[4 * 64 * 4];
    int t = blockIdx.x;
    const int pi = t < a.tiles0 ? 0 : 1;
    if (pi) t -= a.tiles0;
    const sgv_mlp_gemm p = a.p[pi];
    const int B = a.B, K = p.K, O = p.O;
    const int mt = cdiv_i(B, 16);
    const int r0 = (t % mt) * 16, c0 = (t / mt) * 16;
    const float* x = p.x;
    const float* W = p.W;
    auto la = [&](int i, int k) { const int r = r0 + i; return (r < B && k < K) ? x[(long)r * K + k] : 0.f; };
    auto lb = [&](int k, int j) { const int c = c0 + j; return (c < O && k < K) ? W[(long)c * K + k] : 0.f; };
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    tile_accumulate(la, lb, K, acc0, acc1);
    const f32x4 d = tile_reduce(acc0, acc1, sh);
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x, c = c0 + (lane & 15);
    if (c >= O) return;
    const float bias = p.bias ? p.bias[c] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + (lane >> 4) * 4 + r;
        if (row < B) {
            float v = d[r] + bias;
            if (a.tanh_out) v = tanhf(v);
            p.z[(long)row * O + c] = v;
        }
    }
}

// ---- row epilogue forward / backward -------------------------------------------------------------------------------------
struct RowArgs {
    sgv_mlp_rows p[MLP_MAX_PROBS];
};

// value of the row chain up to (and including) the activation, before the optional LayerNorm c
struct RowCtx {
    const float *za, *zb, *r;
    float ma, ra, mb, rb;
    __device__ __forceinline__ float pre(const sgv_mlp_rows& p, int j) const {
        float v = (za[j] - ma) * ra * p.ga[j] + p.ba[j];
        if (zb) v += (zb[j] - mb) * rb * p.gb[j] + p.bb[j];
        else if (r) v += r[j];
        return v;
    }
};

__global__ __launch_bounds__(MLP_THREADS) void mlp_rows_fwd_kernel(RowArgs a, int B) {
    __shared__ float sh[4 * 2];
    const sgv_mlp_rows& p = a.p[blockIdx.y];
    const int row = blockIdx.x, O = p.O;
    const long off = (long)row * O;
    RowCtx c;
    c.za = p.za + off; c.zb = p.zb ? p.zb + off : nullptr; c.r = p.r ? p.r + off : nullptr;
    float s[2] = {0.f, 0.f};
    for (int j = threadIdx.x; j < O; j += MLP_THREADS) { s[0] += c.za[j]; if (c.zb) s[1] += c.zb[j]; }
    block_sum<2>(s, sh);
    c.ma = s[0] / O; c.mb = s[1] / O;
    float q[2] = {0.f, 0.f};
    for (int j = threadIdx.x; j < O; j += MLP_THREADS) {
        const float d = c.za[j] - c.ma;
        q[0] += d * d;
        if (c.zb) { const float e = c.zb[j] - c.mb; q[1] += e * e; }
    }
    block_sum<2>(q, sh);
    c.ra = 1.f / sqrtf(q[0] / O + 1e-5f); c.rb = 1.f / sqrtf(q[1] / O + 1e-5f);
    float mc = 0.f, rc = 0.f;
    if (p.gc) {
        float u[1] = {0.f};
        for (int j = threadIdx.x; j < O; j += MLP_THREADS) { const float v = c.pre(p, j); u[0] += p.gelu ? mlp_gelu(v) : v; }
        block_sum<1>(u, sh);
        mc = u[0] / O;
        float uq[1] = {0.f};
        for (int j = threadIdx.x; j < O; j += MLP_THREADS) {
            const float v = c.pre(p, j), d = (p.gelu ? mlp_gelu(v) : v) - mc;
            uq[0] += d * d;
        }
        block_sum<1>(uq, sh);
        rc = 1.f / sqrtf(uq[0] / O + 1e-5f);
    }
    for (int j = threadIdx.x; j < O; j += MLP_THREADS) {
        float v = c.pre(p, j);
        if (p.gelu) v = mlp_gelu(v);
        if (p.gc) v = (v - mc) * rc * p.gc[j] + p.bc[j];
        if (p.mask) v = p.mask[off + j] >= p.mask_thr ? v * p.mask_scale : 0.f;
        p.out[off + j] = v;
    }
    if (threadIdx.x == 0 && p.stats) {
        float* st = p.stats + (long)row * 6;
        st[0] = c.ma; st[1] = c.ra; st[2] = c.mb; st[3] = c.rb; st[4] = mc; st[5] = rc;
    }
}

// part: five [B][O] planes: 0 ds*xhat_a (dgamma_a), 1 ds (dbeta_a = dbeta_b), 2 ds*xhat_b (dgamma_b), 3 dw*uhat (dgamma_c),
// 4 dw (dbeta_c); ds = gradient at the pre-activation sum, dw = gradient at the output of LayerNorm c
__global__ __launch_bounds__(MLP_THREADS) void mlp_rows_bwd_kernel(RowArgs a, int B) {
    __shared__ float sh[4 * 4];
    const sgv_mlp_rows& p = a.p[blockIdx.y];
    const int row = blockIdx.x, O = p.O;
    const long off = (long)row * O, plane = (long)B * O;
    const float* st = p.stats + (long)row * 6;
    RowCtx c;
    c.za = p.za + off; c.zb = p.zb ? p.zb + off : nullptr; c.r = p.r ? p.r + off : nullptr;
    c.ma = st[0]; c.ra = st[1]; c.mb = st[2]; c.rb = st[3];
    const float mc = st[4], rc = st[5];
    const float* dout = p.dout + off;
    float* pga = p.part + off;
    float* pb = p.part + plane + off;
    float* pgb = p.part + 2 * plane + off;
    float* pgc = p.part + 3 * plane + off;
    float* pbc = p.part + 4 * plane + off;
    auto dw = [&](int j) { const float d = dout[j]; return p.mask ? (p.mask[off + j] >= p.mask_thr ? d * p.mask_scale : 0.f) : d; };
    float m1 = 0.f, m2 = 0.f;
    if (p.gc) {
        float t[2] = {0.f, 0.f};
        for (int j = threadIdx.x; j < O; j += MLP_THREADS) {
            const float v = c.pre(p, j), uh = ((p.gelu ? mlp_gelu(v) : v) - mc) * rc, g = p.gc[j] * dw(j);
            t[0] += g; t[1] += g * uh;
        }
        block_sum<2>(t, sh);
        m1 = t[0] / O; m2 = t[1] / O;
    }
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = threadIdx.x; j < O; j += MLP_THREADS) {
        const float v = c.pre(p, j);
        float du;
        if (p.gc) {
            const float uh = ((p.gelu ? mlp_gelu(v) : v) - mc) * rc, d = dw(j);
            du = rc * (p.gc[j] * d - m1 - uh * m2);
            pgc[j] = d * uh; pbc[j] = d;
        } else {
            du = dw(j);
        }
        const float ds = p.gelu ? du * mlp_gelu_grad(v) : du;
        const float xa = (c.za[j] - c.ma) * c.ra;
        pga[j] = ds * xa; pb[j] = ds;
        t[0] += p.ga[j] * ds; t[1] += p.ga[j] * ds * xa;
        if (c.zb) {
            const float xb = (c.zb[j] - c.mb) * c.rb;
            pgb[j] = ds * xb;
            t[2] += p.gb[j] * ds; t[3] += p.gb[j] * ds * xb;
        }
        if (p.dr) p.dr[off + j] = ds;
    }
    block_sum<4>(t, sh);
    const float a1 = t[0] / O, a2 = t[1] / O, b1 = t[2] / O, b2 = t[3] / O;
    for (int j = threadIdx.x; j < O; j += MLP_THREADS) {
        const float ds = pb[j];                        // written by this thread above
        if (p.dza) { const float xa = (c.za[j] - c.ma) * c.ra; p.dza[off + j] = c.ra * (p.ga[j] * ds - a1 - xa * a2); }
        if (p.dzb) { const float xb = (c.zb[j] - c.mb) * c.rb; p.dzb[off + j] = c.rb * (p.gb[j] * ds - b1 - xb * b2); }
    }
}

// ---- backward GEMM ------------------------------------------------------------------------------------------------------
struct GemmBwdArgs {
    sgv_mlp_gemm_bwd p[MLP_MAX_PROBS];
    sgv_mlp_colsum cs[MLP_MAX_SUMS];
    const float* dx_addend;
    int np, ncs, B, dx_sum;
    // segment ends (exclusive, in blocks): dX tiles of problem 0 / 1, dW tiles of problem 0 / 1, db of problem 0 / 1, column sums
    int seg[7];
    int cs_start[MLP_MAX_SUMS + 1];
};

__device__ __forceinline__ float dz_eff(const sgv_mlp_gemm_bwd& p, long idx) {
    const float d = p.dz[idx];
    if (!p.y_tanh) return d;
    const float y = p.y_tanh[idx];
    return d * (1.f - y * y);
}

__global__ __launch_bounds__(MLP_THREADS) void mlp_gemm_bwd_kernel(GemmBwdArgs a) {
    __shared__ float sh[4 * 64 * 4];
    const int B = a.B, mt = cdiv_i(B, 16);
    int t = blockIdx.x;
    const int lane = threadIdx.x & 63;
    if (t < a.seg[1]) {                                          // dX tiles
        const int pi = t < a.seg[0] ? 0 : 1;
        if (pi) t -= a.seg[0];
        const int K = a.p[pi].K;
        const int r0 = (t % mt) * 16, c0 = (t / mt) * 16;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int q = 0; q < a.np; ++q) {
            if (!(a.dx_sum ? a.p[q].W != nullptr && a.p[q].dz != nullptr : q == pi)) continue;
            const sgv_mlp_gemm_bwd& p = a.p[q];
            const int O = p.O;
            auto la = [&](int i, int k) { const int r = r0 + i; return (r < B && k < O) ? dz_eff(p, (long)r * O + k) : 0.f; };
            auto lb = [&](int k, int j) { const int col = c0 + j; return (col < K && k < O) ? p.W[(long)k * K + col] : 0.f; };
            tile_accumulate(la, lb, O, acc0, acc1);
        }
        const f32x4 d = tile_reduce(acc0, acc1, sh);
        if (threadIdx.x >= 64) return;
        const int col = c0 + (lane & 15);
        if (col >= K) return;
        float* dx = a.p[pi].dx;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + (lane >> 4) * 4 + r;
            if (row < B) {
                float v = d[r];
                if (a.dx_addend) v += a.dx_addend[(long)row * K + col];
                dx[(long)row * K + col] = v;
            }
        }
        return;
    }
    if (t < a.seg[3]) {                                          // dW tiles: dW[o][k] = sum_b dZ[b][o] X[b][k]
        t -= a.seg[1];
        const int pi = t < a.seg[2] - a.seg[1] ? 0 : 1;
        if (pi) t -= a.seg[2] - a.seg[1];
        const sgv_mlp_gemm_bwd& p = a.p[pi];
        const int K = p.K, O = p.O, ot = cdiv_i(O, 16);
        const int o0 = (t % ot) * 16, k0 = (t / ot) * 16;
        auto la = [&](int i, int b) { const int o = o0 + i; return (o < O && b < B) ? dz_eff(p, (long)b * O + o) : 0.f; };
        auto lb = [&](int b, int j) { const int k = k0 + j; return (k < K && b < B) ? p.x[(long)b * K + k] : 0.f; };
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        tile_accumulate(la, lb, B, acc0, acc1);
        const f32x4 d = tile_reduce(acc0, acc1, sh);
        if (threadIdx.x >= 64) return;
        const int k = k0 + (lane & 15);
        if (k >= K) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + (lane >> 4) * 4 + r;
            if (o < O) p.dW[(long)o * K + k] = d[r];
        }
        return;
    }
    if (t < a.seg[5]) {                                          // bias gradients: db[o] = sum_b dZ[b][o], rows in order
        t -= a.seg[3];
        const int pi = t < a.seg[4] - a.seg[3] ? 0 : 1;
        if (pi) t -= a.seg[4] - a.seg[3];
        const sgv_mlp_gemm_bwd& p = a.p[pi];
        const int o = t * MLP_THREADS + threadIdx.x;
        if (o >= p.O) return;
        float s = 0.f;
#pragma unroll 8
        for (int b = 0; b < B; ++b) s += dz_eff(p, (long)b * p.O + o);      // unrolled: loads issued ahead, adds in row order
        p.db[o] = s;
        return;
    }
    t -= a.seg[5];                                               // LayerNorm parameter gradients from the row partials
    int ci = 0;
    while (ci + 1 < a.ncs && t >= a.cs_start[ci + 1]) ++ci;
    const sgv_mlp_colsum& cs = a.cs[ci];
    const int col = (t - a.cs_start[ci]) * MLP_THREADS + threadIdx.x;
    if (col >= cs.n) return;
    float s = 0.f;
#pragma unroll 8
    for (int b = 0; b < B; ++b) s += cs.src[(long)b * cs.n + col];
    cs.out[col] = s;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------
#define MLPCHK(cond, ...) do { if (!(cond)) return sgv_set_error(-1, __VA_ARGS__); } while (0)
#define MLPLAUNCH_OK() (hipGetLastError() == hipSuccess ? 0 : sgv_set_error(-2, "kernel launch failed in %s", __func__))

extern "C" {

int sgv_op_mlp_gemm_fwd(const sgv_mlp_gemm* probs, int n_probs, int B, int tanh_out, void* stream) {
    MLPCHK(probs && n_probs >= 1 && n_probs <= MLP_MAX_PROBS && B > 0, "sgv_op_mlp_gemm_fwd: bad argument (n_probs %d, B %d)", n_probs, B);
    GemmFwdArgs a = {};
    int total = 0;
    for (int i = 0; i < n_probs; ++i) {
        const sgv_mlp_gemm& p = probs[i];
        MLPCHK(p.x && p.W && p.z && p.K > 0 && p.O > 0, "sgv_op_mlp_gemm_fwd: problem %d needs x, W, z and K, O > 0", i);
        a.p[i] = p;
        total += cdiv_i(B, 16) * cdiv_i(p.O, 16);
        if (i == 0) a.tiles0 = total;
    }
    a.B = B; a.tanh_out = tanh_out ? 1 : 0;
    hipLaunchKernelGGL(mlp_gemm_fwd_kernel, dim3(total), dim3(MLP_THREADS), 0, (hipStream_t)stream, a);
    return MLPLAUNCH_OK();
}

static int rows_check(const sgv_mlp_rows* probs, int n_probs, int B, bool bwd) {
    MLPCHK(probs && n_probs >= 1 && n_probs <= MLP_MAX_PROBS && B > 0, "sgv_op_mlp_rows: bad argument (n_probs %d, B %d)", n_probs, B);
    for (int i = 0; i < n_probs; ++i) {
        const sgv_mlp_rows& p = probs[i];
        MLPCHK(p.za && p.ga && p.ba && p.O > 0, "sgv_op_mlp_rows: problem %d needs za, ga, ba and O > 0", i);
        MLPCHK(!p.zb || (p.gb && p.bb), "sgv_op_mlp_rows: problem %d: zb needs gb, bb", i);
        MLPCHK(!(p.zb && p.r), "sgv_op_mlp_rows: problem %d: zb and r are exclusive", i);
        MLPCHK(!p.gc == !p.bc, "sgv_op_mlp_rows: problem %d: gc and bc go together", i);
        if (bwd) {
            MLPCHK(p.dout && p.stats && p.part, "sgv_op_mlp_rows_bwd: problem %d needs dout, stats and part", i);
            MLPCHK(!p.dzb || p.zb, "sgv_op_mlp_rows_bwd: problem %d: dzb without zb", i);
        } else {
            MLPCHK(p.out, "sgv_op_mlp_rows_fwd: problem %d needs out", i);
        }
    }
    return 0;
}

int sgv_op_mlp_rows_fwd(const sgv_mlp_rows* probs, int n_probs, int B, void* stream) {
    if (int rc = rows_check(probs, n_probs, B, false)) return rc;
    RowArgs a = {};
    for (int i = 0; i < n_probs; ++i) a.p[i] = probs[i];
    hipLaunchKernelGGL(mlp_rows_fwd_kernel, dim3(B, n_probs), dim3(MLP_THREADS), 0, (hipStream_t)stream, a, B);
    return MLPLAUNCH_OK();
}

int sgv_op_mlp_rows_bwd(const sgv_mlp_rows* probs, int n_probs, int B, void* stream) {
    if (int rc = rows_check(probs, n_probs, B, true)) return rc;
    RowArgs a = {};
    for (int i = 0; i < n_probs; ++i) a.p[i] = probs[i];
    hipLaunchKernelGGL(mlp_rows_bwd_kernel, dim3(B, n_probs), dim3(MLP_THREADS), 0, (hipStream_t)stream, a, B);
    return MLPLAUNCH_OK();
}

int sgv_op_mlp_gemm_bwd(const sgv_mlp_gemm_bwd* probs, int n_probs, int dx_sum, const float* dx_addend, const sgv_mlp_colsum* sums, int n_sums,
                        int B, void* stream) {
    MLPCHK(n_probs >= 0 && n_probs <= MLP_MAX_PROBS && n_sums >= 0 && n_sums <= MLP_MAX_SUMS && B > 0 && (n_probs == 0 || probs) &&
               (n_sums == 0 || sums) && n_probs + n_sums > 0,
           "sgv_op_mlp_gemm_bwd: bad argument (n_probs %d, n_sums %d, B %d)", n_probs, n_sums, B);
    GemmBwdArgs a = {};
    a.np = n_probs; a.ncs = n_sums; a.B = B; a.dx_sum = dx_sum ? 1 : 0; a.dx_addend = dx_addend;
    const int mt = cdiv_i(B, 16);
    int n_dx[2] = {0, 0}, n_dw[2] = {0, 0}, n_db[2] = {0, 0};
    for (int i = 0; i < n_probs; ++i) {
        const sgv_mlp_gemm_bwd& p = probs[i];
        MLPCHK(p.dz && p.K > 0 && p.O > 0, "sgv_op_mlp_gemm_bwd: problem %d needs dz and K, O > 0", i);
        MLPCHK(!p.dx || p.W, "sgv_op_mlp_gemm_bwd: problem %d: dx needs W", i);
        MLPCHK(!p.dW || p.x, "sgv_op_mlp_gemm_bwd: problem %d: dW needs x", i);
        a.p[i] = p;
        if (p.dW) n_dw[i] = cdiv_i(p.O, 16) * cdiv_i(p.K, 16);
        if (p.db) n_db[i] = cdiv_i(p.O, MLP_THREADS);
        if (!a.dx_sum && p.dx) n_dx[i] = mt * cdiv_i(p.K, 16);
    }
    if (a.dx_sum) {
        MLPCHK(n_probs > 0 && probs[0].dx, "sgv_op_mlp_gemm_bwd: dx_sum writes problem 0's dx");
        for (int i = 0; i < n_probs; ++i)
            MLPCHK(probs[i].K == probs[0].K && probs[i].W, "sgv_op_mlp_gemm_bwd: dx_sum needs the same K and W for every problem");
        n_dx[0] = mt * cdiv_i(probs[0].K, 16);
    } else {
        MLPCHK(!dx_addend, "sgv_op_mlp_gemm_bwd: dx_addend needs dx_sum");
    }
    a.seg[0] = n_dx[0]; a.seg[1] = a.seg[0] + n_dx[1];
    a.seg[2] = a.seg[1] + n_dw[0]; a.seg[3] = a.seg[2] + n_dw[1];
    a.seg[4] = a.seg[3] + n_db[0]; a.seg[5] = a.seg[4] + n_db[1];
    int total = a.seg[5];
    for (int i = 0; i < n_sums; ++i) {
        MLPCHK(sums[i].src && sums[i].out && sums[i].n > 0, "sgv_op_mlp_gemm_bwd: column sum %d needs src, out and n > 0", i);
        a.cs[i] = sums[i];
        a.cs_start[i] = total - a.seg[5];
        total += cdiv_i(sums[i].n, MLP_THREADS);
    }
    a.cs_start[n_sums] = total - a.seg[5];
    a.seg[6] = total;
    if (total == 0) return 0;
    hipLaunchKernelGGL(mlp_gemm_bwd_kernel, dim3(total), dim3(MLP_THREADS), 0, (hipStream_t)stream, a);
    return MLPLAUNCH_OK();
}

}  // extern "C"
