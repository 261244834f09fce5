// Geometry and per-thread context of the GroupNorm-family kernels on channels-last [B*T][C] maps, and the one derivation of a group's
// mean / rstd.  Shared by ew.hip (GroupNorm forward / backward, the recon loss) and recon_out.hip (the recon tails); nobody else includes it.
#pragma once
#include "sgv_ew.h"

static inline int cdiv_i(long a, long b) { return (int)((a + b - 1) / b); }

// ------------------------------------------------------------------------------------------
// geometry shared by the GroupNorm-family kernels
// ------------------------------------------------------------------------------------------
struct GNGeom {
    int CV, RL, rowsplit;
    dim3 grid;
};
static GNGeom gn_geom(int B, int T, int C, int target = 2048) {
    GNGeom g;
    const int nv = C / 8;
    int cv = 1;
    while (cv < nv && cv < 256) cv <<= 1;
    g.CV = cv;
    g.RL = 256 / cv;
    const int colblocks = cdiv_i(nv, cv);
    // aim for >= ~target blocks, at least RL rows per block
    int rs = cdiv_i(target, (long)colblocks * B);
    int maxrs = cdiv_i(T, g.RL);
    if (rs > maxrs) rs = maxrs;
    if (rs < 1) rs = 1;
    g.rowsplit = rs;
    g.grid = dim3(colblocks, rs, B);
    return g;
}

struct GNCtx {
    int tx, ty, c0, b, t_lo, t_hi, RL;
    bool col_ok;
};
__device__ __forceinline__ GNCtx gn_ctx(const GNParams& p) {
    GNCtx c;
    const int tid = threadIdx.x;
    c.tx = tid % p.CV;
    c.ty = tid / p.CV;
    c.RL = 256 / p.CV;
    c.c0 = (blockIdx.x * p.CV + c.tx) * 8;
    c.col_ok = c.c0 < p.C;
    c.b = blockIdx.z;
    const int rps = (p.T + gridDim.y - 1) / gridDim.y;
    c.t_lo = blockIdx.y * rps;
    c.t_hi = min(p.T, c.t_lo + rps);
    return c;
}

// mean and 1 / sqrt(var + eps) of group g of sample b from the fp64 (sum, sum of squares) in p.sums: the one place they are derived
__device__ __forceinline__ void gn_mean_rstd(const GNParams& p, int b, int g, float& mean, float& rstd) {
    const double n = (double)p.Cg * (double)p.T;
    const double s = p.sums[((long)b * p.G + g) * 2 + 0];
    const double ss = p.sums[((long)b * p.G + g) * 2 + 1];
    const double m = s / n;
    double var = ss / n - m * m;
    if (var < 0.0) var = 0.0;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + 1e-5));
}

// per-element mean / rstd (and, WITH_M, the backward means m1 = s1/n, m2 = s2/n) of the element's group.
// The fp64 divide/sqrt chain runs once per block on G threads and is broadcast through LDS: done per
// thread it cost more than the streaming work of the small layers.  Must be called by all 256 threads.
template <bool WITH_M = false>
__device__ __forceinline__ void gn_consts(const GNParams& p, const GNCtx& c, float mean[8], float rstd[8],
                                          float* m1 = nullptr, float* m2 = nullptr) {
    __shared__ float gc[SGV_GN_MAX_GROUPS][4];
    if ((int)threadIdx.x < p.G) {
        const int g = threadIdx.x;
        gn_mean_rstd(p, c.b, g, gc[g][0], gc[g][1]);
        if constexpr (WITH_M) {
            const double n = (double)p.Cg * (double)p.T;
            gc[g][2] = (float)(p.sums2[((long)c.b * p.G + g) * 2 + 0] / n);
            gc[g][3] = (float)(p.sums2[((long)c.b * p.G + g) * 2 + 1] / n);
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int g = min((c.c0 + e) / p.Cg, p.G - 1);
        mean[e] = gc[g][0];
        rstd[e] = gc[g][1];
        if constexpr (WITH_M) { m1[e] = gc[g][2]; m2[e] = gc[g][3]; }
    }
}

#define GN_LAUNCH(KERN, P, S, ...)                                         \
    do {                                                                   \
        GNGeom g_ = gn_geom((P).B, (P).T, (P).C);                          \
        (P).CV = g_.CV;                                                    \
        hipLaunchKernelGGL(KERN, g_.grid, dim3(256), 0, S, P, ##__VA_ARGS__); \
    } while (0)
