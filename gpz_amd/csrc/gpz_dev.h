// Shared device-side definitions for the gfx950 kernels of libgpz_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));

// v_mfma_f64_16x16x4_f64: D(16x16) += A(16x4) * B(4x16), one wave.
//   A operand: lane l supplies A[i = l&15][k = l>>4]
//   B operand: lane l supplies B[k = l>>4][j = l&15]
//   C/D:       lane l, reg r holds C[row = (l>>4) + 4r][col = l&15]     (f64-specific map)
#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

#define GPZ_KIND_DIAG 0   // GL, VL, GD, VD: Gamma expanded to m x d   (getPHI.m:28-35)
#define GPZ_KIND_COV  1   // GC, VC:         Gamma expanded to d x d x m (getPHI.m:36-39)

#define GPZ_LOG2   0.69314718055994530942
#define GPZ_LOG2PI 1.83787706640934548356

// padded leading dimension of K-major LDS tiles read with the MFMA operand pattern
// (16 consecutive doubles x 4 k-rows per ds_read_b64): stride == 16 (mod 32) doubles is conflict-free.
#define LDS_LD128 144
#define LDS_LD64   80

// 1/u for u > 0 without the library divide (~25 instructions, correctly rounded): v_rcp_f64 seed + two Newton steps, <= 1 ulp.
__device__ __forceinline__ double gpz_rcp(double u) {
    double y = __builtin_amdgcn_rcp(u);
    double e = fma(-u, y, 1.0);
    y = fma(y, e, y);
    e = fma(-u, y, 1.0);
    y = fma(y, e, y);
    return y;
}

// The same with ONE Newton step: the v_rcp_f64 seed is good to ~2^-27, one step squares that - a few ulps, not correctly rounded.  For the
// per-(row, basis function, dimension) factors 1 / (1 + psi gamma^2) of the input-noise kernels, whose results are summed over d dimensions
// and n rows and gated at 1e-8: two multiply-adds less of the ~14 a triple costs.
__device__ __forceinline__ double gpz_rcp1(double u) {
    double y = __builtin_amdgcn_rcp(u);
    const double e = fma(-u, y, 1.0);
    return fma(y, e, y);
}

// 1 / sqrt(p) in fp64 without the library's sqrt + divide (~50 instructions): v_rsq_f64 seed and two Newton steps.
__device__ __forceinline__ double rsqrt_nr2(double p) {
    double y = __builtin_amdgcn_rsq(p);
    const double h = 0.5 * p;
    double e = fma(-h * y, y, 0.5);
    y = fma(y, e, y);
    e = fma(-h * y, y, 0.5);
    y = fma(y, e, y);
    return y;
}

// the pair (i, j), j <= i, of the triangular index q = i (i + 1) / 2 + j
__device__ __forceinline__ void gpz_pair_of(long q, int *pi, int *pj) {
    long i = (long)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= q) ++i;
    while (i * (i + 1) / 2 > q) --i;
    *pi = (int)i;
    *pj = (int)(q - i * (i + 1) / 2);
}

// The per-output tail of the pair record of (i, j), j <= i: cf [3k] = [f w_i w_j, f v_i v_j, f iS(i, j)] per output, f = 2 off the diagonal
// and 1 on it (predictDiag.m:113-119, :191-198, :277-284).  w, v: m x k column-major (v nullptr: 0); iS: m x m x k column-major, read at
// i >= j only as the reference does.
__device__ __forceinline__ void gpz_pair_coef(double *cf, int i, int j, int m, int k, const double *__restrict__ w,
                                              const double *__restrict__ v, const double *__restrict__ iS) {
    const double f = i == j ? 1.0 : 2.0;
    for (int o = 0; o < k; ++o) {
        cf[3 * o] = f * (w[i + (size_t)m * o] * w[j + (size_t)m * o]);
        cf[3 * o + 1] = v ? f * (v[i + (size_t)m * o] * v[j + (size_t)m * o]) : 0.0;
        cf[3 * o + 2] = f * iS[i + (size_t)m * j + (size_t)m * m * o];
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Sum over the block (256 threads = 4 waves); result valid in thread 0.
__device__ __forceinline__ double block_sum_256(double v, double *sh4) {
    v = wave_sum(v);
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh4[w] = v;
    __syncthreads();
    return sh4[0] + sh4[1] + sh4[2] + sh4[3];
}
