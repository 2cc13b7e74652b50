// gamma under every weight draw for rows with input noise (gpz_predictor_stack_noisy / _stack_noisy_dev / _draws_gamma_noisy_dev,
// gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab E[phi_a phi_b](x_i, psi_i) w_s,a w_s,b - mu_s,i^2 per output, predictNoisy's gamma
// (predictDiag.m:111-124) with the draw's weights in place of w; f_ab = 2 off the diagonal, 1 on it.
//
//   k_predict_noisy_gamma<DT>   predict_gamma_body (k_predict_gamma_impl.h: the f64 MFMA product of pair densities and weight products,
//                               its LDS stages, chunks and passes) with GammaDiag<DT>: the pair density of k_predict_noisy_small's
//                               arithmetic (one r = (C_ab + psi)^-1/2 per dimension by v_rsq_f64 + two Newton steps, z = exp(lnZ - 1/2 sum
//                               (Delta r)^2) prod r) from the record head [lnZ | c_ab | C_ab], the first 1 + 2 d doubles of the handle's
//                               pair table; nothing is kept across K steps.  8 blocks (128 columns) of accumulators per pass.
//   k_gamma_finish_dev          sum of the chunks in chunk order, gamma_s = fma(-mu_s, mu_s, sum) -> the caller's Gam (n x k x nd).
//   k_gamma_finish_s2           the same gamma_s -> the widths of the stack: s2 [(1 + nd) k][nt], row o = (nu + beta) + gamma of nout,
//                               row (1 + s) k + o = beta + max(gamma_s, 0).
#include "k_predict_gamma_impl.h"

#define GPZ_GAMMA_NB 8   // 16-column blocks of accumulators per pass (128 columns)

template <int DT>
struct GammaDiag {
    static constexpr int D = DT, PW = DT, RL = 1 + 2 * DT, NB = GPZ_GAMMA_NB;
    __device__ __forceinline__ void init(const double *, const double (&)[DT]) {}
    __device__ __forceinline__ double z(const double *t, const double (&x)[DT], const double (&ps)[DT]) const {
        double q = 0.0, rp = 1.0;
#pragma unroll
        for (int c = 0; c < DT; ++c) {
            const double r = rsqrt_nr2(t[1 + DT + c] + ps[c]);      // (Cij + Psi)^-1/2            predictDiag.m:105
            const double dl = (x[c] - t[1 + c]) * r;
            q = fma(dl, dl, q);
            rp *= r;
        }
        return exp(t[0] - 0.5 * q) * rp;                            // :107
    }
};

template <int DT>
__global__ __launch_bounds__(256) void k_predict_noisy_gamma(PredGammaArgs a) { predict_gamma_body<GammaDiag<DT>>(a); }

// the chunks' sums of column col = o nd + s in chunk order, then gamma_s = sum - mu_s^2 in one fma
__device__ __forceinline__ double pg_gamma(const double *__restrict__ part, int nchunk, long ldp, int ncol, int col, int i, double mu) {
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += part[((size_t)c * ncol + col) * ldp + i];
    return fma(-mu, mu, s);
}

__global__ __launch_bounds__(256) void k_gamma_finish_dev(const double *__restrict__ part, int nchunk, long ldp, const double *__restrict__ dout,
                                                          int nt, int k, int nd, long ns, long r0, double *__restrict__ Gam) {
    const int i = blockIdx.x * 256 + threadIdx.x, col = blockIdx.y, o = col / nd, s = col - o * nd;
    if (i >= nt) return;
    Gam[((size_t)s * k + o) * ns + r0 + i] = pg_gamma(part, nchunk, ldp, nd * k, col, i, dout[(size_t)col * nt + i]);
}

__global__ __launch_bounds__(256) void k_gamma_finish_s2(const double *__restrict__ part, int nchunk, long ldp, const double *__restrict__ nout,
                                                         const double *__restrict__ dout, int nt, int k, int nd, double *__restrict__ s2) {
    const int i = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, c = q / k, o = q - c * k;
    if (i >= nt) return;
    const double beta = nout[(size_t)(2 * k + o) * nt + i];
    double w;
    if (c == 0) {
        w = nout[(size_t)(k + o) * nt + i] + beta + nout[(size_t)(3 * k + o) * nt + i];   // (nu + beta) + gamma: k_pred_finish_noisy_dev's sigma
    } else {
        const int col = o * nd + (c - 1);
        w = beta + fmax(pg_gamma(part, nchunk, ldp, nd * k, col, i, dout[(size_t)col * nt + i]), 0.0);
    }
    s2[(size_t)q * nt + i] = w;
}

// pair chunks: one per 4096 pairs, at most 4 (it changes at m = 91, 128, 157).  The model's shape only, never the rows or the draws.
// The cap stays at 4 for 256 < ceil16(m) <= 1024 (GPZ_PREDICT_LARGE_M; no measurement decided that).  predict_gamma_body's p0, p1, npair
// and (pa, pb) are ints: npair = 524 800 at m = 1024, and pa (pa + 1) / 2 stays below it.
int predict_gamma_chunks(int m) {
    const long c = ((long)m * (m + 1) / 2 + 4095) / 4096;
    return (int)(c < 1 ? 1 : (c > 4 ? 4 : c));
}

int launch_predict_noisy_gamma(hipStream_t st, int d, const double *Xc, const double *Psic, long ldx, int n, int m, const double *tab,
                               int rec, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > 20 || nchunk < 1 || ldw % 16 || ncol > ldw || rec < 1 + 2 * d) return -1;
    const PredGammaArgs a = predict_gamma_args(Xc, Psic, ldx, n, m, tab, rec, W, ldw, ncol, nchunk, part, ldp);
    const dim3 grid = predict_gamma_grid(a, nchunk, GPZ_GAMMA_NB);
    switch (d) {
#define PG_CASE(DD) case DD: hipLaunchKernelGGL((k_predict_noisy_gamma<DD>), grid, dim3(256), 0, st, a); break;
        PG_CASE(1) PG_CASE(2) PG_CASE(3) PG_CASE(4) PG_CASE(5) PG_CASE(6) PG_CASE(7) PG_CASE(8) PG_CASE(9) PG_CASE(10)
        PG_CASE(11) PG_CASE(12) PG_CASE(13) PG_CASE(14) PG_CASE(15) PG_CASE(16) PG_CASE(17) PG_CASE(18) PG_CASE(19) PG_CASE(20)
#undef PG_CASE
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_gamma_finish_dev(hipStream_t st, const double *part, int nchunk, long ldp, const double *dout, int nt, int k, int nd, long ns,
                            long r0, double *Gam) {
    if (nt <= 0) return 0;
    hipLaunchKernelGGL(k_gamma_finish_dev, dim3((unsigned)((nt + 255) / 256), (unsigned)(nd * k)), dim3(256), 0, st, part, nchunk, ldp, dout, nt,
                       k, nd, ns, r0, Gam);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_gamma_finish_s2(hipStream_t st, const double *part, int nchunk, long ldp, const double *nout, const double *dout, int nt, int k,
                           int nd, double *s2) {
    if (nt <= 0) return 0;
    hipLaunchKernelGGL(k_gamma_finish_s2, dim3((unsigned)((nt + 255) / 256), (unsigned)((1 + nd) * k)), dim3(256), 0, st, part, nchunk, ldp, nout,
                       dout, nt, k, nd, s2);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
