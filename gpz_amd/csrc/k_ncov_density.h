// The pair / basis density of the predictor's tile kernels for rows with input noise on a covariance kind (k_predict_noisy_cov.hip: the
// moments and E_x[PHI]; k_predict_noisy_cov_gamma.hip: gamma under every weight draw), in one place so that every kernel forms a
// density with the same operations: the packed Cholesky of S + diag(psi) and a forward substitution, all in registers.
#pragma once
#include "gpz_dev.h"
#include "k_chol_packed.h"   // LT, chol_packed_rd

// M <- S + diag(ps), factorised in place by chol_packed_rd (rd[c] = 1 / L_cc, *prd = their product = |M|^-1/2; a non-positive pivot
// gives NaN as sqrt() would).  S: a packed lower triangle, the same address in every lane.
template <int D>
__device__ __forceinline__ void ncov_factor(const double *S, const double (&ps)[D], double (&M)[D * (D + 1) / 2], double (&rd)[D],
                                            double *prd) {
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) M[LT(r, c)] = (r == c) ? S[LT(r, c)] + ps[r] : S[LT(r, c)];   // Sigma + Psi    getPHI.m:84, predictCov.m:109
    chol_packed_rd<D>(M, rd, prd);
}

// exp(lnz - 1/2 |L^-1 (x - cen)|^2) prod(1 / L_cc): N(x; cen, M) up to the constant that lnz carries - no logarithm, no division
template <int D>
__device__ __forceinline__ double ncov_density(const double *cen, double lnz, const double (&x)[D], const double (&M)[D * (D + 1) / 2],
                                               const double (&rd)[D], double prd) {
    double q = 0.0, y[D];
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double s = x[r] - cen[r];
#pragma unroll
        for (int c = 0; c < r; ++c) s = fma(-M[LT(r, c)], y[c], s);
        y[r] = s * rd[r];
        q = fma(y[r], y[r], q);
    }
    return exp(lnz - 0.5 * q) * prd;
}
