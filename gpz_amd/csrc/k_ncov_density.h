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

// M <- S + Psi_i over the whole packed triangle (rows with a full input-noise covariance: k_predict_psi_cube.hip,
// k_predict_psi_cube_gamma.hip), factorised as above.  Element q = LT(r, c) of the row's Psi is P[q * ldp]: a lane's own array with
// ldp = 1, or the lane's place in the staged columns Psic [d (d + 1) / 2][ldx] with ldp = ldx.  With zero off the diagonal the sums
// are S + 0.0 and the factor has the bits of ncov_factor's.
template <int D>
__device__ __forceinline__ void ncov_factor_tri(const double *S, const double *P, long ldp, double (&M)[D * (D + 1) / 2],
                                                double (&rd)[D], double *prd) {
#pragma unroll
    for (int q = 0; q < D * (D + 1) / 2; ++q) M[q] = S[q] + P[(size_t)q * ldp];   // Cij + Psi(:, :, i)     predictCov.m:109
    chol_packed_rd<D>(M, rd, prd);
}

// Where a VC lane keeps its row's triangle across the records: in registers up to this width, above it read again from the staged
// columns at every record (DESIGN.md section 33 has the compiler's numbers and the tile times behind the choice).  GC needs the triangle
// only in front of a loop and always loads it there.
#ifndef GPZ_PSI_CUBE_REG_D
#define GPZ_PSI_CUBE_REG_D 10
#endif
constexpr bool psi_cube_regs(int d) { return d <= GPZ_PSI_CUBE_REG_D; }

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
