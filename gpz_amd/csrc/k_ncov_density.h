// The pair / basis density of the predictor's tile kernels for rows with input noise on a covariance kind (k_predict_noisy_cov.hip and
// k_predict_psi_cube.hip: the moments and E_x[PHI], on the bodies of k_predict_ncov_impl.h; k_predict_noisy_cov_gamma.hip and
// k_predict_psi_cube_gamma.hip: gamma under every weight draw), in one place so that every kernel forms a density with the same
// operations: the packed Cholesky of S + Psi_i and a forward substitution, all in registers.  Psi_i comes in two forms, a variance per
// dimension and a full matrix as a packed triangle: the policies PsiDiag and PsiTri below are all that tells the kernels apart.
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
// k_predict_psi_cube_gamma.hip), factorised as above.  Element q = LT(r, c) of the row's Psi is P[q * ldp]; the kernels pass a lane's own
// array with ldp = 1.  With zero off the diagonal the sums are S + 0.0 and the factor has the bits of ncov_factor's.
template <int D>
__device__ __forceinline__ void ncov_factor_tri(const double *S, const double *P, long ldp, double (&M)[D * (D + 1) / 2],
                                                double (&rd)[D], double *prd) {
#pragma unroll
    for (int q = 0; q < D * (D + 1) / 2; ++q) M[q] = S[q] + P[(size_t)q * ldp];   // Cij + Psi(:, :, i)     predictCov.m:109
    chol_packed_rd<D>(M, rd, prd);
}

// A row's Psi in the two forms a tile's slot holds it, for the kernels of k_predict_ncov_impl.h and for GammaNcov below.  W: the columns
// of the slot [W][ldx] a lane loads for its row, element q at Pg[q ldx] (ncov_psi_load).  factor: M <- S + Psi_i, factorised.
// RELOAD: what a SHARED (GC) tile kernel does with the W values, which it needs only for the one factorisation in front of a phase.
// The D of a diagonal stay in registers from the kernel's start; a triangle is loaded again in front of each phase and dies in the
// factorisation, so that it is never live beside the sums of the other phase (DESIGN.md section 33 has the register counts that this
// keeps).  Without SHARED (VC) every record needs them and both forms stay in registers beside M.
template <int DD>
struct PsiDiag {   // a variance per dimension: Psic [d][ldx], the layout of Xc
    static constexpr int D = DD, W = DD;
    static constexpr bool RELOAD = false;
    static __device__ __forceinline__ void factor(const double *S, const double (&ps)[W], double (&M)[DD * (DD + 1) / 2], double (&rd)[DD],
                                                  double *prd) {
        ncov_factor<DD>(S, ps, M, rd, prd);
    }
};
template <int DD>
struct PsiTri {   // a full d x d matrix: Psiq [d (d + 1) / 2][ldx], column q = LT(r, c) the element (r, c), r >= c
    static constexpr int D = DD, W = DD * (DD + 1) / 2;
    static constexpr bool RELOAD = true;
    static __device__ __forceinline__ void factor(const double *S, const double (&ps)[W], double (&M)[W], double (&rd)[DD], double *prd) {
        ncov_factor_tri<DD>(S, ps, 1, M, rd, prd);
    }
};

template <int W>
__device__ __forceinline__ void ncov_psi_load(const double *Pg, long ldx, double (&ps)[W]) {
#pragma unroll
    for (int q = 0; q < W; ++q) ps[q] = Pg[(size_t)q * ldx];
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

// The policy of predict_gamma_body (k_predict_gamma_impl.h) for both forms: k_predict_noisy_cov_gamma<D, SHARED> with PsiDiag<D>,
// k_predict_psi_cube_gamma<D, SHARED> with PsiTri<D>; NBLK: the unit's 16-column blocks of accumulators per pass.  The body loads the
// row's PW values of Psi.  A lane keeps the factor M, rd, prd across K steps.  SHARED (GC): every C_ab is one matrix, so init factorises
// C + Psi_i of the row once, from record 0 (the same bits in every chunk and pass), nothing of Psi_i is live in the loop and a K step
// is the substitution alone.  VC: the PW values stay in registers beside M and z factorises at every K step.
template <class Psi, bool SHARED, int NBLK>
struct GammaNcov {
    static constexpr int D = Psi::D, PW = Psi::W, NP = D * (D + 1) / 2, RL = 1 + D + NP, NB = NBLK;
    double M[NP], rd[D], prd;
    __device__ __forceinline__ void init(const double *tab, const double (&ps)[PW]) {
        if (SHARED) Psi::factor(tab + 1 + D, ps, M, rd, &prd);   // C + Psi_i of the row, once                predictCov.m:109
    }
    __device__ __forceinline__ double z(const double *t, const double (&x)[D], const double (&ps)[PW]) {
        if (!SHARED) Psi::factor(t + 1 + D, ps, M, rd, &prd);    // Cij + Psi_i                               :109
        return ncov_density<D>(t + 1, t[0], x, M, rd, prd);      //                                           :111
    }
};
