// The density of one record for rows with input noise and missing inputs on a covariance kind (k_predict_noisy_missing_cov.hip, where
// the records are described and written) and the switch over the observed dimensions, in one place so that every body of
// k_predict_nmcov_impl.h forms a density with the same operations.
#pragma once
#include "gpz_dev.h"
#include "k_pmcv_density.h"   // PMCV_MAXD, PmcvPat, pmcv_pat
#include "k_ncov_density.h"   // PsiDiag, PsiTri, ncov_density, LT

// ---- the density every tile kernel shares ----------------------------------------------------------------------------------------------
// t: the record, the same address in every lane; x: the row's observed inputs; nu: the missing dimensions.  P: the policy of
// k_ncov_density.h for the row's Psi_oo over the NO = P::D observed dimensions, ps its P::W values - PsiDiag<NO> a variance per observed
// dimension (k_predict_noisy_missing_cov*.hip), PsiTri<NO> the packed lower triangle of the observed x observed block of a full matrix
// (k_predict_psi_cube_missing*.hip).  The policy's factor step is all that differs: J x, the nu squares and ncov_density are the same.
template <class P>
__device__ __forceinline__ double pnmc_density(const double *t, int nu, const double (&x)[P::D], const double (&ps)[P::W]) {
    constexpr int NO = P::D, TRI = NO * (NO + 1) / 2;
    const double *J = t + 1 + NO + TRI, *A2 = J + NO * NO, *b2 = A2 + nu * NO;
    double w[NO], q2 = 0.0;
#pragma unroll
    for (int r = 0; r < NO; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < NO; ++c) s = fma(J[r * NO + c], x[c], s);
        w[r] = s;
    }
#pragma unroll 1
    for (int r = 0; r < nu; ++r) {
        double s = b2[r];
#pragma unroll
        for (int c = 0; c < NO; ++c) s = fma(A2[r * NO + c], x[c], s);
        q2 = fma(s, s, q2);
    }
    double M[TRI], rd[NO], prd;
    P::factor(t + 1 + NO, ps, M, rd, &prd);
    return ncov_density<NO>(t + 1, t[0] - 0.5 * q2, w, M, rd, prd);
}

#define PNMC_CASES(MACRO)                                                                                  \
    switch (pt.no) {                                                                                       \
        case 1: MACRO(1); break; case 2: MACRO(2); break; case 3: MACRO(3); break; case 4: MACRO(4); break; \
        case 5: MACRO(5); break; case 6: MACRO(6); break; case 7: MACRO(7); break; case 8: MACRO(8); break; \
        case 9: MACRO(9); break;                                                                           \
        default: return -1;                                                                                \
    }
