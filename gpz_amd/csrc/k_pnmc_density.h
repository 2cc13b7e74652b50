// What the units for rows with input noise and missing inputs on a covariance kind share (k_predict_noisy_missing_cov.hip, where the
// records are described and written, and k_predict_noisy_missing_cov_gamma.hip): the density of one record and the switch over the
// observed dimensions, in one place so that every kernel forms a density with the same operations.
#pragma once
#include "gpz_dev.h"
#include "k_pmcv_density.h"   // PMCV_MAXD, PmcvPat, pmcv_pat
#include "k_ncov_density.h"   // ncov_factor, ncov_density, LT

// ---- the density every tile kernel shares ----------------------------------------------------------------------------------------------
// t: the record, the same address in every lane; x, ps: the row's observed inputs and their variances; nu: the missing dimensions
template <int NO>
__device__ __forceinline__ double pnmc_density(const double *t, int nu, const double (&x)[NO], const double (&ps)[NO]) {
    constexpr int TRI = NO * (NO + 1) / 2;
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
    ncov_factor<NO>(t + 1 + NO, ps, M, rd, &prd);
    return ncov_density<NO>(t + 1, t[0] - 0.5 * q2, w, M, rd, prd);
}

#define PNMC_CASES(MACRO)                                                                                  \
    switch (pt.no) {                                                                                       \
        case 1: MACRO(1); break; case 2: MACRO(2); break; case 3: MACRO(3); break; case 4: MACRO(4); break; \
        case 5: MACRO(5); break; case 6: MACRO(6); break; case 7: MACRO(7); break; case 8: MACRO(8); break; \
        case 9: MACRO(9); break;                                                                           \
        default: return -1;                                                                                \
    }
