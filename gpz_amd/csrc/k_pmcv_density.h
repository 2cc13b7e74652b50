// What the units for rows with missing inputs on a covariance kind share (k_predict_missing_cov.hip, where the records are described and
// written, and k_predict_missing_cov_gamma.hip): the NaN pattern, the density of one record and the switch over the observed dimensions.
#pragma once
#include "gpz_dev.h"

#define PMCV_MAXD 10
#define PMCV_SB 16                    // records per LDS stage of a pair (the pair kernel: per wave; the gamma kernel: per pair slot)

struct PmcvPat {
    int d, no, nu;
    int o[PMCV_MAXD], u[PMCV_MAXD];
};

static inline PmcvPat pmcv_pat(int d, unsigned obs) {
    PmcvPat pt{};
    pt.d = d;
    for (int c = 0; c < d; ++c) {
        if ((obs >> c) & 1u) pt.o[pt.no++] = c;
        else pt.u[pt.nu++] = c;
    }
    return pt;
}

// ---- the density every tile kernel shares ----------------------------------------------------------------------------------------------
template <int NO>
__device__ __forceinline__ double pmcv_density(const double *t, const double (&x)[NO ? NO : 1]) {
    double xa[NO ? NO : 1];
#pragma unroll
    for (int c = 0; c < NO; ++c) xa[c] = x[c] - t[1 + c];
    double q = 0.0;
    int e = 1 + NO;
#pragma unroll
    for (int r = 0; r < NO; ++r) {
        double y = 0.0;
#pragma unroll
        for (int c = r; c < NO; ++c) y = fma(t[e++], xa[c], y);
        q = fma(y, y, q);
    }
    return exp(t[0] - 0.5 * q);
}

#define PMCV_CASES(MACRO)                                                                                  \
    switch (pt.no) {                                                                                       \
        case 0: MACRO(0); break; case 1: MACRO(1); break; case 2: MACRO(2); break; case 3: MACRO(3); break; \
        case 4: MACRO(4); break; case 5: MACRO(5); break; case 6: MACRO(6); break; case 7: MACRO(7); break; \
        case 8: MACRO(8); break; case 9: MACRO(9); break;                                                  \
        default: return -1;                                                                                \
    }
