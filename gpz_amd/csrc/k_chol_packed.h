// The packed d x d Cholesky of the register-resident kernels (k_psi.hip: the one-shot routes; k_predict_noisy_cov.hip: the predictor's
// tile kernels), in one place so that both factorise with the same operations.
#pragma once
#include "gpz_dev.h"

// packed lower triangle, row-major: element (r, c), c <= r, at r(r+1)/2 + c
#define LT(r, c) ((r) * ((r) + 1) / 2 + (c))

// In-place Cholesky of a packed lower triangle, division-free: rd[c] = 1 / L_cc (the diagonal slots of M hold L_cc for the
// callers that read them), *prod_rd = prod_c rd[c] = |M|^-1/2.  A non-positive pivot gives NaN as sqrt() would.
template <int D>
__device__ __forceinline__ void chol_packed_rd(double (&M)[D * (D + 1) / 2], double (&rd)[D], double *prod_rd) {
    double prod = 1.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        double p = M[LT(c, c)];
#pragma unroll
        for (int q = 0; q < c; ++q) p = fma(-M[LT(c, q)], M[LT(c, q)], p);
        const double inv = rsqrt_nr2(p);
        rd[c] = inv;
        M[LT(c, c)] = p * inv;
        prod *= inv;
#pragma unroll
        for (int r = c + 1; r < D; ++r) {
            double s = M[LT(r, c)];
#pragma unroll
            for (int q = 0; q < c; ++q) s = fma(-M[LT(r, q)], M[LT(c, q)], s);
            M[LT(r, c)] = s * inv;
        }
    }
    *prod_rd = prod;
}
