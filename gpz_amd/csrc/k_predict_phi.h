// PHI of a block of 32 rows in LDS: the no-missing forms of k_phi_diag / k_phi_cov, element by element (getPHI.m:73-113).
// Shared by the fused predict kernels (k_predict_small.hip: mu, nu, beta; k_predict_draws.hip: posterior draws of the mean), so that a
// row's PHI has the same bits in both.  PSI (diagonal kinds; the draws of k_predict_noisy.hip) takes the rows' per-dimension noise
// variances as well and forms E_x[PHI] (getPHI.m:104) in k_phi_diag<.., PSI>'s arithmetic.
//
// Mapping: thread (column j = tid % nk, row group g = tid / nk) keeps the parameters of basis function j in registers for the whole
// launch and walks rows g, g + 256 / nk, ...; threads past the last row group idle.  Columns m .. nk - 1 and rows past n are zero.
#pragma once
#include "gpz_dev.h"

// PS_LDA, the row stride of the PHI block in LDS (doubles), is the including kernel's: its LDS layout (and the ISA guards that read it)
#ifndef PS_LDA
#error "define PS_LDA before including k_predict_phi.h"
#endif

// the block's rows of X (de x ldx column layout) -> sX [32][D], rows past n zero
template <int D>
__device__ __forceinline__ void ps_load_x(const double *Xc, long ldx, int n, long i0, double *sX, int tid) {
    for (int e = tid; e < 32 * D; e += 256) {
        const int r = e / D, c = e % D;
        sX[e] = (i0 + r < n) ? Xc[(size_t)c * ldx + i0 + r] : 0.0;
    }
}

// the block's rows of Psi (the layout of Xc) -> sPsi [32][D], rows past n zero
template <int D>
__device__ __forceinline__ void ps_load_psi(const double *Psic, long ldx, int n, long i0, double *sPsi, int tid) {
    for (int e = tid; e < 32 * D; e += 256) {
        const int r = e / D, c = e % D;
        sPsi[e] = (i0 + r < n) ? Psic[(size_t)c * ldx + i0 + r] : 0.0;
    }
}

// D = padded input dimension, COV = covariance kind.  P: m x D row-major; G: gamma^2 (diagonal kinds) or [R_j packed upper | R_j p_j]
// (covariance kinds).
template <int D, bool COV, bool PSI = false>
struct PsPhiBuilder {
    static_assert(!(PSI && COV), "input noise in the fused builder: diagonal kinds only");
    int m, jc, grp, ngr;
    bool builder;
    const double *G;
    double pj[COV ? 1 : D], gj[COV ? 1 : D];   // diagonal kinds: centre and gamma^2 of basis function jc

    __device__ __forceinline__ PsPhiBuilder(const double *P, const double *G_, int m_, int nk, int tid) {
        m = m_;
        G = G_;
        jc = tid % nk;
        grp = tid / nk;
        ngr = 256 / nk;
        builder = grp < ngr;
        if constexpr (!COV) {
            const int jj = jc < m ? jc : 0;
#pragma unroll
            for (int c = 0; c < D; ++c) { pj[c] = P[(size_t)jj * D + c]; gj[c] = G[(size_t)jj * D + c]; }
        }
    }

    // PHI of rows i0 .. i0 + 31 -> sA [32][PS_LDA] (covariance kinds: the running quadratic form first)
    // PSI: sPsi [32][D], and an element is exp(-1/2 (sum_c Delta^2 gamma^2 / (1 + psi gamma^2) + ln prod_c (1 + psi gamma^2)))
    __device__ __forceinline__ void build(double *sA, const double *sX, long i0, int n, const double *sPsi = nullptr) const {
        if (!builder) return;
        if constexpr (!COV) {
            for (int r = grp; r < 32; r += ngr) {
                double q = 0.0;
                [[maybe_unused]] double pr = 1.0;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const double dl = sX[r * D + c] - pj[c];
                    if constexpr (PSI) {
                        const double u = fma(sPsi[r * D + c], gj[c], 1.0);   // 1 + psi / sigma
                        q = fma(dl * dl, gj[c] * gpz_rcp1(u), q);           // getPHI.m:104  Delta.^2 ./ (Psi + Sigma)
                        pr *= u;
                    } else {
                        q = fma(dl * dl, gj[c], q);                    // getPHI.m:97  Delta.^2 ./ Sigma
                    }
                }
                if constexpr (PSI) q += log(pr);                       // sum_c ln(1 + psi / sigma)
                sA[r * PS_LDA + jc] = (jc < m && i0 + r < n) ? exp(-0.5 * q) : 0.0;   // getPHI.m:113
            }
        } else {
            constexpr int NT = D * (D + 1) / 2;
            const double *rj = G + (size_t)(jc < m ? jc : 0) * (NT + D);
            // |R_j x - c_j|^2 row of R_j by row: the row's D - a entries in registers, the running sum in sA (k_phi_cov's order per element)
#pragma unroll
            for (int aa = 0; aa < D; ++aa) {
                double ra[D];
                const int off = aa * D - aa * (aa - 1) / 2;
#pragma unroll
                for (int b = aa; b < D; ++b) ra[b] = rj[off + (b - aa)];
                const double ca = rj[NT + aa];
                for (int r = grp; r < 32; r += ngr) {
                    double s = -ca;
#pragma unroll
                    for (int b = aa; b < D; ++b) s = fma(ra[b], sX[r * D + b], s);
                    const double q = aa == 0 ? 0.0 : sA[r * PS_LDA + jc];
                    sA[r * PS_LDA + jc] = fma(s, s, q);                 // getPHI.m:73,76
                }
            }
            for (int r = grp; r < 32; r += ngr) {
                const double q = sA[r * PS_LDA + jc];
                sA[r * PS_LDA + jc] = (jc < m && i0 + r < n) ? exp(-0.5 * q) : 0.0;
            }
        }
    }
};

// the input widths the fused kernels are instantiated for (the widths of k_phi_diag / k_phi_cov)
inline bool ps_width_instantiated(int de) {
    switch (de) {
        case 1: case 2: case 3: case 4: case 5: case 6: case 8: case 10: case 12: case 16: case 20: return true;
        default: return false;
    }
}
