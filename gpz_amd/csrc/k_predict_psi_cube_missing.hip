// Rows with a full input-noise covariance AND missing inputs through the streaming predictor, covariance kinds
// (gpz_predictor_run_psi_cube_missing_dev / _draws_psi_cube_missing_dev, gpz_predictor.hip): predictNoisyMissing of GC and VC
// (predictCov.m:233-337) for one tile of ONE group of rows that share a NaN pattern and carry a d x d matrix Psi each, the cube of
// fixPsi.m:36.  Its records (predict_noisy_missing_cov_rec doubles, which do not depend on Psi), slabs, chunk rule and tables are
// k_predict_noisy_missing_cov.hip's, and its tile kernels are that unit's with another Psi policy.  What differs is Psi_oo, the
// observed x observed block of the row's matrix, in
//     v' (S + G Psi_oo G')^-1 v = |A2 x + b2|^2 + w' (M + Psi_oo)^-1 w,          |S + G Psi_oo G'| = |S| |R_B|^2 |M + Psi_oo|:
// nothing in that identity needs a diagonal Psi_oo (the whitening by S, the QR of G and the determinant product hold for any symmetric
// positive semidefinite one), so the density is pnmc_density with PsiTri<NO> for PsiDiag<NO>: the packed Cholesky of M + Psi_oo over
// the whole no (no + 1) / 2 triangle (ncov_factor_tri through the policy), everything else unchanged.  With zeros off the diagonal the
// sums are M + 0.0 and every result has the bits of k_predict_noisy_missing_cov.hip's.
//
// The tile's Psi slot is Psio [no (no + 1) / 2][ldx]: column LT(ro, co) holds element (o[ro], o[co]), ro >= co, of every row's matrix
// with o the observed dimensions in ascending order, so o[ro] >= o[co], the element lies in the lower triangle of the caller's matrix,
// and a lane's loads are coalesced as they are for Xc.  Psi in a missing row or column is never read.
//
//   k_pcm_check_psi       word 3 of the device entries' record is set when an element of the lower triangle of an observed x observed
//                         block is NaN or infinite, itself or after its division, or a diagonal element is negative
//   k_pcm_stage_psi<T>    the caller's cube (f64 or f32; element (r, c) of row i at Psi[r sr + c sc + i sn]) -> Psio, a plain f64
//                         division by div[LT(o[ro], o[co])] (fixPsi.m:36)
//   k_pcm_ex<NO>, k_pcm_phi<NO>, k_predict_psi_cube_missing_pairs<NO, KM>   the tile kernels: wrappers of the bodies of
//                         k_predict_nmcov_impl.h with PsiTri<NO>, where the frame, the LDS and what keeps them from faulting are
//                         written.  A matrix that passes the scan but is not positive semidefinite gives its own row NaN.
// The tables (k_pnmc_basis, k_pnmc_phirec, k_pnmc_triples), k_pmcv_hd and k_pmd_finish are the twins': reached through their launchers.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_predict_nmcov_impl.h"   // the bodies and launchers; PsiTri; PMCV_MAXD, PmcvPat, pmcv_pat; LT

// ---- byte movers of the device entries -------------------------------------------------------------------------------------------------
// npo = no (no + 1) / 2 elements per row, element q = LT(ro, co) the one at (o[ro], o[co]).  div: the divisors sdX[r] sdX[c] of the
// whole d x d triangle in LT order on the device (nullptr: none)
__global__ __launch_bounds__(256) void k_pcm_check_psi(const void *__restrict__ Psi, int f32, long ns, PmcvPat pt, long sr, long sc,
                                                       long sn, const double *__restrict__ div, unsigned *__restrict__ rec) {
    const int npo = pt.no * (pt.no + 1) / 2;
    const long ne = ns * npo, step = (long)gridDim.x * 256;
    int bad = 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < ne; e += step) {
        const int q = (int)(e / ns);          // rows fastest: a contiguous d x d x n cube is read coalesced
        const long i = e - (long)q * ns;
        int ro = 0;
        while ((ro + 1) * (ro + 2) / 2 <= q) ++ro;
        const int co = q - ro * (ro + 1) / 2, r = pt.o[ro], c = pt.o[co];   // r >= c: the lower triangle
        const long at = r * sr + c * sc + i * sn;
        const double v = f32 ? (double)((const float *)Psi)[at] : ((const double *)Psi)[at];
        const double w = div ? v / div[LT(r, c)] : v;
        bad |= !(fabs(v) <= 1.7976931348623157e308) || !(fabs(w) <= 1.7976931348623157e308) || (r == c && !(v >= 0.0));
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(rec + 3, 1u);
}

template <typename T>
__global__ __launch_bounds__(256) void k_pcm_stage_psi(const T *__restrict__ Psi, long sr, long sc, long sn, long r0, int nt, PmcvPat pt,
                                                       const double *__restrict__ div, double *__restrict__ Psio, long ldx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const T *row = Psi + (r0 + i) * sn;
    for (int ro = 0; ro < pt.no; ++ro)
        for (int co = 0; co <= ro; ++co) {
            const int r = pt.o[ro], c = pt.o[co];
            double v = (double)row[r * sr + c * sc];
            if (div) v = v / div[LT(r, c)];                                  // Psi ./ (sdX' sdX)        fixPsi.m:36
            Psio[(size_t)LT(ro, co) * ldx + i] = v;
        }
}

int launch_pcm_check_psi(hipStream_t st, const void *Psi, int f32, long ns, int d, unsigned obs, long sr, long sc, long sn,
                         const double *div, unsigned *rec) {
    if (ns <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD) return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.no < 1) return 0;                  // nothing observed: nothing of Psi is read
    long nb = (ns * (pt.no * (pt.no + 1) / 2) + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_pcm_check_psi, dim3((unsigned)nb), dim3(256), 0, st, Psi, f32, ns, pt, sr, sc, sn, div, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pcm_stage_psi(hipStream_t st, const void *Psi, int f32, long sr, long sc, long sn, long r0, int nt, int d, unsigned obs,
                         const double *div, double *Psio, long ldx) {
    if (nt <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || ldx < nt) return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.no < 1) return 0;
    const dim3 grid((unsigned)((nt + 255) / 256));
    if (f32)
        hipLaunchKernelGGL(k_pcm_stage_psi<float>, grid, dim3(256), 0, st, (const float *)Psi, sr, sc, sn, r0, nt, pt, div, Psio, ldx);
    else
        hipLaunchKernelGGL(k_pcm_stage_psi<double>, grid, dim3(256), 0, st, (const double *)Psi, sr, sc, sn, r0, nt, pt, div, Psio, ldx);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the tile kernels ------------------------------------------------------------------------------------------------------------------
template <int NO>
__global__ __launch_bounds__(256) void k_pcm_ex(PredNmcovArgs a) { nmcov_ex_body<PsiTri<NO>, true>(a); }

template <int NO>
__global__ __launch_bounds__(256) void k_pcm_phi(PredNmcovArgs a) { nmcov_phi_body<PsiTri<NO>, true>(a); }

template <int NO, int KM>
__global__ __launch_bounds__(256) void k_predict_psi_cube_missing_pairs(PredNmcovArgs a) { nmcov_pairs_body<PsiTri<NO>, KM>(a); }

struct PcmKernels {
    static constexpr size_t stage_lds = PNMC_STD * sizeof(double);
    template <int NO> static auto ex() { return k_pcm_ex<NO>; }
    template <int NO> static auto phi() { return k_pcm_phi<NO>; }
    template <int NO, int KM> static auto pairs() { return k_predict_psi_cube_missing_pairs<NO, KM>; }
};

// launch_pnmc_rows with the observed triangles: Pio [m][ldr], Phi [nrow][mp] and hd [2k][ldh] from the twin's Ex and PHI records
int launch_pcm_rows(hipStream_t st, const double *Xc, const double *Psio, long ldx, int n, int nrow, int m, int mp, int d, int k,
                    unsigned obs, const double *exrec, const double *phirec, const double *w, const double *v, double *Pio, long ldr,
                    double *Phi, double *hd, long ldh) {
    return nmcov_launch_rows<PcmKernels>(st, Xc, Psio, ldx, n, nrow, m, mp, d, k, obs, exrec, phirec, w, v, Pio, ldr, Phi, hd, ldh);
}

// launch_predict_noisy_missing_cov_pairs with the observed triangles: the twin's slabs, kept under the same flag
int launch_predict_psi_cube_missing_pairs(hipStream_t st, const double *Xc, const double *Psio, long ldx, int n, const double *Pio,
                                          long ldr, int m, int d, int k, unsigned obs, const double *raw, const double *bas,
                                          const double *coef, double *slab, bool *slab_kept, int nchunk, double *part, long ldp,
                                          const double *hd, long ldh, const double *bvec, double *out) {
    return nmcov_launch_pairs<PcmKernels>(st, Xc, Psio, ldx, n, Pio, ldr, m, d, k, obs, raw, bas, coef, slab, slab_kept, nchunk, part, ldp,
                                          hd, ldh, bvec, out);
}
