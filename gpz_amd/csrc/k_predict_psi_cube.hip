// Rows with a full input-noise covariance through the streaming predictor, covariance kinds (gpz_predictor_run_psi_cube_dev /
// _draws_psi_cube_dev, gpz_predictor.hip): predictNoisy of GC and VC (predictCov.m:70-132) with Psi(:, :, i) as fixPsi.m:36 leaves it,
// the d x d x n cube divided by sdX' sdX.  The tile's Psi slot is Psic [d (d + 1) / 2][ldx], column q = LT(r, c) the element (r, c),
// r >= c, of every row's matrix, so that a lane's reads are coalesced as they are for Xc.  Only the lower triangle of a row's matrix is
// ever read.
//
//   k_pred_check_psi_cube           word 3 of the device entries' record is set when an element of a row's lower triangle is NaN or
//                                   infinite, itself or after its division, or a diagonal element is negative
//   k_pred_stage_psi_cube<T>        the caller's cube (f64 or f32; element (r, c) of row i at Psi[r sr + c sc + i sn]) ->
//                                   Psic [d (d + 1) / 2][ldx] = double(psi) / div[LT(r, c)], a plain f64 division (fixPsi.m:36)
//   k_predict_psi_cube_small<D, SHARED, KM>   predict_ncov_small_body (k_predict_ncov_impl.h: the frame, the records, the chunks and
//   k_predict_psi_cube_phi<D, SHARED>         the order of every sum, k_predict_noisy_cov.hip's) and predict_ncov_phi_body with
//                                             PsiTri<D>: M = S + Psi_i over the whole packed triangle
// The chunk count comes from the caller: predict_noisy_cov_chunks(m, d, k) of k_predict_noisy_cov.hip.
#include "k_predict_ncov_impl.h"

template <int D, bool SHARED, int KM>
__global__ __launch_bounds__(256) void k_predict_psi_cube_small(PredNcovArgs a) {
    predict_ncov_small_body<PsiTri<D>, SHARED, KM>(a);
}

template <int D, bool SHARED>
__global__ __launch_bounds__(256) void k_predict_psi_cube_phi(PredNcovArgs a) {
    predict_ncov_phi_body<PsiTri<D>, SHARED>(a);
}

// ---- byte movers of the device entries ----------------------------------------------------------------------------------------------
// np = d (d + 1) / 2 elements per row, element q = LT(r, c).  div: the divisors sdX[r] sdX[c] in LT order on the device (nullptr: none)
__global__ __launch_bounds__(256) void k_pred_check_psi_cube(const void *__restrict__ Psi, int f32, long ns, int np, long sr, long sc,
                                                             long sn, const double *__restrict__ div, unsigned *__restrict__ rec) {
    const long ne = ns * np, step = (long)gridDim.x * 256;
    int bad = 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < ne; e += step) {
        const int q = (int)(e / ns);          // rows fastest: a contiguous d x d x n cube is read coalesced
        const long i = e - (long)q * ns;
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= q) ++r;
        const int c = q - r * (r + 1) / 2;
        const long at = r * sr + c * sc + i * sn;
        const double v = f32 ? (double)((const float *)Psi)[at] : ((const double *)Psi)[at];
        const double w = div ? v / div[q] : v;
        bad |= !(fabs(v) <= 1.7976931348623157e308) || !(fabs(w) <= 1.7976931348623157e308) || (r == c && !(v >= 0.0));
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(rec + 3, 1u);
}

template <typename T>
__global__ __launch_bounds__(256) void k_pred_stage_psi_cube(const T *__restrict__ Psi, long sr, long sc, long sn, long r0, int nt, int d,
                                                             const double *__restrict__ div, double *__restrict__ Psic, long ldx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const T *row = Psi + (r0 + i) * sn;
    for (int r = 0; r < d; ++r)
        for (int c = 0; c <= r; ++c) {
            double v = (double)row[r * sr + c * sc];
            if (div) v = v / div[LT(r, c)];                                  // Psi ./ (sdX' sdX)        fixPsi.m:36
            Psic[(size_t)LT(r, c) * ldx + i] = v;
        }
}

int launch_pred_check_psi_cube(hipStream_t st, const void *Psi, int f32, long ns, int d, long sr, long sc, long sn, const double *div,
                               unsigned *rec) {
    if (ns <= 0) return 0;
    const int np = d * (d + 1) / 2;
    long nb = (ns * np + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_pred_check_psi_cube, dim3((unsigned)nb), dim3(256), 0, st, Psi, f32, ns, np, sr, sc, sn, div, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pred_stage_psi_cube(hipStream_t st, const void *Psi, int f32, long sr, long sc, long sn, long r0, int nt, int d,
                               const double *div, double *Psic, long ldx) {
    if (nt <= 0) return 0;
    const dim3 grid((unsigned)((nt + 255) / 256));
    if (f32)
        hipLaunchKernelGGL(k_pred_stage_psi_cube<float>, grid, dim3(256), 0, st, (const float *)Psi, sr, sc, sn, r0, nt, d, div, Psic, ldx);
    else
        hipLaunchKernelGGL(k_pred_stage_psi_cube<double>, grid, dim3(256), 0, st, (const double *)Psi, sr, sc, sn, r0, nt, d, div, Psic,
                           ldx);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

struct PsiCubeKernels {
    template <int D, bool SHARED, int KM> static auto small() { return k_predict_psi_cube_small<D, SHARED, KM>; }
    template <int D, bool SHARED> static auto phi() { return k_predict_psi_cube_phi<D, SHARED>; }
};

int launch_predict_psi_cube_small(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m, int k,
                                  const double *brec, const double *prec, const double *bvec, int nchunk, double *part, long ldp,
                                  double *out) {
    return predict_ncov_launch_small<PsiCubeKernels>(st, d, shared, Xc, Psic, ldx, n, m, k, brec, prec, bvec, nchunk, part, ldp, out);
}

int launch_predict_psi_cube_phi(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m,
                                int mp, int k, const double *brec, int nchunk, double *Phi) {
    return predict_ncov_launch_phi<PsiCubeKernels>(st, d, shared, Xc, Psic, ldx, n, nrow, m, mp, k, brec, nchunk, Phi);
}
