// gamma under every weight draw for rows with input noise on a covariance kind (gpz_predictor_stack_noisy_cov_dev /
// _draws_gamma_noisy_cov_dev, gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab z_ab(x_i, psi_i) w_s,a w_s,b - mu_s,i^2 per output,
// predictNoisy's gamma of GC and VC (predictCov.m:105-119) with the draw's weights in place of w; f_ab = 2 off the diagonal, 1 on it.
//
//   k_predict_noisy_cov_gamma<D, SHARED>
//       predict_gamma_body (k_predict_gamma_impl.h: k_predict_noisy_gamma's frame, the f64 MFMA product of pair densities and weight
//       products, its LDS stages, chunks and passes) with GammaNcov<PsiDiag<D>, SHARED, ncg_blocks(D)> (k_ncov_density.h).  The density
//       is k_predict_noisy_cov_small's: the packed Cholesky of C_ab + diag(psi_i) and a forward substitution,
//       z = exp(lnZ - 1/2 q) prod(1 / L_cc), from the record head [lnZ | c_ab | C_ab packed lower], the first 1 + d + d (d + 1) / 2
//       doubles of the handle's packed pair records.
//       ncg_blocks(D) 16-column blocks of accumulators per pass: 8 (128 columns) for d <= 7, 4 for d >= 8, where the packed triangle
//       leaves the accumulators less room.
// k_gamma_finish_dev / k_gamma_finish_s2 (k_predict_noisy_gamma.hip) add the chunks and take mu_s^2 off.
#include "k_predict_gamma_impl.h"
#include "k_ncov_density.h"   // GammaNcov, PsiDiag

// 16-column blocks of accumulators per pass
constexpr int ncg_blocks(int d) { return d <= 7 ? 8 : 4; }

// D = 9 is held to 256 registers (two workgroups per compute unit) by the second launch bound: left alone it takes 252 (VC) and 258
// (GC).  D = 10 does not fit 256 without scratch and keeps one workgroup per compute unit.
template <int D, bool SHARED>
__global__ __launch_bounds__(256, D == 9 ? 2 : 1) void k_predict_noisy_cov_gamma(PredGammaArgs a) {
    predict_gamma_body<GammaNcov<PsiDiag<D>, SHARED, ncg_blocks(D)>>(a);
}

template <int D>
static void launch_ncg(hipStream_t st, const PredGammaArgs &a, int nchunk, bool shared) {
    const dim3 grid = predict_gamma_grid(a, nchunk, ncg_blocks(D));
    if (shared) hipLaunchKernelGGL((k_predict_noisy_cov_gamma<D, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_predict_noisy_cov_gamma<D, false>), grid, dim3(256), 0, st, a);
}

int launch_predict_noisy_cov_gamma(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m,
                                   const double *tab, int rec, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > 10 || m < 1 || nchunk < 1 || ldw % 16 || ncol > ldw || rec < 1 + d + d * (d + 1) / 2 || ldp < n) return -1;
    const PredGammaArgs a = predict_gamma_args(Xc, Psic, ldx, n, m, tab, rec, W, ldw, ncol, nchunk, part, ldp);
    switch (d) {
#define NCG_CASE(DD) case DD: launch_ncg<DD>(st, a, nchunk, shared); break;
        NCG_CASE(1) NCG_CASE(2) NCG_CASE(3) NCG_CASE(4) NCG_CASE(5) NCG_CASE(6) NCG_CASE(7) NCG_CASE(8) NCG_CASE(9) NCG_CASE(10)
#undef NCG_CASE
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
