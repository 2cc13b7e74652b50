// gamma under every weight draw for rows with a full input-noise covariance on a covariance kind (gpz_predictor_stack_psi_cube_dev /
// _draws_gamma_psi_cube_dev, gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab z_ab(x_i, Psi_i) w_s,a w_s,b - mu_s,i^2 per output,
// predictNoisy's gamma of GC and VC (predictCov.m:105-119) with the draw's weights in place of w.
//
//   k_predict_psi_cube_gamma<D, SHARED>
//       predict_gamma_body (k_predict_gamma_impl.h: the f64 MFMA product of pair densities and weight products, its LDS stages, chunks
//       and passes) with GammaNcov<PsiTri<D>, SHARED, pcg_blocks(D)> (k_ncov_density.h): k_predict_noisy_cov_gamma's policy with
//       M = C_ab + Psi_i over the whole packed triangle, the density of k_predict_psi_cube_small.  The row's triangle is the
//       d (d + 1) / 2 columns of the tile's Psic at the lane's row, which the body loads into registers.
//       pcg_blocks(D) 16-column blocks of accumulators per pass.
// k_gamma_finish_dev / k_gamma_finish_s2 (k_predict_noisy_gamma.hip) add the chunks and take mu_s^2 off.  The chunk count is the
// caller's predict_gamma_chunks(m).
#include "k_predict_gamma_impl.h"
#include "k_ncov_density.h"   // GammaNcov, PsiTri

// 16-column blocks of accumulators per pass: 8 (128 columns) up to d = 6, then 4 - one width earlier than k_predict_noisy_cov_gamma,
// so that d = 7 with the row's triangle beside M stays within 256 registers (two workgroups per compute unit)
constexpr int pcg_blocks(int d) { return d <= 6 ? 8 : 4; }

template <int D, bool SHARED>
__global__ __launch_bounds__(256) void k_predict_psi_cube_gamma(PredGammaArgs a) {
    predict_gamma_body<GammaNcov<PsiTri<D>, SHARED, pcg_blocks(D)>>(a);
}

template <int D>
static void launch_pcg(hipStream_t st, const PredGammaArgs &a, int nchunk, bool shared) {
    const dim3 grid = predict_gamma_grid(a, nchunk, pcg_blocks(D));
    if (shared) hipLaunchKernelGGL((k_predict_psi_cube_gamma<D, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_predict_psi_cube_gamma<D, false>), grid, dim3(256), 0, st, a);
}

int launch_predict_psi_cube_gamma(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m,
                                  const double *tab, int rec, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > 10 || m < 1 || nchunk < 1 || ldw % 16 || ncol > ldw || rec < 1 + d + d * (d + 1) / 2 || ldp < n || ldx < n) return -1;
    const PredGammaArgs a = predict_gamma_args(Xc, Psic, ldx, n, m, tab, rec, W, ldw, ncol, nchunk, part, ldp);
    switch (d) {
#define PCG_CASE(DD) case DD: launch_pcg<DD>(st, a, nchunk, shared); break;
        PCG_CASE(1) PCG_CASE(2) PCG_CASE(3) PCG_CASE(4) PCG_CASE(5) PCG_CASE(6) PCG_CASE(7) PCG_CASE(8) PCG_CASE(9) PCG_CASE(10)
#undef PCG_CASE
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
