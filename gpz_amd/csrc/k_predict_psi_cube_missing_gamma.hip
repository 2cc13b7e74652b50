// gamma under every weight draw for rows with a full input-noise covariance AND missing inputs on a covariance kind
// (gpz_predictor_stack_psi_cube_missing_dev / _draws_gamma_psi_cube_missing_dev, gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab
// z_ab(x_i, Psi_i) w_s,a w_s,b - mu_s,i^2 per output, predictNoisyMissing's gamma of GC and VC (predictCov.m:233-337) with the draw's
// weights in place of w.  One tile of ONE group of rows that share a NaN pattern and carry a d x d matrix Psi each; z_ab is the pair
// quantity of k_predict_psi_cube_missing_pairs, from the same slab records (k_predict_noisy_missing_cov.hip, where they are described)
// and the tile's Pio, on the observed triangle Psio [no (no + 1) / 2][ldx] (k_predict_psi_cube_missing.hip stages it).
//
//   k_predict_psi_cube_missing_gamma<NO>   nmcov_gamma_body<PsiTri<NO>, pcmg_nb(NO)> of k_predict_nmcov_impl.h, where the frame, the
//       LDS (the twin's: predict_noisy_missing_cov_gamma_lds(m, d, no), the triangle lives in registers) and what keeps the kernel
//       from faulting are written; one instantiation per NO: 9 kernels.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_predict_nmcov_impl.h"

// most 16-column blocks of accumulators per pass and the workgroups per compute unit the registers are bounded for, by the observed
// dimensions alone.  The triangle adds no (no - 1) / 2 doubles to the twin's registers: 8 blocks under 256 registers up to NO = 5;
// NO = 6 fits 256 registers with 4 blocks (the usual 64 draws of one output are one pass still); NO = 7, 8 and 9 take one workgroup
// per compute unit (up to 512 registers) and 8 blocks.  DESIGN.md section 34 has the compile report behind this.
constexpr int pcmg_nb(int no) { return no == 6 ? 4 : 8; }
constexpr int pcmg_wg(int no) { return no <= 6 ? 2 : 1; }

template <int NO>
__global__ __launch_bounds__(256, pcmg_wg(NO)) void k_predict_psi_cube_missing_gamma(PredNmcovGammaArgs a) {
    nmcov_gamma_body<PsiTri<NO>, pcmg_nb(NO)>(a);
}

struct PcmgKernels {
    template <int NO> static auto gamma() { return k_predict_psi_cube_missing_gamma<NO>; }
    static constexpr int nb(int no) { return pcmg_nb(no); }
};

int launch_predict_psi_cube_missing_gamma(hipStream_t st, const double *Xc, const double *Psio, long ldx, int n, const double *Pio,
                                          long ldr, int m, int d, unsigned obs, const double *raw, const double *bas, double *slab,
                                          bool *slab_kept, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp) {
    return nmcov_launch_gamma<PcmgKernels>(st, Xc, Psio, ldx, n, Pio, ldr, m, d, obs, raw, bas, slab, slab_kept, W, ldw, ncol, nchunk, part,
                                           ldp);
}
