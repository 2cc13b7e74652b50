// gamma under every weight draw for rows with input noise AND missing inputs on a covariance kind (gpz_predictor_stack_noisy_missing_cov_dev /
// _draws_gamma_noisy_missing_cov_dev, gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab z_ab(x_i, psi_i) w_s,a w_s,b - mu_s,i^2 per output,
// predictNoisyMissing's gamma of GC and VC (predictCov.m:233-337) with the draw's weights in place of w.  One tile of ONE group of rows
// that share a NaN pattern and carry a variance psi per observed input.  z_ab(x, psi) = sum_l Pio_l(x, psi) N(record_abl; x_o, psi_o) is
// the pair quantity of k_predict_noisy_missing_cov_pairs, from the same slab records (k_predict_noisy_missing_cov.hip, where they are
// described) and the tile's Pio.
//
//   k_predict_noisy_missing_cov_gamma<NO>   nmcov_gamma_body<PsiDiag<NO>, nmcg_nb(NO)> of k_predict_nmcov_impl.h, where the frame, the
//       LDS and what keeps the kernel from faulting are written; one instantiation per NO: 9 kernels.  x_o and psi_o of the observed
//       dimensions stay in registers (Psi of a missing dimension is never loaded).
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_predict_nmcov_impl.h"

// most 16-column blocks of accumulators per pass and the workgroups per compute unit the registers are bounded for, by the observed
// dimensions alone: 8 blocks (128 columns) under 256 registers up to NO = 6; NO = 7 fits 256 registers with 4 blocks (the usual 64
// draws of one output are one pass still); NO = 8 and 9 take one workgroup per compute unit (up to 512 registers: the packed factor of
// M + diag(psi) alone is 36 and 45 doubles), which LDS allows them from about m = 112 anyway, and 8 blocks
constexpr int nmcg_nb(int no) { return no == 7 ? 4 : 8; }
constexpr int nmcg_wg(int no) { return no <= 7 ? 2 : 1; }

template <int NO>
__global__ __launch_bounds__(256, nmcg_wg(NO)) void k_predict_noisy_missing_cov_gamma(PredNmcovGammaArgs a) {
    nmcov_gamma_body<PsiDiag<NO>, nmcg_nb(NO)>(a);
}

struct NmcgKernels {
    template <int NO> static auto gamma() { return k_predict_noisy_missing_cov_gamma<NO>; }
    static constexpr int nb(int no) { return nmcg_nb(no); }
};

// dynamic LDS of the gamma kernel of either form, bytes: the Pio block and the stages of four pair slots.  m, d and no alone.
size_t predict_noisy_missing_cov_gamma_lds(int m, int d, int no) {
    return ((size_t)m * 64 + 4 * (size_t)nmcg_stride(predict_noisy_missing_cov_rec(d, no))) * sizeof(double);
}

int launch_predict_noisy_missing_cov_gamma(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio,
                                           long ldr, int m, int d, unsigned obs, const double *raw, const double *bas, double *slab,
                                           bool *slab_kept, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp) {
    return nmcov_launch_gamma<NmcgKernels>(st, Xc, Psic, ldx, n, Pio, ldr, m, d, obs, raw, bas, slab, slab_kept, W, ldw, ncol, nchunk, part,
                                           ldp);
}
