// gamma under every weight draw for rows with both input noise and missing inputs (gpz_predictor_stack_noisy_missing_dev /
// _draws_gamma_noisy_missing_dev, gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab EcC_ab(x_i, psi_i) w_s,a w_s,b - mu_s,i^2 per output,
// predictNoisyMissing's gamma (predictDiag.m:257-295) with the draw's weights in place of w; f_ab = 2 off the diagonal, 1 on it.  One tile
// of ONE group of rows that share a NaN pattern, each row with a variance psi per input dimension (Psic, in the layout of Xc).
//
//   k_predict_noisy_missing_gamma   Two MFMAs chained: the z with Psi and the gamma sink of k_predict_group_impl.h, where the layout is
//                             described once.  Of a record of the SECOND table (k_pnm_records: C, not 1 / C, and lnZ without the
//                             determinant) only [lnZ | c | C] is staged.  Instantiated for every count of column blocks 1 .. 8: the
//                             rsqrt chains of the epilogue end before the second product begins, so all eight fit two workgroups per
//                             compute unit without a spill (118 .. 244 VGPRs).  Launched by
//                             launch_predict_missing_gamma (k_predict_missing_gamma.hip) when it is given Psic.
//                             LDS: max(32 (nk + 2) + 64 (1 + 2 d) + 64 d + 64, 2048) doubles (predict_missing_gamma_lds with psi).
//   k_gamma_finish_dev / _s2  (k_predict_noisy_gamma.hip) add the chunks in chunk order and subtract mu_s^2.
// No atomics; every sum starts from zero and runs in one order that the model's shape fixes: a row's gamma_s has the same bits for any
// tile size, row order, position in its block, other rows or groups of the call and any number of draws > s.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_predict_group_impl.h"

template <int NB>
__global__ __launch_bounds__(256, 2) void k_predict_noisy_missing_gamma(PredGroupArgs a) {
    predict_group_body<true, PredGammaSink<NB>>(a);
}
template __global__ void k_predict_noisy_missing_gamma<1>(PredGroupArgs);
template __global__ void k_predict_noisy_missing_gamma<2>(PredGroupArgs);
template __global__ void k_predict_noisy_missing_gamma<3>(PredGroupArgs);
template __global__ void k_predict_noisy_missing_gamma<4>(PredGroupArgs);
template __global__ void k_predict_noisy_missing_gamma<5>(PredGroupArgs);
template __global__ void k_predict_noisy_missing_gamma<6>(PredGroupArgs);
template __global__ void k_predict_noisy_missing_gamma<7>(PredGroupArgs);
template __global__ void k_predict_noisy_missing_gamma<8>(PredGroupArgs);
