// Rows with both input noise and missing inputs through the streaming predictor (gpz_predictor_run_noisy_missing_dev /
// _draws_noisy_missing_dev, gpz_predictor.hip): predictNoisyMissing of the diagonal kinds (predictDiag.m:211-297) for one tile of ONE
// group of rows that share a NaN pattern, each row with a variance psi per input dimension (Psic, in the layout of Xc, as
// k_pred_stage_psi left it).  obs is the bit mask of the observed dimensions, uniform over every launch.  Psi touches the observed
// dimensions only: NijS, the priors and U(q, l) = Nu_q(l) are k_predict_missing.hip's tables of the pattern, reused as built; No widens by
// psi, and the pair density over the observed dimensions becomes N(x_o; c_q,o, C_q,o + psi_o), k_predict_noisy_small's per-row form.
// Every loop over the dimensions here runs over the set bits of obs: no NaN of X and no value of Psi from a missing dimension enters
// arithmetic, whatever it holds.
//
// Per handle, once (the model's alone: the pattern enters through the loops, not through the table):
//   k_pnm_records  the second pair-record table [lnZ_q | c_q (d) | C_q (d) | per output f w_i w_j, f v_i v_j, f iS(i, j)] for
//                  q = i (i + 1) / 2 + j, j <= i, f = 2 off the diagonal and 1 on it (:277-284), iS read at i >= j only as the reference
//                  does.  lnZ_q = lnz_i + lnz_j - 1/2 sum (p_i - p_j)^2 / (sigma_i + sigma_j) - 1/2 sum ln(sigma_i + sigma_j) (:275)
//                  comes WITHOUT the -1/2 sum_o ln C_q of k_pmd_pairs: with psi the determinant depends on the row.  c_q and C_q (not
//                  1 / C_q) are stored for every dimension.  Records past the last pair are zero with C_q = 1; predict_missing_rec(d, k)
//                  doubles each, whole groups of 64.
// Per tile, on Xc and Psic [d][ldx]:
//   launch_pmd_no (k_pnm_no, k_predict_missing.hip), launch_tgemm, k_pmd_phi: No widened by psi, then as for a group without noise
//                  (T = Pio NijS, PHI = No o T, mu, ElnS - b)                                                                  :227-250
//   k_predict_noisy_missing_pairs<KM>   the hot one (:257-285): the z with Psi and the pairs sink of k_predict_group_impl.h, where the
//                  layout is described once; k_predict_missing_pairs' in everything that sets the accumulator layout.  Launched by
//                  launch_predict_missing_pairs (k_predict_missing.hip) when it is given Psic.
//                  LDS: (32 (nk + 2) + 64 (1 + 2 d + 3 k) + 64 d) doubles - the block's rows of X and of Psi - at least 4 * 32 * 3 KM for
//                  the last reduction.
//   launch_pmd_finish                             the chunks in chunk order -> out [4k][nt] = mu | nu | beta | gamma                   :289-295
//   launch_pnm_check_psi (k_predict_noisy.hip)    word 3 of the device entries' record is set when Psi is NaN, negative or infinite in an
//                  OBSERVED dimension.
// A row's results depend on its own values and the model only: the same bits for any tile size, position in the block and row order.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_predict_group_impl.h"

// one thread per pair of the padded table (npad = whole groups of 64); G2: gamma^2 = 1 / sigma, m x de row-major
__global__ __launch_bounds__(256) void k_pnm_records(long npair, long npad, int m, int d, int de, int k, const double *__restrict__ P,
                                                     const double *__restrict__ G2, const double *__restrict__ w,
                                                     const double *__restrict__ v, const double *__restrict__ iS, double *__restrict__ rec,
                                                     int nrec) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= npad) return;
    double *r = rec + (size_t)q * nrec;
    if (q >= npair) {
        for (int e = 0; e < nrec; ++e) r[e] = (e > d && e <= 2 * d) ? 1.0 : 0.0;
        return;
    }
    int i, j;
    gpz_pair_of(q, &i, &j);
    double lz = 0.0, qd = 0.0, ls = 0.0;
    for (int c = 0; c < d; ++c) {
        const double isi = G2[(size_t)i * de + c], isj = G2[(size_t)j * de + c];
        const double C = 1.0 / (isi + isj);                                                      // :260
        const double cv = (P[(size_t)i * de + c] * isi + P[(size_t)j * de + c] * isj) * C;       // :261
        lz += log(isi) + log(isj);
        const double s = 1.0 / isi + 1.0 / isj, dl = P[(size_t)i * de + c] - P[(size_t)j * de + c];
        qd += dl * dl / s;
        ls += log(s);
        r[1 + c] = cv;
        r[1 + d + c] = C;
    }
    r[0] = -0.5 * lz - 0.5 * qd - 0.5 * ls;                                                      // :275, the row-free part
    gpz_pair_coef(r + 1 + 2 * d, i, j, m, k, w, v, iS);
}

template <int KM>
__global__ __launch_bounds__(256, 2) void k_predict_noisy_missing_pairs(PredGroupArgs a) {
    predict_group_body<true, PredPairsSink<KM>>(a);
}
template __global__ void k_predict_noisy_missing_pairs<1>(PredGroupArgs);
template __global__ void k_predict_noisy_missing_pairs<8>(PredGroupArgs);

int launch_pnm_records(hipStream_t st, int m, int d, int de, int k, const double *P, const double *G2, const double *w, const double *v,
                       const double *iS, double *rec) {
    const long npair = (long)m * (m + 1) / 2, npad = predict_missing_groups(m) * 64;
    hipLaunchKernelGGL(k_pnm_records, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, npair, npad, m, d, de, k, P, G2, w, v, iS, rec,
                       predict_missing_rec(d, k));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
