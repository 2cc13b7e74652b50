// gamma under every weight draw for rows with missing inputs (gpz_predictor_stack_missing_dev / _draws_gamma_missing_dev, gpz_predictor.hip):
// gamma_s,i = sum_{a >= b} f_ab EcC_ab(x_i) w_s,a w_s,b - mu_s,i^2 per output, predictMissing's gamma (predictDiag.m:172-198, :209) with the
// draw's weights in place of w; f_ab = 2 off the diagonal, 1 on it.  One tile of ONE group of rows that share a NaN pattern.
//
//   k_predict_missing_gamma   Two MFMAs chained: the clean z and the gamma sink of k_predict_group_impl.h, where the layout is described
//                             once.  Up to GPZ_MGAMMA_NB = 8 column blocks (128 columns, 128 accumulator registers) per launch, the
//                             kernel instantiated for every count 1 .. 8 (a count read at run time kept one test per block in scalar
//                             registers and spilled them); more columns are further launches that form z again.  gridDim.y:
//                             predict_missing_chunks(m) chunks of the groups, into part [C][ncol][ldp].
//                             LDS: max(32 (nk + 2) + 64 (1 + 2 d) + 32 d + 64, 2048) doubles (predict_missing_gamma_lds).
//                             k_predict_noisy_missing_gamma<NB> (k_predict_noisy_missing_gamma.hip, rows with Psi too) is launched
//                             from here as well.
//   k_gamma_finish_dev / _s2  (k_predict_noisy_gamma.hip) add the chunks in chunk order and subtract mu_s^2.
// No atomics; every sum starts from zero and runs in one order that the model's shape fixes (the pairs of a wave's blocks in table order,
// the waves in wave order, the chunks in chunk order): a row's gamma_s has the same bits for any tile size, row order, position in its
// block, other rows or groups of the call and any number of draws > s.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_predict_group_impl.h"

#define GPZ_MGAMMA_NB 8   // most 16-column blocks of accumulators per launch

template <int NB>
__global__ __launch_bounds__(256, 2) void k_predict_missing_gamma(PredGroupArgs a) {
    predict_group_body<false, PredGammaSink<NB>>(a);
}

// dynamic LDS of the gamma kernels, bytes: the Pio block, [lnZ | c | 1 / C or C] of a group's 64 records, the block's rows of X and, with
// psi, of Psi, the group's (a, b)
size_t predict_missing_gamma_lds(int m, int d, bool psi) {
    const size_t nk = ((size_t)m + 15) / 16 * 16;
    const size_t work = psi ? 32 * (nk + 2) + 64 * (1 + 2 * (size_t)d) + 64 * (size_t)d + 64
                            : 32 * (nk + 2) + 64 * (1 + 2 * (size_t)d) + 32 * (size_t)d + 64;
    const size_t red = 4 * 32 * 16;
    return (work > red ? work : red) * sizeof(double);
}

// the kernel for nb column blocks, with Psi or without
template <int NBT>
static int launch_gamma_nb(bool psi, hipStream_t st, dim3 grid, size_t lds, const PredGroupArgs &a) {
    return psi ? launch_predict_group<k_predict_noisy_missing_gamma<NBT>>(st, grid, lds, a)
               : launch_predict_group<k_predict_missing_gamma<NBT>>(st, grid, lds, a);
}

int launch_predict_missing_gamma(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio, int ldpio, int m,
                                 int d, int k, unsigned obs, const double *U, const double *rec, const double *W, int ldw, int ncol,
                                 int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > 20 || k < 1 || k > 8 || m < 1 || ((m + 15) / 16) * 16 > 256 || nchunk != predict_missing_chunks(m) || ldw % 16 ||
        ncol > ldw || ldp < n)
        return -1;
    PredGroupArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.Pio = Pio; a.ldpio = ldpio; a.nk = ((m + 15) / 16) * 16; a.U = U; a.rec = rec;
    a.nrec = predict_missing_rec(d, k); a.d = d; a.k = k; a.obs = obs;
    a.npair = m * (m + 1) / 2;
    a.ngrp = (int)predict_missing_groups(m);
    a.gpc = (a.ngrp + nchunk - 1) / nchunk;
    a.W = W; a.ldw = ldw; a.ncol = ncol;
    a.part = part; a.ldp = ldp;
    const bool psi = Psic != nullptr;
    const size_t lds = predict_missing_gamma_lds(m, d, psi);
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)nchunk);
    const int nbw = (ncol + 15) / 16;   // <= ldw / 16
    // GPZ_MGAMMA_NB blocks per launch and the rest in a last one, each instantiated for its count: no test per block in the kernel
    for (a.cb0 = 0; a.cb0 < nbw; a.cb0 += GPZ_MGAMMA_NB) {
        int rc = -1;
        switch (nbw - a.cb0 < GPZ_MGAMMA_NB ? nbw - a.cb0 : GPZ_MGAMMA_NB) {
            case 1: rc = launch_gamma_nb<1>(psi, st, grid, lds, a); break;
            case 2: rc = launch_gamma_nb<2>(psi, st, grid, lds, a); break;
            case 3: rc = launch_gamma_nb<3>(psi, st, grid, lds, a); break;
            case 4: rc = launch_gamma_nb<4>(psi, st, grid, lds, a); break;
            case 5: rc = launch_gamma_nb<5>(psi, st, grid, lds, a); break;
            case 6: rc = launch_gamma_nb<6>(psi, st, grid, lds, a); break;
            case 7: rc = launch_gamma_nb<7>(psi, st, grid, lds, a); break;
            case 8: rc = launch_gamma_nb<8>(psi, st, grid, lds, a); break;
        }
        if (rc) return -1;
    }
    return 0;
}
