// gamma under every weight draw for one group of rows with missing inputs past ceil16(m) = 256 (a handle with
// GPZ_PREDICT_LARGE_M_MISSING; gpz_predictor_stack_missing_dev / _draws_gamma_missing_dev and their noisy_missing twins): what
// k_predict_missing_gamma<NB> and k_predict_noisy_missing_gamma<NB> compute, on the same tables and into the same slab
// part [predict_missing_chunks(m)][ncol][ldp], which k_gamma_finish_dev / _s2 add in chunk order.
//
//   k_pml_gamma<NB>       Two MFMAs chained: the clean z and the gamma sink on predict_group_large_body (k_predict_group_large_impl.h).
//                         The batch's accumulators take 64 registers that the other body does not hold, so a launch carries at most
//                         GPZ_PML_GAMMA_NB = 4 column blocks (64 columns, 64 accumulator registers) where k_predict_missing_gamma
//                         carries 8: the two together are what that kernel's 8 blocks are.  More columns are further launches that
//                         form z again.  Instantiated for every count 1 .. 4.
//   k_pml_gamma_psi<NB>   the z with Psi, on the second record table ([lnZ | c | C]).
// LDS: (32 (128 + 2) + 64 (1 + 2 d) + 32 d, with Psi 64 d, + 64) doubles, the same for every m (predict_missing_large_lds with gamma).
// No atomics; every sum starts from zero and runs in one order that the model's shape fixes: a row's gamma_s has the same bits for any
// tile size, row order, position in its block, other rows or groups of the call and any number of draws > s.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_predict_group_large_impl.h"

#define GPZ_PML_GAMMA_NB 4   // most 16-column blocks of accumulators per launch

template <int NB>
__global__ __launch_bounds__(256, 2) void k_pml_gamma(PredGroupArgs a) {
    predict_group_large_body<false, PredGammaSink<NB>, GPZ_PML_GB>(a);
}
template __global__ void k_pml_gamma<1>(PredGroupArgs);
template __global__ void k_pml_gamma<2>(PredGroupArgs);
template __global__ void k_pml_gamma<3>(PredGroupArgs);
template __global__ void k_pml_gamma<4>(PredGroupArgs);

template <int NB>
__global__ __launch_bounds__(256, 2) void k_pml_gamma_psi(PredGroupArgs a) {
    predict_group_large_body<true, PredGammaSink<NB>, GPZ_PML_GB>(a);
}
template __global__ void k_pml_gamma_psi<1>(PredGroupArgs);
template __global__ void k_pml_gamma_psi<2>(PredGroupArgs);
template __global__ void k_pml_gamma_psi<3>(PredGroupArgs);
template __global__ void k_pml_gamma_psi<4>(PredGroupArgs);

// the kernel for nb column blocks, with Psi or without
template <int NBT>
static int launch_pml_gamma_nb(bool psi, hipStream_t st, dim3 grid, size_t lds, const PredGroupArgs &a) {
    return psi ? launch_predict_group<k_pml_gamma_psi<NBT>>(st, grid, lds, a) : launch_predict_group<k_pml_gamma<NBT>>(st, grid, lds, a);
}

int launch_predict_missing_large_gamma(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio, int ldpio,
                                       int m, int d, int k, unsigned obs, const double *U, const double *rec, const double *W, int ldw,
                                       int ncol, int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    const int nk = ((m + 15) / 16) * 16;
    // (m - 1) ldw + ldw <= 1024 * 2^20 stays an int in the sink's row offsets into W
    if (d < 1 || d > 20 || k < 1 || k > 8 || m < 1 || nk > GPZ_PREDICT_LARGE_M_MAX || ldpio < nk || nchunk != predict_missing_chunks(m) ||
        ldw % 16 || ldw > (1 << 20) || ncol > ldw || ldp < n || (Psic && (obs >> d)))
        return -1;
    PredGroupArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.Pio = Pio; a.ldpio = ldpio; a.nk = nk; a.U = U; a.rec = rec;
    a.nrec = predict_missing_rec(d, k); a.d = d; a.k = k; a.obs = obs;
    a.npair = m * (m + 1) / 2;   // 524 800 at m = 1024
    a.ngrp = (int)predict_missing_groups(m);
    a.gpc = (a.ngrp + nchunk - 1) / nchunk;
    a.W = W; a.ldw = ldw; a.ncol = ncol;
    a.part = part; a.ldp = ldp;
    const bool psi = Psic != nullptr;
    const size_t lds = predict_missing_large_lds(m, d, k, psi, true);
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)nchunk);
    const int nbw = (ncol + 15) / 16;   // <= ldw / 16
    // GPZ_PML_GAMMA_NB blocks per launch and the rest in a last one, each instantiated for its count: no test per block in the kernel
    for (a.cb0 = 0; a.cb0 < nbw; a.cb0 += GPZ_PML_GAMMA_NB) {
        int rc = -1;
        switch (nbw - a.cb0 < GPZ_PML_GAMMA_NB ? nbw - a.cb0 : GPZ_PML_GAMMA_NB) {
            case 1: rc = launch_pml_gamma_nb<1>(psi, st, grid, lds, a); break;
            case 2: rc = launch_pml_gamma_nb<2>(psi, st, grid, lds, a); break;
            case 3: rc = launch_pml_gamma_nb<3>(psi, st, grid, lds, a); break;
            case 4: rc = launch_pml_gamma_nb<4>(psi, st, grid, lds, a); break;
        }
        if (rc) return -1;
    }
    return 0;
}
