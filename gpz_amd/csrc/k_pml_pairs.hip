// The moments' pair sums of one group of rows with missing inputs past ceil16(m) = 256 (a handle with GPZ_PREDICT_LARGE_M_MISSING;
// gpz_predictor_run_missing_dev / _run_noisy_missing_dev and the stacks' column 0, gpz_predictor.hip): what k_predict_missing_pairs<KM>
// and k_predict_noisy_missing_pairs<KM> compute, on the same tables of the pattern (k_pmd_pairs / k_pnm_records, k_pmd_u) and into the
// same slab part [predict_missing_chunks(m)][3k][ldp], which k_pmd_finish adds in chunk order.
//
//   k_pml_pairs<KM>       the clean z and the pairs sink on predict_group_large_body (k_predict_group_large_impl.h, where the K panels
//                         and the batch of groups are described once).  KM = 1 or 8 outputs in registers, in batches of
//                         GPZ_PML_GB = 4 and GPZ_PML_GB8 = 2 groups.
//   k_pml_pairs_psi<KM>   the z with Psi, on the second record table.
// LDS: (32 (128 + 2) + 64 (1 + 2 d + 3 k) + 32 d, with Psi 64 d) doubles, the same for every m (predict_missing_large_lds); above 64 KB
// the launch opts in (launch_predict_group).
// A row's results depend on its own values and the model only: the same bits for any tile size, position in the block and row order.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_predict_group_large_impl.h"

template <int KM>
__global__ __launch_bounds__(256, 2) void k_pml_pairs(PredGroupArgs a) {
    predict_group_large_body<false, PredPairsSink<KM>, KM == 1 ? GPZ_PML_GB : GPZ_PML_GB8>(a);
}
template __global__ void k_pml_pairs<1>(PredGroupArgs);
template __global__ void k_pml_pairs<8>(PredGroupArgs);

template <int KM>
__global__ __launch_bounds__(256, 2) void k_pml_pairs_psi(PredGroupArgs a) {
    predict_group_large_body<true, PredPairsSink<KM>, KM == 1 ? GPZ_PML_GB : GPZ_PML_GB8>(a);
}
template __global__ void k_pml_pairs_psi<1>(PredGroupArgs);
template __global__ void k_pml_pairs_psi<8>(PredGroupArgs);

// predict_missing_fits with the limit of GPZ_PREDICT_LARGE_M_MISSING in place of 256
bool predict_missing_large_fits(int kind, int de, int m, int k) {
    bool width = false;
    for (int s : {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20}) width |= de == s;
    return kind == GPZ_KIND_DIAG && width && k >= 1 && k <= 8 && m >= 1 && ((m + 15) / 16) * 16 <= GPZ_PREDICT_LARGE_M_MAX;
}

// dynamic LDS of the panelled kernels, bytes: one K panel of the Pio block, the 64 records of a group (gamma: their first 1 + 2 d doubles
// and the group's (a, b)), the block's rows of X and, with psi, of Psi; at least the sink's last reduction.  m does not enter.
size_t predict_missing_large_lds(int m, int d, int k, bool psi, bool gamma) {
    (void)m;
    const size_t km = k == 1 ? 1 : 8;
    const size_t rec = gamma ? 1 + 2 * (size_t)d : (size_t)predict_missing_rec(d, k);
    const size_t work = 32 * (GPZ_PML_KP + 2) + 64 * rec + (psi ? 64 : 32) * (size_t)d + (gamma ? 64 : 0);
    const size_t red = gamma ? 4 * 32 * 16 : 4 * 32 * 3 * km;
    return (work > red ? work : red) * sizeof(double);
}

int launch_predict_missing_large_pairs(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio, int ldpio,
                                       int m, int d, int k, unsigned obs, const double *U, const double *rec, int nchunk, double *part,
                                       long ldp, const double *hd, long ldh, const double *bvec, double *out) {
    if (n <= 0) return 0;
    const int nk = ((m + 15) / 16) * 16;
    if (d < 1 || d > 20 || k < 1 || k > 8 || m < 1 || nk > GPZ_PREDICT_LARGE_M_MAX || ldpio < nk || ldp < n ||
        nchunk != predict_missing_chunks(m) || (Psic && (obs >> d)))
        return -1;
    PredGroupArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.Pio = Pio; a.ldpio = ldpio; a.nk = nk; a.U = U; a.rec = rec;
    a.nrec = predict_missing_rec(d, k); a.d = d; a.k = k; a.obs = obs;
    a.ngrp = (int)predict_missing_groups(m);   // 8200 at m = 1024
    a.gpc = (a.ngrp + nchunk - 1) / nchunk;
    a.part = part; a.ldp = ldp;
    const size_t lds = predict_missing_large_lds(m, d, k, Psic != nullptr);
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)nchunk);
    if (Psic ? (k == 1 ? launch_predict_group<k_pml_pairs_psi<1>>(st, grid, lds, a) : launch_predict_group<k_pml_pairs_psi<8>>(st, grid, lds, a))
             : (k == 1 ? launch_predict_group<k_pml_pairs<1>>(st, grid, lds, a) : launch_predict_group<k_pml_pairs<8>>(st, grid, lds, a)))
        return -1;
    return launch_pmd_finish(st, part, nchunk, ldp, hd, ldh, n, k, bvec, out);
}
