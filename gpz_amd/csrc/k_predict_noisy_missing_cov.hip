// Rows with input noise AND missing inputs through the streaming predictor, covariance kinds (gpz_predictor_run_noisy_missing_cov_dev /
// _draws_noisy_missing_cov_dev, gpz_predictor.hip): predictNoisyMissing of GC and VC (predictCov.m:233-337) for one tile of ONE group of
// rows that share a NaN pattern and carry a variance psi per observed input.  k_predict_missing_cov.hip is the frame (the pattern, the
// model's tables, slabs of whole pairs, the chunks, the order of every sum) and gpz_predict_missing with Psi the parity partner.
//
// Every density of predictNoisyMissing is N(X_hat_l(x) - c ; S + Psi_hat_row) with S = C + CU_l on (u, u) and T = [I; R_l'] of
// k_predict_missing_cov.hip, and Psi_hat_row = T Psi_oo T' with Psi_oo = diag(psi_o) the row's own - ASSIGNED through `unshuffle`
// (:271-273), the inverse of the permutation [find(o) find(~o)], which is the intended placement only where that permutation is its own
// inverse.  The quirk is kept, as k_pmiss_cov.hip keeps it: the covariance is S + G Psi_oo G' with G the rows of T moved
// where `unshuffle` puts them, and the mean stays T x_o + s.  With G = T the density is the one without noise convolved with
// N(0, Psi_oo) in the observed dimensions; with G != T it is not a convolution in x_o, and the record carries the general form.
// Whitened by S = L L': A = L^-1 T, B = L^-1 G, b = L^-1 s.  A Householder QR of B (d x no, full column rank) gives B = Q [R_B; 0];
// Q'(A x + b) splits into its first no entries z and its last nu entries y2, and with w = R_B^-1 z = J x + j, M = (R_B' R_B)^-1:
//     v' (S + G Psi G')^-1 v = |A2 x + b2|^2 + w' (M + Psi_oo)^-1 w,          |S + G Psi G'| = |S| |R_B|^2 |M + Psi_oo|
// - a sum of nu squares and one no x no form, never a difference.  So (the reference's densities carry no 2 pi, and none appears)
//     rec = [lnw0 - 1/2 ln|S| - sum ln|R_B,cc| | -j (no) | M, packed lower triangle by rows (no (no + 1) / 2) | J (no x no by rows) |
//            A2 (nu x no by rows) | b2 (nu)],        predict_noisy_missing_cov_rec(d, no) doubles
// and the density of a row is ncov_factor<NO> + ncov_density<NO> of k_ncov_density.h as they stand - the packed Cholesky of
// M + diag(psi_o) and a forward substitution in registers, at J x against the centre -j - with |A2 x + b2|^2 taken off the exponent.
// Where G = T: J = I, -j = a, A2 = 0 and |b2|^2 = h of k_predict_missing_cov.hip.  M is positive definite on its own, so psi = 0 in
// some or all observed dimensions is allowed, and gives the density without noise whatever G is.  Ex (:266) has no such scatter: its
// record is that of N(x_o - P_l,o ; Sigma_l,oo + Psi_oo), J = I, nu rows of zeros, ln prior_l folded in.
//
//   k_pnmc_basis / k_pnmc_phirec / k_pnmc_triples   the three record tables, one lane per record, from the pattern's [R | CU | off]
//                    (k_pmcv_basis), Sigma_i / the raw pair records: run-time loops over d and no, temporaries in scratch memory, off
//                    the hot path.  The pair-component table passes through slabs of whole pairs of at most 64 MB
//                    (predict_noisy_missing_cov_slabs(m, d, no): the rule of predict_missing_cov_slabs at this record length).
//   k_pnmc_ex<NO>, k_pnmc_phi<NO>, k_predict_noisy_missing_cov_pairs<NO, KM>   the tile kernels: wrappers of the bodies of
//                    k_predict_nmcov_impl.h with PsiDiag<NO>, where the frame, the LDS and what keeps them from faulting are written
//                    once for this unit, its gamma unit and the twins with a full Psi per row (k_predict_psi_cube_missing*.hip).
// k_pmcv_hd, k_pmcv_coef, k_pmd_finish and the draws' product are k_predict_missing_cov.hip's.
// A group with nothing observed (no = 0) has no Psi to read and is k_predict_missing_cov.hip's own (the host sends it there).
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_predict_nmcov_impl.h"   // the bodies, the launchers and the stage sizes; PMCV_MAXD, PmcvPat, pmcv_pat; LT

#define PNMC_SLAB_BYTES (64L << 20)   // most bytes of a slab of pair-component records

// ---- records ---------------------------------------------------------------------------------------------------------------------------
// S: n x n, lower triangle read, leading dimension PMCV_MAXD, destroyed.  V: columns 0 .. no - 1 the map T, column no the offset s,
// columns no + 1 .. 2 no the scatter G, each of n values PMCV_MAXD apart, destroyed.  nz: rows of zeros behind the n - no rows of A2 | b2.
__host__ __device__ inline void pnmc_record(int n, int no, int nz, double *S, double *V, double lnw0, double *rec) {
    constexpr int LD = PMCV_MAXD;
    double hl = 0.0;
    for (int c = 0; c < n; ++c) {
        double p = S[c * LD + c];
        for (int q = 0; q < c; ++q) p = fma(-S[c * LD + q], S[c * LD + q], p);
        const double dd = sqrt(p);
        S[c * LD + c] = dd;
        hl += log(dd);
        for (int r = c + 1; r < n; ++r) {
            double s = S[r * LD + c];
            for (int q = 0; q < c; ++q) s = fma(-S[r * LD + q], S[c * LD + q], s);
            S[r * LD + c] = s / dd;
        }
    }
    for (int c = 0; c <= 2 * no; ++c)   // L^-1 [A | b | B]
        for (int r = 0; r < n; ++r) {
            double s = V[c * LD + r];
            for (int q = 0; q < r; ++q) s = fma(-S[r * LD + q], V[c * LD + q], s);
            V[c * LD + r] = s / S[r * LD + r];
        }
    double *B = V + (no + 1) * LD, ld = 0.0;
    for (int c = 0; c < no; ++c) {   // Householder: reflector c zeroes B(c + 1 .., c) and is applied to the later columns of B and to [A | b]
        double nn = 0.0;
        for (int r = c; r < n; ++r) nn = fma(B[c * LD + r], B[c * LD + r], nn);
        const double nrm = sqrt(nn), al = B[c * LD + c] > 0.0 ? -nrm : nrm;
        double u[LD], uu = 0.0;
        for (int r = c; r < n; ++r) u[r] = B[c * LD + r];
        u[c] -= al;
        for (int r = c; r < n; ++r) uu = fma(u[r], u[r], uu);
        B[c * LD + c] = al;
        ld += log(nrm);
        if (uu > 0.0)
            for (int c2 = 0; c2 <= 2 * no; ++c2) {
                if (c2 > no && c2 <= no + 1 + c) continue;   // the columns of B up to c are done
                double s = 0.0;
                for (int r = c; r < n; ++r) s = fma(u[r], V[c2 * LD + r], s);
                s *= 2.0 / uu;
                for (int r = c; r < n; ++r) V[c2 * LD + r] = fma(-s, u[r], V[c2 * LD + r]);
            }
    }
    // R_B: (r, c), r <= c, at B[c * LD + r].  [J | j] = R_B^-1 (Q'[A | b])(0 .. no - 1, :) by back substitution, column by column
    double *cen = rec + 1, *M = cen + no, *J = M + no * (no + 1) / 2, *A2 = J + no * no, *b2 = A2 + (n - no + nz) * no;
    for (int c = 0; c <= no; ++c)
        for (int r = no - 1; r >= 0; --r) {
            double s = V[c * LD + r];
            for (int q = r + 1; q < no; ++q) s = fma(-B[q * LD + r], V[c * LD + q], s);
            V[c * LD + r] = s / B[r * LD + r];
            if (c < no) J[r * no + c] = V[c * LD + r];
            else cen[r] = -V[c * LD + r];
        }
    for (int r = 0; r < n - no + nz; ++r) {
        for (int c = 0; c < no; ++c) A2[r * no + c] = r < n - no ? V[c * LD + no + r] : 0.0;
        b2[r] = r < n - no ? V[no * LD + no + r] : 0.0;
    }
    double W[LD * LD];               // W = R_B^-1 (upper), column c: R_B W(:, c) = e_c;  M = W W'
    for (int c = 0; c < no; ++c)
        for (int r = c; r >= 0; --r) {
            double s = r == c ? 1.0 : 0.0;
            for (int q = r + 1; q <= c; ++q) s = fma(-B[q * LD + r], W[q * LD + c], s);
            W[r * LD + c] = s / B[r * LD + r];
        }
    for (int r = 0; r < no; ++r)
        for (int c = 0; c <= r; ++c) {
            double s = 0.0;
            for (int q = r; q < no; ++q) s = fma(W[r * LD + q], W[c * LD + q], s);
            M[LT(r, c)] = s;
        }
    rec[0] = lnw0 - hl - ld;
}

// the record of centre cen (by dimension) with covariance Cm (d x d row-major) against component l (bas = [R | CU | off] of l)
__host__ __device__ inline void pnmc_cond_record(const PmcvPat &pt, const double *Cm, const double *cen, double lnw0, const double *bas,
                                                 double *rec) {
    constexpr int LD = PMCV_MAXD;
    const int d = pt.d, no = pt.no, nu = pt.nu;
    const double *R = bas, *CU = bas + no * nu, *off = CU + nu * nu;
    double S[LD * LD], V[(2 * LD + 1) * LD];
    int inv[LD];                     // inv[dimension] = its index in [o | u]: `unshuffle`
    for (int a = 0; a < d; ++a) inv[a < no ? pt.o[a] : pt.u[a - no]] = a;
    for (int a = 0; a < d; ++a) {
        const int pa = a < no ? pt.o[a] : pt.u[a - no];
        for (int b = 0; b <= a; ++b) {
            const int pb = b < no ? pt.o[b] : pt.u[b - no];
            S[a * LD + b] = Cm[pa * d + pb] + (b >= no ? CU[(a - no) * nu + (b - no)] : 0.0);
        }
        V[no * LD + a] = (a < no ? 0.0 : off[a - no]) - cen[pa];
        const int ga = inv[inv[a]];   // row a of T Psi T' lands on dimension unshuffle(a), which lies at index inv[inv[a]] of [o | u]   :273
        for (int c = 0; c < no; ++c) {
            const double t = a < no ? (a == c ? 1.0 : 0.0) : R[c * nu + (a - no)];
            V[c * LD + a] = t;
            V[(no + 1 + c) * LD + ga] = t;
        }
    }
    pnmc_record(d, no, 0, S, V, lnw0, rec);
}

// the Ex record of component l: N(x_o - P_l,o ; Sigma_l,oo + Psi_oo) prior_l                                              :266
__host__ __device__ inline void pnmc_ex_record(const PmcvPat &pt, const double *Sg, const double *p, double lnw0, double *rec) {
    constexpr int LD = PMCV_MAXD;
    const int d = pt.d, no = pt.no;
    double S[LD * LD], V[(2 * LD + 1) * LD];
    for (int a = 0; a < no; ++a) {
        for (int b = 0; b <= a; ++b) S[a * LD + b] = Sg[pt.o[a] * d + pt.o[b]];
        V[no * LD + a] = -p[pt.o[a]];
        for (int c = 0; c < no; ++c) V[c * LD + a] = V[(no + 1 + c) * LD + a] = a == c ? 1.0 : 0.0;
    }
    pnmc_record(no, no, pt.nu, S, V, lnw0, rec);
}

__global__ __launch_bounds__(64) void k_pnmc_basis(PmcvPat pt, int m, int de, const double *__restrict__ P, const double *__restrict__ Sig,
                                                   const double *__restrict__ priors, double *__restrict__ exrec, int rl) {
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l >= m) return;
    pnmc_ex_record(pt, Sig + (size_t)l * pt.d * pt.d, P + (size_t)l * de, log(priors ? priors[l] : 1.0 / m), exrec + (size_t)l * rl);
}

__global__ __launch_bounds__(64) void k_pnmc_phirec(PmcvPat pt, int m, int de, const double *__restrict__ P, const double *__restrict__ Sig,
                                                    const double *__restrict__ lnS, const double *__restrict__ bas, int nb,
                                                    double *__restrict__ phirec, int rl) {
    const long e = (long)blockIdx.x * 64 + threadIdx.x;
    if (e >= (long)m * m) return;
    const int i = (int)(e / m), j = (int)(e - (long)i * m);
    pnmc_cond_record(pt, Sig + (size_t)i * pt.d * pt.d, P + (size_t)i * de, 0.5 * lnS[i], bas + (size_t)j * nb, phirec + (size_t)e * rl);
}

// records [0, cnt * m) of the slab that starts at pair q0; raw: launch_pair_table's [lnZ | c_ab | C_ab (d x d)]
__global__ __launch_bounds__(64) void k_pnmc_triples(PmcvPat pt, long q0, long cnt, int m, const double *__restrict__ raw,
                                                     const double *__restrict__ bas, int nb, double *__restrict__ slab, int rl) {
    const long e = (long)blockIdx.x * 64 + threadIdx.x;
    if (e >= cnt * m) return;
    const long q = e / m;
    const int l = (int)(e - q * m);
    const double *t = raw + (size_t)(q0 + q) * (1 + pt.d + pt.d * pt.d);
    pnmc_cond_record(pt, t + 1 + pt.d, t + 1, t[0], bas + (size_t)l * nb, slab + (size_t)e * rl);
}

// ---- the tile kernels ------------------------------------------------------------------------------------------------------------------
template <int NO>
__global__ __launch_bounds__(256) void k_pnmc_ex(PredNmcovArgs a) { nmcov_ex_body<PsiDiag<NO>, false>(a); }

template <int NO>
__global__ __launch_bounds__(256) void k_pnmc_phi(PredNmcovArgs a) { nmcov_phi_body<PsiDiag<NO>, false>(a); }

template <int NO, int KM>
__global__ __launch_bounds__(256) void k_predict_noisy_missing_cov_pairs(PredNmcovArgs a) { nmcov_pairs_body<PsiDiag<NO>, KM>(a); }

struct PnmcKernels {
    static constexpr size_t stage_lds = 0;
    template <int NO> static auto ex() { return k_pnmc_ex<NO>; }
    template <int NO> static auto phi() { return k_pnmc_phi<NO>; }
    template <int NO, int KM> static auto pairs() { return k_predict_noisy_missing_cov_pairs<NO, KM>; }
};

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// [lnw | -j (no) | M (no (no + 1) / 2) | J (no no) | A2 ((d - no) no) | b2 (d - no)]
int predict_noisy_missing_cov_rec(int d, int no) { return 1 + no + no * (no + 1) / 2 + no * no + (d - no) * (no + 1); }

// slabs of whole pairs: predict_missing_cov_slabs at this record length.  m, d and no alone.
int predict_noisy_missing_cov_slabs(int m, int d, int no) {
    const long npair = (long)m * (m + 1) / 2, per = (long)m * predict_noisy_missing_cov_rec(d, no) * (long)sizeof(double);
    int s = 1;
    while (((npair + s - 1) / s) * per > PNMC_SLAB_BYTES) s *= 2;
    return s;
}

long predict_noisy_missing_cov_slab_pairs(int m, int d, int no) {
    const long npair = (long)m * (m + 1) / 2, s = predict_noisy_missing_cov_slabs(m, d, no);
    return (npair + s - 1) / s;
}

// dynamic LDS of the pair kernel, bytes: the Pio block and four stages of records, at least the three partials of the last reduction
size_t predict_noisy_missing_cov_lds(int m, int d, int no, int k) {
    const size_t work = (size_t)m * 64 + 4 * (size_t)PNMC_SB * predict_noisy_missing_cov_rec(d, no),
                 red = 3 * 64 * 3 * (size_t)(k == 1 ? 1 : 8);
    return (work > red ? work : red) * sizeof(double);
}

// the Ex and PHI records of (obs, priors) in this unit's form; bas: [R | CU | off] per basis function as launch_pmcv_tables left it
int launch_pnmc_tables(hipStream_t st, int m, int d, int de, unsigned obs, const double *P, const double *Sig, const double *lnS,
                       const double *priors, const double *bas, double *exrec, double *phirec) {
    if (d < 1 || d > PMCV_MAXD || m < 1) return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.no < 1 || pt.nu < 1) return -1;
    const int nb = predict_missing_cov_bas(d, pt.no), rl = predict_noisy_missing_cov_rec(d, pt.no);
    hipLaunchKernelGGL(k_pnmc_basis, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, pt, m, de, P, Sig, priors, exrec, rl);
    hipLaunchKernelGGL(k_pnmc_phirec, dim3((unsigned)(((long)m * m + 63) / 64)), dim3(64), 0, st, pt, m, de, P, Sig, lnS, bas, nb, phirec,
                       rl);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// records [0, cnt * m) of the slab that starts at pair q0 (the slab loop of k_predict_nmcov_impl.h fills every slab through it)
int launch_pnmc_triples(hipStream_t st, int d, unsigned obs, long q0, long cnt, int m, const double *raw, const double *bas, double *slab) {
    if (cnt <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || m < 1) return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.no < 1 || pt.nu < 1) return -1;
    hipLaunchKernelGGL(k_pnmc_triples, dim3((unsigned)((cnt * m + 63) / 64)), dim3(64), 0, st, pt, q0, cnt, m, raw, bas,
                       predict_missing_cov_bas(d, pt.no), slab, predict_noisy_missing_cov_rec(d, pt.no));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pnmc_rows(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m, int mp, int d, int k,
                     unsigned obs, const double *exrec, const double *phirec, const double *w, const double *v, double *Pio, long ldr,
                     double *Phi, double *hd, long ldh) {
    return nmcov_launch_rows<PnmcKernels>(st, Xc, Psic, ldx, n, nrow, m, mp, d, k, obs, exrec, phirec, w, v, Pio, ldr, Phi, hd, ldh);
}

// launch_predict_missing_cov_pairs with Psic and this unit's records and slabs
int launch_predict_noisy_missing_cov_pairs(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio,
                                           long ldr, int m, int d, int k, unsigned obs, const double *raw, const double *bas,
                                           const double *coef, double *slab, bool *slab_kept, int nchunk, double *part, long ldp,
                                           const double *hd, long ldh, const double *bvec, double *out) {
    return nmcov_launch_pairs<PnmcKernels>(st, Xc, Psic, ldx, n, Pio, ldr, m, d, k, obs, raw, bas, coef, slab, slab_kept, nchunk, part, ldp,
                                           hd, ldh, bvec, out);
}
