// The frame of the tile kernels for complete rows with input noise on a covariance kind, predictNoisy of GC and VC (predictCov.m:70-132):
// k_predict_noisy_cov_small / _phi (k_predict_noisy_cov.hip: Psi a variance per input dimension, the diagonal that fixPsi puts into the
// d x d x n cube of these kinds) and k_predict_psi_cube_small / _phi (k_predict_psi_cube.hip: Psi(:, :, i) as fixPsi.m:36 leaves it, a
// full matrix per row).  Each is a thin __global__ wrapper of a body below; what differs between the twins is the Psi policy (PsiDiag,
// PsiTri: k_ncov_density.h), that is the width of the tile's Psi slot and the matrix of the density, S + diag(psi_i) or S + Psi_i over
// the whole packed triangle.  1 <= d <= 10: every d x d matrix is a packed lower triangle with compile-time indices, in registers.
//
//   predict_ncov_small_body<Psi, SHARED, KM>
//       k_predict_noisy_small's frame: lane = row (coalesced reads of Xc [d][ldx] and of the Psi slot [Psi::W][ldx]), 256 rows per
//       workgroup, gridDim.y = chunks, partial sums part [C][5k][ldp] for k_predict_noisy_finish, KM = 1 or 8 outputs in registers.  The
//       records are the same for every row: a workgroup stages 32 of them at a time in static LDS with coalesced loads between two
//       barriers and its lanes read them as broadcasts.
//       Basis functions [j0, j1) of the chunk, records [1/2 ln|Sigma_j| | p_j | Sigma_j packed lower | w_j | v_j]: per (row, j) the packed
//       Cholesky of Sigma_j + Psi_i (Psi::factor -> chol_packed_rd, k_chol_packed.h: the one-shot route's), a forward substitution,
//       PHI = exp(1/2 ln|Sigma_j| - 1/2 q) prod(1 / L_cc) (getPHI.m:78-89), mu += PHI w_j, ElnS - b += PHI v_j.  These two sums are stored
//       before the pair phase, so that they and the three pair sums are never live together.
//       Pairs [p0, p1) of the chunk, records [lnZ_ab | c_ab | C_ab packed lower | per output f w_a w_b, f v_a v_b, f iS(a, b)] (f = 2 off
//       the diagonal, 1 on it; iS read at a >= b only, as the reference does): per (row, pair) the Cholesky of C_ab + Psi_i, a forward
//       substitution, z = exp(lnZ - 1/2 q) prod(1 / L_cc), three FMAs per output (predictCov.m:105-119).
//       SHARED (GC): every Sigma_j is the same matrix and every C_ab = Sigma / 2, so Sigma + Psi_i and C + Psi_i are factorised once per
//       row, not once per record (from record 0 of either table: the same bits in every chunk).
//       Where the row's Psi lives: in registers from the start of the kernel, except that a SHARED kernel on a policy with RELOAD loads it
//       in front of each phase for the one factorisation there and drops it (k_ncov_density.h).
//   predict_ncov_phi_body<Psi, SHARED>
//       the same basis-record loop writing E_x[PHI] of the tile as launch_tgemm takes it: [nrow][mp] row-major, zeros in the rows >= n and
//       the columns >= m.  The draws are then PHI W on the T-GEMM: mu is linear in w, so draw s = E_x[PHI] w_s is exact.
//   predict_ncov_launch_small<K> / _phi<K>
//       the launchers of a unit, K naming its two wrappers: the guard, the arguments, the switch over d, GC / VC and KM.
// The records are k_noisy_cov_records' and the chunk count C is the caller's predict_noisy_cov_chunks(m, d, k) (k_predict_noisy_cov.hip):
// it depends on the model's shape only, and every sum runs in one fixed order from zero: no atomics, and a row's results have the same
// bits for any tile size, position in the tile and row order.  A cube of diagonals gives the bits of the diagonal form on the same
// variances: S + 0.0 off the diagonal, the same factor and density functions, the same order of the sums.
#pragma once
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_ncov_density.h"   // LT, PsiDiag, PsiTri, ncov_psi_load, ncov_density (shared with the two gamma units)

#define NCOV_TP 32   // records per LDS stage

struct PredNcovArgs {
    const double *Xc, *Psic; long ldx;   // [d][ldx] and [Psi::W][ldx] column layout, n rows
    int n, m, k;
    const double *brec; int rb;          // basis records, rb = 1 + d + d (d + 1) / 2 + 2 k doubles each
    const double *prec; int rp;          // pair records, rp = 1 + d + d (d + 1) / 2 + 3 k doubles each
    int jpc; long ppc;                   // basis functions and pairs per chunk
    double *part; long ldp;              // [chunks][5 k][ldp]
    double *Phi; int nrow, mp;           // the phi body: [nrow][mp]
};

template <class Psi, bool SHARED, int KM>
__device__ __forceinline__ void predict_ncov_small_body(const PredNcovArgs &a) {
    constexpr int D = Psi::D, NP = D * (D + 1) / 2, H = 1 + D + NP;   // H: the head of either record, in front of the per-output values
    constexpr int RJ = H + 2 * KM;                                    // a staged basis record: outputs k .. KM - 1 hold zeros
    constexpr bool KEEP = !(SHARED && Psi::RELOAD);
    __shared__ double sT[NCOV_TP * (H + 3 * KM)];   // one stage of basis records (RJ each) or pair records (as they lie in the table)
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const bool act = i < a.n;
    const int ic = act ? i : a.n - 1;
    const int ch = blockIdx.y, m = a.m, k = a.k;
    const double *Pg = a.Psic + ic;   // value q of the row's Psi at Pg[q ldx]
    double x[D], ps[Psi::W];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = a.Xc[(size_t)c * a.ldx + ic];
    if (KEEP) ncov_psi_load(Pg, a.ldx, ps);
    double M[NP], rd[D], prd;
    double *pp = a.part + (size_t)ch * 5 * k * a.ldp + i;
    // ---- mu and ElnS - b over the chunk's basis functions                                          predictCov.m:75-79
    {
        double mu[KM], el[KM];
#pragma unroll
        for (int o = 0; o < KM; ++o) { mu[o] = 0.0; el[o] = 0.0; }
        const int j0 = ch * a.jpc, j1 = min(m, j0 + a.jpc);
        if (SHARED) {
            if (!KEEP) ncov_psi_load(Pg, a.ldx, ps);
            Psi::factor(a.brec + 1 + D, ps, M, rd, &prd);
        }
        for (int jb = j0; jb < j1; jb += NCOV_TP) {
            const int nj = min(NCOV_TP, j1 - jb);
            __syncthreads();   // the stage before is read
            for (int t = tid; t < nj * RJ; t += 256) {
                const int jj = t / RJ, f = t - jj * RJ;
                const double *src = a.brec + (size_t)(jb + jj) * a.rb;
                double val;
                if (f < H) val = src[f];
                else if (f < H + KM) val = f - H < k ? src[H + f - H] : 0.0;
                else val = f - H - KM < k ? src[H + k + f - H - KM] : 0.0;
                sT[t] = val;
            }
            __syncthreads();
#pragma unroll 1
            for (int jj = 0; jj < nj; ++jj) {
                const double *t = sT + jj * RJ;   // the same address in every lane: a broadcast read
                if (!SHARED) Psi::factor(t + 1 + D, ps, M, rd, &prd);
                const double ph = ncov_density<D>(t + 1, t[0], x, M, rd, prd);
#pragma unroll
                for (int o = 0; o < KM; ++o) {
                    mu[o] = fma(ph, t[H + o], mu[o]);
                    el[o] = fma(ph, t[H + KM + o], el[o]);
                }
            }
        }
        if (act) {
#pragma unroll
            for (int o = 0; o < KM; ++o)
                if (o < k) {
                    pp[(size_t)(0 * k + o) * a.ldp] = mu[o];
                    pp[(size_t)(1 * k + o) * a.ldp] = el[o];
                }
        }
    }
    // ---- the chunk's pairs                                                                         predictCov.m:81-125
    double ga[KM], vl[KM], nu[KM];
#pragma unroll
    for (int o = 0; o < KM; ++o) { ga[o] = 0.0; vl[o] = 0.0; nu[o] = 0.0; }
    const long npair = (long)m * (m + 1) / 2;
    const long p0 = (long)ch * a.ppc, p1 = min(npair, p0 + a.ppc);
    const int rp = a.rp;
    if (SHARED) {
        if (!KEEP) ncov_psi_load(Pg, a.ldx, ps);
        Psi::factor(a.prec + 1 + D, ps, M, rd, &prd);
    }
    for (long pb = p0; pb < p1; pb += NCOV_TP) {
        const int np = (int)min((long)NCOV_TP, p1 - pb);
        __syncthreads();
        const double *src = a.prec + (size_t)pb * rp;
        for (int t = tid; t < np * rp; t += 256) sT[t] = src[t];
        __syncthreads();
#pragma unroll 1
        for (int e = 0; e < np; ++e) {
            const double *t = sT + e * rp;
            if (!SHARED) Psi::factor(t + 1 + D, ps, M, rd, &prd);          // Cij + Psi_i                 :109
            const double z = ncov_density<D>(t + 1, t[0], x, M, rd, prd);  //                             :111
            const double *cf = t + H;
#pragma unroll
            for (int o = 0; o < KM; ++o)
                if (o < k) {
                    ga[o] = fma(z, cf[3 * o], ga[o]);                      //                             :113-119
                    vl[o] = fma(z, cf[3 * o + 1], vl[o]);
                    nu[o] = fma(z, cf[3 * o + 2], nu[o]);
                }
        }
    }
    if (!act) return;
#pragma unroll
    for (int o = 0; o < KM; ++o)
        if (o < k) {
            pp[(size_t)(2 * k + o) * a.ldp] = ga[o];
            pp[(size_t)(3 * k + o) * a.ldp] = vl[o];
            pp[(size_t)(4 * k + o) * a.ldp] = nu[o];
        }
}

template <class Psi, bool SHARED>
__device__ __forceinline__ void predict_ncov_phi_body(const PredNcovArgs &a) {
    constexpr int D = Psi::D, NP = D * (D + 1) / 2, H = 1 + D + NP;
    __shared__ double sT[NCOV_TP * H];   // the heads of one stage of basis records
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const bool act = i < a.n, st = i < a.nrow;   // rows n .. nrow - 1 are written as zeros
    const int ic = act ? i : a.n - 1;
    const int ch = blockIdx.y, m = a.m;
    double x[D], ps[Psi::W];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = a.Xc[(size_t)c * a.ldx + ic];
    ncov_psi_load(a.Psic + ic, a.ldx, ps);   // (one phase: SHARED factorises below and the values die there)
    double M[NP], rd[D], prd;
    double *row = a.Phi + (size_t)(st ? i : 0) * a.mp;
    const int j0 = ch * a.jpc, j1 = min(m, j0 + a.jpc);
    if (SHARED) Psi::factor(a.brec + 1 + D, ps, M, rd, &prd);
    for (int jb = j0; jb < j1; jb += NCOV_TP) {
        const int nj = min(NCOV_TP, j1 - jb);
        __syncthreads();
        for (int t = tid; t < nj * H; t += 256) {
            const int jj = t / H;
            sT[t] = a.brec[(size_t)(jb + jj) * a.rb + (t - jj * H)];
        }
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < nj; ++jj) {
            const double *t = sT + jj * H;
            if (!SHARED) Psi::factor(t + 1 + D, ps, M, rd, &prd);
            const double ph = ncov_density<D>(t + 1, t[0], x, M, rd, prd);
            if (st) row[jb + jj] = act ? ph : 0.0;
        }
    }
    if (ch == 0 && st)
        for (int j = m; j < a.mp; ++j) row[j] = 0.0;
}

// ---- the launchers of a unit.  K: a struct with small<D, SHARED, KM>() and phi<D, SHARED>(), the unit's __global__ wrappers -----------
#define NCOV_CASES(MACRO)                                                                                  \
    switch (d) {                                                                                           \
        case 1: MACRO(1); break; case 2: MACRO(2); break; case 3: MACRO(3); break; case 4: MACRO(4); break; \
        case 5: MACRO(5); break; case 6: MACRO(6); break; case 7: MACRO(7); break; case 8: MACRO(8); break; \
        case 9: MACRO(9); break; case 10: MACRO(10); break;                                                \
        default: return -1;                                                                                \
    }

static inline PredNcovArgs predict_ncov_args(int d, const double *Xc, const double *Psic, long ldx, int n, int m, int k, const double *brec,
                                             const double *prec, int nchunk) {
    const long npair = (long)m * (m + 1) / 2;
    PredNcovArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.m = m; a.k = k;
    a.brec = brec; a.rb = predict_noisy_cov_brec(d, k);
    a.prec = prec; a.rp = predict_noisy_cov_prec(d, k);
    a.jpc = (m + nchunk - 1) / nchunk;
    a.ppc = (npair + nchunk - 1) / nchunk;
    return a;
}

template <class K, int D>
static void predict_ncov_launch_small_d(hipStream_t st, const PredNcovArgs &a, dim3 grid, bool shared) {
    if (a.k == 1) {
        if (shared) hipLaunchKernelGGL((K::template small<D, true, 1>()), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((K::template small<D, false, 1>()), grid, dim3(256), 0, st, a);
    } else {
        if (shared) hipLaunchKernelGGL((K::template small<D, true, 8>()), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((K::template small<D, false, 8>()), grid, dim3(256), 0, st, a);
    }
}

// the moments of a tile: the small kernel over nchunk chunks, then k_predict_noisy_finish
template <class K>
static int predict_ncov_launch_small(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m, int k,
                                     const double *brec, const double *prec, const double *bvec, int nchunk, double *part, long ldp,
                                     double *out) {
    if (n <= 0) return 0;
    if (k < 1 || k > 8 || m < 1 || nchunk < 1 || ldx < n || ldp < n) return -1;
    PredNcovArgs a = predict_ncov_args(d, Xc, Psic, ldx, n, m, k, brec, prec, nchunk);
    a.part = part; a.ldp = ldp;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nchunk);
#define NCOV_SMALL(DD) predict_ncov_launch_small_d<K, DD>(st, a, grid, shared)
    NCOV_CASES(NCOV_SMALL)
#undef NCOV_SMALL
    if (hipGetLastError() != hipSuccess) return -1;
    return launch_predict_noisy_finish(st, part, nchunk, ldp, n, k, bvec, out);
}

template <class K>
static int predict_ncov_launch_phi(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m,
                                   int mp, int k, const double *brec, int nchunk, double *Phi) {
    if (n <= 0) return 0;
    if (m < 1 || nchunk < 1 || nrow < n || mp < m || ldx < n) return -1;
    PredNcovArgs a = predict_ncov_args(d, Xc, Psic, ldx, n, m, k, brec, nullptr, nchunk);
    a.Phi = Phi; a.nrow = nrow; a.mp = mp;
    const dim3 grid((unsigned)((nrow + 255) / 256), (unsigned)nchunk);
#define NCOV_PHI(DD)                                                                                            \
    do {                                                                                                        \
        if (shared) hipLaunchKernelGGL((K::template phi<DD, true>()), grid, dim3(256), 0, st, a);               \
        else hipLaunchKernelGGL((K::template phi<DD, false>()), grid, dim3(256), 0, st, a);                     \
    } while (0)
    NCOV_CASES(NCOV_PHI)
#undef NCOV_PHI
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
