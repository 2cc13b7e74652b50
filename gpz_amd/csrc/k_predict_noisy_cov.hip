// Rows with input noise through the streaming predictor, covariance kinds (gpz_predictor_run_noisy_cov_dev / _draws_noisy_cov_dev,
// gpz_predictor.hip): predictNoisy of GC and VC (predictCov.m:70-132) for one tile as ONE kernel plus the finish kernel of the diagonal
// kinds (k_predict_noisy_finish, k_predict_noisy.hip), and E_x[PHI] of a tile for the draws.  Psi is a variance per input dimension in
// the layout of Xc: the diagonal that fixPsi puts into the d x d x n cube of these kinds.  1 <= d <= 10: every d x d matrix is a packed
// lower triangle with compile-time indices, in registers.
//
//   k_predict_noisy_cov_small<D, SHARED, KM>
//       k_predict_noisy_small's frame: lane = row (coalesced reads of Xc / Psic [d][ldx]), 256 rows per workgroup, gridDim.y = chunks,
//       partial sums part [C][5k][ldp], KM = 1 or 8 outputs in registers.  The records are the same for every row: a workgroup stages
//       32 of them at a time in static LDS with coalesced loads between two barriers and its lanes read them as broadcasts.
//       Basis functions [j0, j1) of the chunk, records [1/2 ln|Sigma_j| | p_j | Sigma_j packed lower | w_j | v_j]: per (row, j) the packed
//       Cholesky of Sigma_j + diag(psi) (chol_packed_rd, k_chol_packed.h: the one-shot route's), a forward substitution, PHI = exp(1/2 ln|Sigma_j| -
//       1/2 q) prod(1 / L_cc) (getPHI.m:78-89), mu += PHI w_j, ElnS - b += PHI v_j.  These two sums are stored before the pair phase, so
//       that they and the three pair sums are never live together.
//       Pairs [p0, p1) of the chunk, records [lnZ_ab | c_ab | C_ab packed lower | per output f w_a w_b, f v_a v_b, f iS(a, b)] (f = 2 off
//       the diagonal, 1 on it; iS read at a >= b only, as the reference does): per (row, pair) the Cholesky of C_ab + diag(psi), a forward
//       substitution, z = exp(lnZ - 1/2 q) prod(1 / L_cc), three FMAs per output (predictCov.m:105-119).
//       SHARED (GC): every Sigma_j is the same matrix and every C_ab = Sigma / 2, so Sigma + Psi_i and C + Psi_i are factorised once per
//       row, not once per record (from record 0 of either table: the same bits in every chunk).
//   k_predict_noisy_cov_phi<D, SHARED>
//       the same basis-record loop (ncov_factor / ncov_density, shared with the kernel above) writing E_x[PHI] of the tile as launch_tgemm
//       takes it: [nrow][mp] row-major, zeros in the rows >= n and the columns >= m.  The draws are then PHI W on the T-GEMM: mu is linear
//       in w, so draw s = E_x[PHI] w_s is exact.
//   k_noisy_cov_records
//       once per handle: Sigma_j and ln|Sigma_j| (launch_gen_prep) and the pair records of launch_pair_table(GPZ_KIND_COV), d x d
//       row-major, repacked into the records above and completed with the weights and gpz_pair_coef's coefficients.
// The chunk count C = predict_noisy_cov_chunks(m, d, k) depends on the model's shape only, and every sum runs in one fixed order from zero:
// no atomics, and a row's results have the same bits for any tile size, position in the tile and row order.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_ncov_density.h"   // LT, ncov_factor, ncov_density (shared with k_predict_noisy_cov_gamma.hip)

#define NC_TP 32   // records per LDS stage

struct PredNoisyCovArgs {
    const double *Xc, *Psic; long ldx;   // [d][ldx] column layout, n rows
    int n, m, k;
    const double *brec; int rb;          // basis records, rb = 1 + d + d (d + 1) / 2 + 2 k doubles each
    const double *prec; int rp;          // pair records, rp = 1 + d + d (d + 1) / 2 + 3 k doubles each
    int jpc; long ppc;                   // basis functions and pairs per chunk
    double *part; long ldp;              // [chunks][5 k][ldp]
    double *Phi; int nrow, mp;           // k_predict_noisy_cov_phi: [nrow][mp]
};

template <int D, bool SHARED, int KM>
__global__ __launch_bounds__(256) void k_predict_noisy_cov_small(PredNoisyCovArgs a) {
    constexpr int NP = D * (D + 1) / 2, H = 1 + D + NP;   // H: the head of either record, in front of the per-output values
    constexpr int RJ = H + 2 * KM;                        // a staged basis record: outputs k .. KM - 1 hold zeros
    __shared__ double sT[NC_TP * (H + 3 * KM)];           // one stage of basis records (RJ each) or pair records (as they lie in the table)
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const bool act = i < a.n;
    const int ic = act ? i : a.n - 1;
    const int ch = blockIdx.y, m = a.m, k = a.k;
    double x[D], ps[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        x[c] = a.Xc[(size_t)c * a.ldx + ic];
        ps[c] = a.Psic[(size_t)c * a.ldx + ic];
    }
    double M[NP], rd[D], prd;
    double *pp = a.part + (size_t)ch * 5 * k * a.ldp + i;
    // ---- mu and ElnS - b over the chunk's basis functions                                          predictCov.m:75-79
    {
        double mu[KM], el[KM];
#pragma unroll
        for (int o = 0; o < KM; ++o) { mu[o] = 0.0; el[o] = 0.0; }
        const int j0 = ch * a.jpc, j1 = min(m, j0 + a.jpc);
        if (SHARED) ncov_factor<D>(a.brec + 1 + D, ps, M, rd, &prd);
        for (int jb = j0; jb < j1; jb += NC_TP) {
            const int nj = min(NC_TP, j1 - jb);
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
                if (!SHARED) ncov_factor<D>(t + 1 + D, ps, M, rd, &prd);
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
    if (SHARED) ncov_factor<D>(a.prec + 1 + D, ps, M, rd, &prd);
    for (long pb = p0; pb < p1; pb += NC_TP) {
        const int np = (int)min((long)NC_TP, p1 - pb);
        __syncthreads();
        const double *src = a.prec + (size_t)pb * rp;
        for (int t = tid; t < np * rp; t += 256) sT[t] = src[t];
        __syncthreads();
#pragma unroll 1
        for (int e = 0; e < np; ++e) {
            const double *t = sT + e * rp;
            if (!SHARED) ncov_factor<D>(t + 1 + D, ps, M, rd, &prd);      // Cij + Psi                   :109
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

template <int D, bool SHARED>
__global__ __launch_bounds__(256) void k_predict_noisy_cov_phi(PredNoisyCovArgs a) {
    constexpr int NP = D * (D + 1) / 2, H = 1 + D + NP;
    __shared__ double sT[NC_TP * H];   // the heads of one stage of basis records
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const bool act = i < a.n, st = i < a.nrow;   // rows n .. nrow - 1 are written as zeros
    const int ic = act ? i : a.n - 1;
    const int ch = blockIdx.y, m = a.m;
    double x[D], ps[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        x[c] = a.Xc[(size_t)c * a.ldx + ic];
        ps[c] = a.Psic[(size_t)c * a.ldx + ic];
    }
    double M[NP], rd[D], prd;
    double *row = a.Phi + (size_t)(st ? i : 0) * a.mp;
    const int j0 = ch * a.jpc, j1 = min(m, j0 + a.jpc);
    if (SHARED) ncov_factor<D>(a.brec + 1 + D, ps, M, rd, &prd);
    for (int jb = j0; jb < j1; jb += NC_TP) {
        const int nj = min(NC_TP, j1 - jb);
        __syncthreads();
        for (int t = tid; t < nj * H; t += 256) {
            const int jj = t / H;
            sT[t] = a.brec[(size_t)(jb + jj) * a.rb + (t - jj * H)];
        }
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < nj; ++jj) {
            const double *t = sT + jj * H;
            if (!SHARED) ncov_factor<D>(t + 1 + D, ps, M, rd, &prd);
            const double ph = ncov_density<D>(t + 1, t[0], x, M, rd, prd);
            if (st) row[jb + jj] = act ? ph : 0.0;
        }
    }
    if (ch == 0 && st)
        for (int j = m; j < a.mp; ++j) row[j] = 0.0;
}

__global__ __launch_bounds__(256) void k_noisy_cov_records(int m, int d, int de, int k, const double *__restrict__ P,
                                                           const double *__restrict__ Sig, const double *__restrict__ lnS,
                                                           const double *__restrict__ raw, const double *__restrict__ w,
                                                           const double *__restrict__ v, const double *__restrict__ iS,
                                                           double *__restrict__ brec, double *__restrict__ prec) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x, npair = (long)m * (m + 1) / 2;
    const int h = 1 + d + d * (d + 1) / 2;
    if (e < m) {
        double *o = brec + (size_t)e * (h + 2 * k);
        o[0] = 0.5 * lnS[e];
        for (int r = 0; r < d; ++r) {
            o[1 + r] = P[(size_t)e * de + r];
            for (int c = 0; c <= r; ++c) o[1 + d + LT(r, c)] = Sig[(size_t)e * d * d + r * d + c];
        }
        for (int q = 0; q < k; ++q) {
            o[h + q] = w[e + (size_t)m * q];
            o[h + k + q] = v ? v[e + (size_t)m * q] : 0.0;
        }
    }
    if (prec && e < npair) {
        const double *src = raw + (size_t)e * (1 + d + d * d);
        double *o = prec + (size_t)e * (h + 3 * k);
        o[0] = src[0];
        for (int r = 0; r < d; ++r) {
            o[1 + r] = src[1 + r];
            for (int c = 0; c <= r; ++c) o[1 + d + LT(r, c)] = src[1 + d + r * d + c];   // the lower triangle, as k_predict_noisy_cov reads it
        }
        int ia, ib;
        gpz_pair_of(e, &ia, &ib);                                          // f: 2x in the loop, 1x on the diagonal  (predictCov.m:113-119)
        gpz_pair_coef(o + h, ia, ib, m, k, w, v, iS);
    }
}

bool predict_noisy_cov_fits(int kind, int d, int m, int k) {
    return kind == GPZ_KIND_COV && d >= 1 && d <= 10 && k >= 1 && k <= 8 && m >= 1 && ((m + 15) / 16) * 16 <= 256;
}

// pair chunks (= chunks of the basis functions): one per 2048 pairs, at most 4.  The model's shape only, never the rows.
int predict_noisy_cov_chunks(int m, int d, int k) {
    (void)d; (void)k;
    const long c = ((long)m * (m + 1) / 2) / 2048;
    return (int)(c < 1 ? 1 : (c > 4 ? 4 : c));
}

int predict_noisy_cov_brec(int d, int k) { return 1 + d + d * (d + 1) / 2 + 2 * k; }
int predict_noisy_cov_prec(int d, int k) { return 1 + d + d * (d + 1) / 2 + 3 * k; }

int launch_noisy_cov_records(hipStream_t st, int m, int d, int de, int k, const double *P, const double *Sig, const double *lnS,
                             const double *raw, const double *w, const double *v, const double *iS, double *brec, double *prec) {
    const long items = prec ? (long)m * (m + 1) / 2 : (long)m;
    hipLaunchKernelGGL(k_noisy_cov_records, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, m, d, de, k, P, Sig, lnS, raw, w, v,
                       iS, brec, prec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

#define NC_CASES(MACRO)                                                                                    \
    switch (d) {                                                                                           \
        case 1: MACRO(1); break; case 2: MACRO(2); break; case 3: MACRO(3); break; case 4: MACRO(4); break; \
        case 5: MACRO(5); break; case 6: MACRO(6); break; case 7: MACRO(7); break; case 8: MACRO(8); break; \
        case 9: MACRO(9); break; case 10: MACRO(10); break;                                                \
        default: return -1;                                                                                \
    }

template <int D>
static void launch_nc(hipStream_t st, const PredNoisyCovArgs &a, dim3 grid, bool shared) {
    if (a.k == 1) {
        if (shared) hipLaunchKernelGGL((k_predict_noisy_cov_small<D, true, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_predict_noisy_cov_small<D, false, 1>), grid, dim3(256), 0, st, a);
    } else {
        if (shared) hipLaunchKernelGGL((k_predict_noisy_cov_small<D, true, 8>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_predict_noisy_cov_small<D, false, 8>), grid, dim3(256), 0, st, a);
    }
}

static PredNoisyCovArgs nc_args(int d, const double *Xc, const double *Psic, long ldx, int n, int m, int k, const double *brec,
                                const double *prec, int nchunk) {
    const long npair = (long)m * (m + 1) / 2;
    PredNoisyCovArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.m = m; a.k = k;
    a.brec = brec; a.rb = predict_noisy_cov_brec(d, k);
    a.prec = prec; a.rp = predict_noisy_cov_prec(d, k);
    a.jpc = (m + nchunk - 1) / nchunk;
    a.ppc = (npair + nchunk - 1) / nchunk;
    return a;
}

int launch_predict_noisy_cov_small(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m, int k,
                                   const double *brec, const double *prec, const double *bvec, int nchunk, double *part, long ldp,
                                   double *out) {
    if (n <= 0) return 0;
    if (k < 1 || k > 8 || m < 1 || nchunk < 1) return -1;
    PredNoisyCovArgs a = nc_args(d, Xc, Psic, ldx, n, m, k, brec, prec, nchunk);
    a.part = part; a.ldp = ldp;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nchunk);
#define NC_SMALL(DD) launch_nc<DD>(st, a, grid, shared)
    NC_CASES(NC_SMALL)
#undef NC_SMALL
    if (hipGetLastError() != hipSuccess) return -1;
    return launch_predict_noisy_finish(st, part, nchunk, ldp, n, k, bvec, out);
}

int launch_predict_noisy_cov_phi(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int nrow,
                                 int m, int mp, int k, const double *brec, int nchunk, double *Phi) {
    if (n <= 0) return 0;
    if (m < 1 || nchunk < 1 || nrow < n || mp < m) return -1;
    PredNoisyCovArgs a = nc_args(d, Xc, Psic, ldx, n, m, k, brec, nullptr, nchunk);
    a.Phi = Phi; a.nrow = nrow; a.mp = mp;
    const dim3 grid((unsigned)((nrow + 255) / 256), (unsigned)nchunk);
#define NC_PHI(DD)                                                                                              \
    do {                                                                                                        \
        if (shared) hipLaunchKernelGGL((k_predict_noisy_cov_phi<DD, true>), grid, dim3(256), 0, st, a);         \
        else hipLaunchKernelGGL((k_predict_noisy_cov_phi<DD, false>), grid, dim3(256), 0, st, a);               \
    } while (0)
    NC_CASES(NC_PHI)
#undef NC_PHI
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
