// Rows with a full input-noise covariance through the streaming predictor, covariance kinds (gpz_predictor_run_psi_cube_dev /
// _draws_psi_cube_dev, gpz_predictor.hip): predictNoisy of GC and VC (predictCov.m:70-132) with Psi(:, :, i) as fixPsi.m:36 leaves it,
// the d x d x n cube divided by sdX' sdX.  The frame, the records, the chunks and the order of every sum are k_predict_noisy_cov.hip's;
// what differs is the density's matrix, S + Psi_i over the whole packed triangle (ncov_factor_tri, k_ncov_density.h) where that unit adds
// a diagonal, and the tile's Psi slot: Psic [d (d + 1) / 2][ldx], column q = LT(r, c) the element (r, c), r >= c, of every row's matrix, so
// that a lane's reads are coalesced as they are for Xc.  Only the lower triangle of a row's matrix is ever read.
//
//   k_pred_check_psi_cube           word 3 of the device entries' record is set when an element of a row's lower triangle is NaN or
//                                   infinite, itself or after its division, or a diagonal element is negative
//   k_pred_stage_psi_cube<T>        the caller's cube (f64 or f32; element (r, c) of row i at Psi[r sr + c sc + i sn]) ->
//                                   Psic [d (d + 1) / 2][ldx] = double(psi) / div[LT(r, c)], a plain f64 division (fixPsi.m:36)
//   k_predict_psi_cube_small<D, SHARED, KM>
//       k_predict_noisy_cov_small with M = S + Psi_i: lane = row, 256 rows per workgroup, 32 records per LDS stage read as broadcasts,
//       gridDim.y = predict_noisy_cov_chunks(m, d, k) chunks, partial sums part [C][5k][ldp] for k_predict_noisy_finish.
//   k_predict_psi_cube_phi<D, SHARED>
//       k_predict_noisy_cov_phi with the same density: E_x[PHI] of the tile as launch_tgemm takes it.
// Where the row's triangle lives (psi_cube_regs): SHARED (GC) loads it in front of each phase, factorises S + Psi_i once and drops it.
// VC needs it at every record: up to D = GPZ_PSI_CUBE_REG_D a lane keeps it in registers beside M; above that it reads the coalesced
// columns of Psic again at every record (L1 / L2: a workgroup's 256 rows of one column are 2 KB), which keeps the kernels free of
// scratch at every width.  A cube of diagonals gives the bits of k_predict_noisy_cov.hip's kernels on the same variances: S + 0.0 off the
// diagonal, the same factor and density functions, the same order of the sums.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_ncov_density.h"   // LT, ncov_factor_tri, ncov_density (shared with k_predict_psi_cube_gamma.hip)

#define PC_TP 32   // records per LDS stage

struct PredPsiCubeArgs {
    const double *Xc; long ldx;          // [d][ldx] column layout, n rows
    const double *Psic;                  // [d (d + 1) / 2][ldx]
    int n, m, k;
    const double *brec; int rb;          // basis records of k_noisy_cov_records
    const double *prec; int rp;          // pair records
    int jpc; long ppc;                   // basis functions and pairs per chunk
    double *part; long ldp;              // [chunks][5 k][ldp]
    double *Phi; int nrow, mp;           // k_predict_psi_cube_phi: [nrow][mp]
};

// the lane's triangle for the whole kernel (VC, registers) or, for SHARED, for the factorisation in front of a phase
template <int D>
__device__ __forceinline__ void psi_cube_load(const double *Pg, long ldx, double (&pt)[D * (D + 1) / 2]) {
#pragma unroll
    for (int q = 0; q < D * (D + 1) / 2; ++q) pt[q] = Pg[(size_t)q * ldx];
}

template <int D, bool SHARED, int KM>
__global__ __launch_bounds__(256) void k_predict_psi_cube_small(PredPsiCubeArgs a) {
    constexpr int NP = D * (D + 1) / 2, H = 1 + D + NP;
    constexpr int RJ = H + 2 * KM;
    constexpr bool REG = !SHARED && psi_cube_regs(D);
    __shared__ double sT[PC_TP * (H + 3 * KM)];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const bool act = i < a.n;
    const int ic = act ? i : a.n - 1;
    const int ch = blockIdx.y, m = a.m, k = a.k;
    const double *Pg = a.Psic + ic;   // element q of the row's triangle at Pg[q ldx]
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = a.Xc[(size_t)c * a.ldx + ic];
    double pt[REG ? NP : 1];
    const double *P = Pg;
    long ldq = a.ldx;
    if constexpr (REG) {
        psi_cube_load<D>(Pg, a.ldx, reinterpret_cast<double (&)[NP]>(pt));
        P = pt;
        ldq = 1;
    }
    double M[NP], rd[D], prd;
    double *pp = a.part + (size_t)ch * 5 * k * a.ldp + i;
    // ---- mu and ElnS - b over the chunk's basis functions                                          predictCov.m:75-79
    {
        double mu[KM], el[KM];
#pragma unroll
        for (int o = 0; o < KM; ++o) { mu[o] = 0.0; el[o] = 0.0; }
        const int j0 = ch * a.jpc, j1 = min(m, j0 + a.jpc);
        if (SHARED) {
            double p1[NP];
            psi_cube_load<D>(Pg, a.ldx, p1);
            ncov_factor_tri<D>(a.brec + 1 + D, p1, 1, M, rd, &prd);
        }
        for (int jb = j0; jb < j1; jb += PC_TP) {
            const int nj = min(PC_TP, j1 - jb);
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
                if (!SHARED) ncov_factor_tri<D>(t + 1 + D, P, ldq, M, rd, &prd);
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
        double p2[NP];
        psi_cube_load<D>(Pg, a.ldx, p2);
        ncov_factor_tri<D>(a.prec + 1 + D, p2, 1, M, rd, &prd);
    }
    for (long pb = p0; pb < p1; pb += PC_TP) {
        const int np = (int)min((long)PC_TP, p1 - pb);
        __syncthreads();
        const double *src = a.prec + (size_t)pb * rp;
        for (int t = tid; t < np * rp; t += 256) sT[t] = src[t];
        __syncthreads();
#pragma unroll 1
        for (int e = 0; e < np; ++e) {
            const double *t = sT + e * rp;
            if (!SHARED) ncov_factor_tri<D>(t + 1 + D, P, ldq, M, rd, &prd);   // Cij + Psi(:, :, i)       :109
            const double z = ncov_density<D>(t + 1, t[0], x, M, rd, prd);       //                          :111
            const double *cf = t + H;
#pragma unroll
            for (int o = 0; o < KM; ++o)
                if (o < k) {
                    ga[o] = fma(z, cf[3 * o], ga[o]);                           //                          :113-119
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
__global__ __launch_bounds__(256) void k_predict_psi_cube_phi(PredPsiCubeArgs a) {
    constexpr int NP = D * (D + 1) / 2, H = 1 + D + NP;
    constexpr bool REG = !SHARED && psi_cube_regs(D);
    __shared__ double sT[PC_TP * H];   // the heads of one stage of basis records
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const bool act = i < a.n, st = i < a.nrow;   // rows n .. nrow - 1 are written as zeros
    const int ic = act ? i : a.n - 1;
    const int ch = blockIdx.y, m = a.m;
    const double *Pg = a.Psic + ic;
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = a.Xc[(size_t)c * a.ldx + ic];
    double pt[REG ? NP : 1];
    const double *P = Pg;
    long ldq = a.ldx;
    if constexpr (REG) {
        psi_cube_load<D>(Pg, a.ldx, reinterpret_cast<double (&)[NP]>(pt));
        P = pt;
        ldq = 1;
    }
    double M[NP], rd[D], prd;
    double *row = a.Phi + (size_t)(st ? i : 0) * a.mp;
    const int j0 = ch * a.jpc, j1 = min(m, j0 + a.jpc);
    if (SHARED) {
        double p1[NP];
        psi_cube_load<D>(Pg, a.ldx, p1);
        ncov_factor_tri<D>(a.brec + 1 + D, p1, 1, M, rd, &prd);
    }
    for (int jb = j0; jb < j1; jb += PC_TP) {
        const int nj = min(PC_TP, j1 - jb);
        __syncthreads();
        for (int t = tid; t < nj * H; t += 256) {
            const int jj = t / H;
            sT[t] = a.brec[(size_t)(jb + jj) * a.rb + (t - jj * H)];
        }
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < nj; ++jj) {
            const double *t = sT + jj * H;
            if (!SHARED) ncov_factor_tri<D>(t + 1 + D, P, ldq, M, rd, &prd);
            const double ph = ncov_density<D>(t + 1, t[0], x, M, rd, prd);
            if (st) row[jb + jj] = act ? ph : 0.0;
        }
    }
    if (ch == 0 && st)
        for (int j = m; j < a.mp; ++j) row[j] = 0.0;
}

// ---- byte movers of the device entries ----------------------------------------------------------------------------------------------
// np = d (d + 1) / 2 elements per row, element q = LT(r, c).  div: the divisors sdX[r] sdX[c] in LT order on the device (nullptr: none)
__global__ __launch_bounds__(256) void k_pred_check_psi_cube(const void *__restrict__ Psi, int f32, long ns, int np, long sr, long sc,
                                                             long sn, const double *__restrict__ div, unsigned *__restrict__ rec) {
    const long ne = ns * np, step = (long)gridDim.x * 256;
    int bad = 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < ne; e += step) {
        const int q = (int)(e / ns);          // rows fastest: a contiguous d x d x n cube is read coalesced
        const long i = e - (long)q * ns;
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= q) ++r;
        const int c = q - r * (r + 1) / 2;
        const long at = r * sr + c * sc + i * sn;
        const double v = f32 ? (double)((const float *)Psi)[at] : ((const double *)Psi)[at];
        const double w = div ? v / div[q] : v;
        bad |= !(fabs(v) <= 1.7976931348623157e308) || !(fabs(w) <= 1.7976931348623157e308) || (r == c && !(v >= 0.0));
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(rec + 3, 1u);
}

template <typename T>
__global__ __launch_bounds__(256) void k_pred_stage_psi_cube(const T *__restrict__ Psi, long sr, long sc, long sn, long r0, int nt, int d,
                                                             const double *__restrict__ div, double *__restrict__ Psic, long ldx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const T *row = Psi + (r0 + i) * sn;
    for (int r = 0; r < d; ++r)
        for (int c = 0; c <= r; ++c) {
            double v = (double)row[r * sr + c * sc];
            if (div) v = v / div[LT(r, c)];                                  // Psi ./ (sdX' sdX)        fixPsi.m:36
            Psic[(size_t)LT(r, c) * ldx + i] = v;
        }
}

int launch_pred_check_psi_cube(hipStream_t st, const void *Psi, int f32, long ns, int d, long sr, long sc, long sn, const double *div,
                               unsigned *rec) {
    if (ns <= 0) return 0;
    const int np = d * (d + 1) / 2;
    long nb = (ns * np + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_pred_check_psi_cube, dim3((unsigned)nb), dim3(256), 0, st, Psi, f32, ns, np, sr, sc, sn, div, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pred_stage_psi_cube(hipStream_t st, const void *Psi, int f32, long sr, long sc, long sn, long r0, int nt, int d,
                               const double *div, double *Psic, long ldx) {
    if (nt <= 0) return 0;
    const dim3 grid((unsigned)((nt + 255) / 256));
    if (f32)
        hipLaunchKernelGGL(k_pred_stage_psi_cube<float>, grid, dim3(256), 0, st, (const float *)Psi, sr, sc, sn, r0, nt, d, div, Psic, ldx);
    else
        hipLaunchKernelGGL(k_pred_stage_psi_cube<double>, grid, dim3(256), 0, st, (const double *)Psi, sr, sc, sn, r0, nt, d, div, Psic,
                           ldx);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

#define PC_CASES(MACRO)                                                                                    \
    switch (d) {                                                                                           \
        case 1: MACRO(1); break; case 2: MACRO(2); break; case 3: MACRO(3); break; case 4: MACRO(4); break; \
        case 5: MACRO(5); break; case 6: MACRO(6); break; case 7: MACRO(7); break; case 8: MACRO(8); break; \
        case 9: MACRO(9); break; case 10: MACRO(10); break;                                                \
        default: return -1;                                                                                \
    }

template <int D>
static void launch_pc(hipStream_t st, const PredPsiCubeArgs &a, dim3 grid, bool shared) {
    if (a.k == 1) {
        if (shared) hipLaunchKernelGGL((k_predict_psi_cube_small<D, true, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_predict_psi_cube_small<D, false, 1>), grid, dim3(256), 0, st, a);
    } else {
        if (shared) hipLaunchKernelGGL((k_predict_psi_cube_small<D, true, 8>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_predict_psi_cube_small<D, false, 8>), grid, dim3(256), 0, st, a);
    }
}

// the chunk count comes from the caller: predict_noisy_cov_chunks(m, d, k) of k_predict_noisy_cov.hip
static PredPsiCubeArgs pc_args(int d, const double *Xc, const double *Psic, long ldx, int n, int m, int k, const double *brec,
                               const double *prec, int nchunk) {
    const long npair = (long)m * (m + 1) / 2;
    PredPsiCubeArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.m = m; a.k = k;
    a.brec = brec; a.rb = predict_noisy_cov_brec(d, k);
    a.prec = prec; a.rp = predict_noisy_cov_prec(d, k);
    a.jpc = (m + nchunk - 1) / nchunk;
    a.ppc = (npair + nchunk - 1) / nchunk;
    return a;
}

int launch_predict_psi_cube_small(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m, int k,
                                  const double *brec, const double *prec, const double *bvec, int nchunk, double *part, long ldp,
                                  double *out) {
    if (n <= 0) return 0;
    if (k < 1 || k > 8 || m < 1 || nchunk < 1 || ldx < n || ldp < n) return -1;
    PredPsiCubeArgs a = pc_args(d, Xc, Psic, ldx, n, m, k, brec, prec, nchunk);
    a.part = part; a.ldp = ldp;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nchunk);
#define PC_SMALL(DD) launch_pc<DD>(st, a, grid, shared)
    PC_CASES(PC_SMALL)
#undef PC_SMALL
    if (hipGetLastError() != hipSuccess) return -1;
    return launch_predict_noisy_finish(st, part, nchunk, ldp, n, k, bvec, out);
}

int launch_predict_psi_cube_phi(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m,
                                int mp, int k, const double *brec, int nchunk, double *Phi) {
    if (n <= 0) return 0;
    if (m < 1 || nchunk < 1 || nrow < n || mp < m || ldx < n) return -1;
    PredPsiCubeArgs a = pc_args(d, Xc, Psic, ldx, n, m, k, brec, nullptr, nchunk);
    a.Phi = Phi; a.nrow = nrow; a.mp = mp;
    const dim3 grid((unsigned)((nrow + 255) / 256), (unsigned)nchunk);
#define PC_PHI(DD)                                                                                             \
    do {                                                                                                       \
        if (shared) hipLaunchKernelGGL((k_predict_psi_cube_phi<DD, true>), grid, dim3(256), 0, st, a);         \
        else hipLaunchKernelGGL((k_predict_psi_cube_phi<DD, false>), grid, dim3(256), 0, st, a);               \
    } while (0)
    PC_CASES(PC_PHI)
#undef PC_PHI
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
