// gamma under every weight draw for rows with both input noise and missing inputs (gpz_predictor_stack_noisy_missing_dev /
// _draws_gamma_noisy_missing_dev, gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab EcC_ab(x_i, psi_i) w_s,a w_s,b - mu_s,i^2 per output,
// predictNoisyMissing's gamma (predictDiag.m:257-295) with the draw's weights in place of w; f_ab = 2 off the diagonal, 1 on it.  One tile
// of ONE group of rows that share a NaN pattern, each row with a variance psi per input dimension (Psic, in the layout of Xc).
//
//   k_predict_noisy_missing_gamma   Two MFMAs chained: k_predict_missing_gamma (k_predict_missing_gamma.hip) with the first half's epilogue
//                             replaced by k_predict_noisy_missing_pairs' (k_predict_noisy_missing.hip).  First half: a workgroup of four
//                             waves holds the Pio block of its 32 rows in LDS (row stride nk + 2) and walks the 64-pair groups of its
//                             chunk; wave w takes the 16-pair block 4 g + w of group g, U the A operand fetched four K steps ahead, two
//                             MFMAs per K step; lane l owns rows l & 15 and 16 + (l & 15) and, in accumulator register r, pair
//                             (l >> 4) + 4 r of the block.  The block's rows of X and of Psi sit in LDS, zero where missing or past n.
//                             Per observed dimension r = (C_qc + psi_ic)^-1/2 (pn_rsqrt), z = acc exp(lnZ_q - 1/2 sum_o (Delta r)^2) prod_o r,
//                             the loop over the set bits of obs (scalar control flow): no NaN of X and no value of Psi from a missing
//                             dimension enters arithmetic.  Of a record of the SECOND table (k_pnm_records: C, not 1 / C, and lnZ without
//                             the determinant) only [lnZ | c | C] is staged; the 3k coefficients carry w, which is the draw's here.
//                             Second half, k_predict_missing_gamma's unchanged: result register r of the first product is, as it stands,
//                             the B operand of one K step over the pairs 4 r .. 4 r + 3; A = Wp = (f W[a, col]) W[b, col] formed in registers
//                             from two rows of the handle's W (m x ldw row-major); (a, b) of the group's 64 pairs formed by 64 threads
//                             while the records are staged, (0, 0) past the last pair (z is 0 there and the rows of W exist).  Per
//                             16-column block one accumulator pair per row half.  Up to GPZ_NMGAMMA_NB = 8 column blocks (128 columns) per
//                             launch, instantiated for every count 1 .. 8: the rsqrt chains of the epilogue end before the second
//                             product begins, so all eight fit two workgroups per compute unit without a spill (118 .. 244 VGPRs,
//                             DESIGN.md section 23).  More columns are further launches that form z again.  gridDim.y:
//                             predict_missing_chunks(m) chunks of the groups.
//                             At the end the four waves are added in wave order through LDS, one column block at a time ([4][32][16]
//                             doubles, inside the block the kernel already holds), into part [C][ncol][ldp].
//                             LDS: max(32 (nk + 2) + 64 (1 + 2 d) + 64 d + 64, 2048) doubles (predict_noisy_missing_gamma_lds).
//   k_gamma_finish_dev / _s2  (k_predict_noisy_gamma.hip) add the chunks in chunk order and subtract mu_s^2.
// No atomics; every sum starts from zero and runs in one order that the model's shape fixes: a row's gamma_s has the same bits for any
// tile size, row order, position in its block, other rows or groups of the call and any number of draws > s.
#include "gpz_dev.h"
#include "gpz_kernels.h"

#define GPZ_NMGAMMA_NB 8  // most 16-column blocks of accumulators per launch

// q = i (i + 1) / 2 + j, j <= i (k_predict_missing.hip's pmd_pair_of)
__device__ __forceinline__ void pnmg_pair_of(long q, int *pi, int *pj) {
    long i = (long)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= q) ++i;
    while (i * (i + 1) / 2 > q) --i;
    *pi = (int)i;
    *pj = (int)(q - i * (i + 1) / 2);
}

// 1 / sqrt(p): v_rsq_f64 seed and two Newton steps (k_predict_noisy.hip's pn_rsqrt)
__device__ __forceinline__ double pnmg_rsqrt(double p) {
    double y = __builtin_amdgcn_rsq(p);
    const double h = 0.5 * p;
    double e = fma(-h * y, y, 0.5);
    y = fma(y, e, y);
    e = fma(-h * y, y, 0.5);
    y = fma(y, e, y);
    return y;
}

struct PredNoisyMissGammaArgs {
    const double *Xc, *Psic; long ldx; int n;   // the tile's rows and their variances, [d][ldx]
    const double *Pio; int ldpio;               // [rows][ldpio]
    int nk;                                     // ceil16(m): K of the first product
    const double *U;                            // in fragment order (k_pmd_u)
    const double *rec; int nrec;                // pair records (k_pnm_records), nrec doubles apart, whole groups of 64; the first 1 + 2 d are read
    int d;
    unsigned obs;
    int npair;                                  // m (m + 1) / 2
    int ngrp, gpc;                              // groups of 64 pairs in all, and per chunk
    const double *W; int ldw;                   // >= m rows x ldw row-major, ldw a multiple of 16, columns >= ncol zero
    int ncol, cb0;                              // columns; the first 16-column block of this launch (cb0 + NB <= ldw / 16)
    double *part; long ldp;                     // [chunks][ncol][ldp]
};

template <int NB>
__global__ __launch_bounds__(256, 2) void k_predict_noisy_missing_gamma(PredNoisyMissGammaArgs a) {
    extern __shared__ double smem[];
    const int nk = a.nk, lda = nk + 2, d = a.d, rl = 1 + 2 * d;
    double *sP = smem;                   // [32][lda]: Pio of the block
    double *sR = sP + 32 * lda;          // [64][rl]: lnZ | c | C of the group's pairs
    double *sX = sR + 64 * rl;           // [32][d]: the block's rows, zero where missing
    double *sS = sX + 32 * d;            // [32][d]: their variances, zero where missing
    int *sAB = (int *)(sS + 32 * d);     // [64][2]: (a, b) of the group's pairs
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long i0 = (long)blockIdx.x * 32;
    const int ch = blockIdx.y, cb0 = a.cb0;
    const unsigned obs = a.obs;
    for (int e = tid; e < 32 * nk; e += 256) {
        const int r = e / nk, c = e - r * nk;
        sP[r * lda + c] = (i0 + r < a.n) ? a.Pio[(size_t)(i0 + r) * a.ldpio + c] : 0.0;
    }
    for (int e = tid; e < 32 * d; e += 256) {
        const int r = e / d, c = e - r * d;
        const bool in = ((obs >> c) & 1u) && i0 + r < a.n;
        sX[e] = in ? a.Xc[(size_t)c * a.ldx + i0 + r] : 0.0;
        sS[e] = in ? a.Psic[(size_t)c * a.ldx + i0 + r] : 0.0;
    }
    d4_t g0a[NB], g1a[NB];   // rows l & 15 and 16 + (l & 15); register r: column 16 (cb0 + qb) + (l >> 4) + 4 r
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) { g0a[qb] = (d4_t){0.0, 0.0, 0.0, 0.0}; g1a[qb] = (d4_t){0.0, 0.0, 0.0, 0.0}; }
    const int nks = nk >> 2;             // K steps of 4 (a multiple of 4)
    const double *pa0 = sP + (lane & 15) * lda + (lane >> 4), *pa1 = pa0 + 16 * lda;
    const double *x0 = sX + (lane & 15) * d, *x1 = x0 + 16 * d;
    const double *s0 = sS + (lane & 15) * d, *s1 = s0 + 16 * d;
    const double *rb = sR + (16 * wv + (lane >> 4)) * rl;     // the records of pairs (lane >> 4) + 4 r of this wave's block, r = 0 .. 3
    const int *ab = sAB + 2 * (16 * wv + (lane >> 4));
    const double *wl = a.W + (size_t)cb0 * 16 + (lane & 15);  // column 16 cb0 + (l & 15) < ldw
    const int g0 = ch * a.gpc, g1 = min(a.ngrp, g0 + a.gpc);
    for (int g = g0; g < g1; ++g) {
        __syncthreads();   // the group before is read (first trip: sP, sX and sS are written)
        {
            const double *src = a.rec + (size_t)g * 64 * a.nrec;
            for (int t = tid; t < 64 * rl; t += 256) {
                const int j = t / rl, f = t - j * rl;
                sR[t] = src[(size_t)j * a.nrec + f];
            }
            if (tid < 64) {
                const int q = g * 64 + tid;
                int pi = 0, pj = 0;
                if (q < a.npair) pnmg_pair_of(q, &pi, &pj);   // past the last pair: (0, 0), rows of W that exist
                sAB[2 * tid] = pi;
                sAB[2 * tid + 1] = pj;
            }
        }
        const double *ub = a.U + ((size_t)(4 * g + wv) * nks) * 64 + lane;
        d4_t acc0 = (d4_t){0.0, 0.0, 0.0, 0.0}, acc1 = (d4_t){0.0, 0.0, 0.0, 0.0};
        double ua[4], un[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q) ua[q] = ub[q * 64];
        for (int ks = 0; ks < nks; ks += 4) {
            if (ks + 4 < nks) {
#pragma unroll
                for (int q = 0; q < 4; ++q) un[q] = ub[(size_t)(ks + 4 + q) * 64];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc0 = MFMA_F64(ua[q], pa0[4 * (ks + q)], acc0);
                acc1 = MFMA_F64(ua[q], pa1[4 * (ks + q)], acc1);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) ua[q] = un[q];
        }
        __syncthreads();   // the records and (a, b) are in LDS
        // ---- acc0[r], acc1[r] = sum_l Pio(row, l) Nu_q(l) for rows l & 15, 16 + (l & 15) and pair q = (l >> 4) + 4 r           :271-272
        double qa[4] = {0.0, 0.0, 0.0, 0.0}, qb4[4] = {0.0, 0.0, 0.0, 0.0};
        double ra[4] = {1.0, 1.0, 1.0, 1.0}, rb4[4] = {1.0, 1.0, 1.0, 1.0};
        for (unsigned mk = obs; mk; mk &= mk - 1) {   // the observed dimensions only (uniform: scalar control flow)
            const int c = __builtin_ctz(mk);
            const double xa = x0[c], xb = x1[c], pa = s0[c], pb = s1[c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double *t = rb + 4 * r * rl;
                const double cc = t[1 + c], C = t[1 + d + c];
                const double ia = pnmg_rsqrt(C + pa), ib = pnmg_rsqrt(C + pb);   // (Cij + Psi)^-1/2            :264-265
                const double da = (xa - cc) * ia, db = (xb - cc) * ib;
                qa[r] = fma(da, da, qa[r]);
                qb4[r] = fma(db, db, qb4[r]);
                ra[r] *= ia;
                rb4[r] *= ib;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double lz = rb[4 * r * rl];
            const double za = acc0[r] * (exp(lz - 0.5 * qa[r]) * ra[r]), zb = acc1[r] * (exp(lz - 0.5 * qb4[r]) * rb4[r]);   // :275
            // ---- z(pair 4 r + (l >> 4), row l & 15) is the B operand of a K step over the pairs 4 r .. 4 r + 3
            const int pa = ab[8 * r], pb = ab[8 * r + 1];
            const double f = pa == pb ? 1.0 : 2.0;                     // :277-284
            const double *wa = wl + pa * a.ldw, *wb = wl + pb * a.ldw;   // < 256 * 528: an int
#pragma unroll
            for (int qb = 0; qb < NB; ++qb) {
                const double wp = (f * wa[16 * qb]) * wb[16 * qb];
                g0a[qb] = MFMA_F64(wp, za, g0a[qb]);
                g1a[qb] = MFMA_F64(wp, zb, g1a[qb]);
            }
        }
    }
    // ---- the waves in their order, one column block at a time
    double *sRed = smem;   // [4 waves][32 rows][16 columns]
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) {
        __syncthreads();   // every wave is done with sP, sR, sX, sS and sAB, or with the block before
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int cl = (lane >> 4) + 4 * r;
            sRed[(wv * 32 + (lane & 15)) * 16 + cl] = g0a[qb][r];
            sRed[(wv * 32 + 16 + (lane & 15)) * 16 + cl] = g1a[qb][r];
        }
        __syncthreads();
        for (int t = tid; t < 32 * 16; t += 256) {
            const int row = t & 31, cl = t >> 5, col = (cb0 + qb) * 16 + cl;
            const int at = row * 16 + cl;
            const double s = ((sRed[at] + sRed[512 + at]) + sRed[1024 + at]) + sRed[1536 + at];
            if (i0 + row < a.n && col < a.ncol) a.part[((size_t)ch * a.ncol + col) * a.ldp + i0 + row] = s;
        }
    }
}

// dynamic LDS of k_predict_noisy_missing_gamma, bytes: k_predict_missing_gamma's block and the block's 32 rows of Psi
size_t predict_noisy_missing_gamma_lds(int m, int d) {
    const size_t nk = ((size_t)m + 15) / 16 * 16;
    const size_t work = 32 * (nk + 2) + 64 * (1 + 2 * (size_t)d) + 64 * (size_t)d + 64, red = 4 * 32 * 16;
    return (work > red ? work : red) * sizeof(double);
}

int launch_predict_noisy_missing_gamma(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio, int ldpio,
                                       int m, int d, int k, unsigned obs, const double *U, const double *rec, const double *W, int ldw,
                                       int ncol, int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > 20 || k < 1 || k > 8 || m < 1 || ((m + 15) / 16) * 16 > 256 || nchunk != predict_missing_chunks(m) || ldw % 16 ||
        ncol > ldw || ldp < n)
        return -1;
    PredNoisyMissGammaArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.Pio = Pio; a.ldpio = ldpio; a.nk = ((m + 15) / 16) * 16; a.U = U; a.rec = rec;
    a.nrec = predict_missing_rec(d, k); a.d = d; a.obs = obs;
    a.npair = m * (m + 1) / 2;
    a.ngrp = (int)predict_missing_groups(m);
    a.gpc = (a.ngrp + nchunk - 1) / nchunk;
    a.W = W; a.ldw = ldw; a.ncol = ncol;
    a.part = part; a.ldp = ldp;
    const size_t lds = predict_noisy_missing_gamma_lds(m, d);
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)nchunk);
    const int nbw = (ncol + 15) / 16;   // <= ldw / 16
    // GPZ_NMGAMMA_NB blocks per launch and the rest in a last one, each instantiated for its count: no test per block in the kernel.
    // The attribute per launch, not once per process: it belongs to the current device's copy of the kernel
    for (a.cb0 = 0; a.cb0 < nbw; a.cb0 += GPZ_NMGAMMA_NB) {
        switch (nbw - a.cb0 < GPZ_NMGAMMA_NB ? nbw - a.cb0 : GPZ_NMGAMMA_NB) {
#define PNMG_CASE(NBT)                                                                                                                 \
    case NBT:                                                                                                                          \
        if (lds > 65536 && hipFuncSetAttribute((const void *)k_predict_noisy_missing_gamma<NBT>,                                       \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)                    \
            return -1;                                                                                                                 \
        hipLaunchKernelGGL(k_predict_noisy_missing_gamma<NBT>, grid, dim3(256), lds, st, a);                                           \
        break;
            PNMG_CASE(1) PNMG_CASE(2) PNMG_CASE(3) PNMG_CASE(4) PNMG_CASE(5) PNMG_CASE(6) PNMG_CASE(7) PNMG_CASE(8)
#undef PNMG_CASE
            default: return -1;
        }
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}
