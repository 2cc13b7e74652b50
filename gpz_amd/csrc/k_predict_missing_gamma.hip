// gamma under every weight draw for rows with missing inputs (gpz_predictor_stack_missing_dev / _draws_gamma_missing_dev, gpz_predictor.hip):
// gamma_s,i = sum_{a >= b} f_ab EcC_ab(x_i) w_s,a w_s,b - mu_s,i^2 per output, predictMissing's gamma (predictDiag.m:172-198, :209) with the
// draw's weights in place of w; f_ab = 2 off the diagonal, 1 on it.  One tile of ONE group of rows that share a NaN pattern.
//
//   k_predict_missing_gamma   Two MFMAs chained.  The first half is k_predict_missing_pairs' own (k_predict_missing.hip): a workgroup of four
//                             waves holds the Pio block of its 32 rows in LDS and walks the 64-pair groups of its chunk; wave w takes the
//                             16-pair block 4 g + w of group g, one K loop over nk with the U fragments fetched four steps ahead, U the A
//                             operand, so that lane l owns rows l & 15 and 16 + (l & 15) and, in accumulator register r, pair
//                             (l >> 4) + 4 r of the block; z = acc exp(lnZ_q - 1/2 sum_c (x_c - c_qc)^2 / C_qc) in the accumulators.  Of a
//                             record only [lnZ | c | 1 / C] is staged (the 3k coefficients carry w, which is the draw's here).
//                             The second half: for v_mfma_f64_16x16x4_f64 the result map (col = l & 15, row = (l >> 4) + 4 reg) of
//                             register r IS the B operand map (B[k = l >> 4][j = l & 15]) of one K step over the pairs 4 r .. 4 r + 3 of
//                             the block, so z goes from the first product into the second without a move.  The A operand is
//                             Wp[col 16 cb + (l & 15)][pair (l >> 4) + 4 r] = (f W[a, col]) W[b, col], formed in registers from two rows of
//                             the handle's W (m x ldw row-major, column o nd + s; L1 / L2).  Per 16-pair block, 16-column block cb, r and
//                             row half one MFMA: the accumulator of (cb, half) then holds, per lane, row l & 15 (or 16 + (l & 15)) and the
//                             columns 16 cb + (l >> 4) + 4 r'.  Each (row, column) lives in one lane of a wave: no lane butterfly.
//                             (a, b) of the group's 64 pairs are formed by 64 threads (pmd_pair_of) while the records are staged, and
//                             read from LDS: stepping a lane's pair by 64 would wrap up to 64 rows of the triangle at small a.  Pairs
//                             past the last one get (0, 0): their z is 0 (U and the records are zero there) and the rows of W exist.
//                             Up to GPZ_MGAMMA_NB = 8 column blocks (128 columns, 128 accumulator registers) per launch, the kernel
//                             instantiated for every count 1 .. 8 (a count read at run time kept one test per block in scalar
//                             registers and spilled them); more columns are further launches that form z again.  gridDim.y:
//                             predict_missing_chunks(m) chunks of the groups.
//                             At the end the four waves are added in wave order through LDS, one column block at a time ([4][32][16]
//                             doubles, inside the block the kernel already holds), into part [C][ncol][ldp].
//                             LDS: max(32 (nk + 2) + 64 (1 + 2 d) + 32 d + 64, 2048) doubles (predict_missing_gamma_lds).
//   k_gamma_finish_dev / _s2  (k_predict_noisy_gamma.hip) add the chunks in chunk order and subtract mu_s^2.
// No atomics; every sum starts from zero and runs in one order that the model's shape fixes (the pairs of a wave's blocks in table order,
// the waves in wave order, the chunks in chunk order): a row's gamma_s has the same bits for any tile size, row order, position in its
// block, other rows or groups of the call and any number of draws > s.
#include "gpz_dev.h"
#include "gpz_kernels.h"

#define GPZ_MGAMMA_NB 8   // most 16-column blocks of accumulators per launch

// q = i (i + 1) / 2 + j, j <= i (k_predict_missing.hip's pmd_pair_of)
__device__ __forceinline__ void pmg_pair_of(long q, int *pi, int *pj) {
    long i = (long)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= q) ++i;
    while (i * (i + 1) / 2 > q) --i;
    *pi = (int)i;
    *pj = (int)(q - i * (i + 1) / 2);
}

struct PredMissGammaArgs {
    const double *Xc; long ldx; int n;   // the tile's rows, [d][ldx]
    const double *Pio; int ldpio;        // [rows][ldpio]
    int nk;                              // ceil16(m): K of the first product
    const double *U;                     // in fragment order (k_pmd_u)
    const double *rec; int nrec;         // pair records, nrec doubles apart, whole groups of 64; the first 1 + 2 d are read
    int d;
    unsigned obs;
    int npair;                           // m (m + 1) / 2
    int ngrp, gpc;                       // groups of 64 pairs in all, and per chunk
    const double *W; int ldw;            // >= m rows x ldw row-major, ldw a multiple of 16, columns >= ncol zero
    int ncol, cb0;                       // columns; the first 16-column block of this launch (cb0 + NB <= ldw / 16)
    double *part; long ldp;              // [chunks][ncol][ldp]
};

template <int NB>
__global__ __launch_bounds__(256, 2) void k_predict_missing_gamma(PredMissGammaArgs a) {
    extern __shared__ double smem[];
    const int nk = a.nk, lda = nk + 2, d = a.d, rl = 1 + 2 * d;
    double *sP = smem;                   // [32][lda]: Pio of the block
    double *sR = sP + 32 * lda;          // [64][rl]: lnZ | c | 1 / C of the group's pairs
    double *sX = sR + 64 * rl;           // [32][d]: the block's rows, zero where missing
    int *sAB = (int *)(sX + 32 * d);     // [64][2]: (a, b) of the group's pairs
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long i0 = (long)blockIdx.x * 32;
    const int ch = blockIdx.y, cb0 = a.cb0;
    for (int e = tid; e < 32 * nk; e += 256) {
        const int r = e / nk, c = e - r * nk;
        sP[r * lda + c] = (i0 + r < a.n) ? a.Pio[(size_t)(i0 + r) * a.ldpio + c] : 0.0;
    }
    for (int e = tid; e < 32 * d; e += 256) {
        const int r = e / d, c = e - r * d;
        sX[e] = (((a.obs >> c) & 1u) && i0 + r < a.n) ? a.Xc[(size_t)c * a.ldx + i0 + r] : 0.0;
    }
    d4_t g0a[NB], g1a[NB];   // rows l & 15 and 16 + (l & 15); register r: column 16 (cb0 + qb) + (l >> 4) + 4 r
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) { g0a[qb] = (d4_t){0.0, 0.0, 0.0, 0.0}; g1a[qb] = (d4_t){0.0, 0.0, 0.0, 0.0}; }
    const int nks = nk >> 2;             // K steps of 4 (a multiple of 4)
    const double *pa0 = sP + (lane & 15) * lda + (lane >> 4), *pa1 = pa0 + 16 * lda;
    const double *x0 = sX + (lane & 15) * d, *x1 = x0 + 16 * d;
    const double *rb = sR + (16 * wv + (lane >> 4)) * rl;     // the records of pairs (lane >> 4) + 4 r of this wave's block, r = 0 .. 3
    const int *ab = sAB + 2 * (16 * wv + (lane >> 4));
    const double *wl = a.W + (size_t)cb0 * 16 + (lane & 15);  // column 16 cb0 + (l & 15) < ldw
    const int g0 = ch * a.gpc, g1 = min(a.ngrp, g0 + a.gpc);
    for (int g = g0; g < g1; ++g) {
        __syncthreads();   // the group before is read (first trip: sP and sX are written)
        {
            const double *src = a.rec + (size_t)g * 64 * a.nrec;
            for (int t = tid; t < 64 * rl; t += 256) {
                const int j = t / rl, f = t - j * rl;
                sR[t] = src[(size_t)j * a.nrec + f];
            }
            if (tid < 64) {
                const int q = g * 64 + tid;
                int pi = 0, pj = 0;
                if (q < a.npair) pmg_pair_of(q, &pi, &pj);   // past the last pair: (0, 0), rows of W that exist
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
        // ---- acc0[r], acc1[r] = sum_l Pio(row, l) Nu_q(l) for rows l & 15, 16 + (l & 15) and pair q = (l >> 4) + 4 r           :185-186
        double qa[4] = {0.0, 0.0, 0.0, 0.0}, qb4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < d; ++c) {
            const double xa = x0[c], xb = x1[c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double *t = rb + 4 * r * rl;
                const double cc = t[1 + c], ic = t[1 + d + c];
                const double da = xa - cc, db = xb - cc;
                qa[r] = fma(da * da, ic, qa[r]);                       // :178-179
                qb4[r] = fma(db * db, ic, qb4[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double lz = rb[4 * r * rl];
            const double za = acc0[r] * exp(lz - 0.5 * qa[r]), zb = acc1[r] * exp(lz - 0.5 * qb4[r]);   // :189
            // ---- z(pair 4 r + (l >> 4), row l & 15) is the B operand of a K step over the pairs 4 r .. 4 r + 3
            const int pa = ab[8 * r], pb = ab[8 * r + 1];
            const double f = pa == pb ? 1.0 : 2.0;                     // :191-198
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
        __syncthreads();   // every wave is done with sP, sR, sX and sAB, or with the block before
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

size_t predict_missing_gamma_lds(int m, int d) {
    const size_t nk = ((size_t)m + 15) / 16 * 16;
    const size_t work = 32 * (nk + 2) + 64 * (1 + 2 * (size_t)d) + 32 * (size_t)d + 64, red = 4 * 32 * 16;
    return (work > red ? work : red) * sizeof(double);
}

int launch_predict_missing_gamma(hipStream_t st, const double *Xc, long ldx, int n, const double *Pio, int ldpio, int m, int d, int k,
                                 unsigned obs, const double *U, const double *rec, const double *W, int ldw, int ncol, int nchunk,
                                 double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > 20 || k < 1 || k > 8 || m < 1 || ((m + 15) / 16) * 16 > 256 || nchunk != predict_missing_chunks(m) || ldw % 16 ||
        ncol > ldw || ldp < n)
        return -1;
    PredMissGammaArgs a{};
    a.Xc = Xc; a.ldx = ldx; a.n = n; a.Pio = Pio; a.ldpio = ldpio; a.nk = ((m + 15) / 16) * 16; a.U = U; a.rec = rec;
    a.nrec = predict_missing_rec(d, k); a.d = d; a.obs = obs;
    a.npair = m * (m + 1) / 2;
    a.ngrp = (int)predict_missing_groups(m);
    a.gpc = (a.ngrp + nchunk - 1) / nchunk;
    a.W = W; a.ldw = ldw; a.ncol = ncol;
    a.part = part; a.ldp = ldp;
    const size_t lds = predict_missing_gamma_lds(m, d);
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)nchunk);
    const int nbw = (ncol + 15) / 16;   // <= ldw / 16
    // GPZ_MGAMMA_NB blocks per launch and the rest in a last one, each instantiated for its count: no test per block in the kernel.
    // The attribute per launch, not once per process: it belongs to the current device's copy of the kernel
    for (a.cb0 = 0; a.cb0 < nbw; a.cb0 += GPZ_MGAMMA_NB) {
        switch (nbw - a.cb0 < GPZ_MGAMMA_NB ? nbw - a.cb0 : GPZ_MGAMMA_NB) {
#define PMG_CASE(NBT)                                                                                                                  \
    case NBT:                                                                                                                          \
        if (lds > 65536 && hipFuncSetAttribute((const void *)k_predict_missing_gamma<NBT>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                               (int)lds) != hipSuccess)                                                                \
            return -1;                                                                                                                 \
        hipLaunchKernelGGL(k_predict_missing_gamma<NBT>, grid, dim3(256), lds, st, a);                                                 \
        break;
            PMG_CASE(1) PMG_CASE(2) PMG_CASE(3) PMG_CASE(4) PMG_CASE(5) PMG_CASE(6) PMG_CASE(7) PMG_CASE(8)
#undef PMG_CASE
            default: return -1;
        }
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}
