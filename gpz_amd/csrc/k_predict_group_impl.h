// The pair product of one group of rows that share a NaN pattern, shared by its four units as k_predict_draws_impl.h is by its two:
//   k_predict_missing.hip               k_predict_missing_pairs<KM>         clean z, the pairs sink
//   k_predict_noisy_missing.hip         k_predict_noisy_missing_pairs<KM>   z with Psi, the pairs sink
//   k_predict_missing_gamma.hip         k_predict_missing_gamma<NB>         clean z, the gamma sink
//   k_predict_noisy_missing_gamma.hip   k_predict_noisy_missing_gamma<NB>   z with Psi, the gamma sink
// The kernels are wrappers around predict_group_body<PSI, Sink>; what follows is described here once.
//
// The product.  A workgroup of four waves holds the Pio block of its 32 rows in LDS (row stride nk + 2) and walks the 64-pair groups of
// its chunk (gridDim.y = predict_missing_chunks(m) chunks of the groups); wave w takes the 16-pair block 4 g + w of group g: one MFMA K
// loop over nk with the U fragments (k_pmd_u's order) fetched four steps ahead, the product transposed (U is the A operand) so that lane l
// owns rows l & 15 and 16 + (l & 15) and, in accumulator register r, pair (l >> 4) + 4 r of the block.  The group's 64 records are staged
// in LDS between the two barriers while the K loop runs and read as broadcasts (one address per 16 lanes).  The block's rows of X (and of
// Psi) sit in LDS, zero where missing or past n.
//
// z from the accumulators, one of two forms:
//   clean   z = acc exp(lnZ_q - 1/2 sum_c (x_c - c_qc)^2 / C_qc) over all d, on k_pmd_pairs' records [lnZ incl. the determinant | c | 1 / C],
//           which are zero in the missing dimensions (predictDiag.m:178-189)
//   PSI     per observed dimension r = (C_qc + psi_ic)^-1/2 (rsqrt_nr2), z = acc exp(lnZ_q - 1/2 sum_o (Delta r)^2) prod_o r, on
//           k_pnm_records' table [lnZ without the determinant | c | C]; the loop runs over the set bits of obs (scalar control flow), so
//           no NaN of X and no value of Psi from a missing dimension enters arithmetic (:264-275)
// and what consumes it, in the same r loop, one of two sinks:
//   PredPairsSink<KM>   three FMAs per output against the record's coefficients [f w_i w_j, f v_i v_j, f iS(i, j)] into the lane's running
//           sums; at the end the sums are added over the four lane groups (two butterfly steps) and over the waves (in wave order,
//           through LDS) into part [C][3k][ldp] = gamma | VlnS | nu.  The whole record is staged.
//   PredGammaSink<NB>   a second MFMA.  For v_mfma_f64_16x16x4_f64 the result map (col = l & 15, row = (l >> 4) + 4 reg) of register r IS
//           the B operand map (B[k = l >> 4][j = l & 15]) of one K step over the pairs 4 r .. 4 r + 3 of the block, so z goes from the first
//           product into the second without a move.  The A operand is Wp[col 16 cb + (l & 15)][pair (l >> 4) + 4 r] = (f W[a, col]) W[b, col],
//           formed in registers from two rows of the handle's W (m x ldw row-major, column o nd + s).  (a, b) of the group's 64 pairs are
//           formed by 64 threads while the records are staged, and read from LDS; pairs past the last one get (0, 0): their z is 0 and
//           the rows of W exist.  Per 16-column block one accumulator pair per row half; each (row, column) lives in one lane of a wave:
//           no lane butterfly.  At the end the four waves are added in wave order through LDS, one column block at a time ([4][32][16]
//           doubles), into part [C][ncol][ldp].  Of a record only the first 1 + 2 d doubles are staged (the coefficients carry w, which
//           is the draw's here).
// No atomics; every sum starts from zero and runs in one order that the model's shape fixes (the pairs of a wave's blocks in table order,
// the waves in wave order, the chunks in chunk order): a row's results have the same bits for any tile size, row order and position.
// LDS: sP [32][nk + 2] | sR [64][record] | sX [32][d] | sS [32][d] with PSI | sAB [64] int2 for the gamma sink, and at least the
// sink's last reduction (predict_missing_lds, predict_missing_gamma_lds).
#pragma once
#include "gpz_dev.h"

struct PredGroupArgs {
    const double *Xc, *Psic; long ldx; int n;   // the tile's rows and, with PSI, their variances, [d][ldx]; Psic nullptr without
    const double *Pio; int ldpio;               // [rows][ldpio]
    int nk;                                     // ceil16(m): K of the product
    const double *U;                            // in fragment order (k_pmd_u)
    const double *rec; int nrec;                // pair records (k_pmd_pairs, with PSI k_pnm_records), nrec doubles apart, whole groups of 64
    int d, k;
    unsigned obs;
    int ngrp, gpc;                              // groups of 64 pairs in all, and per chunk
    double *part; long ldp;                     // pairs: [chunks][3 k][ldp] = gamma | VlnS | nu; gamma: [chunks][ncol][ldp]
    // the gamma sink only
    int npair;                                  // m (m + 1) / 2
    const double *W; int ldw;                   // >= m rows x ldw row-major, ldw a multiple of 16, columns >= ncol zero
    int ncol, cb0;                              // columns; the first 16-column block of this launch (cb0 + NB <= ldw / 16)
};

// where a thread stands: its lane and wave, the block's first row and the chunk
struct PredGroupAt {
    int tid, lane, wv, ch;
    long i0;
};

template <int KM>
struct PredPairsSink {
    static constexpr bool FULL_RECORD = true;
    double ga[2][KM], vl[2][KM], nu[2][KM];

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int o = 0; o < KM; ++o) { ga[0][o] = ga[1][o] = 0.0; vl[0][o] = vl[1][o] = 0.0; nu[0][o] = nu[1][o] = 0.0; }
    }
    __device__ __forceinline__ void stage(const PredGroupArgs &, const PredGroupAt &, int2 *, int) {}
    // za, zb: z of rows l & 15, 16 + (l & 15) and pair (l >> 4) + 4 r; t: that pair's record
    __device__ __forceinline__ void take(const PredGroupArgs &a, const PredGroupAt &, const int2 *, int, double za, double zb, const double *t) {
        const int k = a.k;
        const double *cf = t + 1 + 2 * a.d;
#pragma unroll
        for (int o = 0; o < KM; ++o) {
            if (o >= k) break;   // (a test per output instead of the break costs four spilled scalar registers at KM = 8)
            const double c0 = cf[3 * o], c1 = cf[3 * o + 1], c2 = cf[3 * o + 2];
            ga[0][o] = fma(za, c0, ga[0][o]); ga[1][o] = fma(zb, c0, ga[1][o]);   // :191-198, :277-284
            vl[0][o] = fma(za, c1, vl[0][o]); vl[1][o] = fma(zb, c1, vl[1][o]);
            nu[0][o] = fma(za, c2, nu[0][o]); nu[1][o] = fma(zb, c2, nu[1][o]);
        }
    }
    // the four lane groups of a wave, then the waves in their order
    __device__ __forceinline__ void reduce(const PredGroupArgs &a, const PredGroupAt &at, double *smem) {
        const int tid = at.tid, lane = at.lane, wv = at.wv, ch = at.ch, k = a.k, n = a.n;
        const long i0 = at.i0, ldp = a.ldp;
        double *part = a.part;
        __syncthreads();   // every wave is done with the working block
        double *sRed = smem;   // [4 waves][32 rows][3 KM]
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int o = 0; o < KM; ++o) {
                double v3[3] = {ga[s][o], vl[s][o], nu[s][o]};
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    double v = v3[q];
                    v += __shfl_xor(v, 16, 64);
                    v += __shfl_xor(v, 32, 64);
                    if (lane < 16) sRed[((wv * 32) + 16 * s + lane) * 3 * KM + q * KM + o] = v;
                }
            }
        __syncthreads();
        for (int t = tid; t < 32 * 3 * k; t += 256) {
            const int row = t & 31, e = t >> 5, q = e / k, o = e - q * k;
            const int ix = row * 3 * KM + q * KM + o;
            const double s = ((sRed[ix] + sRed[32 * 3 * KM + ix]) + sRed[2 * 32 * 3 * KM + ix]) + sRed[3 * 32 * 3 * KM + ix];
            if (i0 + row < n) part[((size_t)ch * 3 * k + e) * ldp + i0 + row] = s;
        }
    }
};

template <int NB>
struct PredGammaSink {
    static constexpr bool FULL_RECORD = false;
    d4_t g0a[NB], g1a[NB];   // rows l & 15 and 16 + (l & 15); register r: column 16 (cb0 + qb) + (l >> 4) + 4 r

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) { g0a[qb] = (d4_t){0.0, 0.0, 0.0, 0.0}; g1a[qb] = (d4_t){0.0, 0.0, 0.0, 0.0}; }
    }
    // sAB [64]: (a, b) of the group's pairs
    __device__ __forceinline__ void stage(const PredGroupArgs &a, const PredGroupAt &at, int2 *sAB, int g) {
        if (at.tid < 64) {
            const int q = g * 64 + at.tid;
            int pi = 0, pj = 0;
            if (q < a.npair) gpz_pair_of(q, &pi, &pj);   // past the last pair: (0, 0), rows of W that exist
            sAB[at.tid] = make_int2(pi, pj);
        }
    }
    // z(pair 4 r + (l >> 4), row l & 15) is the B operand of a K step over the pairs 4 r .. 4 r + 3
    __device__ __forceinline__ void take(const PredGroupArgs &a, const PredGroupAt &at, const int2 *sAB, int r, double za, double zb,
                                         const double *) {
        const int2 *ab = sAB + 16 * at.wv + (at.lane >> 4);
        const double *wl = a.W + (size_t)a.cb0 * 16 + (at.lane & 15);   // column 16 cb0 + (l & 15) < ldw
        const int pa = ab[4 * r].x, pb = ab[4 * r].y;
        const double f = pa == pb ? 1.0 : 2.0;                       // :191-198, :277-284
        const double *wa = wl + pa * a.ldw, *wb = wl + pb * a.ldw;   // < 256 * 528: an int
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
            const double wp = (f * wa[16 * qb]) * wb[16 * qb];
            g0a[qb] = MFMA_F64(wp, za, g0a[qb]);
            g1a[qb] = MFMA_F64(wp, zb, g1a[qb]);
        }
    }
    // the waves in their order, one column block at a time
    __device__ __forceinline__ void reduce(const PredGroupArgs &a, const PredGroupAt &at, double *smem) {
        // (copies: what is read through a reference inside the loop is read again behind every barrier)
        const int tid = at.tid, lane = at.lane, wv = at.wv, ch = at.ch, cb0 = a.cb0, ncol = a.ncol, n = a.n;
        const long i0 = at.i0, ldp = a.ldp;
        double *part = a.part;
        double *sRed = smem;   // [4 waves][32 rows][16 columns]
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
            __syncthreads();   // every wave is done with the working block, or with the block before
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cl = (lane >> 4) + 4 * r;
                sRed[(wv * 32 + (lane & 15)) * 16 + cl] = g0a[qb][r];
                sRed[(wv * 32 + 16 + (lane & 15)) * 16 + cl] = g1a[qb][r];
            }
            __syncthreads();
            for (int t = tid; t < 32 * 16; t += 256) {
                const int row = t & 31, cl = t >> 5, col = (cb0 + qb) * 16 + cl;
                const int ix = row * 16 + cl;
                const double s = ((sRed[ix] + sRed[512 + ix]) + sRed[1024 + ix]) + sRed[1536 + ix];
                if (i0 + row < n && col < ncol) part[((size_t)ch * ncol + col) * ldp + i0 + row] = s;
            }
        }
    }
};

// z of one group from its accumulators into the sink: the epilogue of predict_group_body and of predict_group_large_body
// (k_predict_group_large_impl.h).  acc0[r], acc1[r] = sum_l Pio(row, l) Nu_q(l) for rows l & 15, 16 + (l & 15) and pair q = (l >> 4) + 4 r   :185-186, :271-272
// The exponent lnZ - q / 2 is ONE fma, written out: the compiler contracts "lz - 0.5 * q" to it only where product and difference
// land in one basic block, which the sink decides, and a row's bits must not depend on the sink.
template <bool PSI, class Sink>
__device__ __forceinline__ void pred_group_epilogue(const PredGroupArgs &a, const PredGroupAt &at, Sink &sink, const int2 *sAB, d4_t acc0, d4_t acc1,
                                             const double *rb, int rl, const double *x0, const double *x1, const double *s0,
                                             const double *s1) {
    const int d = a.d;
    double qa[4] = {0.0, 0.0, 0.0, 0.0}, qb[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (!PSI) {
        for (int c = 0; c < d; ++c) {
            const double xa = x0[c], xb = x1[c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double *t = rb + 4 * r * rl;
                const double cc = t[1 + c], ic = t[1 + d + c];
                const double da = xa - cc, db = xb - cc;
                qa[r] = fma(da * da, ic, qa[r]);                   // :178-179
                qb[r] = fma(db * db, ic, qb[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double *t = rb + 4 * r * rl;
            const double lz = t[0];
            const double za = acc0[r] * exp(fma(-0.5, qa[r], lz)), zb = acc1[r] * exp(fma(-0.5, qb[r], lz));   // :189
            sink.take(a, at, sAB, r, za, zb, t);
        }
    } else {
        double ra[4] = {1.0, 1.0, 1.0, 1.0}, rb4[4] = {1.0, 1.0, 1.0, 1.0};
        for (unsigned mk = a.obs; mk; mk &= mk - 1) {   // the observed dimensions only (uniform: scalar control flow)
            const int c = __builtin_ctz(mk);
            const double xa = x0[c], xb = x1[c], pa = s0[c], pb = s1[c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double *t = rb + 4 * r * rl;
                const double cc = t[1 + c], C = t[1 + d + c];
                const double ia = rsqrt_nr2(C + pa), ib = rsqrt_nr2(C + pb);   // (Cij + Psi)^-1/2            :264-265
                const double da = (xa - cc) * ia, db = (xb - cc) * ib;
                qa[r] = fma(da, da, qa[r]);
                qb[r] = fma(db, db, qb[r]);
                ra[r] *= ia;
                rb4[r] *= ib;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double *t = rb + 4 * r * rl;
            const double lz = t[0];
            const double za = acc0[r] * (exp(fma(-0.5, qa[r], lz)) * ra[r]), zb = acc1[r] * (exp(fma(-0.5, qb[r], lz)) * rb4[r]);   // :275
            sink.take(a, at, sAB, r, za, zb, t);
        }
    }
}

template <bool PSI, class Sink>
__device__ __forceinline__ void predict_group_body(const PredGroupArgs &a) {
    extern __shared__ double smem[];
    const int nk = a.nk, lda = nk + 2, d = a.d, rl = Sink::FULL_RECORD ? a.nrec : 1 + 2 * d;
    double *sP = smem;                   // [32][lda]: Pio of the block (2 mod 4: the 16 rows of an operand read start 4 banks apart)
    double *sR = sP + 32 * lda;          // [64][rl]: the records of the group
    double *sX = sR + 64 * rl;           // [32][d]: the block's rows, zero where missing
    double *sS = sX + 32 * d;            // [32][d] with PSI: their variances, zero where missing
    PredGroupAt at;
    at.tid = threadIdx.x; at.lane = at.tid & 63; at.wv = __builtin_amdgcn_readfirstlane(at.tid >> 6);
    at.i0 = (long)blockIdx.x * 32; at.ch = blockIdx.y;
    const int tid = at.tid, lane = at.lane, wv = at.wv;
    const long i0 = at.i0;
    const unsigned obs = a.obs;
    for (int e = tid; e < 32 * nk; e += 256) {
        const int r = e / nk, c = e - r * nk;
        sP[r * lda + c] = (i0 + r < a.n) ? a.Pio[(size_t)(i0 + r) * a.ldpio + c] : 0.0;
    }
    for (int e = tid; e < 32 * d; e += 256) {
        const int r = e / d, c = e - r * d;
        const bool in = ((obs >> c) & 1u) && i0 + r < a.n;
        sX[e] = in ? a.Xc[(size_t)c * a.ldx + i0 + r] : 0.0;
        if constexpr (PSI) sS[e] = in ? a.Psic[(size_t)c * a.ldx + i0 + r] : 0.0;
    }
    int2 *sAB = (int2 *)((PSI ? sS : sX) + 32 * d);   // [64], the gamma sink's
    Sink sink;   // (the accumulators alone: a pointer kept beside them stays in memory until their loops are unrolled)
    sink.init();
    const int nks = nk >> 2;             // K steps of 4 (a multiple of 4)
    const double *pa0 = sP + (lane & 15) * lda + (lane >> 4), *pa1 = pa0 + 16 * lda;
    const double *x0 = sX + (lane & 15) * d, *x1 = x0 + 16 * d;
    const double *s0 = sS + (lane & 15) * d, *s1 = s0 + 16 * d;   // PSI
    const double *rb = sR + (16 * wv + (lane >> 4)) * rl;   // the records of pairs (lane >> 4) + 4 r of this wave's block, r = 0 .. 3
    const int g0 = at.ch * a.gpc, g1 = min(a.ngrp, g0 + a.gpc);
    for (int g = g0; g < g1; ++g) {
        __syncthreads();   // the group before is read (first trip: sP, sX and sS are written)
        {
            const double *src = a.rec + (size_t)g * 64 * a.nrec;
            if constexpr (Sink::FULL_RECORD) {
                for (int t = tid; t < 64 * rl; t += 256) sR[t] = src[t];
            } else {
                for (int t = tid; t < 64 * rl; t += 256) {
                    const int j = t / rl, f = t - j * rl;
                    sR[t] = src[(size_t)j * a.nrec + f];
                }
            }
            sink.stage(a, at, sAB, g);
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
        __syncthreads();   // the records (and the sink's own staging) are in LDS
        pred_group_epilogue<PSI, Sink>(a, at, sink, sAB, acc0, acc1, rb, rl, x0, x1, s0, s1);
    }
    sink.reduce(a, at, smem);
}

// The kernels, each defined and instantiated in the unit of its name; the launchers (k_predict_missing.hip, k_predict_missing_gamma.hip)
// launch the ones with Psi from their own units.
template <int KM> __global__ __launch_bounds__(256, 2) void k_predict_missing_pairs(PredGroupArgs a);
template <int KM> __global__ __launch_bounds__(256, 2) void k_predict_noisy_missing_pairs(PredGroupArgs a);
template <int NB> __global__ __launch_bounds__(256, 2) void k_predict_missing_gamma(PredGroupArgs a);
template <int NB> __global__ __launch_bounds__(256, 2) void k_predict_noisy_missing_gamma(PredGroupArgs a);

// per launch, not once per process: the attribute belongs to the current device's copy of the kernel
template <void (*KERNEL)(PredGroupArgs)>
static int launch_predict_group(hipStream_t st, dim3 grid, size_t lds, const PredGroupArgs &a) {
    if (lds > 65536 && hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
