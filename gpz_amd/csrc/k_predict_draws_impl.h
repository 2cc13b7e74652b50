// The fused draws kernel (see k_predict_draws.hip for the scheme), shared by its two units as k_cpsi4_impl.h is by its own.  The including
// unit chooses the kernel with PREDICT_DRAWS_PSI:
//   k_predict_draws.hip   (not defined)  k_predict_draws<D, COV>(a): PHI of noise-free rows
//   k_predict_noisy.hip   (defined)      k_predict_draws_psi<D>(a, Psic): E_x[PHI] of rows with per-dimension input noise, diagonal kinds
// With PSI the block's rows of Psi sit in sPsi [32][D] behind sX, and PsPhiBuilder forms getPHI.m:104 instead of :97; everything after
// the PHI block is in LDS is the same text, so a row's draws keep the properties listed there.  The parameter is a macro and not a
// template argument so that the noise-free kernels keep their names and their code, instruction for instruction.
#pragma once
#include "gpz_dev.h"

#ifndef PS_LDA
#define PS_LDA 262   // row stride of the PHI block in LDS (doubles): 2 (mod 4) - the 16 rows of an A-operand read start 4 banks apart
#endif
#include "k_predict_phi.h"

struct PredDrawsArgs {
    const double *Xc; long ldx;   // de x ldx column layout (the tile's rows; dimensions >= d are zero)
    int n;                        // rows of this tile
    int m, nk;                    // nk = ceil16(m): K of the product (PHI columns m .. nk - 1 are zero)
    int ncol, nbw;                // columns of F; 16-column blocks of W (nbw = ldw / 16)
    const double *P, *G;          // as k_predict_small
    const double *W; int ldw;     // nk x ldw row-major; columns >= ncol zero
    double *out; long ldo;        // [ncol][ldo]
};

#ifdef PREDICT_DRAWS_PSI
// Psic: the tile's Psi in the layout of Xc
template <int D>
__global__ __launch_bounds__(256, 2) void k_predict_draws_psi(PredDrawsArgs a, const double *Psic) {
    constexpr bool COV = false, PSI = true;
#else
template <int D, bool COV>
__global__ __launch_bounds__(256, 2) void k_predict_draws(PredDrawsArgs a) {
    constexpr bool PSI = false;
#endif
    extern __shared__ double smem[];
    double *sA = smem;                    // [32][PS_LDA]: PHI of the block
    double *sX = sA + 32 * PS_LDA;        // [32][D]: the block's rows of X
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = a.nk, nbw = a.nbw, ldw = a.ldw;
    const int nblocks = (a.n + 31) >> 5;
    const PsPhiBuilder<D, COV, PSI> phi(a.P, a.G, a.m, nk, tid);
    const int ks_n = nk >> 2;   // K steps of 4 (a multiple of 4)
    const double *wl = a.W + (size_t)(lane >> 4) * ldw + (lane & 15);
    for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long i0 = (long)blk * 32;
        __syncthreads();   // the previous block's K loops are done with sA
        ps_load_x<D>(a.Xc, a.ldx, a.n, i0, sX, tid);
#ifdef PREDICT_DRAWS_PSI
        double *sPsi = sX + 32 * D;       // [32][D]: the block's rows of Psi
        ps_load_psi<D>(Psic, a.ldx, a.n, i0, sPsi, tid);
        __syncthreads();
        phi.build(sA, sX, i0, a.n, sPsi);
#else
        __syncthreads();
        phi.build(sA, sX, i0, a.n);
#endif
        __syncthreads();
        for (int cb = 0; cb < nbw; cb += 16) {
            const int nbc = nbw - cb < 16 ? nbw - cb : 16;
            // deal: both strips of blocks cb + wv + 4q, or (nbc < 4) strip wv & 1 of blocks cb + (wv >> 1) + 2q
            const bool split = nbc < 4;
            const int s0 = split ? (wv & 1) : 0;
            const int b0 = split ? (wv >> 1) : wv, bs = split ? 2 : 4;
            const int nq = __builtin_amdgcn_readfirstlane(nbc > b0 ? (nbc - b0 + bs - 1) / bs : 0);
            if (nq == 0) continue;
            const double *pa0 = sA + (16 * s0 + (lane & 15)) * PS_LDA + (lane >> 4);
            const double *pa1 = split ? pa0 : pa0 + 16 * PS_LDA;   // (split: not used)
            const double *wb = wl + (size_t)(cb + b0) * 16;
            d4_t acc[2][4];
            double ba[4], bb[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[0][q] = (d4_t){0.0, 0.0, 0.0, 0.0};
                acc[1][q] = (d4_t){0.0, 0.0, 0.0, 0.0};
                ba[q] = q < nq ? wb[q * bs * 16] : 0.0;
            }
            // two K steps per trip (ks_n is even): each step's W fragments are loaded while the step before it runs
            for (int ks = 0; ks < ks_n; ks += 2) {
                const double *w1 = wb + (size_t)(ks + 1) * 4 * ldw;
#pragma unroll
                for (int q = 0; q < 4; ++q) bb[q] = q < nq ? w1[q * bs * 16] : 0.0;
                {
                    const double a0 = pa0[4 * ks], a1 = pa1[4 * ks];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < nq) {
                            acc[0][q] = MFMA_F64(ba[q], a0, acc[0][q]);
                            if (!split) acc[1][q] = MFMA_F64(ba[q], a1, acc[1][q]);
                        }
                }
                if (ks + 2 < ks_n) {
                    const double *w2 = w1 + (size_t)4 * ldw;
#pragma unroll
                    for (int q = 0; q < 4; ++q) ba[q] = q < nq ? w2[q * bs * 16] : 0.0;
                }
                {
                    const double a0 = pa0[4 * ks + 4], a1 = pa1[4 * ks + 4];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < nq) {
                            acc[0][q] = MFMA_F64(bb[q], a0, acc[0][q]);
                            if (!split) acc[1][q] = MFMA_F64(bb[q], a1, acc[1][q]);
                        }
                }
            }
            // ---- epilogue: lane l, register r of strip s holds F[row = 16 s + (l & 15)][col = 16 gb + (l >> 4) + 4 r]
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (split && s == 1) break;
                const long row = i0 + 16 * (s + s0) + (lane & 15);
                if (row >= a.n) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < nq) {
                        const int gb = cb + b0 + q * bs;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int col = gb * 16 + (lane >> 4) + 4 * r;
                            if (col < a.ncol) a.out[(size_t)col * a.ldo + row] = acc[s][q][r];
                        }
                    }
            }
        }
    }
}
