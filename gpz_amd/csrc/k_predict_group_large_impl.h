// The pair product of one group of rows that share a NaN pattern past ceil16(m) = 256 (a handle with GPZ_PREDICT_LARGE_M_MISSING), shared
// by its two units as k_predict_group_impl.h is by its four:
//   k_pml_pairs.hip   k_pml_pairs<KM>, k_pml_pairs_psi<KM>   clean z and z with Psi, the pairs sink
//   k_pml_gamma.hip   k_pml_gamma<NB>, k_pml_gamma_psi<NB>   clean z and z with Psi, the gamma sink
// predict_group_large_body<PSI, Sink> computes what predict_group_body<PSI, Sink> computes, on the same tables (U in k_pmd_u's fragment
// order as the A operand from global memory, Pio as the B operand from LDS, v_mfma_f64_16x16x4_f64, the epilogue in the accumulators) and
// with the same sinks (PredPairsSink, PredGammaSink, unchanged); read that header for the operand maps, the two forms of z and the sinks.
// It differs in one way: the Pio block of the workgroup's 32 rows does not sit whole in LDS (32 (nk + 2) doubles: 263 KB at nk = 1024)
// but passes through it in K panels of GPZ_PML_KP = 128 columns, sP [32][KP + 2], so that LDS does not grow with m.
//
// The batch.  Re-staging Pio for every group of 64 pairs would read 32 nk doubles of Pio for 64 nk doubles of U; so a workgroup takes a
// batch of GPZ_PML_GB = 4 consecutive groups of its chunk, and wave w keeps the accumulators of its 16-pair block 4 g + w of each of them
// (4 x 2 x 4 doubles: 64 registers).  Per panel the workgroup stages sP once (two barriers) and every wave runs the panel's K steps for
// its four blocks, the U fragments fetched four steps ahead as in the other body.  Pio is read once per batch: 32 nk doubles against
// 256 nk of U.  With 8 outputs in registers (PredPairsSink<8>: 96 registers) the batch is GPZ_PML_GB8 = 2 groups: four left the kernel
// with Psi six registers short of two workgroups per compute unit; Pio is then 32 nk doubles against 128 nk of U.  The batch is a template
// argument chosen by k = 1 or k > 1, the model's shape.  After the last panel the epilogue runs group by group, the group's 64 records staged between two barriers as in the
// other body (the records of one group only: LDS for four would be 133 KB at d = 20, k = 8).
//
// Orders.  The panel width, the batch, the chunk count (predict_missing_chunks) and every order of summation are functions of the
// model's shape alone: a block's K sum runs over l = 0 .. nk - 1 in order (the panels in order, the steps of a panel in order, in one
// accumulator), the blocks of a wave enter the sink in table order (the batches in order, the groups of a batch in order), then the
// sink's own wave and chunk order.  No atomics; every sum starts from zero: a row's results have the same bits for any tile size, row
// order, company, split into calls and any number of draws > s.
// LDS: sP [32][KP + 2] | sR [64][record] | sX [32][d] | sS [32][d] with PSI | sAB [64] int2 for the gamma sink, and at least the sink's
// last reduction (predict_missing_large_lds): 35 to 77 KB, the same for every m.
#pragma once
#include "gpz_kernels.h"
#include "k_predict_group_impl.h"

template <bool PSI, class Sink, int GB>
__device__ __forceinline__ void predict_group_large_body(const PredGroupArgs &a) {
    extern __shared__ double smem[];
    constexpr int KP = GPZ_PML_KP, lda = KP + 2;
    const int nk = a.nk, d = a.d, rl = Sink::FULL_RECORD ? a.nrec : 1 + 2 * d;
    double *sP = smem;                   // [32][lda]: one K panel of Pio of the block (2 mod 4, as in the other body)
    double *sR = sP + 32 * lda;          // [64][rl]: the records of one group
    double *sX = sR + 64 * rl;           // [32][d]: the block's rows, zero where missing
    double *sS = sX + 32 * d;            // [32][d] with PSI: their variances, zero where missing
    PredGroupAt at;
    at.tid = threadIdx.x; at.lane = at.tid & 63; at.wv = __builtin_amdgcn_readfirstlane(at.tid >> 6);
    at.i0 = (long)blockIdx.x * 32; at.ch = blockIdx.y;
    const int tid = at.tid, lane = at.lane, wv = at.wv;
    const long i0 = at.i0;
    const unsigned obs = a.obs;
    for (int e = tid; e < 32 * d; e += 256) {
        const int r = e / d, c = e - r * d;
        const bool in = ((obs >> c) & 1u) && i0 + r < a.n;
        sX[e] = in ? a.Xc[(size_t)c * a.ldx + i0 + r] : 0.0;
        if constexpr (PSI) sS[e] = in ? a.Psic[(size_t)c * a.ldx + i0 + r] : 0.0;
    }
    int2 *sAB = (int2 *)((PSI ? sS : sX) + 32 * d);   // [64], the gamma sink's
    Sink sink;
    sink.init();
    const int nks = nk >> 2;             // K steps of 4 in all (a multiple of 4)
    const double *pa0 = sP + (lane & 15) * lda + (lane >> 4), *pa1 = pa0 + 16 * lda;
    const double *x0 = sX + (lane & 15) * d, *x1 = x0 + 16 * d;
    const double *s0 = sS + (lane & 15) * d, *s1 = s0 + 16 * d;   // PSI
    const double *rb = sR + (16 * wv + (lane >> 4)) * rl;   // the records of pairs (lane >> 4) + 4 r of this wave's block, r = 0 .. 3
    // the row of Pio that this thread stages: element e = tid + 256 j of a panel is row e >> 7, column e & 127 (KP = 128)
    static_assert(KP == 128, "the staging loop shifts by 7");
    const int g0 = at.ch * a.gpc, g1 = min(a.ngrp, g0 + a.gpc);
    for (int gb = g0; gb < g1; gb += GB) {
        // acc0[j], acc1[j]: group gb + j.  The loops over the batch are NOT unrolled (one copy of the K loop and of the epilogue, as in the
        // other body): each trip works on slot 0 and then turns the slots by one, a register move per accumulator against the trip's
        // 2 * 32 MFMAs per panel; after GB trips every group is back in its slot.
        d4_t acc0[GB], acc1[GB];
#pragma unroll
        for (int j = 0; j < GB; ++j) { acc0[j] = (d4_t){0.0, 0.0, 0.0, 0.0}; acc1[j] = (d4_t){0.0, 0.0, 0.0, 0.0}; }
        for (int k0 = 0; k0 < nk; k0 += KP) {
            const int kw = min(KP, nk - k0);   // a multiple of 16
            __syncthreads();   // the panel before is read
            for (int e = tid; e < 32 * KP; e += 256) {
                const int r = e >> 7, c = e & (KP - 1);
                if (c < kw) sP[r * lda + c] = (i0 + r < a.n) ? a.Pio[(size_t)(i0 + r) * a.ldpio + k0 + c] : 0.0;   // k0 + c < nk <= ldpio
            }
            __syncthreads();
            const int ns = kw >> 2, ks0 = k0 >> 2;   // the panel's K steps (a multiple of 4) and its first
#pragma nounroll
            for (int b = 0; b < GB; ++b) {
                // past the chunk's last group: that group again, into a slot whose epilogue does not run (no test inside the K loop)
                const int g = min(gb + b, g1 - 1);
                const double *ub = a.U + ((size_t)(4 * g + wv) * nks + ks0) * 64 + lane;
                d4_t c0 = acc0[0], c1 = acc1[0];
                double ua[4], un[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < 4; ++q) ua[q] = ub[q * 64];
                for (int ks = 0; ks < ns; ks += 4) {
                    if (ks + 4 < ns) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) un[q] = ub[(size_t)(ks + 4 + q) * 64];
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        c0 = MFMA_F64(ua[q], pa0[4 * (ks + q)], c0);
                        c1 = MFMA_F64(ua[q], pa1[4 * (ks + q)], c1);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) ua[q] = un[q];
                }
#pragma unroll
                for (int j = 0; j + 1 < GB; ++j) { acc0[j] = acc0[j + 1]; acc1[j] = acc1[j + 1]; }
                acc0[GB - 1] = c0; acc1[GB - 1] = c1;
            }
        }
        // ---- the epilogue, group by group: acc0[0][r], acc1[0][r] = sum_l Pio(row, l) Nu_q(l) for rows l & 15, 16 + (l & 15) and pair
        // q = (l >> 4) + 4 r of this wave's block of group gb + b
#pragma nounroll
        for (int b = 0; b < GB; ++b) {
            const int g = gb + b;
            if (g < g1) {   // (uniform)
                __syncthreads();   // the group before is read (first trip: sX and sS are written)
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
                __syncthreads();   // the records (and the sink's own staging) are in LDS
                pred_group_epilogue<PSI, Sink>(a, at, sink, sAB, acc0[0], acc1[0], rb, rl, x0, x1, s0, s1);
            }
#pragma unroll
            for (int j = 0; j + 1 < GB; ++j) { acc0[j] = acc0[j + 1]; acc1[j] = acc1[j + 1]; }
        }
    }
    sink.reduce(a, at, smem);
}

// The kernels, each defined and instantiated in the unit of its sink; the launchers are there too.
template <int KM> __global__ __launch_bounds__(256, 2) void k_pml_pairs(PredGroupArgs a);
template <int KM> __global__ __launch_bounds__(256, 2) void k_pml_pairs_psi(PredGroupArgs a);
template <int NB> __global__ __launch_bounds__(256, 2) void k_pml_gamma(PredGroupArgs a);
template <int NB> __global__ __launch_bounds__(256, 2) void k_pml_gamma_psi(PredGroupArgs a);
