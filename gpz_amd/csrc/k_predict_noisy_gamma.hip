// gamma under every weight draw for rows with input noise (gpz_predictor_stack_noisy / _stack_noisy_dev / _draws_gamma_noisy_dev,
// gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab E[phi_a phi_b](x_i, psi_i) w_s,a w_s,b - mu_s,i^2 per output, predictNoisy's gamma
// (predictDiag.m:111-124) with the draw's weights in place of w; f_ab = 2 off the diagonal, 1 on it.
//
//   k_predict_noisy_gamma<DT>   The sum over the pairs is a product E (rows x pairs) Wp (pairs x columns), Wp[ab, col] = f_ab W[a, col] W[b, col],
//                               taken transposed on v_mfma_f64_16x16x4_f64 as k_predict_draws takes its own: Wp is the A operand, z the B
//                               operand, so an accumulator lane holds one row and 4 columns per 16-column block.  A wave owns 16 rows; in
//                               a K step lane l forms ONE pair density z(row l & 15, pair 4 ks + (l >> 4)) in k_predict_noisy_small's
//                               arithmetic (one r = (C_ab + psi)^-1/2 per dimension by v_rsq_f64 + two Newton steps, z = exp(lnZ - 1/2 sum
//                               (Delta r)^2) prod r): all 64 lanes do density work and no z reaches memory or LDS.  The 16 lanes that
//                               share a pair read its record [lnZ | c_ab | C_ab] (the first 1 + 2 d doubles of the handle's pair table)
//                               as an LDS broadcast; the workgroup (4 waves, 64 rows) stages 32 records at a time between two barriers,
//                               the next stage's loads in flight in registers while this one is worked on.
//                               Wp is formed in registers: two rows of W (L1 / L2: W is m x ldw, 51 KB at m = 100 and 64 columns) and two
//                               multiplies per 16-column block, no table; the loads of the first 4 blocks are issued ahead of the
//                               density work.  A lane carries its pair's (a, b) and steps them by 4 pairs.
//                               Up to GPZ_GAMMA_NB = 8 blocks (128 columns) of accumulators per pass; more columns are further passes on
//                               gridDim.z that form z again.  gridDim.y: the pair chunks, predict_gamma_chunks(m) of the model's shape alone;
//                               chunk c writes its partial sums to part [C][ncol][ldp].
//   k_gamma_finish_dev          sum of the chunks in chunk order, gamma_s = fma(-mu_s, mu_s, sum) -> the caller's Gam (n x k x nd).
//   k_gamma_finish_s2           the same gamma_s -> the widths of the stack: s2 [(1 + nd) k][nt], row o = (nu + beta) + gamma of nout,
//                               row (1 + s) k + o = beta + max(gamma_s, 0).
// No atomics; every sum starts from zero and runs in one order that the model's shape fixes (pairs in table order, four per K step from
// the chunk's first pair, chunks in chunk order): a row's gamma_s has the same bits for any tile size, row order, position in its block,
// other rows of the call and any number of draws > s.
#include "gpz_dev.h"
#include "gpz_kernels.h"

#define GPZ_GAMMA_TP 32   // pair records per LDS stage: 8 K steps
#define GPZ_GAMMA_NB 8    // 16-column blocks of accumulators per pass
#define GPZ_GAMMA_PF 4    // of these, the blocks whose W rows are fetched ahead of the density work (64 columns: the usual 64 draws)

struct PredGammaArgs {
    const double *Xc, *Psic; long ldx;   // [d][ldx] column layout, n rows
    int n, m;
    const double *tab; int rec;          // pair records, rec doubles apart; the first 1 + 2 d are read
    long ppc;                            // pairs per chunk (a multiple of 4)
    const double *W; int ldw;            // ceil16(m) x ldw row-major, columns >= ncol zero
    int ncol, nbw;                       // columns; 16-column blocks (nbw = ldw / 16)
    double *part; long ldp;              // [chunks][ncol][ldp]
};

template <int DT>
__global__ __launch_bounds__(256) void k_predict_noisy_gamma(PredGammaArgs a) {
    constexpr int RL = 1 + 2 * DT, NST = GPZ_GAMMA_TP * RL, NPRE = (NST + 255) / 256;
    __shared__ double sT[NST];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, lr = lane & 15;
    const long i = ((long)blockIdx.x * 4 + wv) * 16 + lr;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    double x[DT], ps[DT];
#pragma unroll
    for (int c = 0; c < DT; ++c) {
        x[c] = a.Xc[(size_t)c * a.ldx + ic];
        ps[c] = a.Psic[(size_t)c * a.ldx + ic];
    }
    const int ch = blockIdx.y, cb0 = blockIdx.z * GPZ_GAMMA_NB;
    const int nb = __builtin_amdgcn_readfirstlane(a.nbw - cb0 < GPZ_GAMMA_NB ? a.nbw - cb0 : GPZ_GAMMA_NB);
    const int npair = a.m * (a.m + 1) / 2;
    const int p0 = (int)(ch * a.ppc), p1 = (int)(p0 + a.ppc < npair ? p0 + a.ppc : npair);
    // the lane's pair e = p0 + g + 4 ks as (pa >= pb): e = pa (pa + 1) / 2 + pb
    int pa, pb;
    {
        const int e = p0 + g;
        pa = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
        while (pa * (pa + 1) / 2 > e) --pa;
        while ((pa + 1) * (pa + 2) / 2 <= e) ++pa;
        pb = e - pa * (pa + 1) / 2;
    }
    d4_t acc[GPZ_GAMMA_NB];
#pragma unroll
    for (int q = 0; q < GPZ_GAMMA_NB; ++q) acc[q] = (d4_t){0.0, 0.0, 0.0, 0.0};
    const double *wl = a.W + (size_t)cb0 * 16 + lr;
    double pre[NPRE];
    // the records [pbase, pbase + 32) of the chunk (clamped to its last one, so that every slot of a stage holds a record)
#define PG_LOAD(pbase)                                                                 \
    _Pragma("unroll") for (int u = 0; u < NPRE; ++u) {                                 \
        const int t = tid + 256 * u;                                                   \
        if (t < NST) {                                                                 \
            const int jj = t / RL, f = t - jj * RL;                                    \
            const int pr = (pbase) + jj < p1 ? (pbase) + jj : p1 - 1;                  \
            pre[u] = a.tab[(size_t)pr * a.rec + f];                                    \
        }                                                                              \
    }
    PG_LOAD(p0)
    for (int pbase = p0; pbase < p1; pbase += GPZ_GAMMA_TP) {
        __syncthreads();   // the stage before is read
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            const int t = tid + 256 * u;
            if (t < NST) sT[t] = pre[u];
        }
        __syncthreads();
        if (pbase + GPZ_GAMMA_TP < p1) { PG_LOAD(pbase + GPZ_GAMMA_TP) }
        const int left = p1 - pbase, nks = ((left < GPZ_GAMMA_TP ? left : GPZ_GAMMA_TP) + 3) >> 2;
#pragma unroll 2
        for (int ks = 0; ks < nks; ++ks) {
            const int slot = 4 * ks + g;
            const bool valid = pbase + slot < p1;
            const int aa = valid ? pa : 0, bb = valid ? pb : 0;
            const double f = aa == bb ? 1.0 : 2.0;                     // 2x off the diagonal, 1x on it       predictDiag.m:113-119
            const double *wa = wl + (size_t)aa * a.ldw, *wb = wl + (size_t)bb * a.ldw;
            // the two rows of W for the first GPZ_GAMMA_PF blocks are fetched here, so that the density work below covers their latency
            double wav[GPZ_GAMMA_PF], wbv[GPZ_GAMMA_PF];
#pragma unroll
            for (int qb = 0; qb < GPZ_GAMMA_PF; ++qb) {
                const int off = qb < nb ? 16 * qb : 0;
                wav[qb] = wa[off];
                wbv[qb] = wb[off];
            }
            const double *t = sT + slot * RL;   // one address per 16 lanes: a broadcast read
            double q = 0.0, rp = 1.0;
#pragma unroll
            for (int c = 0; c < DT; ++c) {
                const double r = rsqrt_nr2(t[1 + DT + c] + ps[c]);      // (Cij + Psi)^-1/2            :105
                const double dl = (x[c] - t[1 + c]) * r;
                q = fma(dl, dl, q);
                rp *= r;
            }
            double z = exp(t[0] - 0.5 * q) * rp;                       // :107
            z = valid ? z : 0.0;
#pragma unroll
            for (int qb = 0; qb < GPZ_GAMMA_NB; ++qb)
                if (qb < nb) {
                    const double wp = qb < GPZ_GAMMA_PF ? (f * wav[qb < GPZ_GAMMA_PF ? qb : 0]) * wbv[qb < GPZ_GAMMA_PF ? qb : 0]
                                                        : (f * wa[16 * qb]) * wb[16 * qb];
                    acc[qb] = MFMA_F64(wp, z, acc[qb]);
                }
            pb += 4;   // four pairs on
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (pb > pa) { pb -= pa + 1; ++pa; }
        }
    }
#undef PG_LOAD
    // ---- lane l, register r of block qb holds the sum of row l & 15 and column 16 (cb0 + qb) + (l >> 4) + 4 r
    if (!act) return;
#pragma unroll
    for (int qb = 0; qb < GPZ_GAMMA_NB; ++qb)
        if (qb < nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = (cb0 + qb) * 16 + g + 4 * r;
                if (col < a.ncol) a.part[((size_t)ch * a.ncol + col) * a.ldp + i] = acc[qb][r];
            }
        }
}

// the chunks' sums of column col = o nd + s in chunk order, then gamma_s = sum - mu_s^2 in one fma
__device__ __forceinline__ double pg_gamma(const double *__restrict__ part, int nchunk, long ldp, int ncol, int col, int i, double mu) {
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += part[((size_t)c * ncol + col) * ldp + i];
    return fma(-mu, mu, s);
}

__global__ __launch_bounds__(256) void k_gamma_finish_dev(const double *__restrict__ part, int nchunk, long ldp, const double *__restrict__ dout,
                                                          int nt, int k, int nd, long ns, long r0, double *__restrict__ Gam) {
    const int i = blockIdx.x * 256 + threadIdx.x, col = blockIdx.y, o = col / nd, s = col - o * nd;
    if (i >= nt) return;
    Gam[((size_t)s * k + o) * ns + r0 + i] = pg_gamma(part, nchunk, ldp, nd * k, col, i, dout[(size_t)col * nt + i]);
}

__global__ __launch_bounds__(256) void k_gamma_finish_s2(const double *__restrict__ part, int nchunk, long ldp, const double *__restrict__ nout,
                                                         const double *__restrict__ dout, int nt, int k, int nd, double *__restrict__ s2) {
    const int i = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, c = q / k, o = q - c * k;
    if (i >= nt) return;
    const double beta = nout[(size_t)(2 * k + o) * nt + i];
    double w;
    if (c == 0) {
        w = nout[(size_t)(k + o) * nt + i] + beta + nout[(size_t)(3 * k + o) * nt + i];   // (nu + beta) + gamma: k_pred_finish_noisy_dev's sigma
    } else {
        const int col = o * nd + (c - 1);
        w = beta + fmax(pg_gamma(part, nchunk, ldp, nd * k, col, i, dout[(size_t)col * nt + i]), 0.0);
    }
    s2[(size_t)q * nt + i] = w;
}

// pair chunks: one per 4096 pairs, at most 4 (it changes at m = 91, 128, 157).  The model's shape only, never the rows or the draws.
int predict_gamma_chunks(int m) {
    const long c = ((long)m * (m + 1) / 2 + 4095) / 4096;
    return (int)(c < 1 ? 1 : (c > 4 ? 4 : c));
}

int launch_predict_noisy_gamma(hipStream_t st, int d, const double *Xc, const double *Psic, long ldx, int n, int m, const double *tab,
                               int rec, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > 20 || nchunk < 1 || ldw % 16 || ncol > ldw || rec < 1 + 2 * d) return -1;
    const long npair = (long)m * (m + 1) / 2;
    PredGammaArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.m = m; a.tab = tab; a.rec = rec;
    a.ppc = ((npair + nchunk - 1) / nchunk + 3) / 4 * 4;
    a.W = W; a.ldw = ldw; a.ncol = ncol; a.nbw = (ncol + 15) / 16;
    a.part = part; a.ldp = ldp;
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)nchunk, (unsigned)((a.nbw + GPZ_GAMMA_NB - 1) / GPZ_GAMMA_NB));
    switch (d) {
#define PG_CASE(DD) case DD: hipLaunchKernelGGL((k_predict_noisy_gamma<DD>), grid, dim3(256), 0, st, a); break;
        PG_CASE(1) PG_CASE(2) PG_CASE(3) PG_CASE(4) PG_CASE(5) PG_CASE(6) PG_CASE(7) PG_CASE(8) PG_CASE(9) PG_CASE(10)
        PG_CASE(11) PG_CASE(12) PG_CASE(13) PG_CASE(14) PG_CASE(15) PG_CASE(16) PG_CASE(17) PG_CASE(18) PG_CASE(19) PG_CASE(20)
#undef PG_CASE
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_gamma_finish_dev(hipStream_t st, const double *part, int nchunk, long ldp, const double *dout, int nt, int k, int nd, long ns,
                            long r0, double *Gam) {
    if (nt <= 0) return 0;
    hipLaunchKernelGGL(k_gamma_finish_dev, dim3((unsigned)((nt + 255) / 256), (unsigned)(nd * k)), dim3(256), 0, st, part, nchunk, ldp, dout, nt,
                       k, nd, ns, r0, Gam);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_gamma_finish_s2(hipStream_t st, const double *part, int nchunk, long ldp, const double *nout, const double *dout, int nt, int k,
                           int nd, double *s2) {
    if (nt <= 0) return 0;
    hipLaunchKernelGGL(k_gamma_finish_s2, dim3((unsigned)((nt + 255) / 256), (unsigned)((1 + nd) * k)), dim3(256), 0, st, part, nchunk, ldp, nout,
                       dout, nt, k, nd, s2);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
