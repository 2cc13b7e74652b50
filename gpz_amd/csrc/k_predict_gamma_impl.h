// The frame of the kernels that form gamma under every weight draw for rows with input noise: k_predict_noisy_gamma<DT>
// (k_predict_noisy_gamma.hip, the diagonal kinds), k_predict_noisy_cov_gamma<D, SHARED> (k_predict_noisy_cov_gamma.hip, GC and VC) and
// k_predict_psi_cube_gamma<D, SHARED> (k_predict_psi_cube_gamma.hip, GC and VC with a full d x d Psi per row).
// Each is a thin __global__ wrapper of predict_gamma_body<Density>; what differs between them is the Density policy of its file.
//
//   predict_gamma_body<Density>
//       The sum over the pairs, sum_{a >= b} f_ab z_ab(x_i, psi_i) w_s,a w_s,b, is a product E (rows x pairs) Wp (pairs x columns),
//       Wp[ab, col] = f_ab W[a, col] W[b, col], taken transposed on v_mfma_f64_16x16x4_f64 as k_predict_draws takes its own: Wp is the
//       A operand, z the B operand, so an accumulator lane holds one row and 4 columns per 16-column block.  A wave owns 16 rows, a
//       workgroup (4 waves) 64; in a K step lane l forms ONE pair density z(row l & 15, pair 4 ks + (l >> 4)) = Density::z: all 64
//       lanes do density work and no z reaches memory or LDS.  The 16 lanes that share a pair read the head of its record (the first
//       Density::RL doubles, read with the table's stride) as an LDS broadcast; the workgroup stages 32 heads at a time between two
//       barriers, the next stage's loads in flight in registers while this one is worked on.  A stage's slots past the chunk's last
//       record hold that record again (the clamp of the load), so every slot is a valid record and only z is zeroed.
//       Wp is formed in registers: two rows of W (L1 / L2: W is m x ldw, 51 KB at m = 100 and 64 columns) and two multiplies per
//       16-column block, no table; the loads of the first GPZ_GAMMA_PF blocks are issued ahead of the density work.  A lane carries
//       its pair's (a, b) and steps them by 4 pairs.
//       Density::NB blocks of accumulators per pass; more columns are further passes on gridDim.z that form z again.  gridDim.y: the
//       pair chunks, predict_gamma_chunks(m) of the model's shape alone; chunk c writes its partial sums to part [C][ncol][ldp].
//   Density    a struct without virtuals: D (the dimension), PW (the values of Psi a lane loads for its row: D columns of Psic, or
//              more where a row's Psi is a packed triangle), RL (the doubles of a record head that are staged), NB (16-column blocks
//              of accumulators per pass), its members (what a lane keeps across K steps), init(tab, ps) once per row before the
//              loop, and z(t, x, ps) for one staged head t.
// No atomics; every sum starts from zero and runs in one order that the model's shape fixes (pairs in table order, four per K step from
// the chunk's first pair, chunks in chunk order): a row's gamma_s has the same bits for any tile size, row order, position in its block,
// other rows of the call and any number of draws > s.
#pragma once
#include "gpz_dev.h"
#include "gpz_kernels.h"

#define GPZ_GAMMA_TP 32   // pair records per LDS stage: 8 K steps
#define GPZ_GAMMA_PF 4    // the blocks whose W rows are fetched ahead of the density work (64 columns: the usual 64 draws)

struct PredGammaArgs {
    const double *Xc, *Psic; long ldx;   // [d][ldx] column layout, n rows
    int n, m;
    const double *tab; int rec;          // pair records, rec doubles apart; the first Density::RL are read
    long ppc;                            // pairs per chunk (a multiple of 4)
    const double *W; int ldw;            // ceil16(m) x ldw row-major, columns >= ncol zero
    int ncol, nbw;                       // columns; 16-column blocks
    double *part; long ldp;              // [chunks][ncol][ldp]
};

// the arguments of a launch over nchunk pair chunks
static inline PredGammaArgs predict_gamma_args(const double *Xc, const double *Psic, long ldx, int n, int m, const double *tab, int rec,
                                               const double *W, int ldw, int ncol, int nchunk, double *part, long ldp) {
    const long npair = (long)m * (m + 1) / 2;
    PredGammaArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.m = m; a.tab = tab; a.rec = rec;
    a.ppc = ((npair + nchunk - 1) / nchunk + 3) / 4 * 4;
    a.W = W; a.ldw = ldw; a.ncol = ncol; a.nbw = (ncol + 15) / 16;
    a.part = part; a.ldp = ldp;
    return a;
}

// and its grid: 64 rows per workgroup, the chunks, the passes of nb blocks (the policy's NB)
static inline dim3 predict_gamma_grid(const PredGammaArgs &a, int nchunk, int nb) {
    return dim3((unsigned)((a.n + 63) / 64), (unsigned)nchunk, (unsigned)((a.nbw + nb - 1) / nb));
}

template <class Density>
__device__ __forceinline__ void predict_gamma_body(const PredGammaArgs &a) {
    constexpr int D = Density::D, PW = Density::PW, RL = Density::RL, NB = Density::NB, NST = GPZ_GAMMA_TP * RL, NPRE = (NST + 255) / 256;
    __shared__ double sT[NST];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, lr = lane & 15;
    const long i = ((long)blockIdx.x * 4 + wv) * 16 + lr;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    double x[D], ps[PW];
    if constexpr (PW == D) {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            x[c] = a.Xc[(size_t)c * a.ldx + ic];
            ps[c] = a.Psic[(size_t)c * a.ldx + ic];
        }
    } else {   // a policy whose row has more (or fewer) values of Psi than dimensions
#pragma unroll
        for (int c = 0; c < D; ++c) x[c] = a.Xc[(size_t)c * a.ldx + ic];
        const double *pq = a.Psic + ic;   // stepped in vector registers: PW uniform offsets at once would not fit the scalar file
#pragma unroll
        for (int c = 0; c < PW; ++c) {
            ps[c] = *pq;
            pq += a.ldx;
            asm volatile("" : "+v"(pq));
        }
    }
    const int ch = blockIdx.y, cb0 = blockIdx.z * NB;
    const int nb = __builtin_amdgcn_readfirstlane(a.nbw - cb0 < NB ? a.nbw - cb0 : NB);
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
    d4_t acc[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) acc[q] = (d4_t){0.0, 0.0, 0.0, 0.0};
    const double *wl = a.W + (size_t)cb0 * 16 + lr;
    Density den;
    den.init(a.tab, ps);
    double pre[NPRE];
    // the heads of the records [pbase, pbase + 32) of the chunk (clamped to its last one, so that every slot of a stage holds a record)
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
#pragma unroll 1
        for (int ks = 0; ks < nks; ++ks) {
            const int slot = 4 * ks + g;
            const bool valid = pbase + slot < p1;
            const int aa = valid ? pa : 0, bb = valid ? pb : 0;
            const double f = aa == bb ? 1.0 : 2.0;                     // 2x off the diagonal, 1x on it   predictDiag.m:113-119, predictCov.m:113-119
            const double *wa = wl + (size_t)aa * a.ldw, *wb = wl + (size_t)bb * a.ldw;
            // the two rows of W for the first GPZ_GAMMA_PF blocks are fetched here, so that the density work below covers their latency
            double wav[GPZ_GAMMA_PF], wbv[GPZ_GAMMA_PF];
#pragma unroll
            for (int qb = 0; qb < GPZ_GAMMA_PF; ++qb) {
                const int off = qb < nb ? 16 * qb : 0;
                wav[qb] = wa[off];
                wbv[qb] = wb[off];
            }
            double z = den.z(sT + slot * RL, x, ps);   // one address per 16 lanes: a broadcast read
            z = valid ? z : 0.0;
#pragma unroll
            for (int qb = 0; qb < NB; ++qb)
                if (qb < nb) {
                    // (the inner conditions repeat the outer one only to keep the constant index of the unrolled dead arm in bounds)
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
    for (int qb = 0; qb < NB; ++qb)
        if (qb < nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = (cb0 + qb) * 16 + g + 4 * r;
                if (col < a.ncol) a.part[((size_t)ch * a.ncol + col) * a.ldp + i] = acc[qb][r];
            }
        }
}
