// gamma under every weight draw for rows with input noise on a covariance kind (gpz_predictor_stack_noisy_cov_dev /
// _draws_gamma_noisy_cov_dev, gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab z_ab(x_i, psi_i) w_s,a w_s,b - mu_s,i^2 per output,
// predictNoisy's gamma of GC and VC (predictCov.m:105-119) with the draw's weights in place of w; f_ab = 2 off the diagonal, 1 on it.
//
//   k_predict_noisy_cov_gamma<D, SHARED>
//       k_predict_noisy_gamma's frame (k_predict_noisy_gamma.hip): the sum over the pairs is a product E (rows x pairs) Wp (pairs x
//       columns), Wp[ab, col] = f_ab W[a, col] W[b, col], taken transposed on v_mfma_f64_16x16x4_f64 with Wp as the A operand and z as
//       the B operand, so an accumulator lane holds one row and 4 columns per 16-column block.  A wave owns 16 rows, a workgroup 64; in
//       a K step lane l forms ONE pair density z(row l & 15, pair 4 ks + (l >> 4)), and no z reaches memory or LDS.
//       The density is k_predict_noisy_cov_small's (ncov_factor / ncov_density, k_ncov_density.h): the packed Cholesky of C_ab +
//       diag(psi_i) and a forward substitution, z = exp(lnZ - 1/2 q) prod(1 / L_cc).  The 16 lanes that share a pair read the head of
//       its record [lnZ | c_ab | C_ab packed lower] (the first 1 + d + d (d + 1) / 2 doubles of the handle's packed pair records, read
//       with the table's stride) as an LDS broadcast; the workgroup stages 32 heads at a time between two barriers, the next stage's
//       loads in flight in registers meanwhile.
//       SHARED (GC): every C_ab is one matrix, so a lane factorises C + psi of its row once, from record 0, before the loop (the same
//       bits in every chunk and pass), and a K step is the substitution alone.
//       Wp is formed in registers from two rows of the handle's W, (f W[a]) W[b], with (a, b) stepped in integers: no table.
//       ncg_blocks(D) 16-column blocks of accumulators per pass: 8 (128 columns) for d <= 7, 4 for d >= 8, where the packed triangle
//       leaves the accumulators less room; more columns are further passes on gridDim.z that form z again.  gridDim.y: the pair
//       chunks, predict_gamma_chunks(m) of the model's shape alone; chunk c writes its partial sums to part [C][ncol][ldp].
// k_gamma_finish_dev / k_gamma_finish_s2 (k_predict_noisy_gamma.hip) add the chunks and take mu_s^2 off.
// No atomics; every sum starts from zero and runs in one order that the model's shape fixes (pairs in table order, four per K step from
// the chunk's first pair, chunks in chunk order): a row's gamma_s has the same bits for any tile size, row order, position in its block,
// other rows of the call and any number of draws > s.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_ncov_density.h"   // ncov_factor, ncov_density

#define NCG_TP 32   // pair records per LDS stage: 8 K steps
#define NCG_PF 4    // the blocks whose W rows are fetched ahead of the density work (64 columns: the usual 64 draws)

// 16-column blocks of accumulators per pass
constexpr int ncg_blocks(int d) { return d <= 7 ? 8 : 4; }

struct PredCovGammaArgs {
    const double *Xc, *Psic; long ldx;   // [d][ldx] column layout, n rows
    int n, m;
    const double *tab; int rec;          // packed pair records, rec doubles apart; the first 1 + d + d (d + 1) / 2 are read
    long ppc;                            // pairs per chunk (a multiple of 4)
    const double *W; int ldw;            // ceil16(m) x ldw row-major, columns >= ncol zero
    int ncol, nbw;                       // columns; 16-column blocks
    double *part; long ldp;              // [chunks][ncol][ldp]
};

// D = 9 is held to 256 registers (two workgroups per compute unit) by the second launch bound: left alone it takes 252 (VC) and 258
// (GC).  D = 10 does not fit 256 without scratch and keeps one workgroup per compute unit.
template <int D, bool SHARED>
__global__ __launch_bounds__(256, D == 9 ? 2 : 1) void k_predict_noisy_cov_gamma(PredCovGammaArgs a) {
    constexpr int NP = D * (D + 1) / 2, RL = 1 + D + NP, NST = NCG_TP * RL, NPRE = (NST + 255) / 256, NB = ncg_blocks(D);
    __shared__ double sT[NST];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, lr = lane & 15;
    const long i = ((long)blockIdx.x * 4 + wv) * 16 + lr;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    double x[D], ps[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        x[c] = a.Xc[(size_t)c * a.ldx + ic];
        ps[c] = a.Psic[(size_t)c * a.ldx + ic];
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
    double M[NP], rd[D], prd;
    if (SHARED) ncov_factor<D>(a.tab + 1 + D, ps, M, rd, &prd);   // C + Psi of the row, once                  predictCov.m:109
    double pre[NPRE];
    // the heads of the records [pbase, pbase + 32) of the chunk (clamped to its last one, so that every slot of a stage holds a record)
#define NCG_LOAD(pbase)                                                                \
    _Pragma("unroll") for (int u = 0; u < NPRE; ++u) {                                 \
        const int t = tid + 256 * u;                                                   \
        if (t < NST) {                                                                 \
            const int jj = t / RL, f = t - jj * RL;                                    \
            const int pr = (pbase) + jj < p1 ? (pbase) + jj : p1 - 1;                  \
            pre[u] = a.tab[(size_t)pr * a.rec + f];                                    \
        }                                                                              \
    }
    NCG_LOAD(p0)
    for (int pbase = p0; pbase < p1; pbase += NCG_TP) {
        __syncthreads();   // the stage before is read
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            const int t = tid + 256 * u;
            if (t < NST) sT[t] = pre[u];
        }
        __syncthreads();
        if (pbase + NCG_TP < p1) { NCG_LOAD(pbase + NCG_TP) }
        const int left = p1 - pbase, nks = ((left < NCG_TP ? left : NCG_TP) + 3) >> 2;
#pragma unroll 1
        for (int ks = 0; ks < nks; ++ks) {
            const int slot = 4 * ks + g;
            const bool valid = pbase + slot < p1;
            const int aa = valid ? pa : 0, bb = valid ? pb : 0;
            const double f = aa == bb ? 1.0 : 2.0;                     // 2x off the diagonal, 1x on it       predictCov.m:113-119
            const double *wa = wl + (size_t)aa * a.ldw, *wb = wl + (size_t)bb * a.ldw;
            // the two rows of W for the first NCG_PF blocks are fetched here, so that the density work below covers their latency
            double wav[NCG_PF], wbv[NCG_PF];
#pragma unroll
            for (int qb = 0; qb < NCG_PF; ++qb) {
                const int off = qb < nb ? 16 * qb : 0;
                wav[qb] = wa[off];
                wbv[qb] = wb[off];
            }
            const double *t = sT + slot * RL;   // one address per 16 lanes: a broadcast read
            if (!SHARED) ncov_factor<D>(t + 1 + D, ps, M, rd, &prd);   // Cij + Psi                           :109
            double z = ncov_density<D>(t + 1, t[0], x, M, rd, prd);    //                                     :111
            z = valid ? z : 0.0;
#pragma unroll
            for (int qb = 0; qb < NB; ++qb)
                if (qb < nb) {
                    // (the inner conditions repeat the outer one only to keep the constant index of the unrolled dead arm in bounds)
                    const double wp = qb < NCG_PF ? (f * wav[qb < NCG_PF ? qb : 0]) * wbv[qb < NCG_PF ? qb : 0]
                                                  : (f * wa[16 * qb]) * wb[16 * qb];
                    acc[qb] = MFMA_F64(wp, z, acc[qb]);
                }
            pb += 4;   // four pairs on
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (pb > pa) { pb -= pa + 1; ++pa; }
        }
    }
#undef NCG_LOAD
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

template <int D>
static void launch_ncg(hipStream_t st, PredCovGammaArgs a, int nchunk, bool shared) {
    const dim3 grid((unsigned)((a.n + 63) / 64), (unsigned)nchunk, (unsigned)((a.nbw + ncg_blocks(D) - 1) / ncg_blocks(D)));
    if (shared) hipLaunchKernelGGL((k_predict_noisy_cov_gamma<D, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_predict_noisy_cov_gamma<D, false>), grid, dim3(256), 0, st, a);
}

int launch_predict_noisy_cov_gamma(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m,
                                   const double *tab, int rec, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > 10 || m < 1 || nchunk < 1 || ldw % 16 || ncol > ldw || rec < 1 + d + d * (d + 1) / 2 || ldp < n) return -1;
    const long npair = (long)m * (m + 1) / 2;
    PredCovGammaArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.m = m; a.tab = tab; a.rec = rec;
    a.ppc = ((npair + nchunk - 1) / nchunk + 3) / 4 * 4;
    a.W = W; a.ldw = ldw; a.ncol = ncol; a.nbw = (ncol + 15) / 16;
    a.part = part; a.ldp = ldp;
    switch (d) {
#define NCG_CASE(DD) case DD: launch_ncg<DD>(st, a, nchunk, shared); break;
        NCG_CASE(1) NCG_CASE(2) NCG_CASE(3) NCG_CASE(4) NCG_CASE(5) NCG_CASE(6) NCG_CASE(7) NCG_CASE(8) NCG_CASE(9) NCG_CASE(10)
#undef NCG_CASE
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
