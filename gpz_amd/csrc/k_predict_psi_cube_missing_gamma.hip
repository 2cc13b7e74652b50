// gamma under every weight draw for rows with a full input-noise covariance AND missing inputs on a covariance kind
// (gpz_predictor_stack_psi_cube_missing_dev / _draws_gamma_psi_cube_missing_dev, gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab
// z_ab(x_i, Psi_i) w_s,a w_s,b - mu_s,i^2 per output, predictNoisyMissing's gamma of GC and VC (predictCov.m:233-337) with the draw's
// weights in place of w.  One tile of ONE group of rows that share a NaN pattern and carry a d x d matrix Psi each; z_ab is the pair
// quantity of k_predict_psi_cube_missing_pairs, from the same slab records (k_predict_noisy_missing_cov.hip, where they are described)
// and the tile's Pio, with pnmc_density<PsiTri<NO>> of k_pnmc_density.h on the observed triangle Psio [no (no + 1) / 2][ldx]
// (k_predict_psi_cube_missing.hip stages it).
//
//   k_predict_psi_cube_missing_gamma<NO>
//       k_predict_noisy_missing_cov_gamma's frame, line for line: the sum over the pairs is a product E (rows x pairs) Wp (pairs x
//       columns) taken transposed on v_mfma_f64_16x16x4_f64, Wp the A operand and z, as it stands in its register, the B operand.
//       64 rows per workgroup, four waves, a wave owns 16 rows; in a K step lane l forms ONE z of (row l & 15, pair 4 ks + (l >> 4)),
//       the m components in index order from zero, Pio from the workgroup's [m][64] block in dynamic LDS, the four pairs' records
//       staged GPZ_PCMG_SB components at a time into four slots an odd stride apart and read as broadcasts.  x_o and the row's
//       no (no + 1) / 2 values of Psi_oo stay in registers for the whole launch, so LDS is the twin's:
//       predict_noisy_missing_cov_gamma_lds(m, d, no).  pcmg_nb(NO) 16-column blocks of accumulators per pass, a function of NO alone;
//       more columns are further passes on gridDim.z that form z again.  Column sums are independent, so no bit depends on the blocks
//       of a pass.  gridDim.y: predict_missing_cov_chunks(m) chunks of the slab's pairs; the first slab stores, later slabs add.
//   k_gamma_finish_dev / _s2  (k_predict_noisy_gamma.hip) add the chunks in chunk order and subtract mu_s^2.
// Where it could fault, and what holds it: a lane past the chunk's last pair reads the record of the chunk's last pair (a valid one),
// its z is zeroed and its (a, b) is (0, 0); a chunk without pairs reads nothing; rows past n are clamped to n - 1 for loads (X, Psi and
// Pio) and never stored; a pass covers blocks cb < nbw = ceil(ncol / 16) <= ldw / 16 only (the launcher refuses ldw % 16 and
// ncol > ldw); record offsets are formed in 64 bits; the stage of a slot holds nl rl <= 4 rl < its stride; dynamic LDS above 64 KB is
// opted in per launch; the launcher refuses a null Psi, patterns without an observed or without a missing dimension, a wrong chunk
// count, leading dimensions below n and shapes outside predict_missing_cov_fits.
// Every sum starts from zero and runs in one order that m, d and no fix: a row's gamma_s has the same bits for any tile size, row
// order, company, position in its block, split into calls and any number of draws > s.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_pnmc_density.h"

#define GPZ_PCMG_SB 4   // components of each pair slot per LDS stage (the twin's: predict_noisy_missing_cov_gamma_lds counts them)
#define GPZ_PCMG_PF 4   // the blocks whose W rows are fetched ahead of the density work (64 columns: the usual 64 draws)

// most 16-column blocks of accumulators per pass and the workgroups per compute unit the registers are bounded for, by the observed
// dimensions alone.  The triangle adds no (no - 1) / 2 doubles to the twin's registers: 8 blocks under 256 registers up to NO = 5;
// NO = 6 fits 256 registers with 4 blocks (the usual 64 draws of one output are one pass still); NO = 7, 8 and 9 take one workgroup
// per compute unit (up to 512 registers) and 8 blocks.  DESIGN.md section 34 has the compile report behind this.
constexpr int pcmg_nb(int no) { return no == 6 ? 4 : 8; }
constexpr int pcmg_wg(int no) { return no <= 6 ? 2 : 1; }

struct PcmgArgs {
    const double *Xc, *Psio; long ldx; int n;   // the tile's rows [d][ldx] and the observed triangles [no (no + 1) / 2][ldx]
    int oidx[PMCV_MAXD];                   // the observed dimensions in ascending order
    int nu, rl;                            // the missing dimensions; doubles per record
    int m;
    const double *Pio; long ldr;           // [m][ldr]
    const double *rec;                     // the slab: cnt pairs of m records
    long q0; int cnt, ppc;                 // the slab's first pair, its pairs, pairs per chunk
    const double *W; int ldw;              // ceil16(m) x ldw row-major, columns >= ncol zero
    int ncol, nbw;                         // columns; 16-column blocks
    double *part; long ldp; int first;     // [chunks][ncol][ldp]; first: the slab's sums are stored, not added
};

// the doubles between the stages of two pair slots: odd, so that four slots start in four different banks (the twin's nmcg_stride)
static inline __host__ __device__ int pcmg_stride(int rl) { return (GPZ_PCMG_SB * rl) | 1; }

template <int NO>
__global__ __launch_bounds__(256, pcmg_wg(NO)) void k_predict_psi_cube_missing_gamma(PcmgArgs a) {
    constexpr int NB = pcmg_nb(NO);
    extern __shared__ double sm[];
    double *sPio = sm;                                   // [m][64]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, lr = lane & 15, m = a.m, rl = a.rl, nu = a.nu;
    const int ss = pcmg_stride(rl);
    double *sRec = sm + (size_t)m * 64;                  // four pair slots, ss doubles apart
    const long row0 = (long)blockIdx.x * 64, i = row0 + wv * 16 + lr;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    for (int e = tid; e < m * 64; e += 256) {
        const long r = min(row0 + (e & 63), (long)a.n - 1);
        sPio[e] = a.Pio[(size_t)(e >> 6) * a.ldr + r];
    }
    double x[NO], ps[NO * (NO + 1) / 2];
#pragma unroll
    for (int c = 0; c < NO; ++c) x[c] = a.Xc[(size_t)a.oidx[c] * a.ldx + ic];
    ncov_psi_load(a.Psio + ic, a.ldx, ps);
    const int ch = blockIdx.y, cb0 = blockIdx.z * NB;
    const int nb = __builtin_amdgcn_readfirstlane(a.nbw - cb0 < NB ? a.nbw - cb0 : NB);
    const int p0 = ch * a.ppc, p1 = min(a.cnt, p0 + a.ppc);
    // the lane's pair e = q0 + p0 + g + 4 ks as (pa >= pb): e = pa (pa + 1) / 2 + pb
    int pa, pb;
    gpz_pair_of(a.q0 + p0 + g, &pa, &pb);
    d4_t acc[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) acc[q] = (d4_t){0.0, 0.0, 0.0, 0.0};
    const double *wl = a.W + (size_t)cb0 * 16 + lr;
    const double *pio = sPio + wv * 16 + lr, *tr = sRec + g * ss;
    double *stage = sRec + wv * ss;
    for (int pbase = p0; pbase < p1; pbase += 4) {       // one K step: the pairs pbase .. pbase + 3
        const bool valid = pbase + g < p1;
        const int aa = valid ? pa : 0, bb = valid ? pb : 0;
        const double f = aa == bb ? 1.0 : 2.0;           // 2x off the diagonal, 1x on it                       predictCov.m:308-320
        const double *wa = wl + (size_t)aa * a.ldw, *wb = wl + (size_t)bb * a.ldw;
        double wav[GPZ_PCMG_PF], wbv[GPZ_PCMG_PF];
#pragma unroll
        for (int qb = 0; qb < GPZ_PCMG_PF; ++qb) {
            const int off = qb < nb ? 16 * qb : 0;
            wav[qb] = wa[off];
            wbv[qb] = wb[off];
        }
        // wave wv copies pair slot wv; a slot past the chunk's last pair holds that pair again, so every slot is a valid record
        const double *src = a.rec + (size_t)min(pbase + wv, p1 - 1) * m * rl;
        double z = 0.0;
        for (int lb = 0; lb < m; lb += GPZ_PCMG_SB) {
            const int nl = min(GPZ_PCMG_SB, m - lb);
            __syncthreads();                             // the stage before is read (and, the first time, sPio is written)
            for (int t = lane; t < nl * rl; t += 64) stage[t] = src[(size_t)lb * rl + t];
            __syncthreads();
#pragma unroll 1
            for (int e = 0; e < nl; ++e)
                z = fma(pio[(lb + e) * 64], pnmc_density<PsiTri<NO>>(tr + e * rl, nu, x, ps), z);   // index order
        }
        z = valid ? z : 0.0;
#pragma unroll
        for (int qb = 0; qb < NB; ++qb)
            if (qb < nb) {
                // (the inner conditions repeat the outer one only to keep the constant index of the unrolled dead arm in bounds)
                const double wp = qb < GPZ_PCMG_PF ? (f * wav[qb < GPZ_PCMG_PF ? qb : 0]) * wbv[qb < GPZ_PCMG_PF ? qb : 0]
                                                   : (f * wa[16 * qb]) * wb[16 * qb];
                acc[qb] = MFMA_F64(wp, z, acc[qb]);
            }
        pb += 4;   // four pairs on
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (pb > pa) { pb -= pa + 1; ++pa; }
    }
    // ---- lane l, register r of block qb holds the sum of row l & 15 and column 16 (cb0 + qb) + (l >> 4) + 4 r
    if (!act) return;
#pragma unroll
    for (int qb = 0; qb < NB; ++qb)
        if (qb < nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = (cb0 + qb) * 16 + g + 4 * r;
                if (col < a.ncol) {
                    double *dst = a.part + ((size_t)ch * a.ncol + col) * a.ldp + i;
                    *dst = a.first ? acc[qb][r] : *dst + acc[qb][r];       // slab order
                }
            }
        }
}

// per launch, not once per process: the attribute belongs to the current device's copy of the kernel
template <int NO>
static int pcmg_launch(hipStream_t st, dim3 grid, size_t lds, const PcmgArgs &a) {
    if (lds > 65536 && hipFuncSetAttribute((const void *)k_predict_psi_cube_missing_gamma<NO>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -1;
    grid.z = (unsigned)((a.nbw + pcmg_nb(NO) - 1) / pcmg_nb(NO));
    hipLaunchKernelGGL((k_predict_psi_cube_missing_gamma<NO>), grid, dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_predict_psi_cube_missing_gamma(hipStream_t st, const double *Xc, const double *Psio, long ldx, int n, const double *Pio,
                                          long ldr, int m, int d, unsigned obs, const double *raw, const double *bas, double *slab,
                                          bool *slab_kept, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || m < 1 || ((m + 15) / 16) * 16 > 256 || nchunk != predict_missing_cov_chunks(m) || ldw < 16 || ldw % 16 ||
        ncol > ldw || ldr < n || ldp < n || ldx < n || !Psio)
        return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.nu < 1 || pt.no < 1) return -1;
    const int nslab = predict_noisy_missing_cov_slabs(m, d, pt.no);
    const long npair = (long)m * (m + 1) / 2, sp = predict_noisy_missing_cov_slab_pairs(m, d, pt.no);
    PcmgArgs a{};
    a.Xc = Xc; a.Psio = Psio; a.ldx = ldx; a.n = n; a.m = m; a.Pio = Pio; a.ldr = ldr; a.rec = slab;
    a.nu = pt.nu; a.rl = predict_noisy_missing_cov_rec(d, pt.no);
    for (int c = 0; c < pt.no; ++c) a.oidx[c] = pt.o[c];
    a.W = W; a.ldw = ldw; a.ncol = ncol; a.nbw = (ncol + 15) / 16;   // <= ldw / 16
    a.part = part; a.ldp = ldp;
    const size_t lds = predict_noisy_missing_cov_gamma_lds(m, d, pt.no);
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)nchunk, 1);   // (z: the passes, set per instantiation)
    for (int s = 0; s < nslab; ++s) {
        const long q0 = s * sp, cnt = (npair - q0 < sp) ? npair - q0 : sp;
        if (cnt <= 0) break;
        // the whole table is one slab: it stays until the pattern's tables change, whichever kernel filled it
        if (!(nslab == 1 && *slab_kept) && launch_pnmc_triples(st, d, obs, q0, cnt, m, raw, bas, slab)) return -1;
        a.q0 = q0; a.cnt = (int)cnt; a.ppc = (int)((cnt + nchunk - 1) / nchunk); a.first = s == 0;
        int rc;
#define PCMG_LAUNCH(NN) rc = pcmg_launch<NN>(st, grid, lds, a)
        PNMC_CASES(PCMG_LAUNCH)
#undef PCMG_LAUNCH
        if (rc) return -1;
    }
    *slab_kept = nslab == 1;
    return 0;
}
