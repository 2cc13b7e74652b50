// The frame of the tile kernels for ONE group of rows that share a NaN pattern and carry input noise, on a covariance kind:
// predictNoisyMissing of GC and VC (predictCov.m:233-337).  k_pnmc_ex / _phi, k_predict_noisy_missing_cov_pairs and
// k_predict_noisy_missing_cov_gamma (Psi a variance per observed input: the slot has Xc's layout, [d][ldx]) and k_pcm_ex / _phi,
// k_predict_psi_cube_missing_pairs and k_predict_psi_cube_missing_gamma (Psi a d x d matrix per row: the slot holds the packed lower
// triangle of its observed x observed block, [no (no + 1) / 2][ldx], column LT(ro, co) the element (o[ro], o[co])).  Each is a thin
// __global__ wrapper of a body below; what differs between the twins is the Psi policy (PsiDiag, PsiTri: k_ncov_density.h), that is
// the width of the row's ps[] and how nmcov_load fills it, and through pnmc_density<P> (k_pnmc_density.h) the matrix of the density,
// M + diag(psi_o) or M + Psi_oo over the whole triangle.  With zeros off the diagonal the sums are M + 0.0: a cube of diagonals has
// the bits of the per-dimension form.  The records (predict_noisy_missing_cov_rec(d, no) = rl doubles, which do not depend on Psi),
// their slabs and the tables are k_predict_noisy_missing_cov.hip's, where they are described; NO = 1 .. 9 observed dimensions.
//
//   nmcov_ex_body<P, DYNAMIC>   lane = row, 256 rows per workgroup, x_o and ps in registers: Ex over the m records in index order,
//                         Pio [l][ldr] = Ex_l / sum (:266, :281).  The records pass through one LDS stage of PNMC_STD doubles, whole
//                         records at a time, between two barriers, and are read as broadcasts.  The stage is the unit's choice
//                         (nmcov_stage): static LDS in k_pnmc_ex / _phi, the launch's dynamic LDS in k_pcm_ex / _phi
//                         (profiles/r27_predict_nmcov_fold.txt part 4b has the times of both forms).
//   nmcov_phi_body<P, DYNAMIC>   the same stage: PHI(i) = sum_j Pio_j z(rec_ij) in index order -> Phi [nrow][mp] as launch_tgemm takes it,
//                         zeros in the rows >= n and the columns >= m; gridDim.y chunks of ipc basis functions           (:291-299)
//   nmcov_pairs_body<P, KM>   the frame of k_predict_missing_cov_pairs: 64 rows per workgroup, lane = row in each of four waves, the
//                         Pio block [m][64] in LDS; the waves deal the chunk's pairs round-robin and stage their pair's records
//                         PNMC_SB at a time, read as broadcasts; the m components in index order, 3 KM multiply-adds per pair;
//                         partials in wave order, slabs in slab order; gridDim.y = predict_missing_cov_chunks(m).  LDS:
//                         predict_noisy_missing_cov_lds(m, d, no, k).
//   nmcov_gamma_body<P, NB>   gamma under every weight draw, gamma_s,i = sum_{a >= b} f_ab z_ab(x_i, Psi_i) w_s,a w_s,b - mu_s,i^2
//                         (f_ab = 2 off the diagonal, 1 on it), with k_predict_missing_cov_gamma's frame: the sum over the pairs is a
//                         product E (rows x pairs) Wp (pairs x columns), Wp[ab, col] = (f_ab W[a, col]) W[b, col], taken transposed
//                         on v_mfma_f64_16x16x4_f64: Wp is the A operand, z the B operand.  64 rows per workgroup, four waves; a wave
//                         owns 16 rows for the whole launch.  In a K step lane l forms ONE z of (row l & 15, pair 4 ks + (l >> 4)): the
//                         m components in index order from zero, Pio from the workgroup's [m][64] block in LDS.  All four waves work
//                         on the same four pairs, so the workgroup stages their records between two barriers, GPZ_NMCG_SB components
//                         of each pair at a time: wave w copies pair slot w.  The 16 lanes that share a pair read a record as a
//                         broadcast; the four slots lie nmcg_stride(rl) = (4 rl) | 1 doubles apart, an odd stride, so that the four
//                         addresses of a wave's read are 0, S, 2 S, 3 S (mod 32 doubles): four different banks.  z is, as it stands,
//                         the B operand; Wp is formed in registers from two rows of W (the handle's Wd, ceil16(m) x ldw), the first
//                         GPZ_NMCG_PF blocks fetched ahead of the density work.  No z reaches memory or LDS, no cross-wave reduction.
//                         NB 16-column blocks of accumulators per pass (the unit's nb(NO), a function of NO alone), the count of a
//                         pass read at run time under that bound; more columns are further passes on gridDim.z that form z again.
//                         Column sums are independent, so no bit depends on the blocks of a pass.  gridDim.y: the chunks of the
//                         slab's pairs, chunk c into part [C][ncol][ldp]; a lane's (a, b) comes from the global pair index q0 + p.
//                         LDS: predict_noisy_missing_cov_gamma_lds(m, d, no) = (64 m + 4 ((4 rl) | 1)) doubles, at most 149792
//                         bytes (m = 256, d = 10, NO = 9).  k_gamma_finish_dev / _s2 (k_predict_noisy_gamma.hip) add the chunks in
//                         chunk order and subtract mu_s^2.
//   nmcov_launch_rows<K> / _pairs<K> / _gamma<K>   the launchers of a unit, K naming its wrappers (and, for gamma, its nb(NO)).
// All other LDS is dynamic, passed at launch.  x_o and the row's ps stay in registers for the whole launch, so neither LDS figure depends on
// the form of Psi; Psi in a missing row or column is never read.  No atomics; every sum starts from zero and runs in one order that m,
// d and no fix (components in index order, pairs in table order from the chunk's first pair, partials in wave order, slabs in slab
// order, chunks in chunk order): a row's results have the same bits for any tile size, row order, company, position in its block,
// split into calls and, for gamma_s, any number of draws > s.
// Where it could fault, and what holds it: rows past n are clamped to n - 1 for loads (X, Psi and Pio) and never stored; a wave of the
// pair kernel without a pair reads the chunk's first pair (a valid record) and adds nothing; a lane of the gamma kernel past the
// chunk's last pair reads the record of the chunk's last pair (a valid one), its z is zeroed and its (a, b) is (0, 0); a chunk without
// pairs reads nothing; a pass covers blocks cb < nbw = ceil(ncol / 16) <= ldw / 16 only (the launcher refuses ldw % 16 and
// ncol > ldw); record offsets are formed in 64 bits; the Ex / PHI stage holds nl rl <= PNMC_STD doubles (the launcher refuses
// rl > PNMC_STD), a wave's stage nl rl <= PNMC_SB rl, its size, a slot's nl rl <= 4 rl < its stride; dynamic LDS above 64 KB is opted
// in per launch; the launchers refuse shapes outside predict_missing_cov_fits, no < 1, nu < 1, a wrong chunk count, leading
// dimensions below n and a null Psi.  A matrix that is not positive semidefinite gives its own row NaN (a non-positive pivot) and
// touches no other row.
#pragma once
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_pnmc_density.h"   // pnmc_density, PNMC_CASES; PsiDiag, PsiTri, ncov_psi_load; PMCV_MAXD, PmcvPat, pmcv_pat; LT

#define PNMC_STD 2048   // doubles of the LDS stage of the Ex and PHI kernels (whole records: at least 13)
#define PNMC_SB 4       // records per LDS stage of a wave of the pair kernel (predict_noisy_missing_cov_lds counts them)
#define GPZ_NMCG_SB 4   // components of each pair slot per LDS stage of the gamma kernel (predict_noisy_missing_cov_gamma_lds counts them)
#define GPZ_NMCG_PF 4   // the blocks whose W rows are fetched ahead of the density work (64 columns: the usual 64 draws)

// the doubles between the stages of two pair slots: odd, so that four slots start in four different banks
static inline __host__ __device__ int nmcg_stride(int rl) { return (GPZ_NMCG_SB * rl) | 1; }

struct PredNmcovArgs {
    const double *Xc, *Psi; long ldx; int n;    // the tile's rows [d][ldx] and the form's Psi slot
    int oidx[PMCV_MAXD];                        // the observed dimensions in ascending order
    int nu, rl;                                 // the missing dimensions; doubles per record
    int m, k;
    double *Pio; long ldr;                      // [m][ldr]
    const double *rec;                          // Ex: m records; PHI: m * m; pairs: the slab
    double *Phi; int nrow, mp, ipc;             // PHI: [nrow][mp], basis functions per gridDim.y chunk
    const double *coef; long q0; int cnt, ppc;  // pairs: the slab's first pair, its pairs, pairs per chunk
    double *part; long ldp; int first;          // pairs: [chunks][3k][ldp]; first: the slab's sums are stored, not added
};

struct PredNmcovGammaArgs {
    const double *Xc, *Psi; long ldx; int n;    // the tile's rows [d][ldx] and the form's Psi slot
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

// what both structs share, from the pattern
template <class A>
static inline void nmcov_fill(A &a, const PmcvPat &pt, const double *Xc, const double *Psi, long ldx, int n, int m, const double *rec) {
    a.Xc = Xc; a.Psi = Psi; a.ldx = ldx; a.n = n; a.m = m; a.rec = rec;
    a.nu = pt.nu; a.rl = predict_noisy_missing_cov_rec(pt.d, pt.no);
    for (int c = 0; c < pt.no; ++c) a.oidx[c] = pt.o[c];
}

// the row's Psi in its policy's layout: by observed dimension from a slot like Xc, or the triangle's columns as they lie
template <int NO, class A>
__device__ __forceinline__ void nmcov_load_psi(PsiDiag<NO>, const A &a, long ic, double (&ps)[NO]) {
#pragma unroll
    for (int c = 0; c < NO; ++c) ps[c] = a.Psi[(size_t)a.oidx[c] * a.ldx + ic];
}
template <int NO, class A>
__device__ __forceinline__ void nmcov_load_psi(PsiTri<NO>, const A &a, long ic, double (&ps)[NO * (NO + 1) / 2]) {
    ncov_psi_load(a.Psi + ic, a.ldx, ps);
}

// the row's observed inputs and its Psi, row ic (clamped by the caller)
template <class P, class A>
__device__ __forceinline__ void nmcov_load(const A &a, long ic, double (&x)[P::D], double (&ps)[P::W]) {
#pragma unroll
    for (int c = 0; c < P::D; ++c) x[c] = a.Xc[(size_t)a.oidx[c] * a.ldx + ic];
    nmcov_load_psi(P{}, a, ic, ps);
}

// the record stage of the Ex and PHI bodies, PNMC_STD doubles: static LDS, or the dynamic LDS that the launcher passes
template <bool DYNAMIC>
__device__ __forceinline__ double *nmcov_stage() {
    if constexpr (DYNAMIC) {
        extern __shared__ double dyn[];
        return dyn;
    } else {
        __shared__ double fix[PNMC_STD];
        return fix;
    }
}

// (the arguments by reference, where the other three bodies take a copy: as a copy k_pnmc_ex<4> issues the loads of x and psi behind
// its scalar set-up and runs 5 % longer; profiles/r27_predict_nmcov_fold.txt part 4c)
template <class P, bool DYNAMIC>
__device__ __forceinline__ void nmcov_ex_body(const PredNmcovArgs &a) {
    double *sT = nmcov_stage<DYNAMIC>();
    const int tid = threadIdx.x, rl = a.rl, nu = a.nu, per = PNMC_STD / rl;   // whole records per stage
    const long i = (long)blockIdx.x * 256 + tid;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    double x[P::D], ps[P::W];
    nmcov_load<P>(a, ic, x, ps);
    double s = 0.0;
    for (int lb = 0; lb < a.m; lb += per) {
        const int nl = min(per, a.m - lb);
        __syncthreads();
        for (int t = tid; t < nl * rl; t += 256) sT[t] = a.rec[(size_t)lb * rl + t];
        __syncthreads();
#pragma unroll 1
        for (int e = 0; e < nl; ++e) {
            const double z = pnmc_density<P>(sT + e * rl, nu, x, ps);
            s += z;                                                        // index order                          :281
            if (act) a.Pio[(size_t)(lb + e) * a.ldr + i] = z;
        }
    }
    if (!act) return;
    for (int l = 0; l < a.m; ++l) a.Pio[(size_t)l * a.ldr + i] /= s;
}

template <class P, bool DYNAMIC>
__device__ __forceinline__ void nmcov_phi_body(PredNmcovArgs a) {
    double *sT = nmcov_stage<DYNAMIC>();
    const int tid = threadIdx.x, rl = a.rl, nu = a.nu, per = PNMC_STD / rl;
    const long i = (long)blockIdx.x * 256 + tid;
    const bool act = i < a.n, st = i < a.nrow;   // rows n .. nrow - 1 are written as zeros
    const long ic = act ? i : a.n - 1;
    double x[P::D], ps[P::W];
    nmcov_load<P>(a, ic, x, ps);
    double *row = a.Phi + (size_t)(st ? i : 0) * a.mp;
    const int i0 = blockIdx.y * a.ipc, i1 = min(a.m, i0 + a.ipc);
    for (int b = i0; b < i1; ++b) {
        double z = 0.0;
        for (int lb = 0; lb < a.m; lb += per) {
            const int nl = min(per, a.m - lb);
            const double *src = a.rec + ((size_t)b * a.m + lb) * rl;
            __syncthreads();
            for (int t = tid; t < nl * rl; t += 256) sT[t] = src[t];
            __syncthreads();
#pragma unroll 1
            for (int e = 0; e < nl; ++e) z = fma(a.Pio[(size_t)(lb + e) * a.ldr + ic], pnmc_density<P>(sT + e * rl, nu, x, ps), z);
        }
        if (st) row[b] = act ? z : 0.0;
    }
    if (blockIdx.y == 0 && st)
        for (int j = a.m; j < a.mp; ++j) row[j] = 0.0;
}

template <class P, int KM>
__device__ __forceinline__ void nmcov_pairs_body(PredNmcovArgs a) {
    extern __shared__ double sm[];
    double *sPio = sm;                                   // [m][64]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, m = a.m, k = a.k, rl = a.rl, nu = a.nu;
    double *sRec = sm + (size_t)m * 64 + (size_t)w * (PNMC_SB * rl);   // this wave's stage
    const long row0 = (long)blockIdx.x * 64, i = row0 + lane;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    for (int e = tid; e < m * 64; e += 256) {
        const long r = min(row0 + (e & 63), (long)a.n - 1);
        sPio[e] = a.Pio[(size_t)(e >> 6) * a.ldr + r];
    }
    double x[P::D], ps[P::W];
    nmcov_load<P>(a, ic, x, ps);
    double acc[3 * KM];
#pragma unroll
    for (int e = 0; e < 3 * KM; ++e) acc[e] = 0.0;
    const int ch = blockIdx.y, p0 = ch * a.ppc, p1 = min(a.cnt, p0 + a.ppc);
    for (int pb = p0; pb < p1; pb += 4) {                // the four waves take pairs pb .. pb + 3
        const int p = pb + w;
        const bool on = p < p1;
        const double *src = a.rec + (size_t)(on ? p : p0) * m * rl;
        double z = 0.0;
        for (int lb = 0; lb < m; lb += PNMC_SB) {
            const int nl = min(PNMC_SB, m - lb);
            __syncthreads();                             // the stage before is read (and, the first time, sPio is written)
            if (on)
                for (int t = lane; t < nl * rl; t += 64) sRec[t] = src[(size_t)lb * rl + t];
            __syncthreads();
            if (on) {
#pragma unroll 1
                for (int e = 0; e < nl; ++e) z = fma(sPio[(lb + e) * 64 + lane], pnmc_density<P>(sRec + e * rl, nu, x, ps), z);
            }
        }
        if (on) {
            const double *cf = a.coef + (size_t)(a.q0 + p) * 3 * k;
#pragma unroll
            for (int o = 0; o < KM; ++o)
                if (o < k) {
                    acc[o] = fma(z, cf[3 * o], acc[o]);                    // gamma                                :308-320
                    acc[KM + o] = fma(z, cf[3 * o + 1], acc[KM + o]);      // VlnS
                    acc[2 * KM + o] = fma(z, cf[3 * o + 2], acc[2 * KM + o]);   // nu
                }
        }
    }
    __syncthreads();                                     // LDS is free: the partials of waves 1 .. 3, [wave - 1][3 KM][64]
    if (w > 0) {
#pragma unroll
        for (int e = 0; e < 3 * KM; ++e) sm[((w - 1) * 3 * KM + e) * 64 + lane] = acc[e];
    }
    __syncthreads();
    if (w > 0 || !act) return;
#pragma unroll
    for (int e = 0; e < 3 * KM; ++e) {
        const int q = e / KM, o = e - q * KM;
        if (o >= k) continue;
        double s = acc[e];
        for (int ww = 0; ww < 3; ++ww) s += sm[(ww * 3 * KM + e) * 64 + lane];   // wave order
        double *dst = a.part + ((size_t)ch * 3 * k + (size_t)q * k + o) * a.ldp + i;
        *dst = a.first ? s : *dst + s;                                     // slab order
    }
}

template <class P, int NB>
__device__ __forceinline__ void nmcov_gamma_body(PredNmcovGammaArgs a) {
    extern __shared__ double sm[];
    double *sPio = sm;                                   // [m][64]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, lr = lane & 15, m = a.m, rl = a.rl, nu = a.nu;
    const int ss = nmcg_stride(rl);
    double *sRec = sm + (size_t)m * 64;                  // four pair slots, ss doubles apart
    const long row0 = (long)blockIdx.x * 64, i = row0 + wv * 16 + lr;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    for (int e = tid; e < m * 64; e += 256) {
        const long r = min(row0 + (e & 63), (long)a.n - 1);
        sPio[e] = a.Pio[(size_t)(e >> 6) * a.ldr + r];
    }
    double x[P::D], ps[P::W];
    nmcov_load<P>(a, ic, x, ps);
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
        double wav[GPZ_NMCG_PF], wbv[GPZ_NMCG_PF];
#pragma unroll
        for (int qb = 0; qb < GPZ_NMCG_PF; ++qb) {
            const int off = qb < nb ? 16 * qb : 0;
            wav[qb] = wa[off];
            wbv[qb] = wb[off];
        }
        // wave wv copies pair slot wv; a slot past the chunk's last pair holds that pair again, so every slot is a valid record
        const double *src = a.rec + (size_t)min(pbase + wv, p1 - 1) * m * rl;
        double z = 0.0;
        for (int lb = 0; lb < m; lb += GPZ_NMCG_SB) {
            const int nl = min(GPZ_NMCG_SB, m - lb);
            __syncthreads();                             // the stage before is read (and, the first time, sPio is written)
            for (int t = lane; t < nl * rl; t += 64) stage[t] = src[(size_t)lb * rl + t];
            __syncthreads();
#pragma unroll 1
            for (int e = 0; e < nl; ++e) z = fma(pio[(lb + e) * 64], pnmc_density<P>(tr + e * rl, nu, x, ps), z);   // index order
        }
        z = valid ? z : 0.0;
#pragma unroll
        for (int qb = 0; qb < NB; ++qb)
            if (qb < nb) {
                // (the inner conditions repeat the outer one only to keep the constant index of the unrolled dead arm in bounds)
                const double wp = qb < GPZ_NMCG_PF ? (f * wav[qb < GPZ_NMCG_PF ? qb : 0]) * wbv[qb < GPZ_NMCG_PF ? qb : 0]
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

// ---- the launchers of a unit.  K: a struct with ex<NO>(), phi<NO>() and pairs<NO, KM>(), or with gamma<NO>() and nb(NO): the unit's
// __global__ wrappers, stage_lds (the dynamic LDS of its Ex and PHI kernels, bytes) and, for gamma, its blocks of a pass --------------------------------------------------------------------------------
// Pio [m][ldr], Phi [nrow][mp] and hd [2k][ldh] from the pattern's Ex and PHI records (launch_pnmc_tables)
template <class K>
static int nmcov_launch_rows(hipStream_t st, const double *Xc, const double *Psi, long ldx, int n, int nrow, int m, int mp, int d, int k,
                             unsigned obs, const double *exrec, const double *phirec, const double *w, const double *v, double *Pio,
                             long ldr, double *Phi, double *hd, long ldh) {
    if (n <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || m < 1 || nrow < n || mp < m || ldr < n || ldx < n || !Psi) return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.no < 1 || pt.nu < 1 || predict_noisy_missing_cov_rec(d, pt.no) > PNMC_STD) return -1;
    PredNmcovArgs a{};
    nmcov_fill(a, pt, Xc, Psi, ldx, n, m, exrec);
    a.k = k; a.Pio = Pio; a.ldr = ldr;
    PredNmcovArgs b = a;
    b.rec = phirec; b.Phi = Phi; b.nrow = nrow; b.mp = mp; b.ipc = 8;
    const dim3 ge((unsigned)((n + 255) / 256)), gp((unsigned)((nrow + 255) / 256), (unsigned)((m + b.ipc - 1) / b.ipc));
#define NMCOV_ROWS(NN)                                                                                       \
    do {                                                                                                     \
        hipLaunchKernelGGL((K::template ex<NN>()), ge, dim3(256), K::stage_lds, st, a);         \
        hipLaunchKernelGGL((K::template phi<NN>()), gp, dim3(256), K::stage_lds, st, b);        \
    } while (0)
    PNMC_CASES(NMCOV_ROWS)
#undef NMCOV_ROWS
    if (hipGetLastError() != hipSuccess) return -1;
    return launch_pmcv_hd(st, Phi, n, m, mp, k, w, v, hd, ldh);
}

// one launch above 64 KB of dynamic LDS.  Per launch, not once per process: the attribute belongs to the current device's copy of the kernel
template <class F, class A>
static int nmcov_launch_lds(hipStream_t st, F kernel, dim3 grid, size_t lds, const A &a) {
    if (lds > 65536 && hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -1;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The slab loop of the pair and gamma launchers: the pattern's pair-component table passes through slabs of whole pairs
// (predict_noisy_missing_cov_slabs), each written through launch_pnmc_triples and then read by launch(a) with a.q0, cnt, ppc and first
// set.  *slab_kept: slab holds the pattern's whole table (one slab) and is not written again, whichever kernel filled it (the records
// do not depend on Psi); the caller clears it where the pattern's tables change.
template <class A, class L>
static int nmcov_slabs(hipStream_t st, const PmcvPat &pt, unsigned obs, int m, const double *raw, const double *bas, double *slab,
                       bool *slab_kept, int nchunk, A &a, L launch) {
    const int d = pt.d, nslab = predict_noisy_missing_cov_slabs(m, d, pt.no);
    const long npair = (long)m * (m + 1) / 2, sp = predict_noisy_missing_cov_slab_pairs(m, d, pt.no);
    for (int s = 0; s < nslab; ++s) {
        const long q0 = s * sp, cnt = (npair - q0 < sp) ? npair - q0 : sp;
        if (cnt <= 0) break;
        if (!(nslab == 1 && *slab_kept) && launch_pnmc_triples(st, d, obs, q0, cnt, m, raw, bas, slab)) return -1;
        a.q0 = q0; a.cnt = (int)cnt; a.ppc = (int)((cnt + nchunk - 1) / nchunk); a.first = s == 0;
        if (launch(a)) return -1;
    }
    *slab_kept = nslab == 1;
    return 0;
}

// the moments of a tile: the pair kernel over the slabs into part [chunks][3k][ldp], then k_pmd_finish -> out
template <class K>
static int nmcov_launch_pairs(hipStream_t st, const double *Xc, const double *Psi, long ldx, int n, const double *Pio, long ldr, int m, int d,
                              int k, unsigned obs, const double *raw, const double *bas, const double *coef, double *slab, bool *slab_kept,
                              int nchunk, double *part, long ldp, const double *hd, long ldh, const double *bvec, double *out) {
    if (n <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || k < 1 || k > 8 || m < 1 || ((m + 15) / 16) * 16 > 256 || nchunk != predict_missing_cov_chunks(m) ||
        ldr < n || ldp < n || ldx < n || !Psi)
        return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.nu < 1 || pt.no < 1) return -1;
    PredNmcovArgs a{};
    nmcov_fill(a, pt, Xc, Psi, ldx, n, m, slab);
    a.k = k; a.Pio = const_cast<double *>(Pio); a.ldr = ldr; a.coef = coef; a.part = part; a.ldp = ldp;
    const size_t lds = predict_noisy_missing_cov_lds(m, d, pt.no, k);
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)nchunk);
    auto launch = [&](const PredNmcovArgs &s) {
#define NMCOV_PAIRS(NN)                                                                          \
    return k == 1 ? nmcov_launch_lds(st, K::template pairs<NN, 1>(), grid, lds, s)               \
                  : nmcov_launch_lds(st, K::template pairs<NN, 8>(), grid, lds, s)
        PNMC_CASES(NMCOV_PAIRS)
#undef NMCOV_PAIRS
    };
    if (nmcov_slabs(st, pt, obs, m, raw, bas, slab, slab_kept, nchunk, a, launch)) return -1;
    return launch_pmd_finish(st, part, nchunk, ldp, hd, ldh, n, k, bvec, out);
}

// the pair sums of a tile under every column of W: part [chunks][ncol][ldp], from Pio of the rows launcher
template <class K>
static int nmcov_launch_gamma(hipStream_t st, const double *Xc, const double *Psi, long ldx, int n, const double *Pio, long ldr, int m, int d,
                              unsigned obs, const double *raw, const double *bas, double *slab, bool *slab_kept, const double *W, int ldw,
                              int ncol, int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || m < 1 || ((m + 15) / 16) * 16 > 256 || nchunk != predict_missing_cov_chunks(m) || ldw < 16 || ldw % 16 ||
        ncol > ldw || ldr < n || ldp < n || ldx < n || !Psi)
        return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.nu < 1 || pt.no < 1) return -1;
    PredNmcovGammaArgs a{};
    nmcov_fill(a, pt, Xc, Psi, ldx, n, m, slab);
    a.Pio = Pio; a.ldr = ldr; a.W = W; a.ldw = ldw; a.ncol = ncol; a.nbw = (ncol + 15) / 16;   // <= ldw / 16
    a.part = part; a.ldp = ldp;
    const size_t lds = predict_noisy_missing_cov_gamma_lds(m, d, pt.no);
    const unsigned gx = (unsigned)((n + 63) / 64);
    auto launch = [&](const PredNmcovGammaArgs &s) {   // (z: the passes, by the instantiation's blocks of a pass)
#define NMCOV_GAMMA(NN) \
    return nmcov_launch_lds(st, K::template gamma<NN>(), dim3(gx, (unsigned)nchunk, (unsigned)((s.nbw + K::nb(NN) - 1) / K::nb(NN))), lds, s)
        PNMC_CASES(NMCOV_GAMMA)
#undef NMCOV_GAMMA
    };
    return nmcov_slabs(st, pt, obs, m, raw, bas, slab, slab_kept, nchunk, a, launch);
}
