// Rows with a full input-noise covariance AND missing inputs through the streaming predictor, covariance kinds
// (gpz_predictor_run_psi_cube_missing_dev / _draws_psi_cube_missing_dev, gpz_predictor.hip): predictNoisyMissing of GC and VC
// (predictCov.m:233-337) for one tile of ONE group of rows that share a NaN pattern and carry a d x d matrix Psi each, the cube of
// fixPsi.m:36.  k_predict_noisy_missing_cov.hip is the frame, line for line: its records (predict_noisy_missing_cov_rec doubles, which
// do not depend on Psi), its slabs and chunk rule, its Pio block, the order of every sum, and its launchers' checks.  What differs is
// Psi_oo, the observed x observed block of the row's matrix, in
//     v' (S + G Psi_oo G')^-1 v = |A2 x + b2|^2 + w' (M + Psi_oo)^-1 w,          |S + G Psi_oo G'| = |S| |R_B|^2 |M + Psi_oo|:
// nothing in that identity needs a diagonal Psi_oo (the whitening by S, the QR of G and the determinant product hold for any symmetric
// positive semidefinite one), so the density is pnmc_density with PsiTri<NO> for PsiDiag<NO>: the packed Cholesky of M + Psi_oo over
// the whole no (no + 1) / 2 triangle (ncov_factor_tri through the policy), everything else unchanged.  With zeros off the diagonal the
// sums are M + 0.0 and every result has the bits of k_predict_noisy_missing_cov.hip's.
//
// The tile's Psi slot is Psio [no (no + 1) / 2][ldx]: column LT(ro, co) holds element (o[ro], o[co]), ro >= co, of every row's matrix
// with o the observed dimensions in ascending order, so o[ro] >= o[co], the element lies in the lower triangle of the caller's matrix,
// and a lane's loads are coalesced as they are for Xc.  Psi in a missing row or column is never read.
//
//   k_pcm_check_psi       word 3 of the device entries' record is set when an element of the lower triangle of an observed x observed
//                         block is NaN or infinite, itself or after its division, or a diagonal element is negative
//   k_pcm_stage_psi<T>    the caller's cube (f64 or f32; element (r, c) of row i at Psi[r sr + c sc + i sn]) -> Psio, a plain f64
//                         division by div[LT(o[ro], o[co])] (fixPsi.m:36)
//   k_pcm_ex<NO>          k_pnmc_ex's frame: lane = row, x_o and the triangle in registers, Ex over the m records in index order (the
//                         record stage of PCM_STD doubles of this kernel and the next is dynamic LDS, as all LDS of the unit is)
//   k_pcm_phi<NO>         k_pnmc_phi's frame: PHI(i) = sum_j Pio_j z(rec_ij) in index order -> Phi [nrow][mp] as launch_tgemm takes it
//   k_predict_psi_cube_missing_pairs<NO, KM>   k_predict_noisy_missing_cov_pairs' frame: 64 rows per workgroup, lane = row in each of
//                         four waves, the Pio block [m][64] in dynamic LDS (predict_noisy_missing_cov_lds: Psi lives in registers),
//                         records staged through LDS PCM_SB at a time and read as broadcasts, the m components in index order,
//                         partials in wave order, slabs in slab order, gridDim.y = predict_missing_cov_chunks(m).  No atomics.
// The tables (k_pnmc_basis, k_pnmc_phirec, k_pnmc_triples), k_pmcv_hd and k_pmd_finish are the twins': reached through their launchers.
// Where it could fault, and what holds it: rows past n are clamped to n - 1 for loads (X, Psi and Pio) and never stored; a wave
// without a pair reads the chunk's first pair (a valid record) and adds nothing; record offsets are formed in 64 bits; a stage holds
// nl rl <= PCM_SB rl doubles, its size; dynamic LDS above 64 KB is opted in per launch; the launchers refuse shapes outside
// predict_missing_cov_fits, no < 1, nu < 1, a wrong chunk count, leading dimensions below n and a null Psi.  A matrix that passes the
// scan but is not positive semidefinite gives its own row NaN (a non-positive pivot) and touches no other row.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_pnmc_density.h"   // pnmc_density, PNMC_CASES; PsiTri; PMCV_MAXD, PmcvPat, pmcv_pat; LT

#define PCM_STD 2048   // doubles per LDS stage of the Ex and PHI kernels (k_predict_noisy_missing_cov.hip's, whole records)
#define PCM_SB 4       // records per LDS stage of a wave of the pair kernel (that unit's: predict_noisy_missing_cov_lds counts them)

// ---- byte movers of the device entries -------------------------------------------------------------------------------------------------
// npo = no (no + 1) / 2 elements per row, element q = LT(ro, co) the one at (o[ro], o[co]).  div: the divisors sdX[r] sdX[c] of the
// whole d x d triangle in LT order on the device (nullptr: none)
__global__ __launch_bounds__(256) void k_pcm_check_psi(const void *__restrict__ Psi, int f32, long ns, PmcvPat pt, long sr, long sc,
                                                       long sn, const double *__restrict__ div, unsigned *__restrict__ rec) {
    const int npo = pt.no * (pt.no + 1) / 2;
    const long ne = ns * npo, step = (long)gridDim.x * 256;
    int bad = 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < ne; e += step) {
        const int q = (int)(e / ns);          // rows fastest: a contiguous d x d x n cube is read coalesced
        const long i = e - (long)q * ns;
        int ro = 0;
        while ((ro + 1) * (ro + 2) / 2 <= q) ++ro;
        const int co = q - ro * (ro + 1) / 2, r = pt.o[ro], c = pt.o[co];   // r >= c: the lower triangle
        const long at = r * sr + c * sc + i * sn;
        const double v = f32 ? (double)((const float *)Psi)[at] : ((const double *)Psi)[at];
        const double w = div ? v / div[LT(r, c)] : v;
        bad |= !(fabs(v) <= 1.7976931348623157e308) || !(fabs(w) <= 1.7976931348623157e308) || (r == c && !(v >= 0.0));
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(rec + 3, 1u);
}

template <typename T>
__global__ __launch_bounds__(256) void k_pcm_stage_psi(const T *__restrict__ Psi, long sr, long sc, long sn, long r0, int nt, PmcvPat pt,
                                                       const double *__restrict__ div, double *__restrict__ Psio, long ldx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const T *row = Psi + (r0 + i) * sn;
    for (int ro = 0; ro < pt.no; ++ro)
        for (int co = 0; co <= ro; ++co) {
            const int r = pt.o[ro], c = pt.o[co];
            double v = (double)row[r * sr + c * sc];
            if (div) v = v / div[LT(r, c)];                                  // Psi ./ (sdX' sdX)        fixPsi.m:36
            Psio[(size_t)LT(ro, co) * ldx + i] = v;
        }
}

int launch_pcm_check_psi(hipStream_t st, const void *Psi, int f32, long ns, int d, unsigned obs, long sr, long sc, long sn,
                         const double *div, unsigned *rec) {
    if (ns <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD) return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.no < 1) return 0;                  // nothing observed: nothing of Psi is read
    long nb = (ns * (pt.no * (pt.no + 1) / 2) + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_pcm_check_psi, dim3((unsigned)nb), dim3(256), 0, st, Psi, f32, ns, pt, sr, sc, sn, div, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pcm_stage_psi(hipStream_t st, const void *Psi, int f32, long sr, long sc, long sn, long r0, int nt, int d, unsigned obs,
                         const double *div, double *Psio, long ldx) {
    if (nt <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || ldx < nt) return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.no < 1) return 0;
    const dim3 grid((unsigned)((nt + 255) / 256));
    if (f32)
        hipLaunchKernelGGL(k_pcm_stage_psi<float>, grid, dim3(256), 0, st, (const float *)Psi, sr, sc, sn, r0, nt, pt, div, Psio, ldx);
    else
        hipLaunchKernelGGL(k_pcm_stage_psi<double>, grid, dim3(256), 0, st, (const double *)Psi, sr, sc, sn, r0, nt, pt, div, Psio, ldx);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the tile kernels ------------------------------------------------------------------------------------------------------------------
struct PcmArgs {
    const double *Xc, *Psio; long ldx; int n;   // the tile's rows [d][ldx] and the observed triangles [no (no + 1) / 2][ldx]
    int oidx[PMCV_MAXD];                        // the observed dimensions in ascending order
    int nu, rl;                                 // the missing dimensions; doubles per record
    int m, k;
    double *Pio; long ldr;                      // [m][ldr]
    const double *rec;                          // Ex: m records; PHI: m * m; pairs: the slab
    double *Phi; int nrow, mp, ipc;             // PHI: [nrow][mp], basis functions per gridDim.y chunk
    const double *coef; long q0; int cnt, ppc;  // pairs: the slab's first pair, its pairs, pairs per chunk
    double *part; long ldp; int first;          // pairs: [chunks][3k][ldp]; first: the slab's sums are stored, not added
};

// the row's observed inputs and its triangle, row ic (clamped by the caller)
template <int NO>
__device__ __forceinline__ void pcm_load(const PcmArgs &a, long ic, double (&x)[NO], double (&ps)[NO * (NO + 1) / 2]) {
#pragma unroll
    for (int c = 0; c < NO; ++c) x[c] = a.Xc[(size_t)a.oidx[c] * a.ldx + ic];
    ncov_psi_load(a.Psio + ic, a.ldx, ps);
}

template <int NO>
__global__ __launch_bounds__(256) void k_pcm_ex(PcmArgs a) {
    extern __shared__ double sT[];                       // PCM_STD doubles, dynamic as all LDS of this unit
    const int tid = threadIdx.x, rl = a.rl, nu = a.nu, per = PCM_STD / rl;   // whole records per stage
    const long i = (long)blockIdx.x * 256 + tid;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    double x[NO], ps[NO * (NO + 1) / 2];
    pcm_load<NO>(a, ic, x, ps);
    double s = 0.0;
    for (int lb = 0; lb < a.m; lb += per) {
        const int nl = min(per, a.m - lb);
        __syncthreads();
        for (int t = tid; t < nl * rl; t += 256) sT[t] = a.rec[(size_t)lb * rl + t];
        __syncthreads();
#pragma unroll 1
        for (int e = 0; e < nl; ++e) {
            const double z = pnmc_density<PsiTri<NO>>(sT + e * rl, nu, x, ps);
            s += z;                                                        // index order                          :281
            if (act) a.Pio[(size_t)(lb + e) * a.ldr + i] = z;
        }
    }
    if (!act) return;
    for (int l = 0; l < a.m; ++l) a.Pio[(size_t)l * a.ldr + i] /= s;
}

template <int NO>
__global__ __launch_bounds__(256) void k_pcm_phi(PcmArgs a) {
    extern __shared__ double sT[];                       // PCM_STD doubles, dynamic as all LDS of this unit
    const int tid = threadIdx.x, rl = a.rl, nu = a.nu, per = PCM_STD / rl;
    const long i = (long)blockIdx.x * 256 + tid;
    const bool act = i < a.n, st = i < a.nrow;   // rows n .. nrow - 1 are written as zeros
    const long ic = act ? i : a.n - 1;
    double x[NO], ps[NO * (NO + 1) / 2];
    pcm_load<NO>(a, ic, x, ps);
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
            for (int e = 0; e < nl; ++e)
                z = fma(a.Pio[(size_t)(lb + e) * a.ldr + ic], pnmc_density<PsiTri<NO>>(sT + e * rl, nu, x, ps), z);
        }
        if (st) row[b] = act ? z : 0.0;
    }
    if (blockIdx.y == 0 && st)
        for (int j = a.m; j < a.mp; ++j) row[j] = 0.0;
}

template <int NO, int KM>
__global__ __launch_bounds__(256) void k_predict_psi_cube_missing_pairs(PcmArgs a) {
    extern __shared__ double sm[];
    double *sPio = sm;                                   // [m][64]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, m = a.m, k = a.k, rl = a.rl, nu = a.nu;
    double *sRec = sm + (size_t)m * 64 + (size_t)w * (PCM_SB * rl);   // this wave's stage
    const long row0 = (long)blockIdx.x * 64, i = row0 + lane;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    for (int e = tid; e < m * 64; e += 256) {
        const long r = min(row0 + (e & 63), (long)a.n - 1);
        sPio[e] = a.Pio[(size_t)(e >> 6) * a.ldr + r];
    }
    double x[NO], ps[NO * (NO + 1) / 2];
    pcm_load<NO>(a, ic, x, ps);
    double acc[3 * KM];
#pragma unroll
    for (int e = 0; e < 3 * KM; ++e) acc[e] = 0.0;
    const int ch = blockIdx.y, p0 = ch * a.ppc, p1 = min(a.cnt, p0 + a.ppc);
    for (int pb = p0; pb < p1; pb += 4) {                // the four waves take pairs pb .. pb + 3
        const int p = pb + w;
        const bool on = p < p1;
        const double *src = a.rec + (size_t)(on ? p : p0) * m * rl;
        double z = 0.0;
        for (int lb = 0; lb < m; lb += PCM_SB) {
            const int nl = min(PCM_SB, m - lb);
            __syncthreads();                             // the stage before is read (and, the first time, sPio is written)
            if (on)
                for (int t = lane; t < nl * rl; t += 64) sRec[t] = src[(size_t)lb * rl + t];
            __syncthreads();
            if (on) {
#pragma unroll 1
                for (int e = 0; e < nl; ++e)
                    z = fma(sPio[(lb + e) * 64 + lane], pnmc_density<PsiTri<NO>>(sRec + e * rl, nu, x, ps), z);
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

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static PcmArgs pcm_args(const PmcvPat &pt, const double *Xc, const double *Psio, long ldx, int n, int m, int k, double *Pio, long ldr,
                        const double *rec) {
    PcmArgs a{};
    a.Xc = Xc; a.Psio = Psio; a.ldx = ldx; a.n = n; a.m = m; a.k = k; a.Pio = Pio; a.ldr = ldr; a.rec = rec;
    a.nu = pt.nu; a.rl = predict_noisy_missing_cov_rec(pt.d, pt.no);
    for (int c = 0; c < pt.no; ++c) a.oidx[c] = pt.o[c];
    return a;
}

// launch_pnmc_rows with the observed triangles: Pio [m][ldr], Phi [nrow][mp] and hd [2k][ldh] from the twin's Ex and PHI records
int launch_pcm_rows(hipStream_t st, const double *Xc, const double *Psio, long ldx, int n, int nrow, int m, int mp, int d, int k,
                    unsigned obs, const double *exrec, const double *phirec, const double *w, const double *v, double *Pio, long ldr,
                    double *Phi, double *hd, long ldh) {
    if (n <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || m < 1 || nrow < n || mp < m || ldr < n || ldx < n || !Psio) return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.no < 1 || pt.nu < 1 || predict_noisy_missing_cov_rec(d, pt.no) > PCM_STD) return -1;
    PcmArgs a = pcm_args(pt, Xc, Psio, ldx, n, m, k, Pio, ldr, exrec);
    PcmArgs b = a;
    b.rec = phirec; b.Phi = Phi; b.nrow = nrow; b.mp = mp; b.ipc = 8;
    const dim3 ge((unsigned)((n + 255) / 256)), gp((unsigned)((nrow + 255) / 256), (unsigned)((m + b.ipc - 1) / b.ipc));
#define PCM_ROWS(NN)                                                                       \
    do {                                                                                   \
        hipLaunchKernelGGL(k_pcm_ex<NN>, ge, dim3(256), PCM_STD * sizeof(double), st, a);  \
        hipLaunchKernelGGL(k_pcm_phi<NN>, gp, dim3(256), PCM_STD * sizeof(double), st, b); \
    } while (0)
    PNMC_CASES(PCM_ROWS)
#undef PCM_ROWS
    if (hipGetLastError() != hipSuccess) return -1;
    return launch_pmcv_hd(st, Phi, n, m, mp, k, w, v, hd, ldh);
}

// per launch, not once per process: the attribute belongs to the current device's copy of the kernel
template <int NO, int KM>
static int pcm_launch_pairs(hipStream_t st, dim3 grid, size_t lds, const PcmArgs &a) {
    if (lds > 65536 && hipFuncSetAttribute((const void *)k_predict_psi_cube_missing_pairs<NO, KM>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -1;
    hipLaunchKernelGGL((k_predict_psi_cube_missing_pairs<NO, KM>), grid, dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// launch_predict_noisy_missing_cov_pairs with the observed triangles: the twin's slabs (written through launch_pnmc_triples, kept under
// the same flag: the records do not depend on Psi), chunk rule, LDS figure and finish
int launch_predict_psi_cube_missing_pairs(hipStream_t st, const double *Xc, const double *Psio, long ldx, int n, const double *Pio,
                                          long ldr, int m, int d, int k, unsigned obs, const double *raw, const double *bas,
                                          const double *coef, double *slab, bool *slab_kept, int nchunk, double *part, long ldp,
                                          const double *hd, long ldh, const double *bvec, double *out) {
    if (n <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || k < 1 || k > 8 || m < 1 || ((m + 15) / 16) * 16 > 256 || nchunk != predict_missing_cov_chunks(m) ||
        ldr < n || ldp < n || ldx < n || !Psio)
        return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.nu < 1 || pt.no < 1) return -1;
    const int nslab = predict_noisy_missing_cov_slabs(m, d, pt.no);
    const long npair = (long)m * (m + 1) / 2, sp = predict_noisy_missing_cov_slab_pairs(m, d, pt.no);
    PcmArgs a = pcm_args(pt, Xc, Psio, ldx, n, m, k, const_cast<double *>(Pio), ldr, slab);
    a.coef = coef; a.part = part; a.ldp = ldp;
    const size_t lds = predict_noisy_missing_cov_lds(m, d, pt.no, k);
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)nchunk);
    for (int s = 0; s < nslab; ++s) {
        const long q0 = s * sp, cnt = (npair - q0 < sp) ? npair - q0 : sp;
        if (cnt <= 0) break;
        // the whole table is one slab: it stays until the pattern's tables change, whichever kernel filled it
        if (!(nslab == 1 && *slab_kept) && launch_pnmc_triples(st, d, obs, q0, cnt, m, raw, bas, slab)) return -1;
        a.q0 = q0; a.cnt = (int)cnt; a.ppc = (int)((cnt + nchunk - 1) / nchunk); a.first = s == 0;
        int rc;
#define PCM_PAIRS(NN) rc = k == 1 ? pcm_launch_pairs<NN, 1>(st, grid, lds, a) : pcm_launch_pairs<NN, 8>(st, grid, lds, a)
        PNMC_CASES(PCM_PAIRS)
#undef PCM_PAIRS
        if (rc) return -1;
    }
    *slab_kept = nslab == 1;
    return launch_pmd_finish(st, part, nchunk, ldp, hd, ldh, n, k, bvec, out);
}
