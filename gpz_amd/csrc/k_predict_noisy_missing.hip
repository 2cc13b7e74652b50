// Rows with both input noise and missing inputs through the streaming predictor (gpz_predictor_run_noisy_missing_dev /
// _draws_noisy_missing_dev, gpz_predictor.hip): predictNoisyMissing of the diagonal kinds (predictDiag.m:211-297) for one tile of ONE
// group of rows that share a NaN pattern, each row with a variance psi per input dimension (Psic, in the layout of Xc, as
// k_pred_stage_psi left it).  obs is the bit mask of the observed dimensions, uniform over every launch.  Psi touches the observed
// dimensions only: NijS, the priors and U(q, l) = Nu_q(l) are k_predict_missing.hip's tables of the pattern, reused as built; No widens by
// psi, and the pair density over the observed dimensions becomes N(x_o; c_q,o, C_q,o + psi_o), k_predict_noisy_small's per-row form.
// Every loop over the dimensions here runs over the set bits of obs: no NaN of X and no value of Psi from a missing dimension enters
// arithmetic, whatever it holds.
//
// Per handle, once (the model's alone: the pattern enters through the loops, not through the table):
//   k_pnm_records  the second pair-record table [lnZ_q | c_q (d) | C_q (d) | per output f w_i w_j, f v_i v_j, f iS(i, j)] for
//                  q = i (i + 1) / 2 + j, j <= i, f = 2 off the diagonal and 1 on it (:277-284), iS read at i >= j only as the reference
//                  does.  lnZ_q = lnz_i + lnz_j - 1/2 sum (p_i - p_j)^2 / (sigma_i + sigma_j) - 1/2 sum ln(sigma_i + sigma_j) (:275)
//                  comes WITHOUT the -1/2 sum_o ln C_q of k_pmd_pairs: with psi the determinant depends on the row.  c_q and C_q (not
//                  1 / C_q) are stored for every dimension.  Records past the last pair are zero with C_q = 1; predict_missing_rec(d, k)
//                  doubles each, whole groups of 64.
// Per tile, on Xc and Psic [d][ldx]:
//   k_pnm_no       No(r, j) = exp(-1/2 sum_o [(x - p_j)^2 / (psi + sigma_jo) + ln(psi + sigma_jo)]), Pio = No prior / sum_j (No prior);
//                  one wave per row, as k_pmd_no.  With u = 1 + psi gamma_j^2: (psi + sigma) = u / gamma^2, so the exponent is
//                  lno_j - 1/2 (sum_o (x - p)^2 gamma^2 / u + sum_o ln u) with k_pmd_basis' lno_j: at psi = 0 the bits of k_pmd_no.     :227-238
//   launch_tgemm, k_pmd_phi                       as for a group without noise (T = Pio NijS, PHI = No o T, mu, ElnS - b)             :244-250
//   k_predict_noisy_missing_pairs<KM>   the hot one (:257-285).  The product is k_predict_missing_pairs' in everything that sets the
//                  accumulator layout: 32 rows per 4-wave workgroup, the Pio block in LDS with row stride nk + 2, wave w takes the
//                  16-pair block 4 g + w of group g, U is the A operand fetched four K steps ahead, lane l owns rows l & 15 and
//                  16 + (l & 15) and in accumulator register r pair (l >> 4) + 4 r of the block; the group's 64 records are staged
//                  between the two barriers while the K loop runs and read as broadcasts.  Epilogue in the accumulators, per observed
//                  dimension r = (C_qc + psi_rc)^-1/2 (pn_rsqrt), z = acc exp(lnZ_q - 1/2 sum_o (Delta r)^2) prod_o r, then three FMAs
//                  per output.  The sums are added over the four lane groups and over the waves in wave order: no atomics, one fixed
//                  order that depends on the model only.  gridDim.y = predict_missing_chunks(m) chunks into part [C][3k][ldp].
//                  LDS: (32 (nk + 2) + 64 (1 + 2 d + 3 k) + 64 d) doubles - the block's rows of X and of Psi - at least 4 * 32 * 3 KM for
//                  the last reduction.
//   launch_pmd_finish                             the chunks in chunk order -> out [4k][nt] = mu | nu | beta | gamma                   :289-295
//   k_pnm_check_psi   word 3 of the device entries' record is set when Psi is NaN, negative or infinite in an OBSERVED dimension.
// A row's results depend on its own values and the model only: the same bits for any tile size, position in the block and row order.
#include "gpz_dev.h"
#include "gpz_kernels.h"

// q = i (i + 1) / 2 + j, j <= i
__device__ __forceinline__ void pnm_pair_of(long q, int *pi, int *pj) {
    long i = (long)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= q) ++i;
    while (i * (i + 1) / 2 > q) --i;
    *pi = (int)i;
    *pj = (int)(q - i * (i + 1) / 2);
}

// 1 / sqrt(p): v_rsq_f64 seed and two Newton steps (k_predict_noisy.hip's pn_rsqrt)
__device__ __forceinline__ double pn_rsqrt(double p) {
    double y = __builtin_amdgcn_rsq(p);
    const double h = 0.5 * p;
    double e = fma(-h * y, y, 0.5);
    y = fma(y, e, y);
    e = fma(-h * y, y, 0.5);
    y = fma(y, e, y);
    return y;
}

// dc: the columns of Psi that differ (1 for a broadcast column).  smin: the smallest sd2 (1 without a normalisation)
__global__ __launch_bounds__(256) void k_pnm_check_psi(const void *__restrict__ Psi, int f32, long ns, int dc, long rs, long cs,
                                                       unsigned obs, double smin, unsigned *__restrict__ rec) {
    const long ne = ns * dc, step = (long)gridDim.x * 256;
    int bad = 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < ne; e += step) {
        const long r = e / dc;
        const int c = (int)(e - r * dc);
        if (dc > 1 && !((obs >> c) & 1u)) continue;                    // a missing dimension: not read
        const long at = r * rs + c * cs;
        const double v = f32 ? (double)((const float *)Psi)[at] : ((const double *)Psi)[at];
        bad |= !(v >= 0.0) || !(v / smin <= 1.7976931348623157e308);   // NaN, negative, infinite (after the division by sd2 too)
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(rec + 3, 1u);
}

// one thread per pair of the padded table (npad = whole groups of 64); G2: gamma^2 = 1 / sigma, m x de row-major
__global__ __launch_bounds__(256) void k_pnm_records(long npair, long npad, int m, int d, int de, int k, const double *__restrict__ P,
                                                     const double *__restrict__ G2, const double *__restrict__ w,
                                                     const double *__restrict__ v, const double *__restrict__ iS, double *__restrict__ rec,
                                                     int nrec) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= npad) return;
    double *r = rec + (size_t)q * nrec;
    if (q >= npair) {
        for (int e = 0; e < nrec; ++e) r[e] = (e > d && e <= 2 * d) ? 1.0 : 0.0;
        return;
    }
    int i, j;
    pnm_pair_of(q, &i, &j);
    double lz = 0.0, qd = 0.0, ls = 0.0;
    for (int c = 0; c < d; ++c) {
        const double isi = G2[(size_t)i * de + c], isj = G2[(size_t)j * de + c];
        const double C = 1.0 / (isi + isj);                                                      // :260
        const double cv = (P[(size_t)i * de + c] * isi + P[(size_t)j * de + c] * isj) * C;       // :261
        lz += log(isi) + log(isj);
        const double s = 1.0 / isi + 1.0 / isj, dl = P[(size_t)i * de + c] - P[(size_t)j * de + c];
        qd += dl * dl / s;
        ls += log(s);
        r[1 + c] = cv;
        r[1 + d + c] = C;
    }
    r[0] = -0.5 * lz - 0.5 * qd - 0.5 * ls;                                                      // :275, the row-free part
    const double f = i == j ? 1.0 : 2.0;
    double *cf = r + 1 + 2 * d;
    for (int o = 0; o < k; ++o) {
        cf[3 * o] = f * (w[i + (size_t)m * o] * w[j + (size_t)m * o]);
        cf[3 * o + 1] = v ? f * (v[i + (size_t)m * o] * v[j + (size_t)m * o]) : 0.0;
        cf[3 * o + 2] = f * iS[i + (size_t)m * j + (size_t)m * m * o];
    }
}

// rows [0, nrow) of No and Pio (ld = mp), rows >= n and columns >= m zero; one wave per row, lanes along the basis functions
__global__ __launch_bounds__(256) void k_pnm_no(const double *__restrict__ Xc, const double *__restrict__ Psic, long ldx, int n, int nrow,
                                                int m, int mp, int de, unsigned obs, const double *__restrict__ P,
                                                const double *__restrict__ G2, const double *__restrict__ bt, double *__restrict__ No,
                                                double *__restrict__ Pio) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nrow) return;
    double *no = No + (size_t)i * mp, *pio = Pio + (size_t)i * mp;
    if (i >= n) {
        for (int j = lane; j < mp; j += 64) { no[j] = 0.0; pio[j] = 0.0; }
        return;
    }
    double s = 0.0;
    for (int j = lane; j < m; j += 64) {
        double q = 0.0, lu = 0.0;
        for (unsigned mk = obs; mk; mk &= mk - 1) {
            const int c = __builtin_ctz(mk);
            const double g = G2[(size_t)j * de + c];
            const double dl = Xc[(size_t)c * ldx + i] - P[(size_t)j * de + c];
            const double u = fma(Psic[(size_t)c * ldx + i], g, 1.0);   // (psi + sigma) / sigma
            q = fma(dl * dl, g / u, q);                                // :231
            lu += log(u);
        }
        const double v = exp(bt[j] - 0.5 * (q + lu));
        no[j] = v;
        s = fma(v, bt[mp + j], s);
    }
    s = wave_sum(s);
    for (int j = lane; j < mp; j += 64) {
        if (j < m) pio[j] = no[j] * bt[mp + j] / s;                    // :238
        else { no[j] = 0.0; pio[j] = 0.0; }
    }
}

struct PredNoisyMissArgs {
    const double *Xc, *Psic; long ldx; int n;   // the tile's rows and their variances, [d][ldx]
    const double *Pio; int ldpio;               // [rows][ldpio]
    int nk;                                     // ceil16(m): K of the product
    const double *U;                            // in fragment order (k_pmd_u)
    const double *rec; int nrec;                // pair records (k_pnm_records), whole groups of 64
    int d, k;
    unsigned obs;
    int ngrp, gpc;                              // groups of 64 pairs in all, and per chunk
    double *part; long ldp;                     // [chunks][3 k][ldp]: gamma | VlnS | nu
};

template <int KM>
__global__ __launch_bounds__(256, 2) void k_predict_noisy_missing_pairs(PredNoisyMissArgs a) {
    extern __shared__ double smem[];
    const int nk = a.nk, lda = nk + 2, nrec = a.nrec, d = a.d, k = a.k;
    double *sP = smem;                   // [32][lda]: Pio of the block (2 mod 4: the 16 rows of an operand read start 4 banks apart)
    double *sR = sP + 32 * lda;          // [64][nrec]: the records of the group
    double *sX = sR + 64 * nrec;         // [32][d]: the block's rows, zero where missing
    double *sS = sX + 32 * d;            // [32][d]: their variances, zero where missing
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long i0 = (long)blockIdx.x * 32;
    const int ch = blockIdx.y;
    const unsigned obs = a.obs;
    for (int e = tid; e < 32 * nk; e += 256) {
        const int r = e / nk, c = e - r * nk;
        sP[r * lda + c] = (i0 + r < a.n) ? a.Pio[(size_t)(i0 + r) * a.ldpio + c] : 0.0;
    }
    for (int e = tid; e < 32 * d; e += 256) {
        const int r = e / d, c = e - r * d;
        const bool in = ((obs >> c) & 1u) && i0 + r < a.n;
        sX[e] = in ? a.Xc[(size_t)c * a.ldx + i0 + r] : 0.0;
        sS[e] = in ? a.Psic[(size_t)c * a.ldx + i0 + r] : 0.0;
    }
    double ga[2][KM], vl[2][KM], nu[2][KM];
#pragma unroll
    for (int o = 0; o < KM; ++o) { ga[0][o] = ga[1][o] = 0.0; vl[0][o] = vl[1][o] = 0.0; nu[0][o] = nu[1][o] = 0.0; }
    const int nks = nk >> 2;             // K steps of 4 (a multiple of 4)
    const double *pa0 = sP + (lane & 15) * lda + (lane >> 4), *pa1 = pa0 + 16 * lda;
    const double *x0 = sX + (lane & 15) * d, *x1 = x0 + 16 * d;
    const double *s0 = sS + (lane & 15) * d, *s1 = s0 + 16 * d;
    const double *rb = sR + (16 * wv + (lane >> 4)) * nrec;   // the records of pairs (lane >> 4) + 4 r of this wave's block, r = 0 .. 3
    const int g0 = ch * a.gpc, g1 = min(a.ngrp, g0 + a.gpc);
    for (int g = g0; g < g1; ++g) {
        __syncthreads();   // the group before is read (first trip: sP, sX and sS are written)
        {
            const double *src = a.rec + (size_t)g * 64 * nrec;
            for (int t = tid; t < 64 * nrec; t += 256) sR[t] = src[t];
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
        __syncthreads();   // the records are in LDS
        // ---- epilogue: acc0[r], acc1[r] = sum_l Pio(row, l) Nu_q(l) for rows l & 15, 16 + (l & 15) and pair q = (l >> 4) + 4 r     :271-272
        double qa[4] = {0.0, 0.0, 0.0, 0.0}, qb[4] = {0.0, 0.0, 0.0, 0.0};
        double ra[4] = {1.0, 1.0, 1.0, 1.0}, rb4[4] = {1.0, 1.0, 1.0, 1.0};
        for (unsigned mk = obs; mk; mk &= mk - 1) {   // the observed dimensions only (uniform: scalar control flow)
            const int c = __builtin_ctz(mk);
            const double xa = x0[c], xb = x1[c], pa = s0[c], pb = s1[c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double *t = rb + 4 * r * nrec;
                const double cc = t[1 + c], C = t[1 + d + c];
                const double ia = pn_rsqrt(C + pa), ib = pn_rsqrt(C + pb);   // (Cij + Psi)^-1/2            :264-265
                const double da = (xa - cc) * ia, db = (xb - cc) * ib;
                qa[r] = fma(da, da, qa[r]);
                qb[r] = fma(db, db, qb[r]);
                ra[r] *= ia;
                rb4[r] *= ib;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double *t = rb + 4 * r * nrec;
            const double lz = t[0];
            const double za = acc0[r] * (exp(lz - 0.5 * qa[r]) * ra[r]), zb = acc1[r] * (exp(lz - 0.5 * qb[r]) * rb4[r]);   // :275
            const double *cf = t + 1 + 2 * d;
#pragma unroll
            for (int o = 0; o < KM; ++o) {
                if (o >= k) break;
                const double c0 = cf[3 * o], c1 = cf[3 * o + 1], c2 = cf[3 * o + 2];
                ga[0][o] = fma(za, c0, ga[0][o]); ga[1][o] = fma(zb, c0, ga[1][o]);   // :277-284
                vl[0][o] = fma(za, c1, vl[0][o]); vl[1][o] = fma(zb, c1, vl[1][o]);
                nu[0][o] = fma(za, c2, nu[0][o]); nu[1][o] = fma(zb, c2, nu[1][o]);
            }
        }
    }
    // ---- the four lane groups of a wave, then the waves in their order
    __syncthreads();   // every wave is done with sP, sR, sX and sS
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
        const int at = row * 3 * KM + q * KM + o;
        const double s = ((sRed[at] + sRed[32 * 3 * KM + at]) + sRed[2 * 32 * 3 * KM + at]) + sRed[3 * 32 * 3 * KM + at];
        if (i0 + row < a.n) a.part[((size_t)ch * 3 * k + e) * a.ldp + i0 + row] = s;
    }
}

// dynamic LDS of k_predict_noisy_missing_pairs, bytes: the Pio block, the 64 records of a group, the block's rows of X and of Psi
size_t predict_noisy_missing_lds(int m, int d, int k) {
    const size_t nk = ((size_t)m + 15) / 16 * 16, km = k == 1 ? 1 : 8;
    const size_t work = 32 * (nk + 2) + 64 * (size_t)predict_missing_rec(d, k) + 64 * (size_t)d, red = 4 * 32 * 3 * km;
    return (work > red ? work : red) * sizeof(double);
}

int launch_pnm_check_psi(hipStream_t st, const void *Psi, int f32, long ns, int d, long rs, long cs, unsigned obs, double smin,
                         unsigned *rec) {
    if (ns <= 0 || obs == 0) return 0;   // nothing observed: Psi is not read at all
    const int dc = (cs == 0) ? 1 : d;    // a broadcast column: once per row
    long nb = (ns * dc + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_pnm_check_psi, dim3((unsigned)nb), dim3(256), 0, st, Psi, f32, ns, dc, rs, cs, obs, smin, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pnm_records(hipStream_t st, int m, int d, int de, int k, const double *P, const double *G2, const double *w, const double *v,
                       const double *iS, double *rec) {
    const long npair = (long)m * (m + 1) / 2, npad = predict_missing_groups(m) * 64;
    hipLaunchKernelGGL(k_pnm_records, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, npair, npad, m, d, de, k, P, G2, w, v, iS, rec,
                       predict_missing_rec(d, k));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pnm_no(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m, int mp, int de, unsigned obs,
                  const double *P, const double *G2, const double *bt, double *No, double *Pio) {
    if (nrow <= 0) return 0;
    hipLaunchKernelGGL(k_pnm_no, dim3((unsigned)((nrow + 3) / 4)), dim3(256), 0, st, Xc, Psic, ldx, n, nrow, m, mp, de, obs, P, G2, bt, No,
                       Pio);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_predict_noisy_missing_pairs(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio, int ldpio,
                                       int m, int d, int k, unsigned obs, const double *U, const double *rec, int nchunk, double *part,
                                       long ldp, const double *hd, long ldh, const double *bvec, double *out) {
    if (n <= 0) return 0;
    if (d < 1 || d > 20 || k < 1 || k > 8 || m < 1 || ((m + 15) / 16) * 16 > 256 || nchunk != predict_missing_chunks(m) || (obs >> d))
        return -1;
    PredNoisyMissArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.Pio = Pio; a.ldpio = ldpio; a.nk = ((m + 15) / 16) * 16; a.U = U; a.rec = rec;
    a.nrec = predict_missing_rec(d, k); a.d = d; a.k = k; a.obs = obs;
    a.ngrp = (int)predict_missing_groups(m);
    a.gpc = (a.ngrp + nchunk - 1) / nchunk;
    a.part = part; a.ldp = ldp;
    const size_t lds = predict_noisy_missing_lds(m, d, k);
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)nchunk);
    // per launch, not once per process: the attribute belongs to the current device's copy of the kernel
    if (k == 1) {
        if (lds > 65536 && hipFuncSetAttribute((const void *)k_predict_noisy_missing_pairs<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds) != hipSuccess)
            return -1;
        hipLaunchKernelGGL(k_predict_noisy_missing_pairs<1>, grid, dim3(256), lds, st, a);
    } else {
        if (lds > 65536 && hipFuncSetAttribute((const void *)k_predict_noisy_missing_pairs<8>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds) != hipSuccess)
            return -1;
        hipLaunchKernelGGL(k_predict_noisy_missing_pairs<8>, grid, dim3(256), lds, st, a);
    }
    if (hipGetLastError() != hipSuccess) return -1;
    return launch_pmd_finish(st, part, nchunk, ldp, hd, ldh, n, k, bvec, out);
}
