// Rows with missing inputs through the streaming predictor (gpz_predictor_run_missing_dev / _draws_missing_dev, gpz_predictor.hip):
// predictMissing of the diagonal kinds (predictDiag.m:127-209) for one tile of ONE group of rows that share a NaN pattern.  The pattern
// is a bit mask of the observed dimensions (bit c set: dimension c is a number in every row); o = observed, u = missing dimensions.
//
// Per pattern (and priors), once, in buffers sized by the model alone:
//   k_pmd_basis    bt [2][mp] = [lno_j = -1/2 sum_o ln sigma_jo | prior_j] and
//                  NijS [l][j] = exp(lnz_j) Nij(j, l), mp x mp row-major: the B operand of PHI's product             :140, :160-163
//   k_pmd_pairs    the pair records [lnZ_q incl. -1/2 sum_o ln C_q | c_q (d) | 1 / C_q (d) | per output f w_i w_j, f v_i v_j, f iS(i, j)] for
//                  q = i (i + 1) / 2 + j, j <= i, f = 2 off the diagonal and 1 on it (:191-198), iS read at i >= j only as the reference
//                  does.  c_q and 1 / C_q are ZERO in the missing dimensions, so the row loop runs over all d without a branch on the
//                  pattern (the staged rows carry zeros there, never a NaN).  Records past the last pair are zero.
//   k_pmd_u        U(q, l) = Nu_q(l) (:181-183) in the order the pair kernel's lanes fetch it: 16-pair block b, K step ks, lane
//                  (l & 3) * 16 + (q & 15) -> U[(b * nk / 4 + ks) * 64 + lane], l = 4 ks + (lane >> 4).  Zero for l >= m and past the last
//                  pair; padded to whole groups of 64 pairs.  One wave load of a fragment is 512 contiguous bytes.
// Per tile, on Xc [d][ldx] as k_pred_stage left it (NaN in the missing dimensions: every kernel here selects on the mask):
//   k_pmd_no       No(r, j) = exp(lno_j - 1/2 sum_o (x - p_j)^2 gamma_j^2), Pio = No prior / sum_j (No prior); one wave per row   :142-154
//   k_pnm_no       the same for rows with Psi: No(r, j) = exp(-1/2 sum_o [(x - p_j)^2 / (psi + sigma_jo) + ln(psi + sigma_jo)]).  With
//                  u = 1 + psi gamma_j^2: (psi + sigma) = u / gamma^2, so the exponent is lno_j - 1/2 (sum_o (x - p)^2 gamma^2 / u +
//                  sum_o ln u): at psi = 0 the bits of k_pmd_no.  The loop runs over the set bits of obs.                      :227-238
//   launch_tgemm   T = Pio NijS on the f64 MFMA (k_gemm.hip)
//   k_pmd_phi      PHI = No o T (over No), mu = PHI w, ElnS - b = PHI v; one wave per row                                        :162-166
//   k_predict_missing_pairs<KM>   the hot one: gamma, VlnS and nu's pair sums (:172-200) with the n x pairs product Pio Nu' never in memory:
//                  the clean z and the pairs sink of k_predict_group_impl.h, where the layout is described once.  KM = 1 or 8 outputs in
//                  registers.  gridDim.y = predict_missing_chunks(m) chunks of the groups, each into its own slab part [C][3k][ldp].
//                  LDS: (32 (nk + 2) + 64 (1 + 2 d + 3 k) + 32 d) doubles, at least 4 * 32 * 3 KM for the last reduction.
//                  k_predict_noisy_missing_pairs<KM> (k_predict_noisy_missing.hip, rows with Psi too) is launched from here as well.
//   k_pmd_finish   the chunks added in chunk order; VlnS -= ElnS^2, beta = exp(ElnS + b) (1 + VlnS / 2), gamma -= mu^2 -> out [4k][nt] =
//                  mu | nu | beta | gamma, the layout k_pred_finish_noisy_dev reads.                                         :203-209
//   k_pmd_check    word 0 of the device entries' record is set when an element's NaN-ness differs from the mask.
// A row's results depend on its own values and the model only: the same bits for any tile size, position in the block and row order.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_predict_group_impl.h"

__device__ __forceinline__ bool pmd_obs(unsigned obs, int c) { return (obs >> c) & 1u; }

__global__ __launch_bounds__(256) void k_pmd_check(const void *__restrict__ X, int f32, long ns, int d, long rs, long cs, unsigned obs,
                                                   unsigned *__restrict__ rec) {
    const long ne = ns * d, step = (long)gridDim.x * 256;
    int bad = 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < ne; e += step) {
        const long r = e / d;
        const int c = (int)(e - r * d);
        const long at = r * rs + c * cs;
        const double v = f32 ? (double)((const float *)X)[at] : ((const double *)X)[at];
        bad |= (v == v) != pmd_obs(obs, c);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(rec + 0, 1u);
}

// G2: gamma^2 = 1 / sigma, m x de row-major
__global__ __launch_bounds__(256) void k_pmd_basis(int m, int mp, int d, int de, unsigned obs, const double *__restrict__ P,
                                                   const double *__restrict__ G2, const double *__restrict__ priors, double *__restrict__ bt,
                                                   double *__restrict__ NijS) {
    const int j = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    if (j >= mp) return;
    double lz = 0.0, lo = 0.0;
    if (j < m)
        for (int c = 0; c < d; ++c) {
            const double lg = log(G2[(size_t)j * de + c]);
            lz += lg;                                                  // lnz_j = -1/2 sum ln iSigma            :140
            if (pmd_obs(obs, c)) lo += lg;                             // -1/2 sum_o ln sigma = +1/2 sum_o ln gamma^2   :147
        }
    if (l == 0) {
        bt[j] = j < m ? 0.5 * lo : 0.0;
        bt[mp + j] = j < m ? (priors ? priors[j] : 1.0 / m) : 0.0;
    }
    double v = 0.0;
    if (j < m && l < m) {
        double q = 0.0, ls = 0.0;
        for (int c = 0; c < d; ++c) {
            if (pmd_obs(obs, c)) continue;
            const double s = 1.0 / G2[(size_t)j * de + c] + 1.0 / G2[(size_t)l * de + c];
            const double dl = P[(size_t)j * de + c] - P[(size_t)l * de + c];
            q += dl * dl / s;
            ls += log(s);
        }
        v = exp(-0.5 * lz - 0.5 * q - 0.5 * ls);                       // :160, :163
    }
    NijS[(size_t)l * mp + j] = v;
}

// one thread per pair of the padded table (npad = whole groups of 64)
__global__ __launch_bounds__(256) void k_pmd_pairs(long npair, long npad, int m, int d, int de, int k, unsigned obs,
                                                   const double *__restrict__ P, const double *__restrict__ G2, const double *__restrict__ w,
                                                   const double *__restrict__ v, const double *__restrict__ iS, double *__restrict__ rec,
                                                   int nrec) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= npad) return;
    double *r = rec + (size_t)q * nrec;
    if (q >= npair) {
        for (int e = 0; e < nrec; ++e) r[e] = 0.0;
        return;
    }
    int i, j;
    gpz_pair_of(q, &i, &j);
    double lz = 0.0, qd = 0.0, ls = 0.0, lo = 0.0;
    for (int c = 0; c < d; ++c) {
        const double isi = G2[(size_t)i * de + c], isj = G2[(size_t)j * de + c];
        const double iC = isi + isj, C = 1.0 / iC;                                               // :175
        const double cv = (P[(size_t)i * de + c] * isi + P[(size_t)j * de + c] * isj) * C;       // :176
        lz += log(isi) + log(isj);
        const double s = 1.0 / isi + 1.0 / isj, dl = P[(size_t)i * de + c] - P[(size_t)j * de + c];
        qd += dl * dl / s;
        ls += log(s);
        const bool o = pmd_obs(obs, c);
        if (o) lo += log(C);
        r[1 + c] = o ? cv : 0.0;
        r[1 + d + c] = o ? iC : 0.0;
    }
    r[0] = -0.5 * lz - 0.5 * qd - 0.5 * ls - 0.5 * lo;                                           // :189 and the row-free part of :179
    gpz_pair_coef(r + 1 + 2 * d, i, j, m, k, w, v, iS);
}

// one thread per element of U in its stored order: e = (b * nks + ks) * 64 + lane
__global__ __launch_bounds__(256) void k_pmd_u(long npair, long nelem, int m, int nk, int d, int de, unsigned obs,
                                               const double *__restrict__ P, const double *__restrict__ G2, double *__restrict__ U) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= nelem) return;
    const int lane = (int)(e & 63), nks = nk >> 2;
    const long bk = e >> 6, b = bk / nks;
    const int ks = (int)(bk - b * nks), l = 4 * ks + (lane >> 4);
    const long q = b * 16 + (lane & 15);
    double val = 0.0;
    if (q < npair && l < m) {
        int i, j;
        gpz_pair_of(q, &i, &j);
        double qd = 0.0, ls = 0.0;
        for (int c = 0; c < d; ++c) {
            if (pmd_obs(obs, c)) continue;
            const double isi = G2[(size_t)i * de + c], isj = G2[(size_t)j * de + c];
            const double C = 1.0 / (isi + isj);
            const double cv = (P[(size_t)i * de + c] * isi + P[(size_t)j * de + c] * isj) * C;
            const double s = 1.0 / G2[(size_t)l * de + c] + C;                                    // :182
            const double dl = P[(size_t)l * de + c] - cv;
            qd += dl * dl / s;
            ls += log(s);
        }
        val = exp(-0.5 * qd - 0.5 * ls);                                                         // :183
    }
    U[e] = val;
}

// rows [0, nrow) of No and Pio (ld = mp), rows >= n and columns >= m zero; one wave per row, lanes along the basis functions
template <bool PSI>
__device__ __forceinline__ void pmd_no_body(const double *__restrict__ Xc, const double *__restrict__ Psic, long ldx, int n, int nrow, int m,
                                            int mp, int d, int de, unsigned obs, const double *__restrict__ P,
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
        double q = 0.0, v;
        if constexpr (!PSI) {
            for (int c = 0; c < d; ++c)
                if (pmd_obs(obs, c)) {
                    const double dl = Xc[(size_t)c * ldx + i] - P[(size_t)j * de + c];
                    q = fma(dl * dl, G2[(size_t)j * de + c], q);
                }
            v = exp(bt[j] - 0.5 * q);
        } else {
            double lu = 0.0;
            for (unsigned mk = obs; mk; mk &= mk - 1) {
                const int c = __builtin_ctz(mk);
                const double g = G2[(size_t)j * de + c];
                const double dl = Xc[(size_t)c * ldx + i] - P[(size_t)j * de + c];
                const double u = fma(Psic[(size_t)c * ldx + i], g, 1.0);   // (psi + sigma) / sigma
                q = fma(dl * dl, g / u, q);                                // :231
                lu += log(u);
            }
            v = exp(bt[j] - 0.5 * (q + lu));
        }
        no[j] = v;
        s = fma(v, bt[mp + j], s);
    }
    s = wave_sum(s);
    for (int j = lane; j < mp; j += 64) {
        if (j < m) pio[j] = no[j] * bt[mp + j] / s;                    // :154, :238
        else { no[j] = 0.0; pio[j] = 0.0; }
    }
}

__global__ __launch_bounds__(256) void k_pmd_no(const double *__restrict__ Xc, long ldx, int n, int nrow, int m, int mp, int d, int de,
                                                unsigned obs, const double *__restrict__ P, const double *__restrict__ G2,
                                                const double *__restrict__ bt, double *__restrict__ No, double *__restrict__ Pio) {
    pmd_no_body<false>(Xc, nullptr, ldx, n, nrow, m, mp, d, de, obs, P, G2, bt, No, Pio);
}

__global__ __launch_bounds__(256) void k_pnm_no(const double *__restrict__ Xc, const double *__restrict__ Psic, long ldx, int n, int nrow,
                                                int m, int mp, int de, unsigned obs, const double *__restrict__ P,
                                                const double *__restrict__ G2, const double *__restrict__ bt, double *__restrict__ No,
                                                double *__restrict__ Pio) {
    pmd_no_body<true>(Xc, Psic, ldx, n, nrow, m, mp, 0, de, obs, P, G2, bt, No, Pio);
}

// PHI = No o T over No; hd [2k][ldh] = PHI w | PHI v; one wave per row
__global__ __launch_bounds__(256) void k_pmd_phi(double *__restrict__ No, const double *__restrict__ T, int n, int m, int mp, int k,
                                                 const double *__restrict__ w, const double *__restrict__ v, double *__restrict__ hd,
                                                 long ldh) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double *ph = No + (size_t)i * mp;
    const double *t = T + (size_t)i * mp;
    for (int j = lane; j < m; j += 64) ph[j] = ph[j] * t[j];
    for (int o = 0; o < k; ++o) {
        double a = 0.0, b = 0.0;
        for (int j = lane; j < m; j += 64) {
            const double f = ph[j];
            a = fma(f, w[j + (size_t)m * o], a);
            if (v) b = fma(f, v[j + (size_t)m * o], b);
        }
        a = wave_sum(a);
        b = wave_sum(b);
        if (lane == 0) {
            hd[(size_t)o * ldh + i] = a;
            hd[(size_t)(k + o) * ldh + i] = b;
        }
    }
}

template <int KM>
__global__ __launch_bounds__(256, 2) void k_predict_missing_pairs(PredGroupArgs a) {
    predict_group_body<false, PredPairsSink<KM>>(a);
}

// hd [2k][ldh] = mu | ElnS - b; part [nchunk][3k][ldp] -> out [4k][nt]
__global__ __launch_bounds__(256) void k_pmd_finish(const double *__restrict__ part, int nchunk, long ldp, const double *__restrict__ hd,
                                                    long ldh, int nt, int k, const double *__restrict__ bvec, double *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
    if (i >= nt) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < nchunk; ++c)   // chunk order
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += part[((size_t)c * 3 * k + (size_t)q * k + o) * ldp + i];
    const double mu = hd[(size_t)o * ldh + i], el = hd[(size_t)(k + o) * ldh + i];
    const double vl = s[1] - el * el;                                  // :203
    out[(size_t)o * nt + i] = mu;
    out[(size_t)(k + o) * nt + i] = s[2];
    out[(size_t)(2 * k + o) * nt + i] = exp(el + bvec[o]) * (1.0 + 0.5 * vl);   // :205-207
    out[(size_t)(3 * k + o) * nt + i] = s[0] - mu * mu;                // :209
}

// de: the padded input width (pad_dim), one of the widths the fused predictor kernels are instantiated for
bool predict_missing_fits(int kind, int de, int m, int k) {
    bool width = false;
    for (int s : {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20}) width |= de == s;
    return kind == GPZ_KIND_DIAG && width && k >= 1 && k <= 8 && m >= 1 && ((m + 15) / 16) * 16 <= 256;
}

int predict_missing_rec(int d, int k) { return 1 + 2 * d + 3 * k; }

long predict_missing_groups(int m) { return ((long)m * (m + 1) / 2 + 63) / 64; }

// chunks of the 64-pair groups: one per 16 groups, at most 8.  The model's shape only, never the rows.
int predict_missing_chunks(int m) {
    const long c = predict_missing_groups(m) / 16;
    return (int)(c < 1 ? 1 : (c > 8 ? 8 : c));
}

// dynamic LDS of the pair kernels, bytes: the Pio block, the 64 records of a group, the block's rows of X and, with psi, of Psi
size_t predict_missing_lds(int m, int d, int k, bool psi) {
    const size_t nk = ((size_t)m + 15) / 16 * 16, km = k == 1 ? 1 : 8;
    const size_t work = psi ? 32 * (nk + 2) + 64 * (size_t)predict_missing_rec(d, k) + 64 * (size_t)d
                            : 32 * (nk + 2) + 64 * (size_t)predict_missing_rec(d, k) + 32 * (size_t)d;
    const size_t red = 4 * 32 * 3 * km;
    return (work > red ? work : red) * sizeof(double);
}

int launch_pmd_check(hipStream_t st, const void *X, int f32, long ns, int d, long rs, long cs, unsigned obs, unsigned *rec) {
    if (ns <= 0) return 0;
    long nb = (ns * d + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_pmd_check, dim3((unsigned)nb), dim3(256), 0, st, X, f32, ns, d, rs, cs, obs, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pmd_tables(hipStream_t st, int m, int mp, int d, int de, int k, unsigned obs, const double *P, const double *G2,
                      const double *priors, const double *w, const double *v, const double *iS, double *bt, double *NijS, double *U,
                      double *rec, bool pairs) {
    hipLaunchKernelGGL(k_pmd_basis, dim3((unsigned)((mp + 255) / 256), (unsigned)mp), dim3(256), 0, st, m, mp, d, de, obs, P, G2, priors, bt,
                       NijS);
    if (hipGetLastError() != hipSuccess) return -1;
    if (!pairs) return 0;
    const long npair = (long)m * (m + 1) / 2, npad = predict_missing_groups(m) * 64;
    const int nk = ((m + 15) / 16) * 16;
    const long nelem = npad * nk;
    hipLaunchKernelGGL(k_pmd_pairs, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, npair, npad, m, d, de, k, obs, P, G2, w, v, iS, rec,
                       predict_missing_rec(d, k));
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_pmd_u, dim3((unsigned)((nelem + 255) / 256)), dim3(256), 0, st, npair, nelem, m, nk, d, de, obs, P, G2, U);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pmd_no(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m, int mp, int d, int de,
                  unsigned obs, const double *P, const double *G2, const double *bt, double *No, double *Pio) {
    if (nrow <= 0) return 0;
    const dim3 grid((unsigned)((nrow + 3) / 4));
    if (Psic) hipLaunchKernelGGL(k_pnm_no, grid, dim3(256), 0, st, Xc, Psic, ldx, n, nrow, m, mp, de, obs, P, G2, bt, No, Pio);
    else hipLaunchKernelGGL(k_pmd_no, grid, dim3(256), 0, st, Xc, ldx, n, nrow, m, mp, d, de, obs, P, G2, bt, No, Pio);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pmd_phi(hipStream_t st, double *No, const double *T, int n, int m, int mp, int k, const double *w, const double *v, double *hd,
                   long ldh) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_pmd_phi, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, No, T, n, m, mp, k, w, v, hd, ldh);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_predict_missing_pairs(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio, int ldpio, int m,
                                 int d, int k, unsigned obs, const double *U, const double *rec, int nchunk, double *part, long ldp,
                                 const double *hd, long ldh, const double *bvec, double *out) {
    if (n <= 0) return 0;
    if (d < 1 || d > 20 || k < 1 || k > 8 || m < 1 || ((m + 15) / 16) * 16 > 256 || nchunk != predict_missing_chunks(m) ||
        (Psic && (obs >> d)))
        return -1;
    PredGroupArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.Pio = Pio; a.ldpio = ldpio; a.nk = ((m + 15) / 16) * 16; a.U = U; a.rec = rec;
    a.nrec = predict_missing_rec(d, k); a.d = d; a.k = k; a.obs = obs;
    a.ngrp = (int)predict_missing_groups(m);
    a.gpc = (a.ngrp + nchunk - 1) / nchunk;
    a.part = part; a.ldp = ldp;
    const size_t lds = predict_missing_lds(m, d, k, Psic != nullptr);
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)nchunk);
    if (Psic ? (k == 1 ? launch_predict_group<k_predict_noisy_missing_pairs<1>>(st, grid, lds, a)
                       : launch_predict_group<k_predict_noisy_missing_pairs<8>>(st, grid, lds, a))
             : (k == 1 ? launch_predict_group<k_predict_missing_pairs<1>>(st, grid, lds, a)
                       : launch_predict_group<k_predict_missing_pairs<8>>(st, grid, lds, a)))
        return -1;
    return launch_pmd_finish(st, part, nchunk, ldp, hd, ldh, n, k, bvec, out);
}

int launch_pmd_finish(hipStream_t st, const double *part, int nchunk, long ldp, const double *hd, long ldh, int n, int k,
                      const double *bvec, double *out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_pmd_finish, dim3((unsigned)((n + 255) / 256), (unsigned)k), dim3(256), 0, st, part, nchunk, ldp, hd, ldh, n, k, bvec,
                       out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
