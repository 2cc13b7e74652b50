// Rows with input noise through the streaming predictor (gpz_predictor_run_noisy_dev / _draws_noisy / _draws_noisy_dev, gpz_predictor.hip):
// predictNoisy of the diagonal kinds (predictDiag.m:75-125) for one tile as ONE kernel plus a finish, the draws kernel behind a PHI block
// built from X and Psi, and the byte movers of the device entries.  Psi is per-dimension variances in the layout of Xc.
//
//   k_predict_noisy_small<DT, KM>   lane = row (coalesced reads of Xc / Psic [d][ldx], no row-major copy), DT = d itself, KM = 1 or 8 outputs
//                                   in registers.  Per row, for the basis functions [j0, j1) of its chunk: PHI_Psi,ij in registers
//                                   (k_phi_diag<.., PSI>'s arithmetic), mu += PHI w_j, ElnS - b += PHI v_j - no PHI matrix, no row-dot
//                                   launch.  Then the pairs [p0, p1) of its chunk, k_predict_noisy_diag's arithmetic: per dimension one
//                                   r = (C_ab + psi)^-1/2, z = exp(lnZ_ab - 1/2 sum (Delta r)^2) prod r, three FMAs per output against
//                                   coefficients that sit in the pair record, so the loop loads nothing but the record:
//                                     [lnZ | c_ab (d) | C_ab (d) | per output: f w_a w_b, f v_a v_b, f iS(a, b)],  f = 1 (a = b) or 2
//                                   (launch_pair_table + k_noisy_pair_coef, once per handle; iS is read in its lower triangle a >= b only,
//                                   as the reference does).  The records are the same for every row: a workgroup (256 rows) stages 32 of
//                                   them at a time in LDS with coalesced loads and its lanes read them as broadcasts (one address per
//                                   instruction, no bank conflict).  Through scalar loads two records of 1 + 2 d + 3 k doubles do not fit
//                                   the scalar registers (spills in every width at k = 8), and every wave would fetch the table for itself.
//                                   Two pairs per trip: their two exp chains are independent, which is what a lane has to hide the
//                                   latency of dependent f64 operations with (a full tile is two waves per SIMD).
//   k_predict_noisy_finish          part [C][5k][ldp] (mu, ElnS - b, gamma, VlnS, nu raw) added in chunk order -> out [4k][nt] =
//                                   mu | nu | beta | gamma with VlnS -= (ElnS - b)^2, gamma -= mu^2, beta = exp(ElnS) (1 + VlnS / 2).
// The chunk count C = predict_noisy_chunks(m, d, k) depends on the model's shape only, and every sum runs in a fixed order from zero: no
// atomics, and a row's results have the same bits for any tile size, position in the tile and row order.
// The chunk rule: C = clamp(floor(npair / 2048), 1, 4) with npair = m (m + 1) / 2, for every m - with GPZ_PREDICT_LARGE_M
// (256 < ceil16(m) <= 1024) the cap of 4 stays, so C = 4 from m = 128 on.  No measurement decided that: a 16 384-row call is 64 workgroups
// per chunk, 256 in all on 256 compute units, and a higher cap was not timed.  predict_noisy_cov_chunks and predict_gamma_chunks keep
// their caps of 4 in the same way.  Index ranges at m = 1024: npair = 524 800 and npair * rec <= 524 800 * 65 fit 32 bits; the table is
// addressed in size_t.
//
//   k_predict_noisy_phi<DT>         E_x[PHI] of a tile as launch_tgemm takes it, Phi [nrow][mp] row-major with zeros in the rows >= n and the
//                                   columns >= m: the draws of a handle with GPZ_PREDICT_LARGE_M off the fused route (PHI W on k_tgemm, as
//                                   the covariance kinds' predict_ncov_phi_body).  The arithmetic of the mu phase above.  A workgroup owns
//                                   64 rows: every wave has lane = row (x and psi in registers) and forms 8 of the 32 basis functions of a
//                                   stage, whose records [P_j | G2_j] lie in LDS and are read as broadcasts.  The 64 x 32 values pass
//                                   through an LDS tile with a row stride of 33 doubles (ds_write_b64 of 16 lanes: 32 banks, no conflict;
//                                   the read is along a row) and leave as 256-byte runs of a PHI row, two rows per wave store; gridDim.y
//                                   splits the columns in multiples of 32, so every run starts on a 256-byte boundary.  No sum: an
//                                   element's bits depend on its row and column alone.
//   k_predict_draws_psi<D>          k_predict_draws' body (k_predict_draws_impl.h) with PsPhiBuilder<D, false, true>: 11 widths.
//   k_pred_check_psi                word 3 of the device entries' record is set when an element of Psi is NaN, negative, or infinite
//                                   (itself or once divided by the smallest sd2).
//   k_pred_stage_psi<T>             the caller's Psi (f64 or f32, any strides, column stride 0 for n x 1) -> Psic [d][ldx] = double(psi) / sd2[c],
//                                   a plain f64 division (sd2 = sdX ** 2 from the host: the bits of fixPsi).
//   k_pred_finish_noisy_dev         out [4k][nt] -> the caller's column-major ns x k arrays at row r0: mu + muY, nu, beta, gamma,
//                                   sigma = (nu + beta) + gamma.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#define PREDICT_DRAWS_PSI   // k_predict_draws_psi<D>
#include "k_predict_draws_impl.h"

struct PredNoisyArgs {
    const double *Xc, *Psic; long ldx;   // [d][ldx] column layout, n rows
    int n, m, k, de;                     // de: row stride of P and G2
    const double *P, *G2;                // m x de row-major: centres and gamma^2
    const double *w, *v;                 // m x k column-major; v nullptr without the heteroscedastic term
    const double *tab; int rec;          // pair records (see above), rec = 1 + 2 d + 3 k doubles each
    int jpc; long ppc;                   // basis functions and pairs per chunk
    double *part; long ldp;              // [chunks][5 k][ldp]
};

#define PN_TP 32   // records per LDS stage

template <int DT, int KM>
__global__ __launch_bounds__(256) void k_predict_noisy_small(PredNoisyArgs a) {
    // one stage of PN_TP pair records (1 + 2 DT + 3 k doubles each, as they lie in the table) or basis records [P_j | G2_j | w_j | v_j]
    // (2 DT + 2 KM <= 1 + 2 DT + 3 KM doubles each)
    __shared__ double sT[PN_TP * (1 + 2 * DT + 3 * KM)];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const bool act = i < a.n;
    const int ic = act ? i : a.n - 1;
    const int ch = blockIdx.y, m = a.m, k = a.k;
    double x[DT], ps[DT];
#pragma unroll
    for (int c = 0; c < DT; ++c) {
        x[c] = a.Xc[(size_t)c * a.ldx + ic];
        ps[c] = a.Psic[(size_t)c * a.ldx + ic];
    }
    double mu[KM], el[KM], ga[KM], vl[KM], nu[KM];
#pragma unroll
    for (int o = 0; o < KM; ++o) { mu[o] = 0.0; el[o] = 0.0; ga[o] = 0.0; vl[o] = 0.0; nu[o] = 0.0; }
    // ---- mu and ElnS - b over the chunk's basis functions                                          predictDiag.m:80-84
    const int j0 = ch * a.jpc, j1 = min(m, j0 + a.jpc);
    constexpr int rj = 2 * DT + 2 * KM;   // outputs k .. KM - 1 hold zeros: the sums below need no test on k
    for (int jb = j0; jb < j1; jb += PN_TP) {
        const int nj = min(PN_TP, j1 - jb);
        __syncthreads();   // the stage before is read
        for (int t = tid; t < nj * rj; t += 256) {
            const int jj = t / rj, f = t - jj * rj, j = jb + jj;
            double val;
            if (f < DT) val = a.P[(size_t)j * a.de + f];
            else if (f < 2 * DT) val = a.G2[(size_t)j * a.de + f - DT];
            else if (f < 2 * DT + KM) val = f - 2 * DT < k ? a.w[j + (size_t)m * (f - 2 * DT)] : 0.0;
            else val = (a.v && f - 2 * DT - KM < k) ? a.v[j + (size_t)m * (f - 2 * DT - KM)] : 0.0;
            sT[t] = val;
        }
        __syncthreads();
#pragma unroll 2
        for (int jj = 0; jj < nj; ++jj) {
            const double *t = sT + jj * rj;   // the same address in every lane: a broadcast read
            double q = 0.0, pr = 1.0;
#pragma unroll
            for (int c = 0; c < DT; ++c) {
                const double dl = x[c] - t[c], gc = t[DT + c];
                const double u = fma(ps[c], gc, 1.0);                  // 1 + psi / sigma
                q = fma(dl * dl, gc * gpz_rcp1(u), q);                 // getPHI.m:104  Delta.^2 ./ (Psi + Sigma)
                pr *= u;
            }
            q += log(pr);
            const double ph = exp(-0.5 * q);
#pragma unroll
            for (int o = 0; o < KM; ++o) {
                mu[o] = fma(ph, t[2 * DT + o], mu[o]);
                el[o] = fma(ph, t[2 * DT + KM + o], el[o]);
            }
        }
    }
    // ---- the chunk's pairs, two per trip                                                           predictDiag.m:86-119
    const long npair = (long)m * (m + 1) / 2;
    const long p0 = (long)ch * a.ppc, p1 = min(npair, p0 + a.ppc);
    const int rec = a.rec;
    for (long pb = p0; pb < p1; pb += PN_TP) {
        const int np = (int)min((long)PN_TP, p1 - pb);
        __syncthreads();
        const double *src = a.tab + (size_t)pb * rec;
        for (int t = tid; t < np * rec; t += 256) sT[t] = src[t];
        __syncthreads();
        int e = 0;
        for (; e + 1 < np; e += 2) {
            const double *t0 = sT + e * rec, *t1 = t0 + rec;
            double q0 = 0.0, q1 = 0.0, r0p = 1.0, r1p = 1.0;
#pragma unroll
            for (int c = 0; c < DT; ++c) {
                const double r0 = rsqrt_nr2(t0[1 + DT + c] + ps[c]);    // (Cij + Psi)^-1/2            :105
                const double r1 = rsqrt_nr2(t1[1 + DT + c] + ps[c]);
                const double d0 = (x[c] - t0[1 + c]) * r0, d1 = (x[c] - t1[1 + c]) * r1;
                q0 = fma(d0, d0, q0);
                q1 = fma(d1, d1, q1);
                r0p *= r0;
                r1p *= r1;
            }
            const double z0 = exp(t0[0] - 0.5 * q0) * r0p, z1 = exp(t1[0] - 0.5 * q1) * r1p;   // :107
            const double *c0 = t0 + 1 + 2 * DT, *c1 = t1 + 1 + 2 * DT;
#pragma unroll
            for (int o = 0; o < KM; ++o)
                if (o < k) {
                    ga[o] = fma(z1, c1[3 * o], fma(z0, c0[3 * o], ga[o]));
                    vl[o] = fma(z1, c1[3 * o + 1], fma(z0, c0[3 * o + 1], vl[o]));
                    nu[o] = fma(z1, c1[3 * o + 2], fma(z0, c0[3 * o + 2], nu[o]));
                }
        }
        if (e < np) {
            const double *t0 = sT + e * rec;
            double q0 = 0.0, r0p = 1.0;
#pragma unroll
            for (int c = 0; c < DT; ++c) {
                const double r0 = rsqrt_nr2(t0[1 + DT + c] + ps[c]);
                const double d0 = (x[c] - t0[1 + c]) * r0;
                q0 = fma(d0, d0, q0);
                r0p *= r0;
            }
            const double z0 = exp(t0[0] - 0.5 * q0) * r0p;
            const double *c0 = t0 + 1 + 2 * DT;
#pragma unroll
            for (int o = 0; o < KM; ++o)
                if (o < k) {
                    ga[o] = fma(z0, c0[3 * o], ga[o]);
                    vl[o] = fma(z0, c0[3 * o + 1], vl[o]);
                    nu[o] = fma(z0, c0[3 * o + 2], nu[o]);
                }
        }
    }
    if (!act) return;
    double *pp = a.part + (size_t)ch * 5 * k * a.ldp + i;
#pragma unroll
    for (int o = 0; o < KM; ++o)
        if (o < k) {
            pp[(size_t)(0 * k + o) * a.ldp] = mu[o];
            pp[(size_t)(1 * k + o) * a.ldp] = el[o];
            pp[(size_t)(2 * k + o) * a.ldp] = ga[o];
            pp[(size_t)(3 * k + o) * a.ldp] = vl[o];
            pp[(size_t)(4 * k + o) * a.ldp] = nu[o];
        }
}

__global__ __launch_bounds__(256) void k_predict_noisy_finish(const double *__restrict__ part, int nchunk, long ldp, int nt, int k,
                                                              const double *__restrict__ bvec, double *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
    if (i >= nt) return;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nchunk; ++c)   // chunk order
#pragma unroll
        for (int q = 0; q < 5; ++q) s[q] += part[((size_t)c * 5 * k + (size_t)q * k + o) * ldp + i];
    const double mu = s[0], el = s[1];
    const double vl = s[3] - el * el;                                  // predictDiag.m:121
    out[(size_t)o * nt + i] = mu;
    out[(size_t)(k + o) * nt + i] = s[4];
    out[(size_t)(2 * k + o) * nt + i] = exp(el + bvec[o]) * (1.0 + 0.5 * vl);   // :125
    out[(size_t)(3 * k + o) * nt + i] = s[2] - mu * mu;                // :123
}

// the per-output coefficients of every pair record (the tail of the record, behind what launch_pair_table wrote)
__global__ __launch_bounds__(256) void k_noisy_pair_coef(int m, int k, int d, const double *__restrict__ w, const double *__restrict__ v,
                                                         const double *__restrict__ iS, double *__restrict__ tab, int rec) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x, npair = (long)m * (m + 1) / 2;
    if (e >= npair) return;
    int a, b;
    gpz_pair_of(e, &a, &b);                                            // f: 2x in the loop, 1x on the diagonal  (predictDiag.m:113-119)
    gpz_pair_coef(tab + (size_t)e * rec + 1 + 2 * d, a, b, m, k, w, v, iS);
}

bool predict_noisy_fits(int kind, int de, int m, int k, bool large_m) {
    return kind == GPZ_KIND_DIAG && de <= 20 && ps_width_instantiated(de) && k <= 8 &&
           ((m + 15) / 16) * 16 <= (large_m ? GPZ_PREDICT_LARGE_M_MAX : 256);
}

// pair chunks (= chunks of the basis functions): one per 2048 pairs, at most 4.  The model's shape only, never the rows.
int predict_noisy_chunks(int m, int d, int k) {
    (void)d; (void)k;
    const long c = ((long)m * (m + 1) / 2) / 2048;
    return (int)(c < 1 ? 1 : (c > 4 ? 4 : c));
}

int predict_noisy_rec(int d, int k) { return 1 + 2 * d + 3 * k; }

int launch_noisy_pair_coef(hipStream_t st, int m, int k, int d, const double *w, const double *v, const double *iS, double *tab, int rec) {
    const long npair = (long)m * (m + 1) / 2;
    hipLaunchKernelGGL(k_noisy_pair_coef, dim3((unsigned)((npair + 255) / 256)), dim3(256), 0, st, m, k, d, w, v, iS, tab, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int DT>
static void launch_pn(hipStream_t st, const PredNoisyArgs &a, dim3 grid) {
    if (a.k == 1) hipLaunchKernelGGL((k_predict_noisy_small<DT, 1>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_predict_noisy_small<DT, 8>), grid, dim3(256), 0, st, a);
}

int launch_predict_noisy_small(hipStream_t st, int d, int de, const double *Xc, const double *Psic, long ldx, int n, int m, int k,
                               const double *P, const double *G2, const double *w, const double *v, const double *bvec,
                               const double *tab, int nchunk, double *part, long ldp, double *out) {
    if (n <= 0) return 0;
    if (d < 1 || d > 20 || k < 1 || k > 8 || nchunk < 1) return -1;
    const long npair = (long)m * (m + 1) / 2;
    PredNoisyArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.m = m; a.k = k; a.de = de; a.P = P; a.G2 = G2; a.w = w; a.v = v;
    a.tab = tab; a.rec = predict_noisy_rec(d, k);
    a.jpc = (m + nchunk - 1) / nchunk;
    a.ppc = (npair + nchunk - 1) / nchunk;
    a.part = part; a.ldp = ldp;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nchunk);
    switch (d) {
#define PN_CASE(DD) case DD: launch_pn<DD>(st, a, grid); break;
        PN_CASE(1) PN_CASE(2) PN_CASE(3) PN_CASE(4) PN_CASE(5) PN_CASE(6) PN_CASE(7) PN_CASE(8) PN_CASE(9) PN_CASE(10)
        PN_CASE(11) PN_CASE(12) PN_CASE(13) PN_CASE(14) PN_CASE(15) PN_CASE(16) PN_CASE(17) PN_CASE(18) PN_CASE(19) PN_CASE(20)
#undef PN_CASE
        default: return -1;
    }
    if (hipGetLastError() != hipSuccess) return -1;
    return launch_predict_noisy_finish(st, part, nchunk, ldp, n, k, bvec, out);
}

// the finish kernel on its own: behind the pair kernel above and that of the covariance kinds (k_predict_noisy_cov.hip)
int launch_predict_noisy_finish(hipStream_t st, const double *part, int nchunk, long ldp, int n, int k, const double *bvec, double *out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_predict_noisy_finish, dim3((unsigned)((n + 255) / 256), (unsigned)k), dim3(256), 0, st, part, nchunk, ldp, n, k,
                       bvec, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- E_x[PHI] of a tile for the T-GEMM (the draws with Psi off the fused route) -----------------------------------------------------
struct PredNoisyPhiArgs {
    const double *Xc, *Psic; long ldx;   // [d][ldx] column layout, n rows
    int n, nrow, m, mp, de;              // nrow rows of mp doubles are written (nrow a multiple of 64); de: row stride of P and G2
    const double *P, *G2;
    int jpc;                             // columns per chunk, a multiple of PNP_TJ
    double *Phi;
};

#define PNP_TJ 32            // basis functions per stage
#define PNP_LD (PNP_TJ + 1)  // row stride of the tile in LDS

template <int DT>
__global__ __launch_bounds__(256) void k_predict_noisy_phi(PredNoisyPhiArgs a) {
    __shared__ double sR[PNP_TJ * 2 * DT];   // one stage of basis records [P_j | G2_j]
    __shared__ double sP[64 * PNP_LD];       // the stage's values, [row][basis function]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long r0 = (long)blockIdx.x * 64, i = r0 + lane;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    const int m = a.m;
    const int j0 = blockIdx.y * a.jpc, jend = min(a.mp, j0 + a.jpc);   // this chunk's columns; those >= m are zeros
    if (j0 >= jend) return;
    double x[DT], ps[DT];
#pragma unroll
    for (int c = 0; c < DT; ++c) {
        x[c] = a.Xc[(size_t)c * a.ldx + ic];
        ps[c] = a.Psic[(size_t)c * a.ldx + ic];
    }
    constexpr int rj = 2 * DT;
    for (int jb = j0; jb < jend; jb += PNP_TJ) {
        const int nj = min(PNP_TJ, jend - jb), njr = max(0, min(PNP_TJ, m - jb));   // columns to write, and those with a basis function
        // (sR was last read, and sP last written, before the second barrier of the stage before; sP is read behind it, and every
        // thread is through with that before it passes the first barrier here)
        for (int t = tid; t < njr * rj; t += 256) {
            const int jj = t / rj, f = t - jj * rj;
            sR[t] = f < DT ? a.P[(size_t)(jb + jj) * a.de + f] : a.G2[(size_t)(jb + jj) * a.de + f - DT];
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < PNP_TJ / 4; ++q) {
            const int jj = wv * (PNP_TJ / 4) + q;
            double ph = 0.0;
            if (jj < njr) {                       // the same in every lane of the wave
                const double *t = sR + jj * rj;   // the same address in every lane: a broadcast read
                double qq = 0.0, pr = 1.0;
#pragma unroll
                for (int c = 0; c < DT; ++c) {
                    const double dl = x[c] - t[c], gc = t[DT + c];
                    const double u = fma(ps[c], gc, 1.0);                  // 1 + psi / sigma
                    qq = fma(dl * dl, gc * gpz_rcp1(u), qq);               // getPHI.m:104  Delta.^2 ./ (Psi + Sigma)
                    pr *= u;
                }
                qq += log(pr);
                ph = act ? exp(-0.5 * qq) : 0.0;
            }
            sP[lane * PNP_LD + jj] = ph;
        }
        __syncthreads();
        // 8 rows per pass: 32 consecutive lanes write 256 consecutive bytes of one row of PHI
        const int c = tid & 31;
#pragma unroll
        for (int ps8 = 0; ps8 < 8; ++ps8) {
            const int row = ps8 * 8 + (tid >> 5);
            if (c < nj && r0 + row < a.nrow) a.Phi[(size_t)(r0 + row) * a.mp + jb + c] = sP[row * PNP_LD + c];
        }
    }
}

template <int DT>
static void launch_pnphi(hipStream_t st, const PredNoisyPhiArgs &a, dim3 grid) {
    hipLaunchKernelGGL((k_predict_noisy_phi<DT>), grid, dim3(256), 0, st, a);
}

int launch_predict_noisy_phi(hipStream_t st, int d, int de, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m, int mp,
                             const double *P, const double *G2, int nchunk, double *Phi) {
    if (n <= 0) return 0;
    if (d < 1 || d > 20 || m < 1 || mp < m || nrow < n || nrow % 64 || ldx < n || nchunk < 1) return -1;
    PredNoisyPhiArgs a{};
    a.Xc = Xc; a.Psic = Psic; a.ldx = ldx; a.n = n; a.nrow = nrow; a.m = m; a.mp = mp; a.de = de; a.P = P; a.G2 = G2; a.Phi = Phi;
    a.jpc = ((mp + nchunk - 1) / nchunk + PNP_TJ - 1) / PNP_TJ * PNP_TJ;
    const dim3 grid((unsigned)(nrow / 64), (unsigned)((mp + a.jpc - 1) / a.jpc));
    switch (d) {
#define PNP_CASE(DD) case DD: launch_pnphi<DD>(st, a, grid); break;
        PNP_CASE(1) PNP_CASE(2) PNP_CASE(3) PNP_CASE(4) PNP_CASE(5) PNP_CASE(6) PNP_CASE(7) PNP_CASE(8) PNP_CASE(9) PNP_CASE(10)
        PNP_CASE(11) PNP_CASE(12) PNP_CASE(13) PNP_CASE(14) PNP_CASE(15) PNP_CASE(16) PNP_CASE(17) PNP_CASE(18) PNP_CASE(19) PNP_CASE(20)
#undef PNP_CASE
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- draws with Psi ---------------------------------------------------------------------------------------------------------------
size_t predict_draws_psi_lds(int de) { return ((size_t)32 * PS_LDA + 2 * 32 * (size_t)de) * sizeof(double); }

template <int D>
static int launch_pdp(hipStream_t st, const PredDrawsArgs &a, const double *Psic, int nwg) {
    const size_t lds = predict_draws_psi_lds(D);
    // per launch, not once per process: the attribute belongs to the current device's copy of the kernel
    if (hipFuncSetAttribute((const void *)k_predict_draws_psi<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -1;
    hipLaunchKernelGGL((k_predict_draws_psi<D>), dim3(nwg), dim3(256), lds, st, a, Psic);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_predict_draws_psi(hipStream_t st, int de, const double *Xc, const double *Psic, long ldx, int n, int m, const double *P,
                             const double *G, const double *W, int ldw, int ncol, double *out, long ldo) {
    if (n <= 0) return 0;
    PredDrawsArgs a{};
    a.Xc = Xc; a.ldx = ldx; a.n = n; a.m = m; a.nk = ((m + 15) / 16) * 16;
    a.ncol = ncol; a.nbw = ldw / 16; a.P = P; a.G = G; a.W = W; a.ldw = ldw; a.out = out; a.ldo = ldo;
    const int nblocks = (n + 31) / 32;
    int nwg = 2 * gpz_cu_count();
    if (nwg > nblocks) nwg = nblocks;
    switch (de) {
        case 1: return launch_pdp<1>(st, a, Psic, nwg);
        case 2: return launch_pdp<2>(st, a, Psic, nwg);
        case 3: return launch_pdp<3>(st, a, Psic, nwg);
        case 4: return launch_pdp<4>(st, a, Psic, nwg);
        case 5: return launch_pdp<5>(st, a, Psic, nwg);
        case 6: return launch_pdp<6>(st, a, Psic, nwg);
        case 8: return launch_pdp<8>(st, a, Psic, nwg);
        case 10: return launch_pdp<10>(st, a, Psic, nwg);
        case 12: return launch_pdp<12>(st, a, Psic, nwg);
        case 16: return launch_pdp<16>(st, a, Psic, nwg);
        case 20: return launch_pdp<20>(st, a, Psic, nwg);
        default: return -1;
    }
}

// ---- byte movers of the device entries ----------------------------------------------------------------------------------------------
// dc: the columns of Psi that differ (1 for a broadcast column).  obs: the dimensions that are read (a group of rows with missing inputs:
// its observed ones; else all ones).  smin: the smallest sd2 (1 without a normalisation) - psi / smin is the largest value a kernel can
// see of this element
__global__ __launch_bounds__(256) void k_pred_check_psi(const void *__restrict__ Psi, int f32, long ns, int dc, long rs, long cs,
                                                        unsigned obs, double smin, unsigned *__restrict__ rec) {
    const long ne = ns * dc, step = (long)gridDim.x * 256;
    int bad = 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < ne; e += step) {
        const long r = e / dc;
        const int c = (int)(e - r * dc);
        if (dc > 1 && !((obs >> (c & 31)) & 1u)) continue;             // a missing dimension: not read
        const long at = r * rs + c * cs;
        const double v = f32 ? (double)((const float *)Psi)[at] : ((const double *)Psi)[at];
        bad |= !(v >= 0.0) || !(v / smin <= 1.7976931348623157e308);   // NaN, negative, infinite (after the division by sd2 too)
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(rec + 3, 1u);
}

template <typename T>
__global__ __launch_bounds__(256) void k_pred_stage_psi(const T *__restrict__ Psi, long rs, long cs, long r0, int nt, int d,
                                                        const double *__restrict__ sd2, double *__restrict__ Psic, long ldx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const T *row = Psi + (r0 + i) * rs;
    for (int c = 0; c < d; ++c) {
        double v = (double)row[c * cs];
        if (sd2) v = v / sd2[c];
        Psic[(size_t)c * ldx + i] = v;
    }
}

__global__ __launch_bounds__(256) void k_pred_finish_noisy_dev(const double *__restrict__ out, int nt, int k, const double *__restrict__ muY,
                                                               long ns, long r0, double *__restrict__ mu, double *__restrict__ sigma,
                                                               double *__restrict__ nu, double *__restrict__ beta,
                                                               double *__restrict__ gamma) {
    const int i = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
    if (i >= nt) return;
    const double m = out[(size_t)o * nt + i], v = out[(size_t)(k + o) * nt + i], b = out[(size_t)(2 * k + o) * nt + i],
                 g = out[(size_t)(3 * k + o) * nt + i];
    const size_t at = (size_t)o * ns + r0 + i;
    mu[at] = muY ? m + muY[o] : m;
    nu[at] = v;
    beta[at] = b;
    if (gamma) gamma[at] = g;
    if (sigma) sigma[at] = v + b + g;
}

int launch_pnm_check_psi(hipStream_t st, const void *Psi, int f32, long ns, int d, long rs, long cs, unsigned obs, double smin,
                         unsigned *rec) {
    if (ns <= 0 || obs == 0) return 0;   // nothing observed: Psi is not read at all
    const int dc = (cs == 0) ? 1 : d;    // a broadcast column: once per row
    long nb = (ns * dc + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_pred_check_psi, dim3((unsigned)nb), dim3(256), 0, st, Psi, f32, ns, dc, rs, cs, obs, smin, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pred_check_psi(hipStream_t st, const void *Psi, int f32, long ns, int d, long rs, long cs, double smin, unsigned *rec) {
    return launch_pnm_check_psi(st, Psi, f32, ns, d, rs, cs, ~0u, smin, rec);
}

int launch_pred_stage_psi(hipStream_t st, const void *Psi, int f32, long rs, long cs, long r0, int nt, int d, const double *sd2,
                          double *Psic, long ldx) {
    if (nt <= 0) return 0;
    const dim3 grid((unsigned)((nt + 255) / 256));
    if (f32) hipLaunchKernelGGL(k_pred_stage_psi<float>, grid, dim3(256), 0, st, (const float *)Psi, rs, cs, r0, nt, d, sd2, Psic, ldx);
    else hipLaunchKernelGGL(k_pred_stage_psi<double>, grid, dim3(256), 0, st, (const double *)Psi, rs, cs, r0, nt, d, sd2, Psic, ldx);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pred_finish_noisy_dev(hipStream_t st, const double *out, int nt, int k, const double *muY, long ns, long r0, double *mu,
                                 double *sigma, double *nu, double *beta, double *gamma) {
    if (nt <= 0) return 0;
    hipLaunchKernelGGL(k_pred_finish_noisy_dev, dim3((unsigned)((nt + 255) / 256), (unsigned)k), dim3(256), 0, st, out, nt, k, muY, ns, r0,
                       mu, sigma, nu, beta, gamma);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
