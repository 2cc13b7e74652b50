// Rows with missing inputs through the streaming predictor, covariance kinds (gpz_predictor_run_missing_cov_dev / _draws_missing_cov_dev,
// gpz_predictor.hip): predictMissing of GC and VC (predictCov.m:134-232) for one tile of ONE group of rows that share a NaN pattern.  The
// pattern is a bit mask of the observed dimensions; o = observed (no of them), u = missing (nu = d - no).  k_pmiss_cov.hip is the
// statement of the mathematics and gpz_predict_missing the parity partner; this unit is the same sums in another form.
//
// Every density of predictMissing is N(X_hat_l(x) - c ; C + Psi_hat_l) with X_hat_l affine in the row's observed inputs x_o (the identity
// on o, P_l,u + R_l' (x_o - P_l,o) on u) and Psi_hat_l = CU_l, the Schur complement of Sigma_l on (u, u), whatever the row is.  So the
// exponent is a quadratic in x_o alone and a record (centre r, component l) is written once per pattern as
//     -1/2 q = lnw - 1/2 |U (x_o - a)|^2,      rec = [lnw | a (no) | U upper triangle by rows (no (no + 1) / 2)]
// With S = C + Psi_hat_l = L L', T = [I; R_l'] and s the offset of the affine form, the whitened map A = L^-1 T and b = L^-1 s go through
// a modified Gram-Schmidt of [A | b]: U is its triangle, U a = -Q1' b, and h = |b - Q1 Q1' b|^2 is what no x_o can remove.  h is formed
// as that sum of squares, never as a difference of two quadratic forms.  lnw = lnw0 - 1/2 ln|S| - 1/2 h with lnw0 = ln prior_l (Ex),
// lnz_i (PHI) or lnZ_ab (the pairs).  Per density the tile kernels then spend no (no + 3) / 2 multiply-adds and one exp, with x_o in
// registers: nothing depends on d or on which dimensions are missing, only on no.
//
// Per pattern and priors (pmcv_tables), kept on the handle:
//   k_pmcv_basis    per basis function l, from ONE Cholesky of Sigma_l permuted to [o | u]: R_l = L_oo'^-1 L_uo', CU_l = L_uu L_uu',
//                   off_l = P_l,u - R_l' P_l,o; and the Ex record of l (:167) with ln prior_l folded into lnw
//   k_pmcv_phirec   the m^2 PHI records (i, j): centre P_i, C = Sigma_i, component j, lnw0 = lnz_i                       (:178-220)
//   k_pmcv_coef     per pair the 3k coefficients of gpz_pair_coef: f w_a w_b, f v_a v_b, f iS(a, b); f = 2 off the diagonal, iS read at
//                   a >= b only (the doubled diagonal term of :212-216 never enters)
// Per tile, on Xc [d][ldx] as k_pred_stage left it (the missing dimensions are never read):
//   k_pmcv_ex<NO>   lane = row: Ex over the m records summed in index order, Pio [l][ldr] = Ex_l / sum (:167-171)
//   k_pmcv_phi<NO>  lane = row: PHI(i) = sum_j Pio_j z(rec_ij) in index order -> Phi [nrow][mp] as launch_tgemm takes it
//   k_pmcv_hd       hd [2k][ldh] = PHI w | PHI v, one wave per row
//   k_pmc_triples   one lane per (pair, component) record of a slab of whole pairs: centre c_ab, C = C_ab, lnw0 = lnZ_ab.  The table of
//                   all m (m + 1) / 2 x m records is never whole in memory: predict_missing_cov_slabs(m, no) slabs of at most 64 MB.
//                   Run-time loops over d and no with the d x d temporaries in scratch memory (about 2.4 KB a lane): it is off the hot
//                   path, one record per 16384 row-uses.
//   k_predict_missing_cov_pairs<NO, KM>   the hot one: 64 rows per workgroup, lane = row in each of four waves; the workgroup's Pio
//                   block [m][64] in dynamic LDS; the waves deal the chunk's pairs of the slab round-robin, each staging its pair's
//                   records through LDS 16 at a time and reading them as broadcasts; per pair the m components in index order, then 3 KM
//                   multiply-adds.  The four partials are added in wave order through LDS and the slab's sum is added to part
//                   [chunk][3k][ldp] behind the slabs before it.  gridDim.y = predict_missing_cov_chunks(m).
//   k_pmd_finish    (k_predict_missing.hip) the chunks in chunk order, VlnS -= ElnS^2, beta, gamma -= mu^2 -> out [4k][n].
// No atomics; every sum starts from zero in an order fixed by m and no.  A row's results depend on its own values and the model only:
// the same bits for any tile size, row order, company, position in its block and split into calls.
#include "gpz_dev.h"
#include "gpz_kernels.h"
#include "k_pmcv_density.h"   // PMCV_MAXD, PMCV_SB, PmcvPat, pmcv_pat, pmcv_density, PMCV_CASES

#define PMCV_ST 64                    // records per LDS stage of the Ex and PHI kernels
#define PMCV_SLAB_BYTES (64L << 20)   // most bytes of a slab of pair-component records

// ---- records ---------------------------------------------------------------------------------------------------------------------------
// S: n x n, lower triangle read, leading dimension PMCV_MAXD, destroyed.  V: columns 0 .. no - 1 the map, column no the offset, each of
// n values PMCV_MAXD apart, destroyed.  rec <- [lnw0 - 1/2 ln|S| - 1/2 h | a | U].
__device__ void pmcv_record(int n, int no, double *S, double *V, double lnw0, double *rec) {
    constexpr int LD = PMCV_MAXD;
    double hl = 0.0;
    for (int c = 0; c < n; ++c) {
        double p = S[c * LD + c];
        for (int q = 0; q < c; ++q) p = fma(-S[c * LD + q], S[c * LD + q], p);
        const double dd = sqrt(p);
        S[c * LD + c] = dd;
        hl += log(dd);
        for (int r = c + 1; r < n; ++r) {
            double s = S[r * LD + c];
            for (int q = 0; q < c; ++q) s = fma(-S[r * LD + q], S[c * LD + q], s);
            S[r * LD + c] = s / dd;
        }
    }
    for (int c = 0; c <= no; ++c)   // L^-1 [A | b]
        for (int r = 0; r < n; ++r) {
            double s = V[c * LD + r];
            for (int q = 0; q < r; ++q) s = fma(-S[r * LD + q], V[c * LD + q], s);
            V[c * LD + r] = s / S[r * LD + r];
        }
    double *a = rec + 1, *U = rec + 1 + no, g[PMCV_MAXD];
    int e = 0;
    for (int c = 0; c < no; ++c) {   // modified Gram-Schmidt; row c of U lies at U[e ...]
        double nn = 0.0;
        for (int r = 0; r < n; ++r) nn = fma(V[c * LD + r], V[c * LD + r], nn);
        const double nrm = sqrt(nn), inv = 1.0 / nrm;
        for (int r = 0; r < n; ++r) V[c * LD + r] *= inv;
        U[e++] = nrm;
        for (int c2 = c + 1; c2 <= no; ++c2) {
            double s = 0.0;
            for (int r = 0; r < n; ++r) s = fma(V[c * LD + r], V[c2 * LD + r], s);
            for (int r = 0; r < n; ++r) V[c2 * LD + r] = fma(-s, V[c * LD + r], V[c2 * LD + r]);
            if (c2 < no) U[e++] = s;
            else g[c] = s;
        }
    }
    double h = 0.0;
    for (int r = 0; r < n; ++r) h = fma(V[no * LD + r], V[no * LD + r], h);
    for (int r = no - 1; r >= 0; --r) {   // U a = -g
        const int row = r * no - r * (r - 1) / 2;
        double s = -g[r];
        for (int c = r + 1; c < no; ++c) s = fma(-U[row + (c - r)], a[c], s);
        a[r] = s / U[row];
    }
    rec[0] = lnw0 - hl - 0.5 * h;
}

// the record of centre cen (by dimension) with covariance Cm (d x d row-major) against component l (bas = [R | CU | off] of l)
__device__ void pmcv_cond_record(const PmcvPat &pt, const double *Cm, const double *cen, double lnw0, const double *bas, double *rec) {
    constexpr int LD = PMCV_MAXD;
    const int d = pt.d, no = pt.no, nu = pt.nu;
    const double *R = bas, *CU = bas + no * nu, *off = CU + nu * nu;
    double S[LD * LD], V[LD * LD];
    for (int a = 0; a < d; ++a) {
        const int pa = a < no ? pt.o[a] : pt.u[a - no];
        for (int b = 0; b <= a; ++b) {
            const int pb = b < no ? pt.o[b] : pt.u[b - no];
            S[a * LD + b] = Cm[pa * d + pb] + (b >= no ? CU[(a - no) * nu + (b - no)] : 0.0);
        }
        V[no * LD + a] = (a < no ? 0.0 : off[a - no]) - cen[pa];
        for (int c = 0; c < no; ++c) V[c * LD + a] = a < no ? (a == c ? 1.0 : 0.0) : R[c * nu + (a - no)];
    }
    pmcv_record(d, no, S, V, lnw0, rec);
}

__global__ __launch_bounds__(64) void k_pmcv_basis(PmcvPat pt, int m, int de, const double *__restrict__ P, const double *__restrict__ Sig,
                                                   const double *__restrict__ priors, double *__restrict__ bas, int nb,
                                                   double *__restrict__ exrec, int rl) {
    constexpr int LD = PMCV_MAXD;
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l >= m) return;
    const int d = pt.d, no = pt.no, nu = pt.nu;
    const double *Sg = Sig + (size_t)l * d * d, *p = P + (size_t)l * de;
    double L[LD * LD];
    for (int a = 0; a < d; ++a)
        for (int b = 0; b <= a; ++b) L[a * LD + b] = Sg[(a < no ? pt.o[a] : pt.u[a - no]) * d + (b < no ? pt.o[b] : pt.u[b - no])];
    for (int c = 0; c < d; ++c) {
        double q = L[c * LD + c];
        for (int t = 0; t < c; ++t) q = fma(-L[c * LD + t], L[c * LD + t], q);
        const double dd = sqrt(q);
        L[c * LD + c] = dd;
        for (int r = c + 1; r < d; ++r) {
            double s = L[r * LD + c];
            for (int t = 0; t < c; ++t) s = fma(-L[r * LD + t], L[c * LD + t], s);
            L[r * LD + c] = s / dd;
        }
    }
    double *R = bas + (size_t)l * nb, *CU = R + no * nu, *off = CU + nu * nu;
    for (int c = 0; c < nu; ++c) {   // L_oo' R(:, c) = L_uo(c, :)'                                              :172
        for (int a = no - 1; a >= 0; --a) {
            double s = L[(no + c) * LD + a];
            for (int t = a + 1; t < no; ++t) s = fma(-L[t * LD + a], R[t * nu + c], s);
            R[a * nu + c] = s / L[a * LD + a];
        }
        double s = p[pt.u[c]];
        for (int a = 0; a < no; ++a) s = fma(-R[a * nu + c], p[pt.o[a]], s);
        off[c] = s;
        for (int c2 = 0; c2 <= c; ++c2) {   // CU = L_uu L_uu'                                                     :174
            double t = 0.0;
            for (int q = 0; q <= c2; ++q) t = fma(L[(no + c) * LD + no + q], L[(no + c2) * LD + no + q], t);
            CU[c * nu + c2] = t;
            CU[c2 * nu + c] = t;
        }
    }
    double S[LD * LD], V[LD * LD];   // Ex: N(x_o - P_l,o ; Sigma_l,oo) prior_l                                       :167
    for (int a = 0; a < no; ++a) {
        for (int b = 0; b <= a; ++b) S[a * LD + b] = Sg[pt.o[a] * d + pt.o[b]];
        V[no * LD + a] = -p[pt.o[a]];
        for (int c = 0; c < no; ++c) V[c * LD + a] = a == c ? 1.0 : 0.0;
    }
    pmcv_record(no, no, S, V, log(priors ? priors[l] : 1.0 / m), exrec + (size_t)l * rl);
}

__global__ __launch_bounds__(64) void k_pmcv_phirec(PmcvPat pt, int m, int de, const double *__restrict__ P, const double *__restrict__ Sig,
                                                    const double *__restrict__ lnS, const double *__restrict__ bas, int nb,
                                                    double *__restrict__ phirec, int rl) {
    const long e = (long)blockIdx.x * 64 + threadIdx.x;
    if (e >= (long)m * m) return;
    const int i = (int)(e / m), j = (int)(e - (long)i * m);
    pmcv_cond_record(pt, Sig + (size_t)i * pt.d * pt.d, P + (size_t)i * de, 0.5 * lnS[i], bas + (size_t)j * nb, phirec + (size_t)e * rl);
}

__global__ __launch_bounds__(256) void k_pmcv_coef(long npair, int m, int k, const double *__restrict__ w, const double *__restrict__ v,
                                                   const double *__restrict__ iS, double *__restrict__ coef) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= npair) return;
    int i, j;
    gpz_pair_of(q, &i, &j);
    gpz_pair_coef(coef + (size_t)q * 3 * k, i, j, m, k, w, v, iS);
}

// records [0, cnt * m) of the slab that starts at pair q0; raw: launch_pair_table's [lnZ | c_ab | C_ab (d x d)]
__global__ __launch_bounds__(64) void k_pmc_triples(PmcvPat pt, long q0, long cnt, int m, const double *__restrict__ raw,
                                                    const double *__restrict__ bas, int nb, double *__restrict__ slab, int rl) {
    const long e = (long)blockIdx.x * 64 + threadIdx.x;
    if (e >= cnt * m) return;
    const long q = e / m;
    const int l = (int)(e - q * m);
    const double *t = raw + (size_t)(q0 + q) * (1 + pt.d + pt.d * pt.d);
    pmcv_cond_record(pt, t + 1 + pt.d, t + 1, t[0], bas + (size_t)l * nb, slab + (size_t)e * rl);
}

// ---- the tile kernels ------------------------------------------------------------------------------------------------------------------
struct PmcvArgs {
    const double *Xc; long ldx; int n;     // the tile's rows, [d][ldx]
    int oidx[PMCV_MAXD];                   // the observed dimensions in ascending order
    int m, k;
    double *Pio; long ldr;                 // [m][ldr]
    const double *rec;                     // Ex: m records; PHI: m * m; pairs: the slab
    double *Phi; int nrow, mp, ipc;        // PHI: [nrow][mp], basis functions per gridDim.y chunk
    const double *coef; long q0; int cnt, ppc;   // pairs: the slab's first pair, its pairs, pairs per chunk
    double *part; long ldp; int first;     // pairs: [chunks][3k][ldp]; first: the slab's sums are stored, not added
};

template <int NO>
__global__ __launch_bounds__(256) void k_pmcv_ex(PmcvArgs a) {
    constexpr int RL = 1 + NO + NO * (NO + 1) / 2;
    __shared__ double sT[PMCV_ST * RL];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + tid;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    double x[NO ? NO : 1];
#pragma unroll
    for (int c = 0; c < NO; ++c) x[c] = a.Xc[(size_t)a.oidx[c] * a.ldx + ic];
    double s = 0.0;
    for (int lb = 0; lb < a.m; lb += PMCV_ST) {
        const int nl = min(PMCV_ST, a.m - lb);
        __syncthreads();
        for (int t = tid; t < nl * RL; t += 256) sT[t] = a.rec[(size_t)lb * RL + t];
        __syncthreads();
#pragma unroll 1
        for (int e = 0; e < nl; ++e) {
            const double z = pmcv_density<NO>(sT + e * RL, x);
            s += z;                                                        // index order                          :169
            if (act) a.Pio[(size_t)(lb + e) * a.ldr + i] = z;
        }
    }
    if (!act) return;
    for (int l = 0; l < a.m; ++l) a.Pio[(size_t)l * a.ldr + i] /= s;       //                                      :171
}

template <int NO>
__global__ __launch_bounds__(256) void k_pmcv_phi(PmcvArgs a) {
    constexpr int RL = 1 + NO + NO * (NO + 1) / 2;
    __shared__ double sT[PMCV_ST * RL];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + tid;
    const bool act = i < a.n, st = i < a.nrow;   // rows n .. nrow - 1 are written as zeros
    const long ic = act ? i : a.n - 1;
    double x[NO ? NO : 1];
#pragma unroll
    for (int c = 0; c < NO; ++c) x[c] = a.Xc[(size_t)a.oidx[c] * a.ldx + ic];
    double *row = a.Phi + (size_t)(st ? i : 0) * a.mp;
    const int i0 = blockIdx.y * a.ipc, i1 = min(a.m, i0 + a.ipc);
    for (int b = i0; b < i1; ++b) {
        double z = 0.0;
        for (int lb = 0; lb < a.m; lb += PMCV_ST) {
            const int nl = min(PMCV_ST, a.m - lb);
            const double *src = a.rec + ((size_t)b * a.m + lb) * RL;
            __syncthreads();
            for (int t = tid; t < nl * RL; t += 256) sT[t] = src[t];
            __syncthreads();
#pragma unroll 1
            for (int e = 0; e < nl; ++e) z = fma(a.Pio[(size_t)(lb + e) * a.ldr + ic], pmcv_density<NO>(sT + e * RL, x), z);
        }
        if (st) row[b] = act ? z : 0.0;
    }
    if (blockIdx.y == 0 && st)
        for (int j = a.m; j < a.mp; ++j) row[j] = 0.0;
}

// hd [2k][ldh] = PHI w | PHI v; one wave per row
__global__ __launch_bounds__(256) void k_pmcv_hd(const double *__restrict__ Phi, int n, int m, int mp, int k, const double *__restrict__ w,
                                                 const double *__restrict__ v, double *__restrict__ hd, long ldh) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const double *ph = Phi + (size_t)i * mp;
    for (int o = 0; o < k; ++o) {
        double s = 0.0, b = 0.0;
        for (int j = lane; j < m; j += 64) {
            const double f = ph[j];
            s = fma(f, w[j + (size_t)m * o], s);
            if (v) b = fma(f, v[j + (size_t)m * o], b);
        }
        s = wave_sum(s);
        b = wave_sum(b);
        if (lane == 0) {
            hd[(size_t)o * ldh + i] = s;
            hd[(size_t)(k + o) * ldh + i] = b;
        }
    }
}

template <int NO, int KM>
__global__ __launch_bounds__(256) void k_predict_missing_cov_pairs(PmcvArgs a) {
    constexpr int RL = 1 + NO + NO * (NO + 1) / 2;
    extern __shared__ double sm[];
    double *sPio = sm;                                   // [m][64]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, m = a.m, k = a.k;
    double *sRec = sm + (size_t)m * 64 + (size_t)w * (PMCV_SB * RL);   // this wave's stage
    const long row0 = (long)blockIdx.x * 64, i = row0 + lane;
    const bool act = i < a.n;
    const long ic = act ? i : a.n - 1;
    for (int e = tid; e < m * 64; e += 256) {
        const long r = min(row0 + (e & 63), (long)a.n - 1);
        sPio[e] = a.Pio[(size_t)(e >> 6) * a.ldr + r];
    }
    double x[NO ? NO : 1];
#pragma unroll
    for (int c = 0; c < NO; ++c) x[c] = a.Xc[(size_t)a.oidx[c] * a.ldx + ic];
    double acc[3 * KM];
#pragma unroll
    for (int e = 0; e < 3 * KM; ++e) acc[e] = 0.0;
    const int ch = blockIdx.y, p0 = ch * a.ppc, p1 = min(a.cnt, p0 + a.ppc);
    for (int pb = p0; pb < p1; pb += 4) {                // the four waves take pairs pb .. pb + 3
        const int p = pb + w;
        const bool on = p < p1;
        const double *src = a.rec + (size_t)(on ? p : p0) * m * RL;
        double z = 0.0;
        for (int lb = 0; lb < m; lb += PMCV_SB) {
            const int nl = min(PMCV_SB, m - lb);
            __syncthreads();                             // the stage before is read (and, the first time, sPio is written)
            if (on)
                for (int t = lane; t < nl * RL; t += 64) sRec[t] = src[(size_t)lb * RL + t];
            __syncthreads();
            if (on) {
#pragma unroll 2
                for (int e = 0; e < nl; ++e) z = fma(sPio[(lb + e) * 64 + lane], pmcv_density<NO>(sRec + e * RL, x), z);
            }
        }
        if (on) {
            const double *cf = a.coef + (size_t)(a.q0 + p) * 3 * k;
#pragma unroll
            for (int o = 0; o < KM; ++o)
                if (o < k) {
                    acc[o] = fma(z, cf[3 * o], acc[o]);                    // gamma                                :183-216
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
bool predict_missing_cov_fits(int kind, int d, int m, int k) {
    return kind == GPZ_KIND_COV && d >= 1 && d <= PMCV_MAXD && k >= 1 && k <= 8 && m >= 1 && ((m + 15) / 16) * 16 <= 256;
}

int predict_missing_cov_rec(int no) { return 1 + no + no * (no + 1) / 2; }

int predict_missing_cov_bas(int d, int no) { return (d - no) * (d + 1); }   // R (no x nu) | CU (nu x nu) | off (nu)

// chunks of a slab's pairs over gridDim.y: the largest power of two <= pairs / 32, between 1 and 16.  m alone, never the rows.
int predict_missing_cov_chunks(int m) {
    const long npair = (long)m * (m + 1) / 2;
    int c = 1;
    while (c < 16 && 2L * c * 32 <= npair) c *= 2;
    return c;
}

// slabs of whole pairs: the smallest power of two S such that ceil(pairs / S) pairs of m records are at most 64 MB.  m and no alone.
int predict_missing_cov_slabs(int m, int no) {
    const long npair = (long)m * (m + 1) / 2, per = (long)m * predict_missing_cov_rec(no) * (long)sizeof(double);
    int s = 1;
    while (((npair + s - 1) / s) * per > PMCV_SLAB_BYTES) s *= 2;
    return s;
}

long predict_missing_cov_slab_pairs(int m, int no) {
    const long npair = (long)m * (m + 1) / 2, s = predict_missing_cov_slabs(m, no);
    return (npair + s - 1) / s;
}

// dynamic LDS of the pair kernel, bytes: the Pio block and four stages of records, at least the three partials of the last reduction
size_t predict_missing_cov_lds(int m, int no, int k) {
    const size_t work = (size_t)m * 64 + 4 * (size_t)PMCV_SB * predict_missing_cov_rec(no), red = 3 * 64 * 3 * (size_t)(k == 1 ? 1 : 8);
    return (work > red ? work : red) * sizeof(double);
}

int launch_pmcv_tables(hipStream_t st, int m, int d, int de, int k, unsigned obs, const double *P, const double *Sig, const double *lnS,
                       const double *priors, const double *w, const double *v, const double *iS, double *bas, double *exrec,
                       double *phirec, double *coef) {
    const PmcvPat pt = pmcv_pat(d, obs);
    const int nb = predict_missing_cov_bas(d, pt.no), rl = predict_missing_cov_rec(pt.no);
    hipLaunchKernelGGL(k_pmcv_basis, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, pt, m, de, P, Sig, priors, bas, nb, exrec, rl);
    hipLaunchKernelGGL(k_pmcv_phirec, dim3((unsigned)(((long)m * m + 63) / 64)), dim3(64), 0, st, pt, m, de, P, Sig, lnS,
                       (const double *)bas, nb, phirec, rl);
    if (coef) {
        const long npair = (long)m * (m + 1) / 2;
        hipLaunchKernelGGL(k_pmcv_coef, dim3((unsigned)((npair + 255) / 256)), dim3(256), 0, st, npair, m, k, w, v, iS, coef);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

static PmcvArgs pmcv_args(const PmcvPat &pt, const double *Xc, long ldx, int n, int m, int k, double *Pio, long ldr, const double *rec) {
    PmcvArgs a{};
    a.Xc = Xc; a.ldx = ldx; a.n = n; a.m = m; a.k = k; a.Pio = Pio; a.ldr = ldr; a.rec = rec;
    for (int c = 0; c < pt.no; ++c) a.oidx[c] = pt.o[c];
    return a;
}

// hd [2k][ldh] = PHI w | PHI v of n rows (k_pmcv_hd), for the units that build PHI of a group themselves
int launch_pmcv_hd(hipStream_t st, const double *Phi, int n, int m, int mp, int k, const double *w, const double *v, double *hd, long ldh) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_pmcv_hd, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, Phi, n, m, mp, k, w, v, hd, ldh);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pmcv_rows(hipStream_t st, const double *Xc, long ldx, int n, int nrow, int m, int mp, int d, int k, unsigned obs,
                     const double *exrec, const double *phirec, const double *w, const double *v, double *Pio, long ldr, double *Phi,
                     double *hd, long ldh) {
    if (n <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || m < 1 || nrow < n || mp < m || ldr < n) return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    PmcvArgs a = pmcv_args(pt, Xc, ldx, n, m, k, Pio, ldr, exrec);
    PmcvArgs b = a;
    b.rec = phirec; b.Phi = Phi; b.nrow = nrow; b.mp = mp; b.ipc = 8;
    const dim3 ge((unsigned)((n + 255) / 256)), gp((unsigned)((nrow + 255) / 256), (unsigned)((m + b.ipc - 1) / b.ipc));
#define PMCV_ROWS(NN)                                                          \
    do {                                                                       \
        hipLaunchKernelGGL(k_pmcv_ex<NN>, ge, dim3(256), 0, st, a);            \
        hipLaunchKernelGGL(k_pmcv_phi<NN>, gp, dim3(256), 0, st, b);           \
    } while (0)
    PMCV_CASES(PMCV_ROWS)
#undef PMCV_ROWS
    if (hipGetLastError() != hipSuccess) return -1;
    return launch_pmcv_hd(st, Phi, n, m, mp, k, w, v, hd, ldh);
}

// records [0, cnt * m) of the slab that starts at pair q0 (k_pmc_triples), for the units that read a slab without the pair kernel
int launch_pmc_triples(hipStream_t st, int d, unsigned obs, long q0, long cnt, int m, const double *raw, const double *bas, double *slab) {
    if (cnt <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || m < 1) return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    hipLaunchKernelGGL(k_pmc_triples, dim3((unsigned)((cnt * m + 63) / 64)), dim3(64), 0, st, pt, q0, cnt, m, raw, bas,
                       predict_missing_cov_bas(d, pt.no), slab, predict_missing_cov_rec(pt.no));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// per launch, not once per process: the attribute belongs to the current device's copy of the kernel
template <int NO, int KM>
static int pmcv_launch_pairs(hipStream_t st, dim3 grid, size_t lds, const PmcvArgs &a) {
    if (lds > 65536 && hipFuncSetAttribute((const void *)k_predict_missing_cov_pairs<NO, KM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds) != hipSuccess)
        return -1;
    hipLaunchKernelGGL((k_predict_missing_cov_pairs<NO, KM>), grid, dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_predict_missing_cov_pairs(hipStream_t st, const double *Xc, long ldx, int n, const double *Pio, long ldr, int m, int d, int k,
                                     unsigned obs, const double *raw, const double *bas, const double *coef, double *slab,
                                     bool *slab_kept, int nchunk, double *part, long ldp, const double *hd, long ldh, const double *bvec,
                                     double *out) {
    if (n <= 0) return 0;
    if (d < 1 || d > PMCV_MAXD || k < 1 || k > 8 || m < 1 || ((m + 15) / 16) * 16 > 256 || nchunk != predict_missing_cov_chunks(m) ||
        ldr < n || ldp < n)
        return -1;
    const PmcvPat pt = pmcv_pat(d, obs);
    if (pt.nu < 1) return -1;
    const int nb = predict_missing_cov_bas(d, pt.no), rl = predict_missing_cov_rec(pt.no), nslab = predict_missing_cov_slabs(m, pt.no);
    const long npair = (long)m * (m + 1) / 2, sp = predict_missing_cov_slab_pairs(m, pt.no);
    PmcvArgs a = pmcv_args(pt, Xc, ldx, n, m, k, const_cast<double *>(Pio), ldr, slab);
    a.coef = coef; a.part = part; a.ldp = ldp;
    const size_t lds = predict_missing_cov_lds(m, pt.no, k);
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)nchunk);
    for (int s = 0; s < nslab; ++s) {
        const long q0 = s * sp, cnt = (npair - q0 < sp) ? npair - q0 : sp;
        if (cnt <= 0) break;
        if (!(nslab == 1 && *slab_kept)) {   // the whole table is one slab: it stays until the pattern's tables change
            hipLaunchKernelGGL(k_pmc_triples, dim3((unsigned)((cnt * m + 63) / 64)), dim3(64), 0, st, pt, q0, cnt, m, raw, bas, nb, slab, rl);
            if (hipGetLastError() != hipSuccess) return -1;
        }
        a.q0 = q0; a.cnt = (int)cnt; a.ppc = (int)((cnt + nchunk - 1) / nchunk); a.first = s == 0;
        int rc;
#define PMCV_PAIRS(NN) rc = k == 1 ? pmcv_launch_pairs<NN, 1>(st, grid, lds, a) : pmcv_launch_pairs<NN, 8>(st, grid, lds, a)
        PMCV_CASES(PMCV_PAIRS)
#undef PMCV_PAIRS
        if (rc) return -1;
    }
    *slab_kept = nslab == 1;
    return launch_pmd_finish(st, part, nchunk, ldp, hd, ldh, n, k, bvec, out);
}
