// Rows with input noise through the streaming predictor, covariance kinds (gpz_predictor_run_noisy_cov_dev / _draws_noisy_cov_dev,
// gpz_predictor.hip): predictNoisy of GC and VC (predictCov.m:70-132) for one tile as ONE kernel plus the finish kernel of the diagonal
// kinds (k_predict_noisy_finish, k_predict_noisy.hip), and E_x[PHI] of a tile for the draws.  Psi is a variance per input dimension in
// the layout of Xc: the diagonal that fixPsi puts into the d x d x n cube of these kinds.
//
//   k_predict_noisy_cov_small<D, SHARED, KM>   predict_ncov_small_body (k_predict_ncov_impl.h: the frame, the records, the chunks and
//   k_predict_noisy_cov_phi<D, SHARED>         the order of every sum) and predict_ncov_phi_body with PsiDiag<D>: M = S + diag(psi_i)
//   k_noisy_cov_records
//       once per handle: Sigma_j and ln|Sigma_j| (launch_gen_prep) and the pair records of launch_pair_table(GPZ_KIND_COV), d x d
//       row-major, repacked into the records of that frame and completed with the weights and gpz_pair_coef's coefficients.
// The chunk count C = predict_noisy_cov_chunks(m, d, k) depends on the model's shape only.
#include "k_predict_ncov_impl.h"

template <int D, bool SHARED, int KM>
__global__ __launch_bounds__(256) void k_predict_noisy_cov_small(PredNcovArgs a) {
    predict_ncov_small_body<PsiDiag<D>, SHARED, KM>(a);
}

template <int D, bool SHARED>
__global__ __launch_bounds__(256) void k_predict_noisy_cov_phi(PredNcovArgs a) {
    predict_ncov_phi_body<PsiDiag<D>, SHARED>(a);
}

__global__ __launch_bounds__(256) void k_noisy_cov_records(int m, int d, int de, int k, const double *__restrict__ P,
                                                           const double *__restrict__ Sig, const double *__restrict__ lnS,
                                                           const double *__restrict__ raw, const double *__restrict__ w,
                                                           const double *__restrict__ v, const double *__restrict__ iS,
                                                           double *__restrict__ brec, double *__restrict__ prec) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x, npair = (long)m * (m + 1) / 2;
    const int h = 1 + d + d * (d + 1) / 2;
    if (e < m) {
        double *o = brec + (size_t)e * (h + 2 * k);
        o[0] = 0.5 * lnS[e];
        for (int r = 0; r < d; ++r) {
            o[1 + r] = P[(size_t)e * de + r];
            for (int c = 0; c <= r; ++c) o[1 + d + LT(r, c)] = Sig[(size_t)e * d * d + r * d + c];
        }
        for (int q = 0; q < k; ++q) {
            o[h + q] = w[e + (size_t)m * q];
            o[h + k + q] = v ? v[e + (size_t)m * q] : 0.0;
        }
    }
    if (prec && e < npair) {
        const double *src = raw + (size_t)e * (1 + d + d * d);
        double *o = prec + (size_t)e * (h + 3 * k);
        o[0] = src[0];
        for (int r = 0; r < d; ++r) {
            o[1 + r] = src[1 + r];
            for (int c = 0; c <= r; ++c) o[1 + d + LT(r, c)] = src[1 + d + r * d + c];   // the lower triangle, as k_predict_noisy_cov reads it
        }
        int ia, ib;
        gpz_pair_of(e, &ia, &ib);                                          // f: 2x in the loop, 1x on the diagonal  (predictCov.m:113-119)
        gpz_pair_coef(o + h, ia, ib, m, k, w, v, iS);
    }
}

bool predict_noisy_cov_fits(int kind, int d, int m, int k, bool large_m) {
    return kind == GPZ_KIND_COV && d >= 1 && d <= 10 && k >= 1 && k <= 8 && m >= 1 &&
           ((m + 15) / 16) * 16 <= (large_m ? GPZ_PREDICT_LARGE_M_MAX : 256);
}

// pair chunks (= chunks of the basis functions): one per 2048 pairs, at most 4.  The model's shape only, never the rows.  The cap stays
// at 4 for 256 < ceil16(m) <= 1024 (GPZ_PREDICT_LARGE_M; no measurement decided that: see k_predict_noisy.hip).  At m = 1024 the
// 524 800 pairs and their record offsets (at most 524 800 * 90 doubles) fit 32 bits; the tables are addressed in size_t.
int predict_noisy_cov_chunks(int m, int d, int k) {
    (void)d; (void)k;
    const long c = ((long)m * (m + 1) / 2) / 2048;
    return (int)(c < 1 ? 1 : (c > 4 ? 4 : c));
}

int predict_noisy_cov_brec(int d, int k) { return 1 + d + d * (d + 1) / 2 + 2 * k; }
int predict_noisy_cov_prec(int d, int k) { return 1 + d + d * (d + 1) / 2 + 3 * k; }

int launch_noisy_cov_records(hipStream_t st, int m, int d, int de, int k, const double *P, const double *Sig, const double *lnS,
                             const double *raw, const double *w, const double *v, const double *iS, double *brec, double *prec) {
    const long items = prec ? (long)m * (m + 1) / 2 : (long)m;
    hipLaunchKernelGGL(k_noisy_cov_records, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, m, d, de, k, P, Sig, lnS, raw, w, v,
                       iS, brec, prec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

struct NoisyCovKernels {
    template <int D, bool SHARED, int KM> static auto small() { return k_predict_noisy_cov_small<D, SHARED, KM>; }
    template <int D, bool SHARED> static auto phi() { return k_predict_noisy_cov_phi<D, SHARED>; }
};

int launch_predict_noisy_cov_small(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m, int k,
                                   const double *brec, const double *prec, const double *bvec, int nchunk, double *part, long ldp,
                                   double *out) {
    return predict_ncov_launch_small<NoisyCovKernels>(st, d, shared, Xc, Psic, ldx, n, m, k, brec, prec, bvec, nchunk, part, ldp, out);
}

int launch_predict_noisy_cov_phi(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int nrow,
                                 int m, int mp, int k, const double *brec, int nchunk, double *Phi) {
    return predict_ncov_launch_phi<NoisyCovKernels>(st, d, shared, Xc, Psic, ldx, n, nrow, m, mp, k, brec, nchunk, Phi);
}
