// gamma under every weight draw for rows with a full input-noise covariance on a covariance kind (gpz_predictor_stack_psi_cube_dev /
// _draws_gamma_psi_cube_dev, gpz_predictor.hip): gamma_s,i = sum_{a >= b} f_ab z_ab(x_i, Psi_i) w_s,a w_s,b - mu_s,i^2 per output,
// predictNoisy's gamma of GC and VC (predictCov.m:105-119) with the draw's weights in place of w.
//
//   k_predict_psi_cube_gamma<D, SHARED>
//       predict_gamma_body (k_predict_gamma_impl.h: the f64 MFMA product of pair densities and weight products, its LDS stages, chunks
//       and passes) with GammaCube<D, SHARED>: k_predict_noisy_cov_gamma's policy with M = C_ab + Psi_i over the whole packed triangle
//       (ncov_factor_tri / ncov_density, k_ncov_density.h), the density of k_predict_psi_cube_small.  The row's triangle is the
//       d (d + 1) / 2 columns of the tile's Psic at the lane's row.
//       SHARED (GC): the body loads the triangle, init factorises C + Psi_i once from record 0 and nothing of it is live in the loop.
//       VC: in registers beside M up to D = GPZ_PSI_CUBE_REG_D (psi_cube_regs); above it z() reads the columns again at every K step
//       (the 16 rows of a wave are 128 contiguous bytes of a column).
//       pcg_blocks(D) 16-column blocks of accumulators per pass.
// k_gamma_finish_dev / k_gamma_finish_s2 (k_predict_noisy_gamma.hip) add the chunks and take mu_s^2 off.  The chunk count is the
// caller's predict_gamma_chunks(m).
#include "k_predict_gamma_impl.h"
#include "k_ncov_density.h"   // ncov_factor_tri, ncov_density, psi_cube_regs

// 16-column blocks of accumulators per pass: 8 (128 columns) up to d = 6, then 4 - one width earlier than k_predict_noisy_cov_gamma,
// so that d = 7 with the row's triangle beside M stays within 256 registers (two workgroups per compute unit)
constexpr int pcg_blocks(int d) { return d <= 6 ? 8 : 4; }

template <int DD, bool SHARED>
struct GammaCube {
    static constexpr int D = DD, NP = DD * (DD + 1) / 2, RL = 1 + DD + NP, NB = pcg_blocks(DD);
    static constexpr bool REG = SHARED || psi_cube_regs(DD);   // the body loads the triangle into the lane's registers
    static constexpr int PW = REG ? NP : 1;
    double M[NP], rd[DD], prd;
    const double *P;   // the lane's place in Psic, element q at P[q ldx]
    long ldx;
    __device__ __forceinline__ void bind(const double *P_, long ldx_) {
        if constexpr (!REG) { P = P_; ldx = ldx_; }
    }
    __device__ __forceinline__ void init(const double *tab, const double (&ps)[PW]) {
        if constexpr (SHARED) ncov_factor_tri<DD>(tab + 1 + DD, ps, 1, M, rd, &prd);   // C + Psi_i of the row, once       predictCov.m:109
    }
    __device__ __forceinline__ double z(const double *t, const double (&x)[DD], const double (&ps)[PW]) {
        if constexpr (!SHARED) {
            if constexpr (REG) ncov_factor_tri<DD>(t + 1 + DD, ps, 1, M, rd, &prd);     // Cij + Psi_i                     :109
            else ncov_factor_tri<DD>(t + 1 + DD, P, ldx, M, rd, &prd);
        }
        return ncov_density<DD>(t + 1, t[0], x, M, rd, prd);                            //                                 :111
    }
};

template <int D, bool SHARED>
__global__ __launch_bounds__(256) void k_predict_psi_cube_gamma(PredGammaArgs a) {
    predict_gamma_body<GammaCube<D, SHARED>>(a);
}

template <int D>
static void launch_pcg(hipStream_t st, const PredGammaArgs &a, int nchunk, bool shared) {
    const dim3 grid = predict_gamma_grid(a, nchunk, pcg_blocks(D));
    if (shared) hipLaunchKernelGGL((k_predict_psi_cube_gamma<D, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_predict_psi_cube_gamma<D, false>), grid, dim3(256), 0, st, a);
}

int launch_predict_psi_cube_gamma(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m,
                                  const double *tab, int rec, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp) {
    if (n <= 0 || ncol <= 0) return 0;
    if (d < 1 || d > 10 || m < 1 || nchunk < 1 || ldw % 16 || ncol > ldw || rec < 1 + d + d * (d + 1) / 2 || ldp < n || ldx < n) return -1;
    const PredGammaArgs a = predict_gamma_args(Xc, Psic, ldx, n, m, tab, rec, W, ldw, ncol, nchunk, part, ldp);
    switch (d) {
#define PCG_CASE(DD) case DD: launch_pcg<DD>(st, a, nchunk, shared); break;
        PCG_CASE(1) PCG_CASE(2) PCG_CASE(3) PCG_CASE(4) PCG_CASE(5) PCG_CASE(6) PCG_CASE(7) PCG_CASE(8) PCG_CASE(9) PCG_CASE(10)
#undef PCG_CASE
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
