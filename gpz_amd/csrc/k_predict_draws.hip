// Posterior draws of the predictive mean for FEW basis functions as ONE kernel (gfx950, v_mfma_f64_16x16x4_f64): the hot path of
// gpz_predictor_draws (gpz_predictor.hip).
//
//   w_s ~ N(w, iSigma_w):  W_o(:, s) = w(:, o) + R_o z(:, s, o),  R_o R_o' = (iSigma_w(:,:,o) + iSigma_w(:,:,o)') / 2
//   F(i, o, s) = PHI(i, :) W_o(:, s)
//
// The n_draws * k columns of W = [W_0 | W_1 | ...] (nk = ceil16(m) rows, rows >= m zero) are formed once per call by k_draws_weights.
// With nk <= 256 a workgroup holds PHI of 32 rows in LDS, so only the draws (n_draws * k doubles per row) leave the kernel:
//   * workgroups are PERSISTENT (two per compute unit: <= 72 KB of dynamic LDS each) and walk blocks of 32 rows;
//   * PHI of the block is built in LDS by k_predict_small's code (k_predict_phi.h: the same bits per element);
//   * the columns are taken in chunks of at most 256 (16 column blocks); per chunk one K loop over nk against the LDS block, W streaming
//     from L2 one K step ahead;
//   * the product is taken TRANSPOSED, F' = W' PHI' (W as the A operand, PHI as the B operand), so that lane l of an accumulator holds
//     row (l & 15) of the strip: every store of the epilogue writes 16 consecutive rows of 4 columns of the [column][row] output;
//   * wave w owns column blocks w, w + 4, w + 8, w + 12 of the chunk for both 16-row strips; a chunk of fewer than 4 blocks is dealt
//     by (strip, block) instead, so that all four waves have work at small n_draws * k.
// No atomics, and every output element is one MFMA chain over K in a fixed order from zero: a row's draws have the same bits whatever
// its tile, its position in the tile, its chunk or the number of draws asked for.
#include "gpz_dev.h"
#include "gpz_kernels.h"

#define PS_LDA 262   // row stride of the PHI block in LDS (doubles): 2 (mod 4) - the 16 rows of an A-operand read start 4 banks apart
// PredDrawsArgs and k_predict_draws<D, COV> itself (with the deal of a chunk, `const bool split = nbc < 4;`) are in
// k_predict_draws_impl.h: the input-noise draws of k_predict_noisy.hip are the same text behind a PHI block built from X and Psi.
#include "k_predict_draws_impl.h"

size_t predict_draws_lds(int de) { return ((size_t)32 * PS_LDA + 32 * (size_t)de) * sizeof(double); }

bool predict_draws_fits(int de, int m) {
    if (phi_is_wide(de, 1) || !ps_width_instantiated(de)) return false;
    return ((m + 15) / 16) * 16 <= 256 && predict_draws_lds(de) <= 80 * 1024;
}

template <int D, bool COV>
static int launch_pd(hipStream_t st, const PredDrawsArgs &a, int nwg) {
    const size_t lds = predict_draws_lds(D);
    // per launch, not once per process: the attribute belongs to the current device's copy of the kernel
    if (hipFuncSetAttribute((const void *)k_predict_draws<D, COV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -1;
    hipLaunchKernelGGL((k_predict_draws<D, COV>), dim3(nwg), dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
template <bool COV>
static int launch_pd_k(hipStream_t st, int de, const PredDrawsArgs &a, int nwg) {
    switch (de) {
        case 1: return launch_pd<1, COV>(st, a, nwg);
        case 2: return launch_pd<2, COV>(st, a, nwg);
        case 3: return launch_pd<3, COV>(st, a, nwg);
        case 4: return launch_pd<4, COV>(st, a, nwg);
        case 5: return launch_pd<5, COV>(st, a, nwg);
        case 6: return launch_pd<6, COV>(st, a, nwg);
        case 8: return launch_pd<8, COV>(st, a, nwg);
        case 10: return launch_pd<10, COV>(st, a, nwg);
        case 12: return launch_pd<12, COV>(st, a, nwg);
        case 16: return launch_pd<16, COV>(st, a, nwg);
        case 20: return launch_pd<20, COV>(st, a, nwg);
        default: return -1;
    }
}

int launch_predict_draws(hipStream_t st, int kind, int de, const double *Xc, long ldx, int n, int m, const double *P, const double *G,
                         const double *W, int ldw, int ncol, double *out, long ldo) {
    if (n <= 0) return 0;
    PredDrawsArgs a{};
    a.Xc = Xc; a.ldx = ldx; a.n = n; a.m = m; a.nk = ((m + 15) / 16) * 16;
    a.ncol = ncol; a.nbw = ldw / 16; a.P = P; a.G = G; a.W = W; a.ldw = ldw; a.out = out; a.ldo = ldo;
    const int nblocks = (n + 31) / 32;
    int nwg = 2 * gpz_cu_count();
    if (nwg > nblocks) nwg = nblocks;
    return kind == GPZ_KIND_COV ? launch_pd_k<true>(st, de, a, nwg) : launch_pd_k<false>(st, de, a, nwg);
}

// ---- standard normals: Philox4x32-10 (Random123's round and key schedule) + Box-Muller -------------------------------------------------
__device__ __forceinline__ double draws_normal(unsigned long long seed, unsigned j, unsigned s, unsigned o) {
    unsigned c0 = j, c1 = s, c2 = o, c3 = 0u;
    unsigned k0 = (unsigned)(seed & 0xffffffffull), k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
    }
    const double u1 = (double)(((((unsigned long long)c1 << 32) | c0) >> 11) + 1ull) * 0x1.0p-53;   // (0, 1]
    const double u2 = (double)((((unsigned long long)c3 << 32) | c2) >> 11) * 0x1.0p-53;           // [0, 1)
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
}

// W (rows x ldw row-major) <- [W_0 | W_1 | ... | 0]: column c = o * nd + s < ncol = nd * k holds w(:, o) + R_o z(:, s, o), rows >= m and
// columns >= ncol zero.  z from the caller's Z (m x nd x k column-major) or, Z == nullptr, from Philox of (seed, j, s, o).  R: m x m x k
// column-major.  One workgroup per column; z of the column in LDS (m doubles of dynamic LDS).  The sum over l runs in ascending order.
__global__ __launch_bounds__(256) void k_draws_weights(const double *__restrict__ w, const double *__restrict__ R,
                                                       const double *__restrict__ Z, unsigned long long seed, int m, int nd, int ncol,
                                                       int rows, int ldw, double *__restrict__ W) {
    extern __shared__ double zs[];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (c >= ncol) {
        for (int j = tid; j < rows; j += 256) W[(size_t)j * ldw + c] = 0.0;
        return;
    }
    const int o = c / nd, s = c % nd;
    for (int l = tid; l < m; l += 256) zs[l] = Z ? Z[(size_t)l + (size_t)m * ((size_t)s + (size_t)nd * o)] : draws_normal(seed, l, s, o);
    __syncthreads();
    const double *Ro = R + (size_t)o * m * m;
    for (int j = tid; j < rows; j += 256) {
        double v = 0.0;
        if (j < m) {
            double t = 0.0;
            for (int l = 0; l < m; ++l) t = fma(Ro[(size_t)j + (size_t)m * l], zs[l], t);
            v = w[(size_t)j + (size_t)m * o] + t;
        }
        W[(size_t)j * ldw + c] = v;
    }
}
void launch_draws_weights(hipStream_t st, const double *w, const double *R, const double *Z, unsigned long long seed, int m, int nd,
                          int k, int rows, int ldw, double *W) {
    hipLaunchKernelGGL(k_draws_weights, dim3(ldw), dim3(256), (size_t)m * sizeof(double), st, w, R, Z, seed, m, nd, nd * k, rows, ldw, W);
}

// ---- the factor R_o -----------------------------------------------------------------------------------------------------------
// S (m x m) <- (iS + iS') / 2 and A (mq x mq row-major) <- S with the identity on the padding (k_chol_step's input)
__global__ void k_draws_sym(const double *__restrict__ iS, int m, int mq, double *__restrict__ S, double *__restrict__ A) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= mq) return;
    double v = (i == j) ? 1.0 : 0.0;
    if (i < m && j < m) {
        v = 0.5 * (iS[(size_t)i + (size_t)m * j] + iS[(size_t)j + (size_t)m * i]);
        S[(size_t)i * m + j] = v;
    }
    A[(size_t)i * mq + j] = v;
}
void launch_draws_sym(hipStream_t st, const double *iS, int m, int mq, double *S, double *A) {
    hipLaunchKernelGGL(k_draws_sym, dim3((mq + 255) / 256, mq), dim3(256), 0, st, iS, m, mq, S, A);
}

// After the Cholesky steps: R (m x m column-major) <- the lower factor of Lm (mq x mq row-major; its upper blocks are never read), and
// *ok = 1 when no pivot was reported and min_j L_jj^2 > m eps max_j S_jj (j < m), else 0 (a NaN pivot counts as a breakdown).
__global__ __launch_bounds__(256) void k_draws_chol_check(const double *__restrict__ Lm, int mq, const double *__restrict__ S, int m,
                                                          const int *__restrict__ info, double *__restrict__ R, int *__restrict__ ok) {
    const int j = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < m; i += 256) R[(size_t)i + (size_t)m * j] = i >= j ? Lm[(size_t)i * mq + j] : 0.0;
    if (j != 0) return;
    __shared__ double sh[2][4];
    double mn = __builtin_inf(), mx = 0.0;
    int nan = 0;
    for (int i = tid; i < m; i += 256) {
        const double l = Lm[(size_t)i * mq + i], l2 = l * l;
        nan |= !(l2 == l2);
        mn = fmin(mn, l2);
        mx = fmax(mx, S[(size_t)i * m + i]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, off, 64));
        mx = fmax(mx, __shfl_xor(mx, off, 64));
    }
    nan = __any(nan);
    __shared__ int shn[4];
    if ((tid & 63) == 0) { sh[0][tid >> 6] = mn; sh[1][tid >> 6] = mx; shn[tid >> 6] = nan; }
    __syncthreads();
    if (tid == 0) {
        mn = fmin(fmin(sh[0][0], sh[0][1]), fmin(sh[0][2], sh[0][3]));
        mx = fmax(fmax(sh[1][0], sh[1][1]), fmax(sh[1][2], sh[1][3]));
        nan = shn[0] | shn[1] | shn[2] | shn[3];
        *ok = (info[0] == 0 && !nan && mn > (double)m * 2.220446049250313e-16 * mx) ? 1 : 0;
    }
}
void launch_draws_chol_check(hipStream_t st, const double *Lm, int mq, const double *S, int m, const int *info, double *R, int *ok) {
    hipLaunchKernelGGL(k_draws_chol_check, dim3(m), dim3(256), 0, st, Lm, mq, S, m, info, R, ok);
}
