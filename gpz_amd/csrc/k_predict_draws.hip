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
#include "k_predict_phi.h"

struct PredDrawsArgs {
    const double *Xc; long ldx;   // de x ldx column layout (the tile's rows; dimensions >= d are zero)
    int n;                        // rows of this tile
    int m, nk;                    // nk = ceil16(m): K of the product (PHI columns m .. nk - 1 are zero)
    int ncol, nbw;                // columns of F; 16-column blocks of W (nbw = ldw / 16)
    const double *P, *G;          // as k_predict_small
    const double *W; int ldw;     // nk x ldw row-major; columns >= ncol zero
    double *out; long ldo;        // [ncol][ldo]
};

template <int D, bool COV>
__global__ __launch_bounds__(256, 2) void k_predict_draws(PredDrawsArgs a) {
    extern __shared__ double smem[];
    double *sA = smem;                    // [32][PS_LDA]: PHI of the block
    double *sX = sA + 32 * PS_LDA;        // [32][D]: the block's rows of X
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = a.nk, nbw = a.nbw, ldw = a.ldw;
    const int nblocks = (a.n + 31) >> 5;
    const PsPhiBuilder<D, COV> phi(a.P, a.G, a.m, nk, tid);
    const int ks_n = nk >> 2;   // K steps of 4 (a multiple of 4)
    const double *wl = a.W + (size_t)(lane >> 4) * ldw + (lane & 15);
    for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long i0 = (long)blk * 32;
        __syncthreads();   // the previous block's K loops are done with sA
        ps_load_x<D>(a.Xc, a.ldx, a.n, i0, sX, tid);
        __syncthreads();
        phi.build(sA, sX, i0, a.n);
        __syncthreads();
        for (int cb = 0; cb < nbw; cb += 16) {
            const int nbc = nbw - cb < 16 ? nbw - cb : 16;
            // deal: both strips of blocks cb + wv + 4q, or (nbc < 4) strip wv & 1 of blocks cb + (wv >> 1) + 2q
            const bool split = nbc < 4;
            const int s0 = split ? (wv & 1) : 0;
            const int b0 = split ? (wv >> 1) : wv, bs = split ? 2 : 4;
            const int nq = __builtin_amdgcn_readfirstlane(nbc > b0 ? (nbc - b0 + bs - 1) / bs : 0);
            if (nq == 0) continue;
            const double *pa0 = sA + (16 * s0 + (lane & 15)) * PS_LDA + (lane >> 4);
            const double *pa1 = split ? pa0 : pa0 + 16 * PS_LDA;   // (split: not used)
            const double *wb = wl + (size_t)(cb + b0) * 16;
            d4_t acc[2][4];
            double ba[4], bb[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[0][q] = (d4_t){0.0, 0.0, 0.0, 0.0};
                acc[1][q] = (d4_t){0.0, 0.0, 0.0, 0.0};
                ba[q] = q < nq ? wb[q * bs * 16] : 0.0;
            }
            // two K steps per trip (ks_n is even): each step's W fragments are loaded while the step before it runs
            for (int ks = 0; ks < ks_n; ks += 2) {
                const double *w1 = wb + (size_t)(ks + 1) * 4 * ldw;
#pragma unroll
                for (int q = 0; q < 4; ++q) bb[q] = q < nq ? w1[q * bs * 16] : 0.0;
                {
                    const double a0 = pa0[4 * ks], a1 = pa1[4 * ks];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < nq) {
                            acc[0][q] = MFMA_F64(ba[q], a0, acc[0][q]);
                            if (!split) acc[1][q] = MFMA_F64(ba[q], a1, acc[1][q]);
                        }
                }
                if (ks + 2 < ks_n) {
                    const double *w2 = w1 + (size_t)4 * ldw;
#pragma unroll
                    for (int q = 0; q < 4; ++q) ba[q] = q < nq ? w2[q * bs * 16] : 0.0;
                }
                {
                    const double a0 = pa0[4 * ks + 4], a1 = pa1[4 * ks + 4];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < nq) {
                            acc[0][q] = MFMA_F64(bb[q], a0, acc[0][q]);
                            if (!split) acc[1][q] = MFMA_F64(bb[q], a1, acc[1][q]);
                        }
                }
            }
            // ---- epilogue: lane l, register r of strip s holds F[row = 16 s + (l & 15)][col = 16 gb + (l >> 4) + 4 r]
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (split && s == 1) break;
                const long row = i0 + 16 * (s + s0) + (lane & 15);
                if (row >= a.n) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < nq) {
                        const int gb = cb + b0 + q * bs;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int col = gb * 16 + (lane >> 4) + 4 * r;
                            if (col < a.ncol) a.out[(size_t)col * a.ldo + row] = acc[s][q][r];
                        }
                    }
            }
        }
    }
}

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
