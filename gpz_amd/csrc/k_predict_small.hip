// predictFull for FEW basis functions as ONE kernel (gfx950, v_mfma_f64_16x16x4_f64): the hot path of a streaming predictor
// (gpz_predictor.hip).
//
//   PHI_ij = exp(-1/2 q_ij)                                  getPHI.m:97,113 (the no-Psi, no-missing forms of k_phi_diag / k_phi_cov)
//   T = PHI [inv(Sigma_o) | w | v]                           predictDiag.m:65,69, predictCov.m:60,64
//   mu_io = T_i,m+o,  nu_io = sum_j<m PHI_ij T_ij,  beta_io = exp(T_i,m+k+o + b_o)     predictDiag.m:65-73, getPHI.m:119,124
//
// gpz_predict_full writes PHI and T (n x mp doubles each) to HBM and reads both back for nu.  With ceil16(m + 2k) <= 256 a workgroup
// holds whole rows of T in its accumulators - 32 rows x ceil16(m + 2k) columns over 4 waves - so only mu, nu and beta (3k doubles per
// row) leave the kernel:
//   * workgroups are PERSISTENT (two per compute unit: 72 KB of dynamic LDS each) and walk blocks of 32 rows;
//   * the block's rows of X go to LDS, PHI (32 x ceil16(m)) is built there once - thread (column j, row group g) keeps the parameters of
//     basis function j in registers and walks its rows - and serves as the A operand of every K step and as PHI_ij of the epilogue;
//   * B_o = [inv(Sigma_o) | w | v] (K = ceil16(m) rows, rows >= m zero) streams from L2 one K step ahead; wave w owns the 16-column blocks
//     w, w + 4, w + 8, w + 12 for both 16-row strips of the block;
//   * nu: each wave's partial row sums over its own columns (a DPP row sum over the 16 lanes of a block) meet in LDS and are added in
//     wave order; mu and ln beta are single accumulator elements;
//   * k > 1: one K loop per output against the same LDS block.
// No atomics, and nothing a row computes depends on its block, its tile or its position in the catalogue: the same row gives the same
// bits whatever the tile size.
#include "gpz_dev.h"
#include "gpz_kernels.h"

#define PS_LDA 262   // row stride of the PHI block in LDS (doubles): 2 (mod 4) - the 16 rows of an A-operand read start 4 banks apart
#include "k_predict_phi.h"

struct PredSmallArgs {
    const double *Xc; long ldx;   // de x ldx column layout (the tile's rows; dimensions >= d are zero)
    int n;                        // rows of this tile
    int m, k, nk;                 // nk = ceil16(m): K of the product (PHI columns m .. nk - 1 are zero)
    int nb;                       // 16-column blocks of B_o = ceil16(m + 2k) / 16
    const double *P, *G;          // P: m x de row-major; G: gamma^2 (diagonal kinds) or [R_j packed upper | R_j p_j] (covariance kinds)
    const double *B; int ldb; long bstride;   // B_o = B + o * bstride: nk x ldb row-major
    const double *bvec;           // k
    double *out; long ldo;        // [3k][ldo]: mu (o), nu (k + o), beta (2k + o) of the tile's rows
    double *phi; long ldphi;      // optional: PHI as [m][ldphi] (column-major rows x m)
};

__device__ __forceinline__ double ps_row_ror(double v, int n) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    int lo, hi;
    switch (n) {   // row_ror:n (DPP control 0x120 + n): rotate within the 16 lanes of a row
        case 8: lo = __builtin_amdgcn_update_dpp(0, (int)(u & 0xffffffffu), 0x128, 0xf, 0xf, false);
                hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), 0x128, 0xf, 0xf, false); break;
        case 4: lo = __builtin_amdgcn_update_dpp(0, (int)(u & 0xffffffffu), 0x124, 0xf, 0xf, false);
                hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), 0x124, 0xf, 0xf, false); break;
        case 2: lo = __builtin_amdgcn_update_dpp(0, (int)(u & 0xffffffffu), 0x122, 0xf, 0xf, false);
                hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), 0x122, 0xf, 0xf, false); break;
        default: lo = __builtin_amdgcn_update_dpp(0, (int)(u & 0xffffffffu), 0x121, 0xf, 0xf, false);
                 hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), 0x121, 0xf, 0xf, false); break;
    }
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// sum over the 16 lanes of a DPP row, the same value in every lane of the row (the order of the additions is the same in every row)
__device__ __forceinline__ double ps_row_sum16(double p) {
    p += ps_row_ror(p, 8);
    p += ps_row_ror(p, 4);
    p += ps_row_ror(p, 2);
    p += ps_row_ror(p, 1);
    return p;
}

// D = padded input dimension (a width k_phi_diag / k_phi_cov are instantiated for), COV = covariance kind
template <int D, bool COV>
__global__ __launch_bounds__(256, 2) void k_predict_small(PredSmallArgs a) {
    extern __shared__ double smem[];
    double *sA = smem;                    // [32][PS_LDA]: PHI of the block (covariance kinds: the running quadratic form first)
    double *sX = sA + 32 * PS_LDA;        // [32][D]: the block's rows of X
    double *sNu = sX + 32 * D;            // [4][32]: the waves' partial nu
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = a.m, k = a.k, nk = a.nk, nb = a.nb;
    const int nblocks = (a.n + 31) >> 5;
    // PHI build (k_predict_phi.h): thread (column j, row group g) keeps the parameters of basis function j in registers for the whole launch
    const PsPhiBuilder<D, COV> phi(a.P, a.G, m, nk, tid);
    // this wave's column blocks: gb = wv + 4 q, q < nqw
    const int nqw = (nb - wv + 3) >> 2;
    const int ks_n = nk >> 2;   // K steps of 4
    for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long i0 = (long)blk * 32;
        __syncthreads();   // the previous block's epilogue is done with sA / sX / sNu
        ps_load_x<D>(a.Xc, a.ldx, a.n, i0, sX, tid);
        __syncthreads();
        phi.build(sA, sX, i0, a.n);   // PHI of the block -> sA
        __syncthreads();
        if (a.phi) {   // PHI requested: 32 consecutive rows of a column per 32 lanes
            for (int e = tid; e < 32 * m; e += 256) {
                const int r = e & 31, j = e >> 5;
                if (i0 + r < a.n) a.phi[(size_t)j * a.ldphi + i0 + r] = sA[r * PS_LDA + j];
            }
        }
        const double *pa0 = sA + (lane & 15) * PS_LDA + (lane >> 4);
        const double *pa1 = pa0 + 16 * PS_LDA;
        for (int o = 0; o < k; ++o) {
            const double *Bo = a.B + (size_t)o * a.bstride + (size_t)(lane >> 4) * a.ldb + (lane & 15);
            d4_t acc[2][4];
            double bc[4], bn[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[0][q] = (d4_t){0.0, 0.0, 0.0, 0.0};
                acc[1][q] = (d4_t){0.0, 0.0, 0.0, 0.0};
                bc[q] = q < nqw ? Bo[(wv + 4 * q) * 16] : 0.0;
            }
            for (int ks = 0; ks < ks_n; ++ks) {
                const bool more = ks + 1 < ks_n;
#pragma unroll
                for (int q = 0; q < 4; ++q)   // next K step's B fragments in flight during this step's products
                    bn[q] = (more && q < nqw) ? Bo[(size_t)(ks + 1) * 4 * a.ldb + (wv + 4 * q) * 16] : 0.0;
                const double a0 = pa0[4 * ks], a1 = pa1[4 * ks];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < nqw) {
                        acc[0][q] = MFMA_F64(a0, bc[q], acc[0][q]);
                        acc[1][q] = MFMA_F64(a1, bc[q], acc[1][q]);
                    }
#pragma unroll
                for (int q = 0; q < 4; ++q) bc[q] = bn[q];
            }
            // ---- epilogue: lane l, register r of strip s holds T[row = 16 s + (l >> 4) + 4 r][col = 16 gb + (l & 15)]
            const int cl = lane & 15;
            const int cmu = m + o, cbe = m + k + o;
            const double bo = a.bvec[o];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * s + (lane >> 4) + 4 * r;
                    double p = 0.0;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q < nqw) {
                            const int col = (wv + 4 * q) * 16 + cl;
                            const double t = acc[s][q][r];
                            if (col < m) p = fma(sA[row * PS_LDA + col], t, p);     // predictDiag.m:69-71
                            if (i0 + row < a.n) {
                                if (col == cmu) a.out[(size_t)o * a.ldo + i0 + row] = t;                            // mu = PHI w
                                if (col == cbe) a.out[(size_t)(2 * k + o) * a.ldo + i0 + row] = exp(t + bo);     // beta_i = exp(b + PHI v)
                            }
                        }
                    p = ps_row_sum16(p);
                    if (cl == 0) sNu[wv * 32 + row] = p;
                }
            __syncthreads();
            if (tid < 32 && i0 + tid < a.n)
                a.out[(size_t)(k + o) * a.ldo + i0 + tid] = ((sNu[tid] + sNu[32 + tid]) + sNu[64 + tid]) + sNu[96 + tid];
            __syncthreads();
        }
    }
}

size_t predict_small_lds(int de) { return ((size_t)32 * PS_LDA + 32 * (size_t)de + 4 * 32) * sizeof(double); }

bool predict_small_fits(int de, int m, int k) {
    if (phi_is_wide(de, k) || !ps_width_instantiated(de)) return false;
    return ((m + 2 * k + 15) / 16) * 16 <= 256 && predict_small_lds(de) <= 80 * 1024;
}

int predict_small_nwg() { return 2 * gpz_cu_count(); }

template <int D, bool COV>
static int launch_ps(hipStream_t st, const PredSmallArgs &a, int nwg) {
    const size_t lds = predict_small_lds(D);
    // per launch, not once per process: the attribute belongs to the current device's copy of the kernel
    if (hipFuncSetAttribute((const void *)k_predict_small<D, COV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -1;
    hipLaunchKernelGGL((k_predict_small<D, COV>), dim3(nwg), dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
template <bool COV>
static int launch_ps_k(hipStream_t st, int de, const PredSmallArgs &a, int nwg) {
    switch (de) {
        case 1: return launch_ps<1, COV>(st, a, nwg);
        case 2: return launch_ps<2, COV>(st, a, nwg);
        case 3: return launch_ps<3, COV>(st, a, nwg);
        case 4: return launch_ps<4, COV>(st, a, nwg);
        case 5: return launch_ps<5, COV>(st, a, nwg);
        case 6: return launch_ps<6, COV>(st, a, nwg);
        case 8: return launch_ps<8, COV>(st, a, nwg);
        case 10: return launch_ps<10, COV>(st, a, nwg);
        case 12: return launch_ps<12, COV>(st, a, nwg);
        case 16: return launch_ps<16, COV>(st, a, nwg);
        case 20: return launch_ps<20, COV>(st, a, nwg);
        default: return -1;
    }
}

int launch_predict_small(hipStream_t st, int kind, int de, const double *Xc, long ldx, int n, int m, int k, const double *P,
                         const double *G, const double *B, int ldb, long bstride, const double *bvec, double *out, long ldo,
                         double *phi, long ldphi) {
    if (n <= 0) return 0;
    PredSmallArgs a{};
    a.Xc = Xc; a.ldx = ldx; a.n = n; a.m = m; a.k = k; a.nk = ((m + 15) / 16) * 16; a.nb = ldb / 16;
    a.P = P; a.G = G; a.B = B; a.ldb = ldb; a.bstride = bstride; a.bvec = bvec; a.out = out; a.ldo = ldo; a.phi = phi; a.ldphi = ldphi;
    const int nblocks = (n + 31) / 32;
    int nwg = predict_small_nwg();
    if (nwg > nblocks) nwg = nblocks;
    return kind == GPZ_KIND_COV ? launch_ps_k<true>(st, de, a, nwg) : launch_ps_k<false>(st, de, a, nwg);
}

// B (rows x ld, row-major) <- [inv(Sigma_o) | W | V | 0]: columns < m from iS (m x m column-major, B[i][j] = iS(i, j) as
// gpz_predict_full uses it), nw columns of W (m x nw column-major) from column wcol, nv columns of V from column vcol (V may be nullptr:
// zeros); rows >= m zero.
__global__ void k_pred_fill_b(const double *__restrict__ iS, const double *__restrict__ W, int nw, int wcol,
                              const double *__restrict__ V, int nv, int vcol, int m, int rows, int ld, double *__restrict__ B) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= ld || i >= rows) return;
    double v = 0.0;
    if (i < m) {
        if (j < m) v = iS[(size_t)i + (size_t)m * j];
        else if (j >= wcol && j < wcol + nw) v = W[(size_t)i + (size_t)m * (j - wcol)];
        else if (V && j >= vcol && j < vcol + nv) v = V[(size_t)i + (size_t)m * (j - vcol)];
    }
    B[(size_t)i * ld + j] = v;
}
void launch_pred_fill_b(hipStream_t st, const double *iS, const double *W, int nw, int wcol, const double *V, int nv, int vcol, int m,
                        int rows, int ld, double *B) {
    hipLaunchKernelGGL(k_pred_fill_b, dim3((ld + 255) / 256, rows), dim3(256), 0, st, iS, W, nw, wcol, V, nv, vcol, m, rows, ld, B);
}

// Tile route finish: out = [mu | nu | beta] ([3k][ldo]) from the T-GEMM's phiw (column m + o of T; phiw + o ldt) and nu partials (nslots
// of stride ldn per output, output o at nupart + o ostride, summed in slot order) and the PHI kernel's ln beta (k x ldt).
__global__ void k_pred_tile_finish(const double *__restrict__ phiw, const double *__restrict__ nupart, int nslots, long ldn, long ostride,
                                   const double *__restrict__ lnbeta, long ldt, int n, int k, double *__restrict__ out, long ldo) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int o = 0; o < k; ++o) {
        double s = 0.0;
        const double *np_ = nupart + (size_t)o * ostride + i;
        for (int q = 0; q < nslots; ++q) s += np_[(size_t)q * ldn];
        out[(size_t)o * ldo + i] = phiw[(size_t)o * ldt + i];
        out[(size_t)(k + o) * ldo + i] = s;
        out[(size_t)(2 * k + o) * ldo + i] = exp(lnbeta[(size_t)o * ldt + i]);
    }
}
void launch_pred_tile_finish(hipStream_t st, const double *phiw, const double *nupart, int nslots, long ldn, long ostride,
                             const double *lnbeta, long ldt, int n, int k, double *out, long ldo) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_pred_tile_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, phiw, nupart, nslots, ldn, ostride, lnbeta,
                       ldt, n, k, out, ldo);
}
