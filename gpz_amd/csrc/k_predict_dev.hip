// Device-resident entries of the streaming predictor (gpz_predictor_run_dev / _draws_dev / _stack_dev): the kernels that stand where
// the host entries have host passes.  All of them move bytes; the tile kernels between them (k_predict_small, k_predict_draws, k_phi_* +
// k_tgemm, k_stack_tile) are the host entries' own.
//
//   k_pred_check_dev    one pass over all rows of a call before its first tile: word 0 of the record is set when an element is NaN,
//                       word 1 when a label is outside [-1, G), word 2 when a weight is negative or not finite (atomicOr from a VGPR,
//                       at most one per wave and word).  A contiguous X is read as one flat array; any other strides row by row.
//   k_pred_stage        the caller's rows (f64 or f32, any strides) -> Xc [de][ldx]: (double(x) - muX[c]) / sdX[c], a plain f64 subtraction
//                       and a plain f64 division, the bits of NumPy's subtract then divide.  256 rows per workgroup.  Rows that are
//                       contiguous along the row index (stride 1: column-major input) go straight through, lane = row.  Anything else
//                       goes through LDS in chunks of up to 16 columns: the chunk is read in the order it lies in memory (lane =
//                       element of the 256 x dc block, so a row-major X is read in full lines), stored [row][dc | 1], and read back lane = row;
//                       the odd row length keeps both sides off each other's banks (the write is then at most 2-way, the read conflict-free).
//   k_pred_finish_dev   out [3k][nt] -> the caller's column-major ns x k arrays at row r0: mu + muY[o], nu, beta, gamma = 0,
//                       sigma = (nu + beta) + gamma.
//   k_pred_phi_dev      phi [m][nt] -> the caller's column-major ns x m PHI at row r0.
//   k_draws_finish_dev  dout [nd k][nt] (row o nd + s) -> F(r0 + i, o, s) + muY[o], F column-major ns x k x nd.
#include <hip/hip_runtime.h>

#include "gpz_kernels.h"

#define PD_ROWS 256   // rows per workgroup of k_pred_stage (= its threads)
#define PD_DC 16      // columns per LDS chunk

__global__ __launch_bounds__(256) void k_pred_check_dev(const void *__restrict__ X, int f32, long ns, int d, long rs, long cs, int flat,
                                                        const int *__restrict__ lab, int G, const double *__restrict__ wt,
                                                        unsigned *__restrict__ rec) {
    const long t0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    int nan = 0, badl = 0, badw = 0;
    if (flat) {   // ns d elements in one run
        const long ne = ns * d;
        if (f32) {
            const float *x = (const float *)X;
            for (long e = t0; e < ne; e += step) { const float v = x[e]; nan |= v != v; }
        } else {
            const double *x = (const double *)X;
            for (long e = t0; e < ne; e += step) { const double v = x[e]; nan |= v != v; }
        }
    } else {
        for (long i = t0; i < ns; i += step)
            for (int c = 0; c < d; ++c) {
                const long at = i * rs + c * cs;
                const double v = f32 ? (double)((const float *)X)[at] : ((const double *)X)[at];
                nan |= v != v;
            }
    }
    if (lab)
        for (long i = t0; i < ns; i += step) { const int g = lab[i]; badl |= g < -1 || g >= G; }
    if (wt)
        for (long i = t0; i < ns; i += step) { const double w = wt[i]; badw |= !(w >= 0.0) || !(w <= 1.7976931348623157e308); }
    const int lane = threadIdx.x & 63;
    if (__ballot(nan) && lane == 0) atomicOr(rec + 0, 1u);
    if (__ballot(badl) && lane == 0) atomicOr(rec + 1, 1u);
    if (__ballot(badw) && lane == 0) atomicOr(rec + 2, 1u);
}

template <typename T>
__global__ __launch_bounds__(PD_ROWS) void k_pred_stage(const T *__restrict__ X, long rs, long cs, long r0, int nt, int d,
                                                        const double *__restrict__ muX, const double *__restrict__ sdX,
                                                        double *__restrict__ Xc, long ldx) {
    __shared__ double tile[PD_ROWS * (PD_DC + 1)];
    const int t = threadIdx.x, i0 = blockIdx.x * PD_ROWS, i = i0 + t;
    const T *xb = X + (r0 + i0) * rs;   // the block's first row
    if (rs == 1) {   // lane = row is already coalesced
        if (i < nt)
            for (int c = 0; c < d; ++c) {
                double v = (double)xb[(long)t + c * cs];
                if (muX) v = (v - muX[c]) / sdX[c];
                Xc[(size_t)c * ldx + i] = v;
            }
        return;
    }
    const int nr = nt - i0 < PD_ROWS ? nt - i0 : PD_ROWS;
    for (int c0 = 0; c0 < d; c0 += PD_DC) {
        const int dc = d - c0 < PD_DC ? d - c0 : PD_DC, dp = dc | 1, ne = nr * dc;
        for (int e = t; e < ne; e += PD_ROWS) {
            const int r = e / dc, c = e - r * dc;
            tile[r * dp + c] = (double)xb[r * rs + (c0 + c) * cs];
        }
        __syncthreads();
        if (i < nt)
            for (int c = 0; c < dc; ++c) {
                double v = tile[t * dp + c];
                if (muX) v = (v - muX[c0 + c]) / sdX[c0 + c];
                Xc[(size_t)(c0 + c) * ldx + i] = v;
            }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_pred_finish_dev(const double *__restrict__ out, int nt, int k, const double *__restrict__ muY,
                                                         long ns, long r0, double *__restrict__ mu, double *__restrict__ sigma,
                                                         double *__restrict__ nu, double *__restrict__ beta, double *__restrict__ gamma) {
    const int i = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
    if (i >= nt) return;
    const double m = out[(size_t)o * nt + i], v = out[(size_t)(k + o) * nt + i], b = out[(size_t)(2 * k + o) * nt + i], g = 0.0;
    const size_t at = (size_t)o * ns + r0 + i;
    mu[at] = muY ? m + muY[o] : m;
    nu[at] = v;
    beta[at] = b;
    if (gamma) gamma[at] = g;
    if (sigma) sigma[at] = v + b + g;
}

__global__ __launch_bounds__(256) void k_pred_phi_dev(const double *__restrict__ phi, int nt, long ns, long r0, double *__restrict__ PHI) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i < nt) PHI[(size_t)j * ns + r0 + i] = phi[(size_t)j * nt + i];
}

__global__ __launch_bounds__(256) void k_draws_finish_dev(const double *__restrict__ dout, int nt, int k, int nd,
                                                          const double *__restrict__ muY, long ns, long r0, double *__restrict__ F) {
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (i >= nt) return;
    const int o = c / nd, s = c - o * nd;
    const double f = dout[(size_t)c * nt + i];
    F[((size_t)s * k + o) * ns + r0 + i] = muY ? f + muY[o] : f;
}

int launch_pred_check_dev(hipStream_t st, const void *X, int f32, long ns, int d, long rs, long cs, const int *lab, int G,
                          const double *wt, unsigned *rec) {
    if (ns <= 0) return 0;
    const int flat = (cs == 1 && rs == d) || (rs == 1 && cs == ns) || (d == 1 && rs == 1) || (ns == 1 && cs == 1);
    const long work = flat ? ns * d : ns;
    long nb = (work + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_pred_check_dev, dim3((unsigned)nb), dim3(256), 0, st, X, f32, ns, d, rs, cs, flat, lab, G, wt, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pred_stage(hipStream_t st, const void *X, int f32, long rs, long cs, long r0, int nt, int d, const double *muX,
                      const double *sdX, double *Xc, long ldx) {
    if (nt <= 0) return 0;
    const dim3 grid((unsigned)((nt + PD_ROWS - 1) / PD_ROWS));
    if (f32)
        hipLaunchKernelGGL(k_pred_stage<float>, grid, dim3(PD_ROWS), 0, st, (const float *)X, rs, cs, r0, nt, d, muX, sdX, Xc, ldx);
    else
        hipLaunchKernelGGL(k_pred_stage<double>, grid, dim3(PD_ROWS), 0, st, (const double *)X, rs, cs, r0, nt, d, muX, sdX, Xc, ldx);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pred_finish_dev(hipStream_t st, const double *out, int nt, int k, const double *muY, long ns, long r0, double *mu,
                           double *sigma, double *nu, double *beta, double *gamma) {
    if (nt <= 0) return 0;
    hipLaunchKernelGGL(k_pred_finish_dev, dim3((unsigned)((nt + 255) / 256), (unsigned)k), dim3(256), 0, st, out, nt, k, muY, ns, r0, mu,
                       sigma, nu, beta, gamma);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pred_phi_dev(hipStream_t st, const double *phi, int nt, int m, long ns, long r0, double *PHI) {
    if (nt <= 0) return 0;
    if (m > 65535) return -1;   // one grid row per basis function
    hipLaunchKernelGGL(k_pred_phi_dev, dim3((unsigned)((nt + 255) / 256), (unsigned)m), dim3(256), 0, st, phi, nt, ns, r0, PHI);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_draws_finish_dev(hipStream_t st, const double *dout, int nt, int k, int nd, const double *muY, long ns, long r0, double *F) {
    if (nt <= 0) return 0;
    hipLaunchKernelGGL(k_draws_finish_dev, dim3((unsigned)((nt + 255) / 256), (unsigned)(nd * k)), dim3(256), 0, st, dout, nt, k, nd, muY,
                       ns, r0, F);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
