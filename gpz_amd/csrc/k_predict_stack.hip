// Stacked predictive densities of one tile of rows (gpz_predictor_stack): per column-output q = c k + o and per group g the weighted
// sum of the rows' normal masses per bin, with the weighted sums of 1, mu and mu^2 next to them.
//
//   k_stack_tile   one wave per workgroup, grid (columns, row slabs).  The rows of a slab are taken 64 at a time: lane = row for the
//                  loads, the width 1 / sqrt(s^2) and the window of edges within +-GPZ_STACK_TCUT widths of mu (two binary searches
//                  over the output's edges); then row by row, the row's numbers broadcast to the wave, lane = edge: each lane
//                  evaluates the tail q = erfc(|t| / sqrt 2) / 2 (stack_tail) of one edge of the window (the far side of every edge, so tails keep
//                  their relative accuracy), takes its right neighbour's from lane + 1, and adds omega * mass to its own bin of the
//                  workgroup's histogram in LDS.  A pass covers 63 bins with 64 edges, or 127 / 255 bins with two / four edges per lane
//                  where that many are left (independent chains per lane); a wider window takes more passes.  The window is the
//                  row's, and the row is the wave's: no lane diverges from its wave on it.
//                  Every add goes to an address that only this lane touches in this instruction, the rows of a slab follow each
//                  other in the wave's program order, and no other wave shares the LDS block: the sum is the same on every run.
//   k_stack_accum  acc[e] += slab_0[e] + slab_1[e] + ... in slab order, on the compute stream in tile order.
//
// Layout of a workgroup's record, of a slab entry and of the running accumulators, per q: [G][B] bins, then [G][3] = sum of omega,
// omega (mu + shift_o), omega (mu + shift_o)^2.  Bins wholly beyond the window are left out: at most Phi(-GPZ_STACK_TCUT) = 1.1e-19 omega per row and side.
//
// k_predict_stack_w.hip includes this text with GPZ_STACK_WIDTHS defined and gets k_stack_tile_w / launch_stack_tile_w instead: the same
// kernel with the row's width^2 read from an array s2 [(1 + nd) k][nt] (rows with input noise: the width of a draw column depends on the
// draw) and column 0's mu from that call's out.  The parameter is a macro, as PREDICT_DRAWS_PSI is, so that this unit keeps its code
// instruction for instruction; k_stack_accum and the two size functions exist in this unit only.
#include <hip/hip_runtime.h>

#include "gpz_kernels.h"

#define GPZ_STACK_TCUT 9.0

#ifdef GPZ_STACK_WIDTHS
#define K_STACK_TILE k_stack_tile_w
#else
#define K_STACK_TILE k_stack_tile
#endif

struct StackArgs {
    const double *out;     // [3k][nt]: mu, nu, beta of the tile (predictor_tile); with GPZ_STACK_WIDTHS only row o = mu is read
#ifdef GPZ_STACK_WIDTHS
    const double *s2;      // [(1 + nd) k][nt]: the width^2 of column-output q = c k + o
#endif
    const double *dout;    // [nd k][nt]: draw s of output o in row o nd + s (nullptr when nd = 0)
    const int *lab;        // nt labels or nullptr (all rows in group 0)
    const double *wt;      // nt weights or nullptr (all 1)
    const double *edges;   // [k][B + 1]
    const double *shift;   // [k]: added to mu in the sums of mu and mu^2 (not in the masses: the edges carry it there)
    double *slab;          // [R][Q][G B + 3 G]
    long nt;
    int k, nd, B, G, rps;  // rps: rows per slab (a multiple of 64)
};

__device__ __forceinline__ double stack_bcast(double x, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}

// The normal tail Q(t) = erfc(t / sqrt 2) / 2 for t >= 0, branch-free (the lanes of a wave sit on all sides of every branch of the
// library erfc): with x = t / sqrt 2 and u = (x - 3) / (x + 3) in [-1, 1), erfc(x) = exp(-x^2) p(u), p the degree-24 Chebyshev
// interpolant of exp(x^2) erfc(x) in u (computed in 50-digit arithmetic, then rounded; the coefficients are below 0.33 in magnitude, so
// Horner's rule in u is benign).  In f64 p is within 2 ulp of exp(x^2) erfc(x) for x <= 7 (t <= 9.9) and within 7 ulp up to x = 27, where
// exp(-x^2) underflows (tests/test_predictor_stack_cpu.py checks the constants against 50-digit values).  x^2 enters exp as its rounded
// value and the product's exact remainder, so the tail keeps its relative accuracy up to the x^2 eps that the rounding of x itself costs.
__device__ __forceinline__ double stack_tail(double t) {
    const double c[25] = {0x1.6e9827d229d2dp-3,  -0x1.4e102b9cf8512p-2,  0x1.f6ff204105974p-3,  -0x1.336ffbef08c77p-3,  0x1.258b13b017b18p-4,
                          -0x1.8fa58eb5c733fp-6, 0x1.17c838ee72f58p-8,   0x1.73101e57d4437p-11, -0x1.39084c4e83548p-11, 0x1.7ba1144c36d3dp-15,
                          0x1.0cac317924353p-14, -0x1.af8826e91042ep-17, -0x1.0bb33fb453e62p-17, 0x1.1c9c05110b825p-19,  0x1.502d9cfbab94bp-20,
                          -0x1.3cb6854982f06p-22, -0x1.f75c21fc07d5bp-23, 0x1.ffdfb289d3993p-26, 0x1.9022ec6057e97p-25,  0x1.9f11465cc7754p-34,
                          -0x1.292225081d82dp-27, -0x1.bd851768367cfp-31, 0x1.5c9f230554f5bp-30, 0x1.15efad5998d23p-33,  -0x1.cd3ca221dfa77p-34};
    const double x = fmin(t * 0.70710678118654752440, 40.0);   // exp(-1600) = 0: the cap changes nothing and keeps u finite
    const double u = (x - 3.0) / (x + 3.0);
    double p = c[24];
#pragma unroll
    for (int i = 23; i >= 0; --i) p = fma(p, u, c[i]);
    const double s = x * x, e = fma(x, x, -s);
    const double ex = exp(-s);
    return 0.5 * p * fma(-ex, e, ex);
}

// One pass of a row over the edges j0 .. j0 + 64 NE - 1 (clamped to rb): lane l takes the edges j0 + l + 64 q, q < NE, and owns the bins
// that start at them, so the adds of one instruction go to 64 different bins; bin j needs edge j + 1, lane l + 1's value of the same q or,
// for lane 63, lane 0's of q + 1.  The pass closes 64 NE - 1 bins (the last edge's bin belongs to the next pass).
template <int NE>
__device__ __forceinline__ void stack_pass(const double *__restrict__ e, double *hg, double rm, double rinv, double rw, int j0, int rb,
                                           int lane) {
    double u[NE], rot[NE];
#pragma unroll
    for (int q = 0; q < NE; ++q) {
        const int j = j0 + lane + 64 * q, jj = j < rb ? j : rb;
        const double t = (e[jj] - rm) * rinv;
        u[q] = copysign(stack_tail(fabs(t)), -t);   // sign set: Phi = 1 - |u|, else Phi = |u|
    }
#pragma unroll
    for (int q = 0; q < NE; ++q) rot[q] = __shfl(u[q], (lane + 1) & 63);
#pragma unroll
    for (int q = 0; q < NE; ++q) {
        const int j = j0 + lane + 64 * q;
        const double un = (lane < 63 || q == NE - 1) ? rot[q] : rot[q + 1 < NE ? q + 1 : q];
        const double ql = fabs(u[q]), qr = fabs(un);
        const bool sl = __double2hiint(u[q]) < 0, sr = __double2hiint(un) < 0;
        const double mass = sl == sr ? (sl ? ql - qr : qr - ql) : (0.5 - ql) + (0.5 - qr);
        if ((lane < 63 || q < NE - 1) && j < rb) hg[j] += rw * mass;
    }
}

__global__ __launch_bounds__(64) void K_STACK_TILE(StackArgs a) {
    extern __shared__ double h[];
    const int lane = threadIdx.x, q = blockIdx.x, r = blockIdx.y, Q = gridDim.x;
    const int c = q / a.k, o = q - c * a.k, B = a.B, ne = B + 1, GB = a.G * B, rec = GB + 3 * a.G;
    for (int i = lane; i < rec; i += 64) h[i] = 0.0;
    __syncthreads();
    const double *mu = c == 0 ? a.out + (size_t)o * a.nt : a.dout + ((size_t)o * a.nd + (c - 1)) * a.nt;
#ifdef GPZ_STACK_WIDTHS
    const double *w2 = a.s2 + (size_t)q * a.nt;
#else
    const double *nu = a.out + (size_t)(a.k + o) * a.nt, *beta = a.out + (size_t)(2 * a.k + o) * a.nt;
#endif
    const double *e = a.edges + (size_t)o * ne;
    const double shift = a.shift[o];
    const long r0 = (long)r * a.rps, r1 = r0 + a.rps < a.nt ? r0 + a.rps : a.nt;
    for (long i0 = r0; i0 < r1; i0 += 64) {
        // ---- lane = row
        const long i = i0 + lane;
        double m = 0.0, inv = 0.0, w = 0.0;
        int g = -1, ja = 0, jb = 0;
        if (i < r1) {
            g = a.lab ? a.lab[i] : 0;
            w = a.wt ? a.wt[i] : 1.0;
            if (!(w > 0.0)) g = -1;
        }
        if (g >= 0) {
            m = mu[i];
#ifdef GPZ_STACK_WIDTHS
            const double s2 = w2[i], s = sqrt(s2);
#else
            const double s2 = c == 0 ? nu[i] + beta[i] : beta[i], s = sqrt(s2);
#endif
            inv = 1.0 / s;
            const double lo = m - GPZ_STACK_TCUT * s, hi = m + GPZ_STACK_TCUT * s;
            int l0 = 0, l1 = ne;   // edges below lo
            while (l0 < l1) {
                const int md = (l0 + l1) >> 1;
                if (e[md] < lo) l0 = md + 1; else l1 = md;
            }
            int u0 = 0, u1 = ne;   // edges up to hi
            while (u0 < u1) {
                const int md = (u0 + u1) >> 1;
                if (e[md] <= hi) u0 = md + 1; else u1 = md;
            }
            ja = l0 > 0 ? l0 - 1 : 0;   // one edge beyond the window on either side closes the bins that straddle it
            jb = u0 < B ? u0 : B;
            if (jb < ja) jb = ja;
        }
        // ---- lane = edge, one row after the other
        unsigned long long todo = __ballot(g >= 0);
        while (todo) {
            const int rr = __builtin_ctzll(todo);
            todo &= todo - 1;
            const double rm = stack_bcast(m, rr), rinv = stack_bcast(inv, rr), rw = stack_bcast(w, rr);
            const int rg = __builtin_amdgcn_readlane(g, rr), ra = __builtin_amdgcn_readlane(ja, rr), rb = __builtin_amdgcn_readlane(jb, rr);
            const double ry = rm + shift;
            if (lane < 3) h[GB + 3 * rg + lane] += lane == 0 ? rw : (lane == 1 ? rw * ry : rw * (ry * ry));
            double *hg = h + (size_t)rg * B;
            int j0 = ra;
            while (j0 < rb) {   // the edges left decide how many each lane takes: independent chains hide the f64 latency
                const int left = rb - j0 + 1;
                if (left > 128) { stack_pass<4>(e, hg, rm, rinv, rw, j0, rb, lane); j0 += 255; }
                else if (left > 64) { stack_pass<2>(e, hg, rm, rinv, rw, j0, rb, lane); j0 += 127; }
                else { stack_pass<1>(e, hg, rm, rinv, rw, j0, rb, lane); j0 += 63; }
            }
        }
    }
    __syncthreads();
    double *dst = a.slab + ((size_t)r * Q + q) * rec;
    for (int i = lane; i < rec; i += 64) dst[i] = h[i];
}

#ifndef GPZ_STACK_WIDTHS
size_t predict_stack_lds(int G, int B) { return ((size_t)G * B + 3 * (size_t)G) * sizeof(double); }

// row slabs per tile for Q columns of records of rec doubles on tiles of T rows: enough workgroups to fill the device when the
// columns are few, one per column when they are many, never more slab memory than 2^24 doubles unless one slab alone is larger
// (tests/test_predictor_stack.py states the same rule in Python for its byte counts: change both)
int predict_stack_slabs(long Q, long rec, long T) {
    long R = (8192 + Q - 1) / Q;
    if (R > 64) R = 64;
    if (R > (T + 255) / 256) R = (T + 255) / 256;
    while (R > 1 && Q * R * rec > (1L << 24)) R >>= 1;
    return R < 1 ? 1 : (int)R;
}
#endif

#ifdef GPZ_STACK_WIDTHS
int launch_stack_tile_w(hipStream_t st, const double *out, const double *s2, const double *dout, const int *lab, const double *wt,
                        const double *edges, const double *shift, long nt, int k, int nd, int B, int G, int R, double *slab) {
    if (nt <= 0) return 0;
    StackArgs a{};
    a.s2 = s2;
#else
int launch_stack_tile(hipStream_t st, const double *out, const double *dout, const int *lab, const double *wt, const double *edges,
                      const double *shift, long nt, int k, int nd, int B, int G, int R, double *slab) {
    if (nt <= 0) return 0;
    StackArgs a{};
#endif
    a.out = out; a.dout = dout; a.lab = lab; a.wt = wt; a.edges = edges; a.shift = shift; a.slab = slab;
    a.nt = nt; a.k = k; a.nd = nd; a.B = B; a.G = G;
    a.rps = (int)(((nt + R - 1) / R + 63) / 64 * 64);
    const size_t lds = predict_stack_lds(G, B);
    // per launch, not once per process: the attribute belongs to the current device's copy of the kernel
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void *)K_STACK_TILE, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -1;
    hipLaunchKernelGGL(K_STACK_TILE, dim3((unsigned)((1 + nd) * k), (unsigned)R), dim3(64), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

#ifndef GPZ_STACK_WIDTHS
__global__ __launch_bounds__(256) void k_stack_accum(const double *__restrict__ slab, int R, size_t count, double *__restrict__ acc) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (size_t)gridDim.x * 256) {
        double s = slab[e];
        for (int r = 1; r < R; ++r) s += slab[(size_t)r * count + e];
        acc[e] += s;
    }
}

int launch_stack_accum(hipStream_t st, const double *slab, int R, size_t count, double *acc) {
    size_t nb = (count + 255) / 256;
    if (nb > 8192) nb = 8192;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(k_stack_accum, dim3((unsigned)nb), dim3(256), 0, st, slab, R, count, acc);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
#endif
