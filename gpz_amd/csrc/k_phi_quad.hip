// PHI build of the covariance kinds on the f64 MFMA (GC / VC, no input noise, no missing values, one output, d = 8 / 10).
//
// With x' = x - mu (mu = the column means of the context's rows: the rows [1 | x' | 0] of Xs), A_j = R_j' R_j (= Gamma_j' Gamma_j,
// R_j the QR factor of k_prep_cov) and p' = p_j - mu
//
//     ln PHI_ij = -1/2 |Gamma_j (x_i - p_j)|^2 = F_i . C_j
//     F_i = [1 | x' | x'_a x'_b (a <= b)]                             NF = 1 + d + d(d+1)/2 row features (those of k_moments_ring)
//     C_j = -1/2 [p''A p' ; -2 A p' ; (2 - delta_ab) A_ab]
//
// so ln PHI is one n x 4 NK x m product (NK = ceil(NF / 4) K steps of v_mfma_f64_16x16x4_f64 per 16 x 16 outputs; d = 10: 17) where
// k_phi_cov spends d(d+1)/2 + 2d vector multiply-adds per element.  Centring matters: about the rows' own means the three groups
// of terms stay of the size of the result (uncentred monomials cancel), and the form does not have k_phi_cov's c_j = R_j p_j.
//
//   * k_phi_quad_coef: one lane per basis function writes Cq[j][0 .. 4 NK) (columns j >= m and features >= NF zero) and the bound
//         B_j = (NF + 2d + 6) 2^-53 sum_f fmax_f Chat_fj
//     on the rounding error of F_i . C_j over the context's rows: Chat_j = the same three expressions from |R_j| and |p'_j| (it
//     dominates |C_j| and the error of forming C_j), fmax_f = max_i |F_if| (host, at context creation).  The last workgroup to finish
//     writes max_j B_j and the route word of this evaluation: GPZ_PHI_ROUTE_QUAD when max_j B_j <= GPZ_PHI_QUAD_TAU, else (also when
//     a B_j is not finite) GPZ_PHI_ROUTE_EXACT.  Both PHI kernels are launched in every evaluation with fixed arguments (the recorded
//     graph stays valid); the workgroups of the one the word does not name return at once, so an evaluation that falls back is
//     k_phi_cov's, bit for bit.
//   * k_phi_quad<D, RB>: a wave owns RB blocks of 16 rows.  A operand = the rows' features (lane l: row l & 15, feature 4 ks +
//     (l >> 4)), formed once from Xs and kept in registers for the whole basis loop; B operand = the coefficients of 16 basis
//     functions, staged per workgroup through a double-buffered LDS block of 16 x 4 NK doubles (row stride 4 NK = 68 doubles at
//     d = 10, 48 at d = 8).
//     The accumulator has lane l = column l & 15, rows (l >> 4) + 4 r: 16 lanes store 128 contiguous, 128-byte-aligned bytes of a
//     row of PHI - no transposition tile.  exp argument clamped at 0 (PHI <= 1 as on the other route); the running sum PHI v
//     is per lane and reduced over the 16 lanes of a row at the end in a fixed order.  Two row blocks per wave: 162 VGPRs at
//     d = 10, three workgroups per CU, no scratch; the eight exps of a lane and step are straight-line code (with a branch per
//     result the compiler cannot interleave their dependent chains: 4.5 ms at c4 against 3.2).
#include <float.h>
#include "gpz_dev.h"
#include "gpz_kernels.h"

template <int D>
struct PhiQuadShape {
    static constexpr int NT = D * (D + 1) / 2;
    static constexpr int NF = 1 + D + NT;
    static constexpr int NK = (NF + 3) / 4;
    static constexpr int CS = 4 * NK;            // doubles per basis function in Cq
};

int phi_quad_stride(int de) { return 4 * ((1 + de + de * (de + 1) / 2 + 3) / 4); }
bool phi_quad_fits(int kind, int de, int mp, int k) { return kind == GPZ_KIND_COV && (de == 8 || de == 10) && mp > 256 && k == 1; }

// ---------------------------------------------------------------------------------------------
// coefficients, bound, route word
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(64) void k_phi_quad_coef(const double *__restrict__ Rc, const double *__restrict__ P,
                                                        const double *__restrict__ xmu, const double *__restrict__ fmx, int m, int mp,
                                                        double *__restrict__ Cq, double *__restrict__ blockmax,
                                                        unsigned *__restrict__ ticket, double *__restrict__ bound,
                                                        int *__restrict__ route) {
    constexpr int NT = PhiQuadShape<D>::NT, NF = PhiQuadShape<D>::NF, CS = PhiQuadShape<D>::CS, NP = NT + D;
    const int j = blockIdx.x * 64 + threadIdx.x;
    double bj = 0.0;
    if (j < m) {
        double R[NT], pq[D], u[D], uh[D];
        const double *rj = Rc + (size_t)j * NP;
#pragma unroll
        for (int e = 0; e < NT; ++e) R[e] = rj[e];                        // packed upper, row a at a D - a (a - 1) / 2, entries b = a .. D - 1
#pragma unroll
        for (int a = 0; a < D; ++a) pq[a] = P[(size_t)j * D + a] - xmu[a];
        // u = R p' (so p''A p' = |u|^2 and A p' = R'u), uh = |R| |p'|
#pragma unroll
        for (int a = 0; a < D; ++a) {
            double s = 0.0, sh = 0.0;
#pragma unroll
            for (int b = a; b < D; ++b) {
                const double r = R[a * D - a * (a - 1) / 2 + (b - a)];
                s = fma(r, pq[b], s);
                sh = fma(fabs(r), fabs(pq[b]), sh);
            }
            u[a] = s; uh[a] = sh;
        }
        double *o = Cq + (size_t)j * CS;
        double c0 = 0.0, c0h = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) { c0 = fma(u[a], u[a], c0); c0h = fma(uh[a], uh[a], c0h); }
        o[0] = -0.5 * c0;
        double bs = fmx[0] * (0.5 * c0h);
#pragma unroll
        for (int a = 0; a < D; ++a) {                                     // -1/2 (-2 A p')_a = (R'u)_a
            double s = 0.0, sh = 0.0;
#pragma unroll
            for (int r = 0; r <= a; ++r) {
                const double v = R[r * D - r * (r - 1) / 2 + (a - r)];
                s = fma(v, u[r], s);
                sh = fma(fabs(v), uh[r], sh);
            }
            o[1 + a] = s;
            bs = fma(fmx[1 + a], sh, bs);
        }
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = a; b < D; ++b) {                                 // A_ab = sum_{r <= a} R_ra R_rb
                double s = 0.0, sh = 0.0;
#pragma unroll
                for (int r = 0; r <= a; ++r) {
                    const double va = R[r * D - r * (r - 1) / 2 + (a - r)], vb = R[r * D - r * (r - 1) / 2 + (b - r)];
                    s = fma(va, vb, s);
                    sh = fma(fabs(va), fabs(vb), sh);
                }
                const int f = 1 + D + a * D - a * (a - 1) / 2 + (b - a);
                const double sc = (a == b) ? 0.5 : 1.0;
                o[f] = -sc * s;
                bs = fma(fmx[f], sc * sh, bs);
            }
#pragma unroll
        for (int f = NF; f < CS; ++f) o[f] = 0.0;
        bj = (double)(NF + 2 * D + 6) * 0x1p-53 * bs;
        if (!(bj <= DBL_MAX)) bj = __longlong_as_double(0x7ff0000000000000LL);   // not finite (NaN included): + infinity, which no threshold admits
    } else if (j < mp) {
        double *o = Cq + (size_t)j * CS;
#pragma unroll
        for (int f = 0; f < CS; ++f) o[f] = 0.0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bj = fmax(bj, __shfl_xor(bj, off, 64));
    // the last workgroup to arrive combines the workgroups' maxima (a maximum: the same bits in any order) and rearms the ticket
    int last = 0;
    if (threadIdx.x == 0) {
        blockmax[blockIdx.x] = bj;
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1 : 0;
        if (last) {
            __threadfence();
            double mx = 0.0;
            for (unsigned g = 0; g < gridDim.x; ++g) mx = fmax(mx, __hip_atomic_load(blockmax + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            *bound = mx;
            *route = mx <= GPZ_PHI_QUAD_TAU ? GPZ_PHI_ROUTE_QUAD : GPZ_PHI_ROUTE_EXACT;
            *ticket = 0u;
        }
    }
}

int launch_phi_quad_coef(hipStream_t st, const double *Rc, const double *P, const double *xmu, const double *fmx, int m, int mp, int de,
                         double *Cq, double *blockmax, unsigned *ticket, double *bound, int *route) {
    dim3 g((mp + 63) / 64), b(64);
    switch (de) {
        case 8: hipLaunchKernelGGL(k_phi_quad_coef<8>, g, b, 0, st, Rc, P, xmu, fmx, m, mp, Cq, blockmax, ticket, bound, route); break;
        case 10: hipLaunchKernelGGL(k_phi_quad_coef<10>, g, b, 0, st, Rc, P, xmu, fmx, m, mp, Cq, blockmax, ticket, bound, route); break;
        default: return -1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// the product
// ---------------------------------------------------------------------------------------------
struct PhiQuadKArgs {
    const double *Xs;            // rows [1 | x - mu | 0] of this launch's rows (D + 2 doubles each)
    const double *Cq;            // [mp][CS]
    const int *route;
    int n, m, mp;                // valid rows (the grid's rows past them are zero-filled), basis functions, columns of PHI
    const double *v, *bvec, *omega, *Y;
    double *Phi, *lnbeta, *wbeta;
    int jgroup;
    double *part;
    long ldp;
};

#ifndef GPZ_PHI_QUAD_RB
#define GPZ_PHI_QUAD_RB 2
#endif
#ifndef GPZ_PHI_QUAD_WGS
#define GPZ_PHI_QUAD_WGS 3   // 162 VGPRs at d = 10: three workgroups per CU
#endif

template <int D, int RB>
__global__ __launch_bounds__(256, GPZ_PHI_QUAD_WGS) void k_phi_quad(PhiQuadKArgs a) {
    constexpr int NF = PhiQuadShape<D>::NF, NK = PhiQuadShape<D>::NK, CS = PhiQuadShape<D>::CS, XL = D + 2;
    constexpr int NPB = 16 * CS;                     // doubles per coefficient block
    constexpr int NLD = (NPB + 255) / 256;
    if (*a.route != GPZ_PHI_ROUTE_QUAD) return;      // this evaluation is k_phi_cov's
    __shared__ double cq[2][NPB];
    __shared__ unsigned char pia[CS], pib[CS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const long row0 = ((long)blockIdx.x * 4 + wave) * (16 * RB);

    // feature f = the product of entries ia, ib of the row [1 | x' | 0] (features past NF: the row's last entry, 0)
    if (tid < CS) {
        const int f = tid;
        int ia = 0, ib = 0;
        if (f >= NF) ia = ib = XL - 1;
        else if (f >= 1) {
            if (f <= D) ia = f;
            else {
                int e2 = f - 1 - D, aa = 0;          // packed upper triangle, row aa: D - aa entries
                while (e2 >= D - aa) { e2 -= D - aa; ++aa; }
                ia = aa + 1; ib = aa + e2 + 1;
            }
        }
        pia[f] = (unsigned char)ia; pib[f] = (unsigned char)ib;
    }
    const int jlo = blockIdx.y * a.jgroup;
    const int jhi = min(a.mp, jlo + a.jgroup);
    double stg[NLD];
    auto pload = [&](int j0) {                        // (Cq holds mp columns and jhi <= mp is a multiple of 16: whole blocks)
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int e = tid + 256 * q;
            stg[q] = e < NPB ? a.Cq[(size_t)j0 * CS + e] : 0.0;
        }
    };
    auto pstore = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int e = tid + 256 * q;
            if (e < NPB) cq[buf][e] = stg[q];
        }
    };
    pload(jlo);
    pstore(0);
    __syncthreads();

    double F[RB][NK];
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
        const int ia = pia[4 * ks + lk], ib = pib[4 * ks + lk];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const long i = row0 + 16 * rb + li;
            const double *xr = a.Xs + (size_t)i * XL;
            F[rb][ks] = xr[ia] * xr[ib];
        }
    }
    double sv[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) sv[rb][r] = 0.0;

    int cur = 0;
    for (int j0 = jlo; j0 < jhi; j0 += 16, cur ^= 1) {
        const bool more = j0 + 16 < jhi;
        if (more) pload(j0 + 16);                    // in flight during the products
        const int j = j0 + li;
        const double vj = (a.v && j < a.m) ? a.v[j] : 0.0;
        d4_t acc[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) acc[rb] = d4_t{0.0, 0.0, 0.0, 0.0};
        const double *cb = &cq[cur][li * CS + lk];
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            const double b = cb[4 * ks];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc[rb] = MFMA_F64(F[rb][ks], b, acc[rb]);
        }
        // all exps of the step in straight-line code (a branch per element keeps the compiler from interleaving their dependent chains)
        double ph[RB][4];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long i = row0 + 16 * rb + lk + 4 * r;
                const double e = exp(fmin(acc[rb][r], 0.0));                     // getPHI.m:113
                ph[rb][r] = i < a.n ? e : 0.0;
                sv[rb][r] = fma(ph[rb][r], vj, sv[rb][r]);                        // getPHI.m:124
            }
        }
        if (j0 + 16 > a.m) {                         // (wave-uniform) the block holds padding columns: [Y | 0]; Y's rows past n are zero
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double y = a.Y ? a.Y[row0 + 16 * rb + lk + 4 * r] : 0.0;
                    if (j >= a.m) ph[rb][r] = j == a.m ? y : 0.0;
                }
            }
        }
        double *const po = a.Phi + (size_t)(row0 + lk) * a.mp + j;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) po[(size_t)(16 * rb + 4 * r) * a.mp] = ph[rb][r];
        }
        if (more) pstore(cur ^ 1);
        __syncthreads();                             // the next block is in place; every wave is done with this one
    }

    // the 16 lanes of a row, added in a fixed order
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) sv[rb][r] += __shfl_xor(sv[rb][r], off, 64);
        }
    if (li != 0) return;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long i = row0 + 16 * rb + lk + 4 * r;
            if (a.part) {   // column-split launch: partial sums [group][2][1][ldp]; k_phi_finalize combines them in a fixed order
                if (i < a.ldp) {
                    a.part[((size_t)blockIdx.y * 2 + 0) * a.ldp + i] = sv[rb][r];
                    a.part[((size_t)blockIdx.y * 2 + 1) * a.ldp + i] = 0.0;
                }
                continue;
            }
            const bool valid = i < a.n;
            const double lb = a.bvec[0] + sv[rb][r];                              // getPHI.m:119,124
            a.lnbeta[i] = valid ? lb : 0.0;
            if (a.wbeta) {
                const double om = a.omega ? a.omega[i] : 1.0;
                a.wbeta[i] = valid ? om * exp(-lb) : 0.0;                         // GPz.m:43,48
            }
        }
}

template <int D>
static int launch_phi_quad_d(hipStream_t st, const PhiArgs &a, const double *Xs, const double *Cq) {
    constexpr int RB = GPZ_PHI_QUAD_RB, JB = 16;
    const int rows_per_wg = 4 * 16 * RB;
    // whole workgroups only: the kernel guards no row (a row set's n_pad and a row tile are multiples of 1024)
    if (a.n_pad <= 0 || a.n_pad % rows_per_wg != 0 || a.n_pad > a.ldx) return -1;
    const int nwg = a.n_pad / rows_per_wg;
    int ngroup = 1;
    if (a.part && nwg < 1024) {   // few rows: split the basis functions into groups as well (as launch_phi does)
        int maxg = a.mp / (4 * JB);
        if (maxg > a.part_groups) maxg = a.part_groups;
        ngroup = phi_pick_groups(nwg, a.mp, JB, 2, 16, maxg < 1 ? 1 : maxg);
    }
    int jgroup = ((a.mp + ngroup - 1) / ngroup + JB - 1) / JB * JB;
    ngroup = (a.mp + jgroup - 1) / jgroup;
    PhiQuadKArgs q{};
    q.Xs = Xs; q.Cq = Cq; q.route = a.route; q.n = a.n; q.m = a.m; q.mp = a.mp;
    q.v = a.v; q.bvec = a.b; q.omega = a.omega; q.Y = a.Y;
    q.Phi = a.Phi; q.lnbeta = a.lnbeta; q.wbeta = a.wbeta;
    q.jgroup = jgroup; q.part = ngroup > 1 ? a.part : nullptr; q.ldp = (long)a.n_pad;
    hipLaunchKernelGGL((k_phi_quad<D, RB>), dim3(nwg, ngroup), dim3(256), 0, st, q);
    if (q.part)
        launch_phi_finalize(st, q.part, ngroup, a, a.route, GPZ_PHI_ROUTE_QUAD);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// a: the arguments of the PHI-storing launch_phi that follows (no PHI w: a.w, a.phiw null) (a.route set, a.route_want = GPZ_PHI_ROUTE_EXACT there); k = 1, a.mp % 16 == 0,
// Xs the plain layout (d + 2 doubles a row) of the rows a.Xc describes, Cq from launch_phi_quad_coef
int launch_phi_quad(hipStream_t st, const PhiArgs &a, const double *Xs, const double *Cq) {
    if (a.k != 1 || a.mp % 16 != 0 || !a.route || a.wgtab || !a.Phi || !a.lnbeta || a.w || a.phiw) return -1;   // the PHI-storing build only
    switch (a.d) {
        case 8: return launch_phi_quad_d<8>(st, a, Xs, Cq);
        case 10: return launch_phi_quad_d<10>(st, a, Xs, Cq);
        default: return -1;
    }
}
