// dP / dGamma moment sums of the fused route for covariance kinds with many basis functions (mp > 256, no input noise, no missing
// values; GPz.m:113,142-159), streamed through an LDS ring.
//
// k_moments_fused (k_rows.hip) prefetches PHI and T into registers: 2 sets x 4 rows beside 66 sums leave two waves per SIMD and
// 8 waves x 64 lanes x 4 rows x 16 B = 32 KB requested per CU; with ~2.1 us of loaded HBM latency that is 8.4 MB / 2.1 us = 4.0 TB/s
// on 256 CUs (Little's law) - what it measures.  Here no row passes through a register before it is used:
//
//   * every wave owns 32 basis functions and a private ring of RG_SLOTS = 4 slots in LDS.  A slot is 8 rows: PHI [8][32] and T [8][32]
//     (four LDS-DMA requests of 1 KB, global_load_lds_dwordx4: four 256-byte row segments each) and one "side" request with the
//     rows' centred inputs [1 | x - mu | 0] (Xs, xs_ld = d + 2 doubles a row) and row scalars [omega beta, c, dbeta, 0] - 5 KB.
//     The rows of a slot are requested again, four at a time, as soon as their K step is consumed, so beside the slot being
//     consumed three slots per wave are requested and not yet consumed: 3 x 4 KB x 8 waves = 96 KB of PHI / T per CU (120 KB with
//     the side blocks), 25 MB on the chip, enough for 8 TB/s at 2.1 us and 1.5 x the 64 KB that 6 TB/s need.  LDS: 4 x 5120 B per
//     wave = 81 920 B per workgroup of four waves, two workgroups (all 160 KB) per CU.  Waves never wait for one another: no
//     barrier in the kernel; a wave's own counted s_waitcnt vmcnt orders its reads behind its requests (they complete in issue
//     order).  (64 basis functions per wave halve the feature work per element but need 128 + 32 accumulator registers: with the
//     operands that spilled 73 registers at d = 10; at 32 the kernel takes 5.1 instead of 5.0 cycles per element, below.)
//   * the sums are raw sums about the rows' column means mu with per-row features F_i = [1 | x' | x'_a x'_b (a <= b)], x' = x - mu:
//     R[j][f] = sum_i dPHI_ij F_if is one product dPHI' F.  The first 16 NFB features go to the f64 MFMA (A = dPHI in the operand
//     layout straight from the ring: lane l = basis function l & 15 of a 16-block, row l >> 4 of the K step; B = the features, each
//     the product of two entries of the row of Xs, formed per lane); the NL features that do not fill another 16-block (d = 10: 2 of
//     66) and the two column sums PHI'c and PHI'dbeta (GPz.m:89,104; A would be PHI, not dPHI) are vector multiply-adds in the same
//     lane layout, their four row classes added at the end in a fixed order.  Per K step (4 rows x 32 basis functions) and wave at
//     d = 10: 8 MFMAs of 64.5 cycles and ~26 vector instructions of 5.3 (profiles/r04_ubench_mfma_f64_valu_overlap.txt: the two
//     ADD on a SIMD) = 5.1 cycles per element, where the all-vector form of the same sums takes 73 x 5.3 / 64 = 6.0 and the all-MFMA
//     form (6 blocks of 16 for 68 values) 6.7.  The mixed form also needs no wave-uniform feature operand: scalar registers cannot
//     hold a row's 68 doubles, and 34 broadcast ds_read_b128 per row and wave are 1.9 x the LDS array's time.  (The all-MFMA form
//     with register prefetch was measured in round 6: 4.40 ms at c4, profiles/r06_dropped.)
//   * registers: 64 accumulators of the MFMAs + 16 of the vector sums + operands: at most 256 (two waves per SIMD, which the LDS
//     allows), no scratch.
//   * records [chunk][j][NF | PHI'c | PHI'dbeta], summed over the chunks in a fixed order and converted to the sums about the basis
//     centres by k_ring_finish (the conversion of k_small_finish); no atomics, the same bits on every run.
#include "gpz_dev.h"
#include "gpz_kernels.h"

#define RG_ROWS 8                    // rows per ring slot (two K steps)
#define RG_SLOTS 4
#define RG_JB 2                      // 16-blocks of basis functions per wave
#define RG_COLS 32                   // = 16 RG_JB
#define RG_SLOT_DOUBLES 640          // PHI 256 | T 256 | side 128
#define RG_SIDE 512                  // the side block's place in a slot
#define RG_SIDE_RS 96                // the row scalars' place in the side block (behind 8 rows of xs_ld <= 12 doubles)
#define RG_GROUP_REQ 5               // requests per slot: 2 PHI, 2 T, 1 side
#define RG_LDS_BYTES 81920           // 4 waves x RG_SLOTS x RG_SLOT_DOUBLES x 8
#define RG_GLDS(g, l) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g), (__attribute__((address_space(3))) void *)(l), 16, 0, 0)
static_assert(RG_LDS_BYTES == 4 * RG_SLOTS * RG_SLOT_DOUBLES * 8 && RG_COLS == 16 * RG_JB && RG_SIDE == 2 * RG_ROWS * RG_COLS, "ring size");

template <int D>
__global__ __launch_bounds__(256, 2) void k_moments_ring(RingMomentArgs a) {
    constexpr int NF = 1 + D + D * (D + 1) / 2, XL = D + 2;
    constexpr int NFB = NF >= 64 ? NF / 16 : (NF + 15) / 16;     // feature blocks of 16 on the MFMA (d = 10: 4 of 66; d = 8: 3 for 45)
    constexpr int NL = NF > 16 * NFB ? NF - 16 * NFB : 0;        // features left to the vector ALU
    static_assert(RG_ROWS * XL <= RG_SIDE_RS, "side block");
    extern __shared__ double rg_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lk = lane >> 4;
    const int ncg = (a.m + 4 * RG_COLS - 1) / (4 * RG_COLS);
    const int cg = blockIdx.x % ncg, chunk = blockIdx.x / ncg;   // column group fastest: the workgroups of a row range run together
    const int j0 = cg * (4 * RG_COLS) + wave * RG_COLS;
    if (j0 >= a.m) return;                                       // (wave-uniform; nothing in this kernel waits for another wave)
    double *const ring = rg_smem + wave * (RG_SLOTS * RG_SLOT_DOUBLES);
    const int r_begin = chunk * a.rows_per_chunk;
    const int r_end = min(a.n, r_begin + a.rows_per_chunk);
    const int ng = (r_end - r_begin + RG_ROWS - 1) / RG_ROWS;
    double wj[RG_JB], vj[RG_JB];
#pragma unroll
    for (int cb = 0; cb < RG_JB; ++cb) {
        const int j = min(j0 + 16 * cb + li, a.m - 1);
        wj[cb] = a.w[j];
        vj[cb] = a.v ? a.v[j] : 0.0;
    }
    // B operand: feature 16 fb + li = the product of entries ia, ib of the row [1 | x' | 0] (features past NF: the row's last entry, 0)
    int fia[NFB], fib[NFB];
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb) {
        const int f = 16 * fb + li;
        int ia = 0, ib = 0;
        if (f >= NF) ia = ib = XL - 1;
        else if (f >= 1) {
            if (f <= D) ia = f;
            else {
                int e2 = f - 1 - D, aa = 0;                      // packed upper triangle, row aa: D - aa entries
                while (e2 >= D - aa) { e2 -= D - aa; ++aa; }
                ia = aa + 1; ib = aa + e2 + 1;
            }
        }
        fia[fb] = ia; fib[fb] = ib;
    }
    // the vector ALU's features (wave-uniform index pairs): the last NL of the packed triangle
    int lia[NL > 0 ? NL : 1], lib[NL > 0 ? NL : 1];
#pragma unroll
    for (int t = 0; t < NL; ++t) {
        int e2 = 16 * NFB + t - 1 - D, aa = 0;
        while (e2 >= D - aa) { e2 -= D - aa; ++aa; }
        lia[t] = aa + 1; lib[t] = aa + e2 + 1;
    }
    d4_t acc[RG_JB][NFB];
    double ev[RG_JB][NL + 2];
#pragma unroll
    for (int cb = 0; cb < RG_JB; ++cb) {
#pragma unroll
        for (int fb = 0; fb < NFB; ++fb) acc[cb][fb] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < NL + 2; ++t) ev[cb][t] = 0.0;
    }
    // Requests.  EVERY request runs with all 64 lanes under wave-uniform control flow (tests/test_isa_guard.py: a request in a divergent
    // branch may take its LDS base from a lane).  PHI / T request q of a slot: rows 4q .. 4q + 3, lane l the column pair l & 15 of row
    // l >> 4; column pairs past the leading dimension re-read the last pair (their basis functions are >= m and never written).
    const unsigned colj = (unsigned)min(j0 + 2 * (lane & 15), a.ld - 2);
    const unsigned voff = (unsigned)(lane >> 4) * (unsigned)a.ld + colj;
    // side request: lanes 0 .. 47 the slot's rows of Xs as they lie in memory (2 doubles each), lanes 48 .. 63 its row scalars
    const bool is_rs = lane >= 48;
    const unsigned soff = is_rs ? 2u * (unsigned)(lane - 48) : min(2u * (unsigned)lane, (unsigned)(RG_ROWS * XL - 2));
    const double *const sbase = is_rs ? a.rowscal : a.Xs;
    const unsigned srow = is_rs ? 4u : (unsigned)XL;             // doubles per row
    const long last = (long)r_end - 1;
    auto stage_half = [&](int g, int slot, int h) {              // rows 4h .. 4h + 3 of group g -> slot
        const long rg = (long)r_begin + (long)g * RG_ROWS + 4 * h;
        double *const l0 = ring + slot * RG_SLOT_DOUBLES + 4 * h * RG_COLS;
        if (rg + 4 <= (long)r_end) {
            const size_t ro = (size_t)rg * (size_t)a.ld;
            RG_GLDS(a.Phi + ro + voff, l0);
            RG_GLDS(a.T + ro + voff, l0 + RG_ROWS * RG_COLS);
        } else {   // the chunk ends inside these rows (wave-uniform): rows past its end re-read its last row - finite, and multiplied by zero row scalars
            long row = rg + (lane >> 4);
            row = row < last ? row : last;
            const size_t ro = (size_t)row * (size_t)a.ld + colj;
            RG_GLDS(a.Phi + ro, l0);
            RG_GLDS(a.T + ro, l0 + RG_ROWS * RG_COLS);
        }
    };
    auto stage_side = [&](int g, int slot) {
        const long rg = (long)r_begin + (long)g * RG_ROWS;
        double *const l0 = ring + slot * RG_SLOT_DOUBLES + RG_SIDE;
        long e = rg * (long)srow + (long)soff;
        const long elast = (long)r_end * (long)srow - 2;         // the last pair of the chunk's rows
        e = e < elast ? e : elast;
        RG_GLDS(sbase + e, l0);
    };
    // One K step: rows 4 kk + lk of the slot.  (Plain pointers: the slot's contents change between reads of the same address.)
    auto kstep = [&](const double *s0, int kk, int rows_left) {
        const int rr = 4 * kk + lk;
        const bool valid = rr < rows_left;
        const double *xr = s0 + RG_SIDE + rr * XL;
        const double *rs = s0 + RG_SIDE + RG_SIDE_RS + rr * 4;
        const double r0 = rs[0], r1 = rs[1], r2 = rs[2];
        const double ob = valid ? r0 : 0.0, cc = valid ? r1 : 0.0, db = valid ? r2 : 0.0;
        double fr[NFB], fl[NL > 0 ? NL : 1];
#pragma unroll
        for (int fb = 0; fb < NFB; ++fb) fr[fb] = xr[fia[fb]] * xr[fib[fb]];
#pragma unroll
        for (int t = 0; t < NL; ++t) fl[t] = xr[lia[t]] * xr[lib[t]];
        // one 16-block of basis functions at a time, its PHI / T values read while the block before it is multiplied (the scheduling
        // barriers keep the compiler from hoisting every read of the K step to its top: that spilled at d = 10)
        const double *pp = s0 + rr * RG_COLS + li;
        double phn = pp[0], ttn = pp[RG_ROWS * RG_COLS];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int cb = 0; cb < RG_JB; ++cb) {
            const double ph = phn, tt = ttn;
            if (cb + 1 < RG_JB) { phn = pp[16 * (cb + 1)]; ttn = pp[RG_ROWS * RG_COLS + 16 * (cb + 1)]; }
            const double dp = fma(-ob, tt, fma(db, vj[cb], -cc * wj[cb])) * ph;
#pragma unroll
            for (int fb = 0; fb < NFB; ++fb) acc[cb][fb] = MFMA_F64(dp, fr[fb], acc[cb][fb]);
#pragma unroll
            for (int t = 0; t < NL; ++t) ev[cb][t] = fma(dp, fl[t], ev[cb][t]);
            ev[cb][NL] = fma(ph, cc, ev[cb][NL]);
            ev[cb][NL + 1] = fma(ph, db, ev[cb][NL + 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // Group g lives in slot g % RG_SLOTS.  When group g is consumed, the wave's youngest requests are those of the groups after it, up to
    // RG_SLOTS - 1 of them and RG_GROUP_REQ each (a group's rows 0 - 3, its rows 4 - 7, its side block): vmcnt(that many) says group g
    // has landed.  The requests of group g + RG_SLOTS follow the K step whose rows they overwrite (lgkmcnt(0): that K step's reads of
    // the slot are done).
    for (int g = 0; g < RG_SLOTS; ++g)
        if (g < ng) { stage_half(g, g, 0); stage_half(g, g, 1); stage_side(g, g); }
    for (int g = 0; g < ng; ++g) {
        const int ahead = ng - 1 - g;                            // groups requested after this one (wave-uniform)
        if (ahead >= 3) asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
        else if (ahead == 2) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int slot = g % RG_SLOTS;
        const double *s0 = ring + slot * RG_SLOT_DOUBLES;
        const int rows_left = r_end - r_begin - g * RG_ROWS;
        const bool more = g + RG_SLOTS < ng;
        kstep(s0, 0, rows_left);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (more) stage_half(g + RG_SLOTS, slot, 0);
        kstep(s0, 1, rows_left);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (more) { stage_half(g + RG_SLOTS, slot, 1); stage_side(g + RG_SLOTS, slot); }
    }
    // records: accumulator register r of a tile = basis function 16 cb + (lane >> 4) + 4 r, feature 16 fb + (lane & 15)
    double *rec = a.slab + (size_t)chunk * a.m * (NF + 2);
#pragma unroll
    for (int cb = 0; cb < RG_JB; ++cb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 16 * cb + lk + 4 * r;
            if (j < a.m) {
                double *o = rec + (size_t)j * (NF + 2);
#pragma unroll
                for (int fb = 0; fb < NFB; ++fb)
                    if (16 * fb + li < NF) o[16 * fb + li] = acc[cb][fb][r];
            }
        }
        // the vector sums: row classes 0 + 1 and 2 + 3, then the two halves (a fixed order); values NF - NL .. NF + 1 of the record
        const int j = j0 + 16 * cb + li;
#pragma unroll
        for (int t = 0; t < NL + 2; ++t) {
            double s = ev[cb][t];
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (lk == 0 && j < a.m) rec[(size_t)j * (NF + 2) + (NF - NL) + t] = s;
        }
    }
}

// Block j: the nrec chunk records of basis function j summed in a fixed order (up to 32 record lanes per value, four loads in flight each),
// then the raw sums about mu converted to the records the finish kernels chain (k_small_finish's conversion):
//   sum dp (x - p)             = R1 - q R0,                                   q = p - mu
//   sum dp (x - p)_a (x - p)_b = R2_ab - q_a R1_b - q_b R1_a + q_a q_b R0
__global__ __launch_bounds__(1024) void k_ring_finish(const double *__restrict__ slab, int nrec, int m, int d, int nf, const double *__restrict__ P,
                                                      const double *__restrict__ xmu, int nm, int mp, double *__restrict__ mom,
                                                      double *__restrict__ cols, int accumulate) {
    __shared__ double part[32][72];
    __shared__ double R[72];
    const int tid = threadIdx.x, j = blockIdx.x, nv = nf + 2;
    const int L = 1024 / nv < 32 ? 1024 / nv : 32;
    const int f = tid % nv, sl = tid / nv;
    if (sl < L) {
        const double *p = slab + (size_t)j * nv + f;
        const size_t stride = (size_t)m * nv;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int r = sl;
        for (; r + 3 * L < nrec; r += 4 * L) {
            s0 += p[(size_t)r * stride];
            s1 += p[(size_t)(r + L) * stride];
            s2 += p[(size_t)(r + 2 * L) * stride];
            s3 += p[(size_t)(r + 3 * L) * stride];
        }
        for (; r < nrec; r += L) s0 += p[(size_t)r * stride];
        part[sl][f] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    if (tid < nv) {
        double t = 0.0;
        for (int q = 0; q < L; ++q) t += part[q][tid];
        R[tid] = t;
    }
    __syncthreads();
    const int q = tid;
    if (q >= nm + 2) return;
    if (q >= nm) {
        cols[(size_t)(q - nm) * mp + j] = R[nf + (q - nm)];
        return;
    }
    double val;
    if (q < d) {
        const double qc = P[(size_t)j * d + q] - xmu[q];
        val = R[1 + q] - qc * R[0];
    } else {
        int e = q - d, aa = 0;
        while (e >= d - aa) { e -= d - aa; ++aa; }                       // packed pair index -> (aa, bb), aa <= bb
        const int bb = aa + e;
        const double qa = P[(size_t)j * d + aa] - xmu[aa], qb = P[(size_t)j * d + bb] - xmu[bb];
        val = R[1 + q] - qa * R[1 + bb] - qb * R[1 + aa] + qa * qb * R[0];
    }
    mom[(size_t)j * nm + q] = accumulate ? mom[(size_t)j * nm + q] + val : val;   // dPHI is a sum over the outputs (GPz.m:113)
}

bool moments_ring_fits(int kind, int de, int mp) { return kind == GPZ_KIND_COV && (de == 8 || de == 10) && mp > 256; }
int moments_ring_cols() { return 4 * RG_COLS; }
int moments_ring_features(int de) { return 1 + de + de * (de + 1) / 2; }

template <int D>
static int ring_launch(hipStream_t st, const RingMomentArgs &a, dim3 g) {
    // more than 64 KB of dynamic LDS: opted into per instantiation
    if (hipFuncSetAttribute((const void *)k_moments_ring<D>, hipFuncAttributeMaxDynamicSharedMemorySize, RG_LDS_BYTES) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_moments_ring<D>, g, dim3(256), RG_LDS_BYTES, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_moments_ring(hipStream_t st, const RingMomentArgs &a) {
    if (a.nchunk <= 0) return 0;
    dim3 g((unsigned)((a.m + 4 * RG_COLS - 1) / (4 * RG_COLS)) * (unsigned)a.nchunk);
    switch (a.d) {
        case 8: return ring_launch<8>(st, a, g);
        case 10: return ring_launch<10>(st, a, g);
        default: return -1;
    }
}

void launch_ring_finish(hipStream_t st, const double *slab, int nrec, int m, int d, const double *P, const double *xmu, int nm, int mp,
                        double *mom, double *cols, int accumulate) {
    hipLaunchKernelGGL(k_ring_finish, dim3(m), dim3(1024), 0, st, slab, nrec, m, d, moments_ring_features(d), P, xmu, nm, mp, mom, cols, accumulate);
}
