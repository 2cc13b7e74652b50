// A stand-alone host program (its own main, no GPU, never loaded into Python): the record of k_predict_noisy_missing_cov.hip against the
// direct d-dimensional density of predictNoisyMissing (predictCov.m:269-305).  The record functions of the two units are compiled for
// the host as they stand and run under the address and undefined-behaviour sanitizers:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Igpz_amd/csrc tools/pnmc_record_check.hip -o pnmc_record_check && ./pnmc_record_check
// For random patterns (d = 2 .. 10, every 1 <= no < d), random Sigma_l, C, centres and rows, psi >= 0 with one psi set to 0 in each case:
//   ln N(T x_o + s - c ; C + CU_l + Psi_hat_row)   in long double, from the d x d matrix itself, with Psi_hat_row = T Psi_oo T' assigned
//   through `unshuffle` as predictCov.m:271-273 assigns it (the kept quirk: not T Psi_oo T' in place unless [o u] is an involution)
// against lnw - 1/2 |A2 x + b2|^2 - 1/2 ln|M + Psi_oo| - 1/2 (J x + j)' (M + Psi_oo)^-1 (J x + j) from the record.  Prints the worst difference of the
// exponent, absolute and relative to 1 + |exponent|, and fails above 1e-10.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "../gpz_amd/csrc/k_predict_missing_cov.hip"
#include "../gpz_amd/csrc/k_predict_noisy_missing_cov.hip"
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

typedef long double ld;

// (the two units' launchers are compiled with them and never called here; this one lives in a third unit)
int launch_pmd_finish(hipStream_t, const double *, int, long, const double *, long, int, int, const double *, double *) { return -1; }

// ln|A| and v' A^-1 v of an n x n SPD matrix (row-major, leading dimension n) in long double
static void logdet_quad(int n, std::vector<ld> A, std::vector<ld> v, ld *logdet, ld *quad) {
    *logdet = 0;
    *quad = 0;
    for (int c = 0; c < n; ++c) {
        ld p = A[c * n + c];
        for (int q = 0; q < c; ++q) p -= A[c * n + q] * A[c * n + q];
        const ld dd = sqrtl(p);
        A[c * n + c] = dd;
        *logdet += 2 * logl(dd);
        for (int r = c + 1; r < n; ++r) {
            ld s = A[r * n + c];
            for (int q = 0; q < c; ++q) s -= A[r * n + q] * A[c * n + q];
            A[r * n + c] = s / dd;
        }
    }
    for (int r = 0; r < n; ++r) {
        ld s = v[r];
        for (int q = 0; q < r; ++q) s -= A[r * n + q] * v[q];
        v[r] = s / A[r * n + r];
        *quad += v[r] * v[r];
    }
}

static std::vector<double> random_spd(int d, std::mt19937_64 &g, double scale) {
    std::normal_distribution<double> nrm;
    std::vector<double> B(d * d), S(d * d);
    for (auto &b : B) b = nrm(g);
    for (int a = 0; a < d; ++a)
        for (int b = 0; b < d; ++b) {
            double s = a == b ? 0.3 : 0.0;
            for (int q = 0; q < d; ++q) s += B[a * d + q] * B[b * d + q];
            S[a * d + b] = scale * s / d;
        }
    return S;
}

int main() {
    std::mt19937_64 g(20261020);
    std::normal_distribution<double> nrm;
    std::uniform_real_distribution<double> uni;
    double worst_abs = 0, worst_rel = 0;
    int cases = 0;
    for (int rep = 0; rep < 12; ++rep)
        for (int d = 2; d <= PMCV_MAXD; ++d)
            for (int no = 1; no < d; ++no) {
                unsigned obs = 0;   // a random pattern with no observed dimensions
                std::vector<int> idx(d);
                for (int c = 0; c < d; ++c) idx[c] = c;
                std::shuffle(idx.begin(), idx.end(), g);
                for (int c = 0; c < no; ++c) obs |= 1u << idx[c];
                const PmcvPat pt = pmcv_pat(d, obs);
                const int nu = pt.nu;
                const std::vector<double> Sig = random_spd(d, g, std::exp(nrm(g))), Cm = random_spd(d, g, std::exp(nrm(g)));
                std::vector<double> P(d), cen(d), x(no), psi(no);
                const double far = rep % 3 == 2 ? 20.0 : 2.0;
                for (int c = 0; c < d; ++c) { P[c] = nrm(g); cen[c] = far * nrm(g); }
                for (int c = 0; c < no; ++c) { x[c] = far * nrm(g); psi[c] = std::exp(2.0 * nrm(g) - 1.0); }
                psi[(size_t)(uni(g) * no) % no] = 0.0;
                if (rep % 4 == 3) for (auto &q : psi) q = 0.0;
                // R = Sig_oo^-1 Sig_ou, CU = Sig_uu - Sig_uo R, off = P_u - R' P_o, in long double by Gauss-Jordan on [Sig_oo | Sig_ou]
                std::vector<ld> A(no * (no + nu));
                for (int a = 0; a < no; ++a) {
                    for (int b = 0; b < no; ++b) A[a * (no + nu) + b] = Sig[pt.o[a] * d + pt.o[b]];
                    for (int b = 0; b < nu; ++b) A[a * (no + nu) + no + b] = Sig[pt.o[a] * d + pt.u[b]];
                }
                for (int c = 0; c < no; ++c) {
                    const ld piv = A[c * (no + nu) + c];
                    for (int b = 0; b < no + nu; ++b) A[c * (no + nu) + b] /= piv;
                    for (int r = 0; r < no; ++r)
                        if (r != c) {
                            const ld f = A[r * (no + nu) + c];
                            for (int b = 0; b < no + nu; ++b) A[r * (no + nu) + b] -= f * A[c * (no + nu) + b];
                        }
                }
                std::vector<double> bas((size_t)no * nu + nu * nu + nu);
                double *R = bas.data(), *CU = R + no * nu, *off = CU + nu * nu;
                for (int a = 0; a < no; ++a)
                    for (int b = 0; b < nu; ++b) R[a * nu + b] = (double)A[a * (no + nu) + no + b];
                for (int a = 0; a < nu; ++a) {
                    ld s = P[pt.u[a]];
                    for (int q = 0; q < no; ++q) s -= (ld)R[q * nu + a] * P[pt.o[q]];
                    off[a] = (double)s;
                    for (int b = 0; b < nu; ++b) {
                        ld t = Sig[pt.u[a] * d + pt.u[b]];
                        for (int q = 0; q < no; ++q) t -= (ld)Sig[pt.u[a] * d + pt.o[q]] * R[q * nu + b];
                        CU[a * nu + b] = (double)t;
                    }
                }
                for (int a = 0; a < nu; ++a)
                    for (int b = 0; b < a; ++b) CU[a * nu + b] = CU[b * nu + a] = 0.5 * (CU[a * nu + b] + CU[b * nu + a]);
                // the record, as the kernels write it
                const double lnw0 = nrm(g);
                std::vector<double> rec(predict_noisy_missing_cov_rec(d, no));
                pnmc_cond_record(pt, Cm.data(), cen.data(), lnw0, bas.data(), rec.data());
                // from the record: lnw - 1/2 |A2 x + b2|^2 - 1/2 ln|M + Psi| - 1/2 (J x + j)' (M + Psi)^-1 (J x + j)
                const double *Mr = rec.data() + 1 + no, *J = Mr + no * (no + 1) / 2, *A2 = J + no * no, *b2 = A2 + nu * no;
                std::vector<ld> M(no * no), xa(no);
                ld q2 = 0;
                for (int r = 0; r < no; ++r) {
                    xa[r] = -(ld)rec[1 + r];
                    for (int c = 0; c < no; ++c) xa[r] += (ld)J[r * no + c] * x[c];
                    for (int c = 0; c <= r; ++c) M[r * no + c] = M[c * no + r] = Mr[LT(r, c)];
                    M[r * no + r] += psi[r];
                }
                for (int r = 0; r < nu; ++r) {
                    ld t = b2[r];
                    for (int c = 0; c < no; ++c) t += (ld)A2[r * no + c] * x[c];
                    q2 += t * t;
                }
                ld ldm, qm, lds, qs;
                logdet_quad(no, M, xa, &ldm, &qm);
                const ld from_rec = (ld)rec[0] - 0.5L * q2 - 0.5L * ldm - 0.5L * qm;
                // direct, in the order [o | u]: S = C + Psi_hat + T Psi T', v = T x_o + s - c
                std::vector<ld> S(d * d), v(d);
                auto T = [&](int a, int c) -> ld { return a < no ? (a == c ? 1.0L : 0.0L) : (ld)R[c * nu + (a - no)]; };
                std::vector<int> inv(d), back(d);   // inv = unshuffle; row a of T Psi T' lands at index inv[inv[a]] of [o | u]: G(inv[inv[a]], :) = T(a, :)
                for (int a = 0; a < d; ++a) inv[a < no ? pt.o[a] : pt.u[a - no]] = a;
                for (int a = 0; a < d; ++a) back[inv[inv[a]]] = a;
                auto G = [&](int a, int c) -> ld { return T(back[a], c); };
                for (int a = 0; a < d; ++a) {
                    const int pa = a < no ? pt.o[a] : pt.u[a - no];
                    ld s = (a < no ? 0.0L : (ld)off[a - no]) - cen[pa];
                    for (int c = 0; c < no; ++c) s += T(a, c) * x[c];
                    v[a] = s;
                    for (int b = 0; b < d; ++b) {
                        const int pb = b < no ? pt.o[b] : pt.u[b - no];
                        ld t = Cm[pa * d + pb];
                        if (a >= no && b >= no) t += CU[(a - no) * nu + (b - no)];
                        for (int c = 0; c < no; ++c) t += G(a, c) * psi[c] * G(b, c);
                        S[a * d + b] = t;
                    }
                }
                logdet_quad(d, S, v, &lds, &qs);
                const ld direct = (ld)lnw0 - 0.5L * lds - 0.5L * qs;
                const double da = (double)fabsl(from_rec - direct), dr = da / (1.0 + (double)fabsl(direct));
                if (da > worst_abs) worst_abs = da;
                if (dr > worst_rel) worst_rel = dr;
                ++cases;
            }
    printf("%d cases: worst |difference of the exponent| %.3e, relative to 1 + |exponent| %.3e\n", cases, worst_abs, worst_rel);
    return worst_rel <= 1e-10 ? 0 : 1;
}
