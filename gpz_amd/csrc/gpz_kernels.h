// Host-side launcher declarations shared by the translation units of libgpz_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpz_options.h"

// ---- host-side helpers shared by gpz_ctx.hip and gpz_mgpu.hip ------------------------------------------------
struct gpz_ctx;
int gpz_fail(int code, const char *fmt, ...);                      // sets gpz_last_error() of the calling thread, returns code
void gpz_ctx_attach_private(gpz_ctx *c, void *priv, void (*free_fn)(void *));   // freed by gpz_ctx_destroy
bool gpz_ctx_allreduce_is(const gpz_ctx *c, int (*fn)(void *, void *, size_t, void *), void **user);   // is this the hook in place? -> its user pointer
int gpz_ctx_device(const gpz_ctx *c);

// ---- theta unpacking (getPHI.m:24-40,117,122; GPz.m:28,32,50,98-101) -------------------------
// Device parameter block produced by k_unpack from the raw theta vector.
struct GpzParams {
    double *P;       // m x d row-major  P[j*d + c]
    double *G;       // diag kinds: gamma[j*d + c];  cov kinds: Gamma_j row-major  G[j*d*d + a*d + b]
    double *G2;      // diag kinds: gamma^2 [j*d + c]                       (unused for cov kinds)
    double *Rc;      // cov kinds: [R_j packed upper | c_j = R_j p_j], R_j = QR triangular factor of Gamma_j
    double *lnAlpha; // m x k column-major (as in theta)
    double *alpha;   // exp(lnAlpha)
    double *b;       // k
    double *v;       // m x k (zeros when homoscedastic)
    double *lnTau;   // m x k
    double *tau;     // exp(lnTau)
};

void launch_unpack(hipStream_t st, const double *theta, int method_id, int m, int d, int de, int k, int hetero,
                   GpzParams pr, int *clear2 = nullptr, double *zero_p = nullptr, int zero_n = 0);   // clear2: two status words, zero_p: zero_n doubles, set to zero by the same launch

// ---- PHI build (getPHI.m:60-125) ---------------------------------------------------------------
struct PhiArgs {
    const double *Xc;    // d x ldx, column-major over rows: Xc[c*ldx + i]
    long ldx;
    int n;               // valid rows
    int n_pad;           // rows written (rows >= n are zero-filled)
    int m, mp, d, k;
    int kind;            // GPZ_KIND_*
    const double *P, *G; // see GpzParams (G = G2 for diag kinds, Rc for cov kinds)
    const double *v;     // m x k or nullptr
    const double *b;     // k
    const double *omega; // n, or k x om_ld (omega[o*om_ld + i]: an n x k omega, GPz.m:48), or nullptr (ones)
    long om_ld;          // 0: one column for every output
    const double *Y;     // k x ldx (Y[o*ldx + i]) or nullptr: written into PHI columns m..m+k-1
    double *Phi;         // n_pad x mp row-major, or nullptr (reduction-only mode)
    double *lnbeta;      // k x ldx
    double *wbeta;       // k x ldx  (omega .* exp(-lnbeta)), or nullptr
    const double *w;     // m x k: when non-null, phiw[o*ldx + i] = sum_j PHI_ij w_jo
    double *phiw;        // k x ldx
    // diagonal kinds only (nullptr = absent): input-noise variances, observed mask (1/0), missing count per row
    const double *Psic;  // d x ldx   (fixPsi.m layout n x d, zero where missing)
    const double *Mc;    // d x ldx
    const double *ucnt;  // ldx
    // scratch for the column-group split used at small row counts ([part_groups][2][k][n_pad]: the rows of THIS launch); nullptr disables it
    double *part;
    int part_groups;
    // cov kinds, rows sorted by NaN pattern: one launch over all patterns.  wgtab holds 4 ints per workgroup:
    // {first row, end of the pattern's rows, pattern index, 0}; G then points at [pattern][m][params] and n_pad / n
    // describe the whole row set.  nullptr = one parameter set for all rows.
    const int *wgtab;
    int nwg_tab;
    // covariance kinds beside k_phi_quad (k_phi_quad.hip): the evaluation's route word; the launch runs when *route == route_want.
    // nullptr = the launch always runs.
    const int *route;
    int route_want;
};
int phi_cov_rows_per_wg(int de, int k);   // rows one workgroup of the cov-kind PHI kernel covers (granularity of wgtab)
bool phi_is_wide(int de, int k);          // d or k beyond the instantiated kernels: the runtime-d route of k_wide.hip
// runtime-d / any-k variants (k_wide.hip): same arguments and output layouts; -1 when the row tiles do not fit the LDS
int phi_wide_rows_per_wg();
int launch_phi_wide(hipStream_t st, const PhiArgs &a);
size_t prep_cov_ws_len(int m, int de);   // workspace (doubles) the QR needs when Gamma_j does not fit the LDS (de > 142), else 0
int launch_prep_cov_wide(hipStream_t st, const double *G, const double *P, int m, int de, double *Rc, double *ws);
void launch_prep_cov(hipStream_t st, const double *G, const double *P, int m, int de, double *Rc, double *ws = nullptr);
int launch_phi(hipStream_t st, const PhiArgs &a);   // returns 0, or -1 if d is not supported
// column groups of a PHI build with few rows (k_phi.hip), and the kernel that combines their per-row sums ([ngroup][2][k][a.n_pad] in part)
int phi_pick_groups(int nwg, int mp, int JB, int min_wgs, int prologue_cols, int max_groups);
void launch_phi_finalize(hipStream_t st, const double *part, int ngroup, const PhiArgs &a, const int *route, int route_want);

// ---- covariance-kind PHI on the f64 MFMA from centred row monomials (k_phi_quad.hip) ---------------------------------------------
// ln PHI = F C with the row features F_i = [1 | x' | x'_a x'_b] (x' = x - the rows' column means: the rows of Xs) and per-basis
// coefficients C_j, taken whenever a bound on the product's rounding error over the context's rows stays below GPZ_PHI_QUAD_TAU.
//
// The threshold 2^-33 = 1.16e-10 on max_j B_j, B_j = (NF + 2d + 6) 2^-53 sum_f max_i|F_if| Chat_fj:
//   * B overestimates the observed error of the exponent by about 100 x (long-double comparison on the benchmark's theta and on
//     Gamma x 10, x 100: DESIGN.md section 8), so it holds the actual |delta q| to about 1e-12, PHI to about 6e-13 relative - four
//     orders of magnitude under the 1e-8 parity gate;
//   * it lies 120 x above the bound at the benchmark's starting theta (c4 9.5e-13, c3 8.4e-13, the test problems 3 - 7e-13): an
//     optimiser can narrow the basis functions tenfold (B grows with |Gamma|^2) before the route changes;
//   * Gamma x 100 exceeds it by 50 x.
#define GPZ_PHI_QUAD_TAU 0x1p-33
#define GPZ_PHI_ROUTE_QUAD 0
#define GPZ_PHI_ROUTE_EXACT 1
bool phi_quad_fits(int kind, int de, int mp, int k);   // GC / VC, d = 8 / 10, mp > 256, one output
int phi_quad_stride(int de);                           // doubles per basis function of Cq: 4 ceil(NF / 4)
// Cq [mp][stride] from Rc ([R_j | c_j] of launch_prep_cov), P and the rows' means; fmx: max_i |F_if| over the rows (nf values);
// blockmax: ceil(mp / 64) doubles of scratch, ticket: a device word that is zero before the first launch; *bound = max_j B_j,
// *route = GPZ_PHI_ROUTE_QUAD / _EXACT.  -1: d not instantiated.
int launch_phi_quad_coef(hipStream_t st, const double *Rc, const double *P, const double *xmu, const double *fmx, int m, int mp, int de,
                         double *Cq, double *blockmax, unsigned *ticket, double *bound, int *route);
// the product for the rows a describes (what the PHI-storing launch_phi(a) delivers: PHI with its [Y | 0] columns and zero rows, ln beta,
// omega beta, the column-group split; a.w / a.phiw null, a.n_pad a multiple of 128); runs when *a.route == GPZ_PHI_ROUTE_QUAD.
// Xs: those rows' [1 | x' | 0].  -1: not launched.
int launch_phi_quad(hipStream_t st, const PhiArgs &a, const double *Xs, const double *Cq);

// ---- MFMA contractions (k_gemm.hip) ------------------------------------------------------------
// off-diagonal 128-tiles: nsplit row ranges of rows_per_split rows; diagonal tiles: nsplit_d ranges of rows_per_split_d
void launch_syrk(hipStream_t st, const double *Phi, int ld, const double *wgt, int n_rows, int mp,
                 int nsplit, int rows_per_split, int nsplit_d, int rows_per_split_d, double *slab, bool tri,
                 bool f32_operands = false);
// k_syrk_small.hip: the same product for mp <= 256 columns - the whole upper triangle of 16 x 16 blocks in one workgroup's registers,
// PHI read once; sums its per-workgroup records into S (+ mirror) itself
bool syrk_small_fits(int mp);
size_t syrk_small_slab_count(int n_rows, int mp);
void launch_syrk_small(hipStream_t st, const double *Phi, int ld, const double *wgt, int n_rows, int mp, double *slab, double *S, int lds,
                       int accumulate);
bool ltl_small_fits(int mq);                                                  // inv(SIGMA) = inv(L)' inv(L) for mq <= 512 as one launch
void launch_ltl_small(hipStream_t st, const double *W, int mq, double *S);
void launch_syrk_reduce(hipStream_t st, const double *slab, int nsplit, int nsplit_d, int mp, double *S, int lds,
                        int accumulate = 0 /* S += instead of S = (row tiles of a streamed evaluation) */);
int gpz_gemm_wave_cols();   // wave columns per 128-wide tile (slots of nupart per column tile)

// ---- few basis functions: T-GEMM + row scalars + moment sums in one kernel, T never written (k_small.hip) -----------------------
struct SmallTailArgs {
    const double *Phi; int ld;              // n_pad x ld row-major (columns m .. m+k-1 hold y)
    const double *B; int ldb;               // mp x ldb: [inv(SIGMA) | w]
    int n, n_pad, m, mp, d, kind;           // d = padded dimension of Xr / P
    int mcol;                               // column of B that holds w (= column of T that is PHI w): m + the output's index
    const double *Xs; int xs_ld;            // n_pad x xs_ld rows [1 | x - mu | 0] (xs_ld = d + 2), mu = the column means (centre of the feature
                                            // expansion); diagonal kinds with missing values: [1 | (x - mu) mk | mk | 0] (xs_ld = 2 d + 2)
    int missing;                            // 1: the masked features of a diagonal kind with missing values
    const double *y, *omega, *lnbeta, *wbeta;   // n_pad each, of THIS output (omega may be nullptr)
    const double *omega1;                   // the first column of an n x k omega (omega(training) of GPz.m:236), = omega otherwise
    const double *w, *v;                    // m; without the heteroscedastic term v = w and vscale = 0 (no branch in the kernel)
    double vscale;
    double *phiw;                           // n_pad: PHI w
    double *dphi; int ldd;                  // when non-null: dPHI (n_pad x ldd, GPz.m:113) is written as well - the input-noise route of the diagonal
                                            // kinds takes its moment sums from it (k_moments_diag), with nf = 0 features here
    double *slab;                           // [nwg][m][nf + 2]: raw sums about xmu, PHI'c, PHI'dbeta
    double *partial;                        // [nwg][GPZ_NS]: sum c delta, sum omega delta^2, sum LL, sum dbeta
    int ncu;                                // compute units (set by the launcher)
    int stagger;                            // start delay of the second workgroup of a compute unit, in s_sleep(127) units of 8128 cycles (set by the launcher)
    int nf;                                 // features: 1 + 2d (diagonal kinds), 1 + d + d(d+1)/2 (covariance kinds)
};
int small_tail_features(int kind, int d, bool missing);
bool small_tail_fits(int kind, int d, int m, int k, int mp, bool missing);   // mp <= 256 columns, <= 32 features, y columns in one block
int small_tail_nwg();                            // persistent workgroups: two per compute unit
void launch_small_tail(hipStream_t st, const SmallTailArgs &a, int nwg);
void launch_small_finish(hipStream_t st, const double *slab, const double *partial, int nwg, int m, int d, int kind, int nf, int missing,
                         const double *P, const double *xmu, int nm, int mp, double *mom, double *cols,
                         double *scal, int accumulate, int cols_only = 0);   // cols_only: records without raw sums (nf = 0)   // the workgroups' records -> moments, column sums, scalar sums (one launch)
int gpz_cu_count();         // compute units of the current device (k_gemm.hip)
// ---- predictFull for few basis functions as one kernel (k_predict_small.hip; the streaming predictor, gpz_predictor.hip) -----------
// fits: an instantiated d (phi_is_wide false) and ceil16(m + 2k) <= 256.  Xc: de x ldx column layout (dimensions >= d zero), n rows;
// B: k blocks (stride bstride) of ceil16(m) x ldb row-major [inv(Sigma_o) | w | v | 0], ldb = ceil16(m + 2k); out: [3k][ldo] = mu, nu, beta;
// phi (optional): [m][ldphi].  Returns -1 when the launch failed.
bool predict_small_fits(int de, int m, int k);
size_t predict_small_lds(int de);
int launch_predict_small(hipStream_t st, int kind, int de, const double *Xc, long ldx, int n, int m, int k, const double *P,
                         const double *G, const double *B, int ldb, long bstride, const double *bvec, double *out, long ldo,
                         double *phi, long ldphi);
// ---- posterior draws of the predictive mean (k_predict_draws.hip; gpz_predictor_draws) -------------------------------------------
// fits: an instantiated d (phi_is_wide(de, 1) false) and ceil16(m) <= 256.  F = PHI W for the n rows of Xc (as launch_predict_small);
// W: ceil16(m) x ldw row-major (ldw % 16 == 0, columns >= ncol zero); out: [ncol][ldo].  Returns -1 when the launch failed.
bool predict_draws_fits(int de, int m);
size_t predict_draws_lds(int de);
int launch_predict_draws(hipStream_t st, int kind, int de, const double *Xc, long ldx, int n, int m, const double *P, const double *G,
                         const double *W, int ldw, int ncol, double *out, long ldo);
// W (rows x ldw row-major) <- [W_0 | .. | W_{k-1} | 0], W_o(:, s) = w(:, o) + R_o z(:, s, o): z from Z (m x nd x k column-major) or, Z null,
// Philox4x32-10 of (seed; j, s, o, 0) through Box-Muller.  R: m x m x k column-major.  Rows >= m zero.
void launch_draws_weights(hipStream_t st, const double *w, const double *R, const double *Z, unsigned long long seed, int m, int nd,
                          int k, int rows, int ldw, double *W);
// S (m x m) <- (iS + iS') / 2;  A (mq x mq row-major) <- S, the identity on the padding (the input of launch_chol_step)
void launch_draws_sym(hipStream_t st, const double *iS, int m, int mq, double *S, double *A);
// after the Cholesky steps: R (m x m column-major) <- the lower factor in Lm; *ok = 1 unless a pivot failed or min L_jj^2 <= m eps max S_jj
void launch_draws_chol_check(hipStream_t st, const double *Lm, int mq, const double *S, int m, const int *info, double *R, int *ok);
// ---- stacked predictive densities per group and per column (k_predict_stack.hip; gpz_predictor_stack) ---------------------------
// One tile: out [3k][nt] (mu, nu, beta) and dout [nd k][nt] (draw s of output o in row o nd + s) as the kernels above leave them, lab
// (nt labels in [-1, G), nullptr: all 0), wt (nt weights, nullptr: all 1), edges [k][B + 1].  Column-output q = c k + o < (1 + nd) k:
// c = 0 the posterior-mean weights (width^2 = nu + beta), c = 1 + s draw s (width^2 = beta).  Every one of the R row slabs writes a
// record of G B bin masses + [G][3] sums of omega, omega y, omega y^2 with y = mu + shift[o] per q: slab [R][(1 + nd) k][G B + 3 G].  launch_stack_accum adds
// the R slabs (count doubles each) to acc in slab order.  Both return -1 when the launch failed.
size_t predict_stack_lds(int G, int B);
int predict_stack_slabs(long Q, long rec, long T);   // R: a function of the column count, the record length and the tile rows only
int launch_stack_tile(hipStream_t st, const double *out, const double *dout, const int *lab, const double *wt, const double *edges,
                      const double *shift, long nt, int k, int nd, int B, int G, int R, double *slab);
int launch_stack_accum(hipStream_t st, const double *slab, int R, size_t count, double *acc);
// ---- device-resident entries of the streaming predictor (k_predict_dev.hip; gpz_predictor_*_dev) ----------------------------------
// X: the caller's rows on the device, f64 or f32 (f32 != 0), element (i, c) at X[i rs + c cs].  check: rec[0] |= 1 when an element of
// the ns rows is NaN, rec[1] when a label (lab, ns values or nullptr) is outside [-1, G), rec[2] when a weight (wt, ns values or nullptr)
// is negative or not finite.  stage: rows r0 .. r0 + nt - 1 -> Xc [d][ldx] as (x - muX[c]) / sdX[c] (muX nullptr: x itself).
// finish: out [3k][nt] -> column-major ns x k arrays at row r0 (mu + muY[o], sigma = nu + beta + gamma; sigma and gamma may be nullptr).
// phi: [m][nt] -> column-major ns x m at row r0.  draws finish: dout [nd k][nt] -> F column-major ns x k x nd, + muY[o].  muY may be
// nullptr.  All return -1 when the launch failed.
int launch_pred_check_dev(hipStream_t st, const void *X, int f32, long ns, int d, long rs, long cs, const int *lab, int G,
                          const double *wt, unsigned *rec);
int launch_pred_stage(hipStream_t st, const void *X, int f32, long rs, long cs, long r0, int nt, int d, const double *muX,
                      const double *sdX, double *Xc, long ldx);
int launch_pred_finish_dev(hipStream_t st, const double *out, int nt, int k, const double *muY, long ns, long r0, double *mu,
                           double *sigma, double *nu, double *beta, double *gamma);
int launch_pred_phi_dev(hipStream_t st, const double *phi, int nt, int m, long ns, long r0, double *PHI);
int launch_draws_finish_dev(hipStream_t st, const double *dout, int nt, int k, int nd, const double *muY, long ns, long r0, double *F);
// ---- rows with input noise through the streaming predictor (k_predict_noisy.hip; gpz_predictor_*_noisy*) --------------------------
// fits: a diagonal kind, an instantiated de <= 20, k <= 8 and ceil16(m) <= 256 (the limit of the fused draws; 1024 with large_m).  Psi: per-dimension
// variances in the layout of Xc ([d][ldx], dimensions >= d zero).  The pair records are predict_noisy_rec(d, k) = 1 + 2 d + 3 k doubles:
// launch_pair_table (record stride rec) writes [lnZ | c_ab | C_ab], launch_noisy_pair_coef the 3 k coefficients behind them (iS: m x m x k
// column-major, read at a >= b only).  launch_predict_noisy_small: part [nchunk][5k][ldp] -> out [4k][n] = mu | nu | beta | gamma.
// predict_noisy_chunks: the pair chunks, a function of the model's shape only - never of the rows - so that a row's results have the
// same bits for any tile size, position and row order.  The launchers return -1 when a launch failed.
// large_m (a handle with GPZ_PREDICT_LARGE_M): ceil16(m) <= GPZ_PREDICT_LARGE_M_MAX in place of 256, for this fits and the covariance
// kinds' below.  launch_predict_noisy_phi: Phi [nrow][mp] row-major <- E_x[PHI] of the n rows, zeros in rows >= n and columns >= m (what
// launch_tgemm takes); nrow a multiple of 64; nchunk splits the columns over gridDim.y and changes no bit.
#define GPZ_PREDICT_LARGE_M_MAX 1024
bool predict_noisy_fits(int kind, int de, int m, int k, bool large_m = false);
int predict_noisy_chunks(int m, int d, int k);
int launch_predict_noisy_phi(hipStream_t st, int d, int de, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m, int mp,
                             const double *P, const double *G2, int nchunk, double *Phi);
int predict_noisy_rec(int d, int k);
int launch_noisy_pair_coef(hipStream_t st, int m, int k, int d, const double *w, const double *v, const double *iS, double *tab, int rec);
int launch_predict_noisy_small(hipStream_t st, int d, int de, const double *Xc, const double *Psic, long ldx, int n, int m, int k,
                               const double *P, const double *G2, const double *w, const double *v, const double *bvec,
                               const double *tab, int nchunk, double *part, long ldp, double *out);
// launch_predict_draws for rows with Psi (diagonal kinds): 32 * de more doubles of LDS for the block's rows of Psi
size_t predict_draws_psi_lds(int de);
int launch_predict_draws_psi(hipStream_t st, int de, const double *Xc, const double *Psic, long ldx, int n, int m, const double *P,
                             const double *G, const double *W, int ldw, int ncol, double *out, long ldo);
// check: rec[3] |= 1 when an element of the caller's Psi (as X: f64 or f32, element (i, c) at Psi[i rs + c cs], cs = 0 for n x 1) is NaN,
// negative, or infinite itself or divided by smin (the smallest sd2; 1 without one).  stage: rows r0 .. r0 + nt - 1 -> Psic [d][ldx] as double(psi) / sd2[c] (sd2 nullptr: psi itself).  finish:
// out [4k][nt] -> column-major ns x k arrays at row r0 (mu + muY[o], gamma, sigma = (nu + beta) + gamma; sigma and gamma may be nullptr).
int launch_pred_check_psi(hipStream_t st, const void *Psi, int f32, long ns, int d, long rs, long cs, double smin, unsigned *rec);
int launch_pred_stage_psi(hipStream_t st, const void *Psi, int f32, long rs, long cs, long r0, int nt, int d, const double *sd2,
                          double *Psic, long ldx);
int launch_pred_finish_noisy_dev(hipStream_t st, const double *out, int nt, int k, const double *muY, long ns, long r0, double *mu,
                                 double *sigma, double *nu, double *beta, double *gamma);
// the finish kernel behind launch_predict_noisy_small, on its own: part [nchunk][5k][ldp] -> out [4k][n]
int launch_predict_noisy_finish(hipStream_t st, const double *part, int nchunk, long ldp, int n, int k, const double *bvec, double *out);
// ---- rows with input noise, covariance kinds (k_predict_noisy_cov.hip; gpz_predictor_*_noisy_cov_dev) -------------------------------
// fits: GC or VC, 1 <= d <= 10, 1 <= k <= 8 and ceil16(m) <= 256 (1024 with large_m).  Xc, Psic: [d][ldx] as above.  The tables are the model's alone:
// basis records brec [m][predict_noisy_cov_brec(d, k)] = [1/2 ln|Sigma_j| | p_j | Sigma_j packed lower | w_j (k) | v_j (k)], pair records
// prec [m (m + 1) / 2][predict_noisy_cov_prec(d, k)] = [lnZ | c_ab | C_ab packed lower | 3 k coefficients as gpz_pair_coef writes them].
// launch_noisy_cov_records repacks them from launch_gen_prep's Sig (m x d x d) and lnS (m) and launch_pair_table's records (raw,
// 1 + d + d d doubles each; prec and raw nullptr: the basis records only).  launch_predict_noisy_cov_small: part [nchunk][5k][ldp] ->
// out [4k][n] = mu | nu | beta | gamma.  launch_predict_noisy_cov_phi: Phi [nrow][mp] row-major <- E_x[PHI] of the n rows, zeros in rows
// >= n and columns >= m (what launch_tgemm takes).  shared: GC, one covariance for every basis function.  nchunk =
// predict_noisy_cov_chunks(m, d, k), the model's shape only.  The launchers return -1 when a launch failed or d is outside 1 .. 10.
bool predict_noisy_cov_fits(int kind, int d, int m, int k, bool large_m = false);
int predict_noisy_cov_chunks(int m, int d, int k);
int predict_noisy_cov_brec(int d, int k);
int predict_noisy_cov_prec(int d, int k);
int launch_noisy_cov_records(hipStream_t st, int m, int d, int de, int k, const double *P, const double *Sig, const double *lnS,
                             const double *raw, const double *w, const double *v, const double *iS, double *brec, double *prec);
int launch_predict_noisy_cov_small(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m, int k,
                                   const double *brec, const double *prec, const double *bvec, int nchunk, double *part, long ldp,
                                   double *out);
int launch_predict_noisy_cov_phi(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int nrow,
                                 int m, int mp, int k, const double *brec, int nchunk, double *Phi);
// ---- gamma under every weight draw for rows with input noise (k_predict_noisy_gamma.hip; gpz_predictor_stack_noisy*, _draws_gamma_noisy_dev)
// part [nchunk][ncol][ldp] <- per pair chunk sum_{a >= b} f_ab E[phi_a phi_b](x_i, psi_i) W[a, col] W[b, col] for the n rows of Xc / Psic
// ([d][ldx]); tab: the handle's pair records (rec doubles apart, [lnZ | c_ab | C_ab] read), W: ceil16(m) x ldw row-major as the draws
// take it (column o nd + s), nchunk = predict_gamma_chunks(m), the model's shape alone.  finish_dev: gamma_s = sum - mu_s^2 with mu_s =
// dout [ncol][nt] -> Gam (ns x k x nd column-major, rows r0 ..).  finish_s2: the stack's widths s2 [(1 + nd) k][nt]: row o = (nu + beta) +
// gamma of nout ([4k][nt]), row (1 + s) k + o = beta + max(gamma_s, 0); nd = 0 reads neither part nor dout.
// launch_stack_tile_w (k_predict_stack_w.hip): launch_stack_tile with the width^2 of column-output q and row i read from s2[q nt + i] and
// column 0's mu from row o of out.  All return -1 when a launch failed.
int predict_gamma_chunks(int m);
int launch_predict_noisy_gamma(hipStream_t st, int d, const double *Xc, const double *Psic, long ldx, int n, int m, const double *tab,
                               int rec, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp);
int launch_gamma_finish_dev(hipStream_t st, const double *part, int nchunk, long ldp, const double *dout, int nt, int k, int nd, long ns,
                            long r0, double *Gam);
int launch_gamma_finish_s2(hipStream_t st, const double *part, int nchunk, long ldp, const double *nout, const double *dout, int nt, int k,
                           int nd, double *s2);
int launch_stack_tile_w(hipStream_t st, const double *out, const double *s2, const double *dout, const int *lab, const double *wt,
                        const double *edges, const double *shift, long nt, int k, int nd, int B, int G, int R, double *slab);
// ---- the same for a covariance kind (k_predict_noisy_cov_gamma.hip; gpz_predictor_stack_noisy_cov_dev, _draws_gamma_noisy_cov_dev) ----
// part [nchunk][ncol][ldp] <- per pair chunk sum_{a >= b} f_ab z_ab(x_i, psi_i) W[a, col] W[b, col] with k_predict_noisy_cov_small's pair
// density; tab: the handle's packed pair records (prec above, rec = predict_noisy_cov_prec(d, k) doubles apart, the head [lnZ | c_ab |
// C_ab packed lower] read), shared: GC.  nchunk = predict_gamma_chunks(m); the finish kernels and the stack kernel are the ones above.
// Returns -1 when the launch failed or d is outside 1 .. 10.
int launch_predict_noisy_cov_gamma(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m,
                                   const double *tab, int rec, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp);
// ---- a full input-noise covariance per row, covariance kinds (k_predict_psi_cube.hip, k_predict_psi_cube_gamma.hip;
// gpz_predictor_*_psi_cube_dev) ----
// The launchers of the three groups above with Psic [d (d + 1) / 2][ldx]: column LT(r, c) holds element (r, c), r >= c, of every row's
// Psi (after fixPsi's division), and the density's matrix is S + Psi_i over the whole packed triangle.  Tables, chunk counts
// (predict_noisy_cov_chunks, predict_gamma_chunks), partial sums and finish kernels are theirs.  check: word 3 of rec is set when an
// element of a lower triangle is NaN or infinite, itself or divided by div[LT(r, c)] (device, nullptr: no division), or a diagonal
// element is negative.  stage: element (r, c) of row i at Psi[r sr + c sc + i sn] -> Psic.  All return -1 when a launch failed or d is
// outside 1 .. 10.
int launch_pred_check_psi_cube(hipStream_t st, const void *Psi, int f32, long ns, int d, long sr, long sc, long sn, const double *div,
                               unsigned *rec);
int launch_pred_stage_psi_cube(hipStream_t st, const void *Psi, int f32, long sr, long sc, long sn, long r0, int nt, int d,
                               const double *div, double *Psic, long ldx);
int launch_predict_psi_cube_small(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m, int k,
                                  const double *brec, const double *prec, const double *bvec, int nchunk, double *part, long ldp,
                                  double *out);
int launch_predict_psi_cube_phi(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m,
                                int mp, int k, const double *brec, int nchunk, double *Phi);
int launch_predict_psi_cube_gamma(hipStream_t st, int d, bool shared, const double *Xc, const double *Psic, long ldx, int n, int m,
                                  const double *tab, int rec, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp);
// ---- rows with missing inputs through the streaming predictor, with or without input noise (k_predict_missing.hip,
// k_predict_noisy_missing.hip, the pair kernels' body in k_predict_group_impl.h; gpz_predictor_*_missing_dev, _*_noisy_missing_dev) ----
// One group of rows sharing a NaN pattern; obs: bit c set = dimension c observed.  fits: a diagonal kind, an instantiated de <= 20,
// k <= 8 and ceil16(m) <= 256.  launch_pmd_tables (per pattern and priors): bt [2][mp], NijS [mp][mp] and, with pairs, the records
// (predict_missing_groups(m) * 64 of predict_missing_rec(d, k) = 1 + 2 d + 3 k doubles) and U (predict_missing_groups(m) * 64 * ceil16(m)
// doubles in fragment order).  launch_pnm_records (per handle) writes the second record table, for rows with Psi: as many records of as
// many doubles, [lnZ without the ln det of the observed block | c | C | coefficients], the model's alone.
// Psic: nullptr, or the tile's Psi in the layout of Xc for a group with input noise too; rec is then the second table, and every loop
// over dimensions runs over the set bits of obs.  Per tile: launch_pmd_no (No, Pio: nrow rows of mp, rows >= n zero; widened by psi:
// k_pnm_no), launch_tgemm, launch_pmd_phi (PHI over No; hd [2k][ldh] = PHI w | PHI v), launch_predict_missing_pairs
// (k_predict_missing_pairs or k_predict_noisy_missing_pairs: part [predict_missing_chunks(m)][3k][ldp] -> out [4k][n] = mu | nu | beta |
// gamma; launch_pmd_finish inside).  The chunk count is a function of m alone.  The launchers return -1 when a launch failed.
bool predict_missing_fits(int kind, int de, int m, int k);
int predict_missing_rec(int d, int k);
long predict_missing_groups(int m);
int predict_missing_chunks(int m);
size_t predict_missing_lds(int m, int d, int k, bool psi);   // dynamic LDS of the pair kernels, bytes
int launch_pmd_check(hipStream_t st, const void *X, int f32, long ns, int d, long rs, long cs, unsigned obs, unsigned *rec);
int launch_pmd_tables(hipStream_t st, int m, int mp, int d, int de, int k, unsigned obs, const double *P, const double *G2,
                      const double *priors, const double *w, const double *v, const double *iS, double *bt, double *NijS, double *U,
                      double *rec, bool pairs);
int launch_pnm_records(hipStream_t st, int m, int d, int de, int k, const double *P, const double *G2, const double *w, const double *v,
                       const double *iS, double *rec);
int launch_pmd_no(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m, int mp, int d, int de,
                  unsigned obs, const double *P, const double *G2, const double *bt, double *No, double *Pio);
int launch_pmd_phi(hipStream_t st, double *No, const double *T, int n, int m, int mp, int k, const double *w, const double *v, double *hd,
                   long ldh);
int launch_predict_missing_pairs(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio, int ldpio, int m,
                                 int d, int k, unsigned obs, const double *U, const double *rec, int nchunk, double *part, long ldp,
                                 const double *hd, long ldh, const double *bvec, double *out);
// the finish kernel behind the pair kernel, on its own: hd [2k][ldh] = mu | ElnS - b and part [nchunk][3k][ldp] -> out [4k][n]
int launch_pmd_finish(hipStream_t st, const double *part, int nchunk, long ldp, const double *hd, long ldh, int n, int k,
                      const double *bvec, double *out);
// launch_pred_check_psi (k_predict_noisy.hip) for such a group: word 3 of rec is set when Psi is NaN, negative or infinite in an observed
// dimension; the missing ones are not read, and with obs == 0 nothing is launched
int launch_pnm_check_psi(hipStream_t st, const void *Psi, int f32, long ns, int d, long rs, long cs, unsigned obs, double smin,
                         unsigned *rec);
// ---- gamma under every weight draw for such a group (k_predict_missing_gamma.hip, k_predict_noisy_missing_gamma.hip;
// gpz_predictor_stack_missing_dev, _draws_gamma_missing_dev and their _noisy_missing_ forms).  part [nchunk][ncol][ldp] <- per pair chunk
// sum_{a >= b} f_ab EcC_ab(x_i) W[a, col] W[b, col] for the n rows of the tile (with Psic: EcC_ab(x_i, psi_i)): Xc, Psic, Pio, U and rec as
// launch_predict_missing_pairs takes them (of a record only [lnZ | c | 1 / C], with Psic [lnZ | c | C], is read), W >= m rows x ldw
// row-major as the draws take it (column o nd + s, ldw a multiple of 16, columns >= ncol zero), nchunk = predict_missing_chunks(m).
// launch_gamma_finish_dev / _s2 (above) take part from there, with nout = the missing tile's out.  Returns -1 when a launch failed.
size_t predict_missing_gamma_lds(int m, int d, bool psi);   // dynamic LDS of the gamma kernels, bytes
int launch_predict_missing_gamma(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio, int ldpio, int m,
                                 int d, int k, unsigned obs, const double *U, const double *rec, const double *W, int ldw, int ncol,
                                 int nchunk, double *part, long ldp);
// ---- the same two products past ceil16(m) = 256, for a handle with GPZ_PREDICT_LARGE_M_MISSING (k_pml_pairs.hip, k_pml_gamma.hip, the
// body in k_predict_group_large_impl.h): Pio passes through LDS in K panels of GPZ_PML_KP columns and a workgroup keeps the accumulators
// of GPZ_PML_GB groups of 64 pairs, so LDS does not grow with m.  fits: predict_missing_fits with ceil16(m) <= GPZ_PREDICT_LARGE_M_MAX.
// The tables, the chunk count (predict_missing_chunks), the slabs and the finish are launch_predict_missing_pairs' / _gamma's, and so
// are the arguments.  gamma: the LDS of the gamma kernels (the short record and the group's (a, b)).
#define GPZ_PML_KP 128   // columns of Pio per K panel
#define GPZ_PML_GB 4     // groups of 64 pairs per batch
#define GPZ_PML_GB8 2    // the same with 8 outputs in registers (k > 1, the pairs sink)
bool predict_missing_large_fits(int kind, int de, int m, int k);
size_t predict_missing_large_lds(int m, int d, int k, bool psi, bool gamma = false);   // dynamic LDS, bytes; the same for every m
int launch_predict_missing_large_pairs(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio, int ldpio,
                                       int m, int d, int k, unsigned obs, const double *U, const double *rec, int nchunk, double *part,
                                       long ldp, const double *hd, long ldh, const double *bvec, double *out);
int launch_predict_missing_large_gamma(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio, int ldpio,
                                       int m, int d, int k, unsigned obs, const double *U, const double *rec, const double *W, int ldw,
                                       int ncol, int nchunk, double *part, long ldp);
// ---- rows with missing inputs, covariance kinds (k_predict_missing_cov.hip; gpz_predictor_*_missing_cov_dev) --------------------------
// One group of rows sharing a NaN pattern with no observed dimensions.  fits: GC or VC, 1 <= d <= 10, 1 <= k <= 8, ceil16(m) <= 256.
// A record is predict_missing_cov_rec(no) = 1 + no + no (no + 1) / 2 doubles, [lnw | a | U]: -1/2 q = lnw - 1/2 |U (x_o - a)|^2.
// launch_pmcv_tables (per pattern and priors; Sig m x d x d and lnS from launch_gen_prep): bas [m][predict_missing_cov_bas(d, no)],
// the m Ex records, the m * m PHI records and, with coef, the 3 k coefficients of every pair as gpz_pair_coef writes them.
// launch_pmcv_rows (per tile): Pio [m][ldr], Phi [nrow][mp] (rows >= n and columns >= m zero, what launch_tgemm takes) and hd [2k][ldh] =
// PHI w | PHI v.  launch_predict_missing_cov_pairs: per slab of predict_missing_cov_slab_pairs(m, no) whole pairs (there are
// predict_missing_cov_slabs(m, no) of them, at most 64 MB each) k_pmc_triples from raw (launch_pair_table's records, 1 + d + d d doubles)
// into slab and k_predict_missing_cov_pairs, part [predict_missing_cov_chunks(m)][3k][ldp] -> out [4k][n] = mu | nu | beta | gamma
// (launch_pmd_finish inside).  *slab_kept: the slab holds the pattern's whole table (one slab) and is not written again; the caller clears
// it when bas or raw change.  Chunks and slabs are functions of m and no alone.  The launchers return -1 when a launch failed.
bool predict_missing_cov_fits(int kind, int d, int m, int k);
int predict_missing_cov_rec(int no);
int predict_missing_cov_bas(int d, int no);
int predict_missing_cov_chunks(int m);
int predict_missing_cov_slabs(int m, int no);
long predict_missing_cov_slab_pairs(int m, int no);
size_t predict_missing_cov_lds(int m, int no, int k);   // dynamic LDS of the pair kernel, bytes
int launch_pmcv_tables(hipStream_t st, int m, int d, int de, int k, unsigned obs, const double *P, const double *Sig, const double *lnS,
                       const double *priors, const double *w, const double *v, const double *iS, double *bas, double *exrec,
                       double *phirec, double *coef);
int launch_pmcv_rows(hipStream_t st, const double *Xc, long ldx, int n, int nrow, int m, int mp, int d, int k, unsigned obs,
                     const double *exrec, const double *phirec, const double *w, const double *v, double *Pio, long ldr, double *Phi,
                     double *hd, long ldh);
int launch_pmc_triples(hipStream_t st, int d, unsigned obs, long q0, long cnt, int m, const double *raw, const double *bas, double *slab);
int launch_predict_missing_cov_pairs(hipStream_t st, const double *Xc, long ldx, int n, const double *Pio, long ldr, int m, int d, int k,
                                     unsigned obs, const double *raw, const double *bas, const double *coef, double *slab,
                                     bool *slab_kept, int nchunk, double *part, long ldp, const double *hd, long ldh, const double *bvec,
                                     double *out);
// launch_predict_missing_cov_gamma (k_predict_missing_cov_gamma.hip; gpz_predictor_stack_missing_cov_dev, _draws_gamma_missing_cov_dev): the
// pair sums of such a group under every column of W (ceil16(m) x ldw row-major, ncol <= ldw columns, ldw a multiple of 16) -> part
// [predict_missing_cov_chunks(m)][ncol][ldp], from Pio of launch_pmcv_rows and the slabs as the pair kernel reads them: a slab that is not
// kept is written here (launch_pmc_triples) and *slab_kept set as launch_predict_missing_cov_pairs sets it.  launch_gamma_finish_dev / _s2
// take part from there.  Returns -1 when a launch failed.
size_t predict_missing_cov_gamma_lds(int m, int no);   // dynamic LDS of the gamma kernel, bytes
int launch_predict_missing_cov_gamma(hipStream_t st, const double *Xc, long ldx, int n, const double *Pio, long ldr, int m, int d,
                                     unsigned obs, const double *raw, const double *bas, double *slab, bool *slab_kept, const double *W,
                                     int ldw, int ncol, int nchunk, double *part, long ldp);
int launch_pmcv_hd(hipStream_t st, const double *Phi, int n, int m, int mp, int k, const double *w, const double *v, double *hd, long ldh);
// ---- rows with input noise and missing inputs, covariance kinds (k_predict_noisy_missing_cov.hip; gpz_predictor_*_noisy_missing_cov_dev)
// The launchers above with Psic [d][ldx] beside Xc and records of predict_noisy_missing_cov_rec(d, no) doubles, [lnw | -j | M packed lower
// triangle | J | A2 | b2] (the unit's head says what they are).  launch_pnmc_tables: the Ex and PHI tables of the pattern from bas as
// launch_pmcv_tables left it (coef is that launcher's too).  The pair launcher writes each slab itself (k_pnmc_triples):
// predict_noisy_missing_cov_slabs(m, d, no) slabs of predict_noisy_missing_cov_slab_pairs whole pairs, at most 64 MB each; chunks:
// predict_missing_cov_chunks(m).  Patterns with 1 <= no < d only.  The launchers return -1 when a launch failed.
int predict_noisy_missing_cov_rec(int d, int no);
int predict_noisy_missing_cov_slabs(int m, int d, int no);
long predict_noisy_missing_cov_slab_pairs(int m, int d, int no);
size_t predict_noisy_missing_cov_lds(int m, int d, int no, int k);   // dynamic LDS of the pair kernel, bytes
int launch_pnmc_tables(hipStream_t st, int m, int d, int de, unsigned obs, const double *P, const double *Sig, const double *lnS,
                       const double *priors, const double *bas, double *exrec, double *phirec);
int launch_pnmc_rows(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, int nrow, int m, int mp, int d, int k,
                     unsigned obs, const double *exrec, const double *phirec, const double *w, const double *v, double *Pio, long ldr,
                     double *Phi, double *hd, long ldh);
int launch_predict_noisy_missing_cov_pairs(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio,
                                           long ldr, int m, int d, int k, unsigned obs, const double *raw, const double *bas,
                                           const double *coef, double *slab, bool *slab_kept, int nchunk, double *part, long ldp,
                                           const double *hd, long ldh, const double *bvec, double *out);
// launch_pnmc_triples: the records of cnt whole pairs from pair q0 into slab, as the pair launcher writes them (launch_pmc_triples' twin).
// launch_predict_noisy_missing_cov_gamma (k_predict_noisy_missing_cov_gamma.hip; gpz_predictor_stack_noisy_missing_cov_dev,
// _draws_gamma_noisy_missing_cov_dev): launch_predict_missing_cov_gamma with Psic and this unit's records and slabs -> part
// [predict_missing_cov_chunks(m)][ncol][ldp], from Pio of launch_pnmc_rows; a slab that is not kept is written here and *slab_kept set
// as launch_predict_noisy_missing_cov_pairs sets it.  Returns -1 when a launch failed.
int launch_pnmc_triples(hipStream_t st, int d, unsigned obs, long q0, long cnt, int m, const double *raw, const double *bas, double *slab);
size_t predict_noisy_missing_cov_gamma_lds(int m, int d, int no);   // dynamic LDS of the gamma kernel, bytes
int launch_predict_noisy_missing_cov_gamma(hipStream_t st, const double *Xc, const double *Psic, long ldx, int n, const double *Pio,
                                           long ldr, int m, int d, unsigned obs, const double *raw, const double *bas, double *slab,
                                           bool *slab_kept, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp);
// ---- such a group whose rows have a full d x d Psi each (k_predict_psi_cube_missing.hip, k_predict_psi_cube_missing_gamma.hip;
// gpz_predictor_*_psi_cube_missing_dev) ----
// The launchers of the group above with Psio [no (no + 1) / 2][ldx] in place of Psic: column LT(ro, co) holds element (o[ro], o[co]),
// ro >= co, of every row's Psi (after fixPsi's division), o the observed dimensions in ascending order, and the density's matrix is
// M + Psi_oo over the whole packed triangle.  Records, tables, slabs (the same slab and *slab_kept: the records do not depend on Psi),
// chunk counts, LDS figures and finish kernels are that group's.  check: word 3 of rec is set when an element of the lower triangle of an
// observed x observed block is NaN or infinite, itself or divided by div[LT(r, c)] (the whole d x d triangle of divisors on the device,
// nullptr: no division), or a diagonal element is negative; nothing observed: nothing is launched.  stage: element (r, c) of row i at
// Psi[r sr + c sc + i sn] -> Psio.  All return -1 when a launch failed or a shape is outside predict_missing_cov_fits.
int launch_pcm_check_psi(hipStream_t st, const void *Psi, int f32, long ns, int d, unsigned obs, long sr, long sc, long sn,
                         const double *div, unsigned *rec);
int launch_pcm_stage_psi(hipStream_t st, const void *Psi, int f32, long sr, long sc, long sn, long r0, int nt, int d, unsigned obs,
                         const double *div, double *Psio, long ldx);
int launch_pcm_rows(hipStream_t st, const double *Xc, const double *Psio, long ldx, int n, int nrow, int m, int mp, int d, int k,
                    unsigned obs, const double *exrec, const double *phirec, const double *w, const double *v, double *Pio, long ldr,
                    double *Phi, double *hd, long ldh);
int launch_predict_psi_cube_missing_pairs(hipStream_t st, const double *Xc, const double *Psio, long ldx, int n, const double *Pio,
                                          long ldr, int m, int d, int k, unsigned obs, const double *raw, const double *bas,
                                          const double *coef, double *slab, bool *slab_kept, int nchunk, double *part, long ldp,
                                          const double *hd, long ldh, const double *bvec, double *out);
int launch_predict_psi_cube_missing_gamma(hipStream_t st, const double *Xc, const double *Psio, long ldx, int n, const double *Pio,
                                          long ldr, int m, int d, unsigned obs, const double *raw, const double *bas, double *slab,
                                          bool *slab_kept, const double *W, int ldw, int ncol, int nchunk, double *part, long ldp);
// B (rows x ld row-major) <- [iS (m x m column-major) | nw columns of W from column wcol | nv columns of V (nullptr: 0) from vcol | 0]
void launch_pred_fill_b(hipStream_t st, const double *iS, const double *W, int nw, int wcol, const double *V, int nv, int vcol, int m,
                        int rows, int ld, double *B);
// tile route: out [3k][ldo] = [phiw | sum of the nslots nu partials (stride ldn, output stride ostride) | exp(lnbeta)]
void launch_pred_tile_finish(hipStream_t st, const double *phiw, const double *nupart, int nslots, long ldn, long ostride,
                             const double *lnbeta, long ldt, int n, int k, double *out, long ldo);
// nupart (optional): [gpz_gemm_wave_cols()*ceil(mp/128)][n_pad] per-wave-column partial sums of PHI.*T over columns < m; phiw: column mcol of T
void launch_tgemm(hipStream_t st, const double *Phi, int ld, const double *B, int ldb, double *T, int n_pad, int mp,
                  double *nupart, double *phiw, int m, int mcol, bool f32_operands = false, int kdim = 0, int ldt = 0,
                  const float *B32 = nullptr);   // B32 (with f32_operands): B rounded to fp32 by launch_round_f32, same leading dimension
void launch_round_f32(hipStream_t st, const double *src, float *dst, size_t n);
// ---- T = PHI * B on the int8 matrix pipe (k_oz.hip): 7 x 7 digit planes, 28 exact int32 products --------------------------------
size_t oz_a_bytes(long n_pad, int mp);
size_t oz_b_bytes(int mp);
int oz_prepare_device();   // once per device, before the first launch_oz_tgemm
void launch_oz_slice_a(hipStream_t st, const double *Phi, int ld, long n_pad, int m, int mp, char *Apl);      // PHI in [0, 1], columns < m
void launch_oz_slice_b(hipStream_t st, const double *B, int ldb, int krows, int mp, double *cs, char *Bpl);   // cs: mp column scales
void launch_oz_tgemm(hipStream_t st, const char *Apl, const char *Bpl, const double *cs, const double *Phi, int ld, double *T, int ldt,
                     long n_pad, int mp, double *nupart, double *phiw, int m, int mcol);                      // outputs as launch_tgemm's
void launch_trtri_level(hipStream_t st, const double *L, double *W, double *Tmp, int ld, int mq, int gs);

#ifndef GPZ_CH_NB
#define GPZ_CH_NB 32   // Cholesky panel width / diagonal block of the triangular inverse (64 measured 1.6x slower)
#endif
// ---- m x m factorisation pieces (k_chol.hip) -----------------------------------------------------
// A (mq x lda, mq % 32 == 0) <- S[0:m,0:m] + diag(alpha), identity on the padding.
void launch_build_sigma(hipStream_t st, const double *S, int lds, const double *alpha, int m, int mq, double *A, int lda, double *Wz = nullptr, double *logdet = nullptr);   // Wz (mq x mq) and *logdet are cleared when given
// panel + trailing update of one step in a single launch (GPZ_CH_NB == 32)
// one step: panel + trailing update, the factor into Lm, the diagonal block of inv(L) into W (W cleared beforehand; nullptr: not wanted)
bool chol_full_inverse_fits(int mq);
void launch_chol_step(hipStream_t st, double *A, double *Lm, double *W, int lda, int mq, int k0, double *logdet, int *info,
                      bool full_inverse = false);   // full_inverse: + block row k0 / 32 of inv(L) (all steps: no k_trtri_level launches)
void launch_zero(hipStream_t st, double *p, size_t count);
// Bext (mp x mp) <- [inv | w column at m | 0]; iS (m x m col-major == row-major, symmetric) copy; w, dwda, diag.
void launch_post_inverse(hipStream_t st, const double *Sinv, int ldsi, const double *S, int lds, const double *alpha,
                         int m, int mp, int out, double *Bext, double *w, double *dwda, double *dgi, int *info,
                         double *logdet);

// ---- rank-truncating pseudo-inverse, the other branch of inv_logdet.m:7-15 (k_pinv.hip) -----------
// info[1] |= 1 when SIGMA = S + diag(alpha) is so ill-conditioned that the reference's SVD might drop singular values
// (part: 128 doubles of scratch)
void launch_cond_flag(hipStream_t st, const double *S, int lds, const double *alpha, const double *Sinv, int ldsi, int m,
                      double *part, int *info);
// one-sided Jacobi SVD -> Xi = V diag(1/s) U' over s > m*eps(max s), *logdet = sum ln s (kept); out3 = [logdet, rank, max s]
// Gt, Vt: m x ld work matrices, sbuf: m doubles, word: 8-byte device word.  Returns the sweeps used, -1 on error.
int run_jacobi_pinv(hipStream_t st, const double *S, int lds, const double *alpha, int m, double *Gt, double *Vt, int ld,
                    double *sbuf, unsigned long long *word, double *Xi, int ldx, double *logdet, double *out3);

// R R' = S (m x m symmetric positive semidefinite, lds) as R = V diag(sqrt(max(lambda, 0))) from the same sweeps; R column-major (ldr)
int run_jacobi_sqrt(hipStream_t st, const double *S, int lds, int m, double *Gt, double *Vt, int ld, unsigned long long *word, double *R,
                    int ldr);

void launch_fill_bext(hipStream_t st, const double *Sinv, int ldsi, const double *w, int m, int mp, int out,
                      double *Bext, double *dgi);

// ---- row epilogue, moments, finish (k_rows.hip) --------------------------------------------------
struct RowArgs {
    const double *Phi; double *T; int ld;   // T is overwritten with dPHI (k==1) or accumulated into dL
    int n, m, mp, k, out;                   // out = output index being processed
    const double *y, *omega, *lnbeta, *wbeta; long ldx;
    long om_ld;                             // omega[out*om_ld + i]; 0 = an n x 1 omega for every output
    const double *w, *v;                    // column `out` of w (m), v (m) (v may be nullptr)
    double *dL;                             // n_pad x ld accumulator when k>1 (else nullptr)
    double *colslab;                        // [nwg][2][mp]: per-workgroup partial PHI'c, PHI'dbeta
    double *scal;                           // [nwg][4]: sum c*delta, sum omega*delta^2, sum LL, sum dbeta
    int nwg;
};
void launch_row_epilogue(hipStream_t st, const RowArgs &a);
void launch_colslab_reduce(hipStream_t st, const double *colslab, const double *scal, int nwg, int mp, double *out_cols,
                           double *out_scal);
void launch_mul_phi(hipStream_t st, const double *dL, const double *Phi, double *T, size_t count);

struct MomentArgs {
    const double *dPhi; int ld;
    const double *Xr;        // n_pad x d row-major
    int n, n_pad, m, d, kind;
    const double *P;
    int nchunk, rows_per_chunk;
    double *slab;            // [nchunk][m][nm]
    int nm;                  // moments per basis: cov d + d(d+1)/2, diag 2d (3d with Psi)
    const double *Psir, *Mr, *G2;   // diag kinds: Psi rows (n_pad x d), observed mask rows, gamma^2 (nullptr = absent)
    const int *chunktab;            // cov kinds, optional: {first row, end row} per chunk instead of chunk*rows_per_chunk
};
int launch_moments(hipStream_t st, const MomentArgs &a);

// Fused single-output path: row scalars from the T-GEMM epilogue, then moments with dPHI formed on the fly.
//   rowscal[i*4 + {0,1,2}] = omega*beta, omega*beta*delta, dbeta   (GPz.m:48,79,93)
//   partial: row_scalars_nwg(n) records of GPZ_NS doubles [sum c*delta, sum omega*delta^2, sum LL, sum dbeta, ...]
#define GPZ_ROWSCAL_MAX_NWG 1024
inline int row_scalars_nwg(int n) {   // one workgroup per 512 rows, 128 .. 1024 (the kernel is bound by load latency)
    const int w = (n + 511) / 512;
    return w < 128 ? 128 : (w > GPZ_ROWSCAL_MAX_NWG ? GPZ_ROWSCAL_MAX_NWG : w);
}
void launch_row_scalars(hipStream_t st, const double *nupart, int nslots, const double *phiw, const double *y,
                        const double *omega, const double *lnbeta, const double *wbeta, long n_pad, int n,
                        double *rowscal, double *partial, long om_off = 0);   // om_off: this output's column of an n x k omega (o * om_ld)
struct FusedMomentArgs {
    const double *Phi, *T; int ld;
    const double *Xr, *rowscal;
    int n, m, d, kind;
    const double *P, *w, *v;   // v may be nullptr
    int nchunk, rows_per_chunk;
    double *slab;              // [nchunk][m][nm + 2]: moments, then PHI'(omega beta delta), PHI'dbeta
    int nm;
    const double *Psir, *Mr, *G2;   // as in MomentArgs
    const int *chunktab;            // as in MomentArgs
};
int launch_moments_fused(hipStream_t st, const FusedMomentArgs &a);
// k_moments_ring.hip: the same sums for GC / VC with mp > 256 and d = 8 / 10 (no input noise, no missing values), PHI and T streamed
// through an LDS ring by LDS-DMA; raw sums about the rows' column means, records [chunk][m][nf + 2] = [features | PHI'c | PHI'dbeta]
struct RingMomentArgs {
    const double *Phi, *T; int ld;
    const double *Xs;          // n x (d + 2) rows [1 | x - mu | 0]
    const double *rowscal;     // [n][4]: omega beta, c, dbeta, -
    int n, m, d;
    const double *w, *v;       // v may be nullptr
    int nchunk, rows_per_chunk;
    double *slab;
};
bool moments_ring_fits(int kind, int de, int mp);
int moments_ring_cols();                                        // basis functions per workgroup (the chunk count is sized by it)
int moments_ring_features(int de);                              // nf = 1 + d + d(d+1)/2
int launch_moments_ring(hipStream_t st, const RingMomentArgs &a);   // 0, or -1 when the launch failed
// the chunk records summed in a fixed order, converted to the sums about the basis centres (mom [m][nm], accumulated over outputs) and
// split off the column sums (cols [2][mp]): what launch_slab_sum + launch_split_fused do for k_moments_fused's records
void launch_ring_finish(hipStream_t st, const double *slab, int nrec, int m, int d, const double *P, const double *xmu, int nm, int mp,
                        double *mom, double *cols, int accumulate);
int launch_moments_wide(hipStream_t st, const MomentArgs &a);
int launch_moments_fused_wide(hipStream_t st, const FusedMomentArgs &a);   // overwrites a.T with dPHI
// split the reduced [m][nm+2] records into mom [m][nm] and cols [2][mp]
void launch_split_fused(hipStream_t st, const double *rec, int m, int nm, int mp, double *mom, double *cols,
                        int accumulate = 0 /* add to mom instead of assigning (outputs after the first) */);
void launch_slab_sum(hipStream_t st, const double *slab, int nslab, size_t count, double *out);
// out[g][count] = sum of slabs seg[g] .. seg[g+1]-1, g < nseg (seg: nseg+1 device ints)
void launch_slab_sum_seg(hipStream_t st, const double *slab, const int *seg, int nseg, size_t count, double *out);

struct FinishArgs {
    int method_id, kind, m, d, k, hetero, g_dim;
    GpzParams pr;
    const double *mom; int nm;            // reduced moments [m][nm]
    const double *cols;                   // [k][2][mp]   PHI'(omega beta delta), PHI'dbeta
    const double *scal;                   // [k][4]
    const double *w, *dwda, *dgi;         // m x k each
    const double *logdet;                 // k
    const double *sums1;                  // [sum omega, sum_i omega_i lnbeta_io (8), n_train]       (GPZ_NS doubles)
    const double *vsums;                  // [sum omega delta^2, sum LL, per-output (8), n_valid, 0]  or nullptr
    const int *info;
    const double *phi_bound;              // k_phi_quad contexts: max_j B_j of this evaluation (nullptr: 0 is reported)
    double *out;                          // [f, grad(p), stats(4), info, n, logdet0, svd-route flag, PHI rounding bound]   (p + 10 doubles)
    double *dGfull;                       // scratch m*d or m*d*d
    int p;
    int nmp;                              // leading dimension of cols (= mp)
    int de;                               // padded dimension of the parameter block / moments
    int psi;                              // diag kinds with input noise: moments are [A1|A2|A3]
    int gen;                              // cov kinds, general path: dP/dGamma already written by k_gen_finish
};
void launch_finish(hipStream_t st, const FinishArgs &a);

// Small row reductions; each writes GPZ_SMALL_NWG partial records of GPZ_NS doubles (sum them with launch_slab_sum).
//   row_stats: [sum omega*delta^2, sum omega*(-0.5 beta delta^2 + 0.5 ln beta), sum omega*beta*delta^2 per output (8), rows, 0]
//   sums1:     [sum omega, sum_i omega_i*lnbeta_io per output (8), 0, rows, 0]  -- rows at index 10 in both
#define GPZ_NS 12
// more than 8 outputs: the records grow by one slot per extra output, appended behind the 12 standard ones
__host__ __device__ inline int gpz_ns(int k) { return GPZ_NS + (k > 8 ? k - 8 : 0); }
__host__ __device__ inline int gpz_ns_idx(int base, int o) { return o < 8 ? base + o : GPZ_NS + (o - 8); }
#define GPZ_SMALL_NWG 128
void launch_row_stats(hipStream_t st, const double *phiw, const double *y, const double *omega, long om_ld, const double *lnbeta,
                      long ldx, int n, int k, double *partial);
void launch_sums1(hipStream_t st, const double *omega, long om_ld, const double *lnbeta, long ldx, int n, int k, double *partial);
// nlogML partial of the solve-only mode (GPz.m:81-82), one value per output.
void launch_solve_partial(hipStream_t st, GpzParams pr, const double *w, const double *logdet, const double *sums1,
                          const double *rstats, int m, int k, double *out);
// NaN-pattern grouping (getPHI.m:43-54): masks, first-occurrence unique list, ids.
size_t nan_groups_work_bytes(long n, int d);
int launch_nan_groups(hipStream_t st, const double *X, long n, int d, void *work /* nan_groups_work_bytes(n, d) */,
                      int *n_groups, int *group_id);

// ---- general covariance-kind path: input noise and/or missing dimensions (k_gen.hip) ---------------
struct GenRows {
    const double *Xr;          // n_pad x de, 0 at missing entries
    const int *gid;            // pattern id per row
    const double *Psi3;        // n_pad x d*d (Psi(:,:,i) column-major) or nullptr
    const int *rows_by_group;  // row indices sorted by pattern id
    int n, n_pad;
};
// ws: runtime-d workspace of gen_rt_threads(d) * gen_ws_per_thread(d) doubles, needed (non-null) when d > 20; the small
// matrices of the general path live there instead of per-thread scratch and the kernels run as grid-stride loops
size_t gen_ws_per_thread(int d);
int gen_rt_threads(int d);   // size of the grid-stride thread pool of the runtime-d kernels (workspace = threads x per-thread doubles)
void launch_gen_prep(hipStream_t st, const double *G, int m, int d, int de, double *Sig, double *iSig,
                     const unsigned char *pat, int ngroups, double *lnS, double *ws = nullptr);
// missing dimensions without input noise: per-pattern parameter block for the tuned PHI kernel ([R~ | c~], layout of
// k_prep_cov) and conversion of the tuned moment sums of a pattern into the records k_gen_finish consumes
void launch_gen_pattern_params(hipStream_t st, const double *Sig, const double *P, const unsigned char *pat, int G, int m,
                               int d, int de, double *RcAll /* G blocks of m*(nt+de) */, double *ws = nullptr);
void launch_gen_convert_moments(hipStream_t st, const double *frecAll /* [G][m][stride] */, int stride, int has_r,
                                const double *Sig, const unsigned char *pat, int G, int m, int d, int de,
                                double *recsAll /* [G][m][nrec] */, int nrec);
void launch_gen_phi(hipStream_t st, const GenRows &r, int m, int mp, int d, int de, int k, const double *P,
                    const double *Sig, const double *lnS, const unsigned char *pat, double *Phi, const double *Y,
                    double *ws = nullptr);
void launch_gen_fill(hipStream_t st, double *Phi, int ld, int n, int n_pad, int m, int mp, int k, const double *Y);
// register-resident variants for Psi without missing dimensions, 2 <= d <= 10 (k_psi.hip); return -1 outside that range
// fp64 GC/VC + Psi for 10 < d <= 64 (k_cpsi.hip): same arguments and records as launch_psi_phi / launch_psi_moments
bool cpsi_available(int d);
int launch_cpsi_phi(hipStream_t st, const GenRows &r, int m, int d, int de, const double *P, const double *Sig,
                    const double *lnS, double *Phi, int ld, const unsigned char *pat);
int launch_cpsi_moments(hipStream_t st, const double *Phi, const double *T, int ld, const double *rowscal, const double *w,
                        const double *v, const GenRows &r, int m, int d, int de, const double *P, const double *Sig,
                        int nchunk, int rows_per_chunk, double *slab, int nrec, const unsigned char *pat,
                        const int *chunktab);
// the same for 10 < d <= 32 with four pairs per wave (k_cpsi4.hip)
bool cpsi4_available(int d);
int launch_cpsi4_phi(hipStream_t st, const GenRows &r, int m, int d, int de, const double *P, const double *Sig,
                     const double *lnS, double *Phi, int ld, const unsigned char *pat, bool shared = false /* GC: one covariance */);
int launch_cpsi4_moments(hipStream_t st, const double *Phi, const double *T, int ld, const double *rowscal, const double *w,
                         const double *v, const GenRows &r, int m, int d, int de, const double *P, const double *Sig,
                         int nchunk, int rows_per_chunk, double *slab, int nrec, const unsigned char *pat,
                         const int *chunktab, const double *minv = nullptr);
size_t cpsi4_minv_len(int d);   // doubles per row of the GC inverse table (k_cpsi4_minv)
int launch_cpsi4_minv(hipStream_t st, const GenRows &r, int d, int de, const double *Sig, const double *lnS, const unsigned char *pat,
                      double *minv, double *qA = nullptr, int lda = 0, const double *ctr = nullptr);   // ctr (with qA): the centre c of launch_gcq_centre
// GC + Psi without missing dimensions, dense form of the PHI build: PHI = exp(-1/2 A * B), A (n x gcq_kpad(d)) from launch_cpsi4_minv(.., qA),
// B (gcq_kpad(d) x ldb) from launch_gcq_tab, the product on launch_tgemm
int gcq_kpad(int d);
void launch_gcq_centre(hipStream_t st, int m, int d, int de, const double *P, double *ctr);   // c = mean basis centre: both factors work on x - c, p - c
void launch_gcq_tab(hipStream_t st, int m, int d, int de, int ldb, const double *P, const double *ctr, double *B);
void launch_gcq_exp(hipStream_t st, const double *Q, int ld, int n, int m, double *Phi);
// 32 < d <= 48, rows without missing values (k_cpsi4w.hip)
bool cpsi4w_available(int d);
int launch_cpsi4w_phi(hipStream_t st, const GenRows &r, int m, int d, int de, const double *P, const double *Sig,
                      const double *lnS, double *Phi, int ld);
int launch_cpsi4w_moments(hipStream_t st, const double *Phi, const double *T, int ld, const double *rowscal, const double *w,
                          const double *v, const GenRows &r, int m, int d, int de, const double *P, const double *Sig,
                          int nchunk, int rows_per_chunk, double *slab, int nrec, const int *chunktab);
int launch_cpsi4w_predict_noisy(hipStream_t st, int n, long ldx, int m, int d, int de, int k, const double *Xr, const double *Psi3,
                                const double *tab, int rec, const double *w, const double *v, const double *iS, int nchunk,
                                long pairs_per_chunk, double *part, bool shared);
int launch_cpsi4_predict_noisy(hipStream_t st, int n, long ldx, int m, int d, int de, int k, const double *Xr, const double *Psi3,
                               const double *tab, int rec, const double *w, const double *v, const double *iS, int nchunk,
                               long pairs_per_chunk, double *part, bool shared /* GC: one covariance for every pair */);
// prediction with missing values, GC/VC, 10 < d <= 32: the record sums on 4 x 4 MFMA tiles (k_pmc4.hip); arguments as pmc_sum (k_pmiss_cov.hip)
bool pmc4_available(int d);
bool launch_pmc4_sum(hipStream_t st, int d, bool noisy, int nrows, int row0, int m, int ld, long R, int nchunk, const double *tab,
                     int ntab, int nw, const double *Pio, const double *XhT, const double *PsT, double *Phi, long ldx,
                     double *part);
bool psi_fast_path_available(int d);
// pat (observed flags [G][d]) non-null: rows carry missing dimensions (r.gid = pattern per row, lnS = [G][m]);
// chunktab (optional): {first row, end row} per moment chunk
int launch_psi_phi(hipStream_t st, const GenRows &r, int m, int d, int de, const double *P, const double *Sig,
                   const double *lnS, double *Phi, int ld, const unsigned char *pat, bool shared = false /* GC: every basis function has the same covariance */);
int launch_psi_moments(hipStream_t st, const double *Phi, const double *T, int ld, const double *rowscal, const double *w,
                       const double *v, const GenRows &r, int m, int d, int de, const double *P, const double *Sig,
                       int nchunk, int rows_per_chunk, double *slab, int nrec, const unsigned char *pat,
                       const int *chunktab, const double *gc_minv = nullptr);   // gc_minv: GC, 10 < d <= 32: the per-row inverse table (launch_cpsi4_minv)
// fp32 per-pair kernels for Psi without missing dimensions, d <= 20 (k_psi32.hip).  PsiT: packed lower triangles of
// Psi_i, element-major [e][ldp] (diag != 0: only the D diagonals), D = psi32_pad_dim(d).
int psi32_pad_dim(int d);
int psi32_raw_len(int d);   // doubles per (chunk, basis) the moment kernel writes: 3 + D + D(D+1)/2
// chunk-summed raw sums [m][psi32_raw_len] -> records [m][nrec]: the layout of k_gen_moments (diag = 0, consumed by
// k_gen_finish) or whitened records (diag = 1, consumed by launch_psi32_finish: dP = R'a, dGamma = -Q C~' R^-T)
void launch_psi32_records(hipStream_t st, const double *raw, int d, int diag, int m, double *recs, int nrec);
void launch_psi32_finish(hipStream_t st, const double *recs, int m, int d, int de, const double *Gam, const double *Rc,
                         int method_id, const double *sums1, int k, double *grad, double *dGfull, double *cols, int mp,
                         int nrec);
int launch_psi32_phi(hipStream_t st, const double *Xr, int de, int d, const float *PsiT, long ldp, int diag, int n, int m,
                     const double *P, const double *Sig, const double *Rc, const double *lnS, double *Phi, int ld);
// the same sums for DIAGONAL Psi on the matrix pipe (k_psi32m.hip): sixteen pairs per wave on v_mfma_f32_4x4x1_16b_f32; writes the raw
// layout of launch_psi32_moments (rows_per_chunk any positive number)
bool psi32m_available(int d);
int launch_psi32m_moments(hipStream_t st, const double *Phi, const double *T, int ld, const double *rowscal, const double *w,
                          const double *v, const double *Xr, int de, int d, const float *PsiT, long ldp, int n, int m,
                          const double *P, const double *Rc, int nchunk, int rows_per_chunk, double *slab);
int launch_psi32_moments(hipStream_t st, const double *Phi, const double *T, int ld, const double *rowscal, const double *w,
                         const double *v, const double *Xr, int de, int d, const float *PsiT, long ldp, int diag, int n, int m,
                         const double *P, const double *Sig, const double *Rc, int nchunk, int rows_per_chunk, double *slab,
                         int nrec);
void launch_gen_rowdot(hipStream_t st, const double *Phi, int ld, int n, long ldx, int m, int k, const double *v,
                       const double *b, const double *omega, const double *w, double *lnbeta, double *wbeta,
                       double *phiw, long om_ld = 0);   // omega[o*om_ld + i]
void launch_gen_moments(hipStream_t st, const double *Phi, const double *T, int ld, const double *rowscal, const double *w,
                        const double *v, const GenRows &r, int g, int row_begin, int nrows, const unsigned char *pat, int m,
                        int d, int de, const double *P, const double *Sig, int nchunk, int rows_per_chunk, double *slab,
                        int nrec, double *ws = nullptr);
void launch_gen_finish(hipStream_t st, const double *recs, int G, const unsigned char *pat, int m, int d, int de,
                       const double *Gam, const double *Sig, const double *iSig, int method_id, const double *sums1, int k,
                       double *grad, double *dGfull, double *cols, int mp, int nrec,
                       double *part /* G*m*(d + d*d + 2) doubles of scratch */,
                       int raw /* records hold plain moment sums (no input noise): see k_gen_convert_moments */,
                       double *ws = nullptr);

// prediction with input noise (predictDiag.m:75-125 / predictCov.m:70-132) and the getPrior iteration (getPrior.m:7-20)
void launch_pair_table(hipStream_t st, int kind, int m, int d, int de, const double *P, const double *G, const double *Sig,
                       const double *iSig, double *tab, int rec, double *ws = nullptr);
int launch_predict_noisy_cov(hipStream_t st, int n, long ldx, int m, int d, int de, int k, const double *Xr, const double *Psi3,
                             const double *tab, int rec, const double *w, const double *v, const double *iS, int nchunk,
                             long pairs_per_chunk, double *part,
                             int flags = 0 /* bit 0: every Psi_i diagonal, bit 1: one covariance for all basis functions (GC) */);   // k_psi.hip: 2 <= d <= 10, else -1
int launch_predict_noisy_diag(hipStream_t st, int n, long ldx, int m, int d, int de, int k, const double *Xr, const double *Psir,
                              const double *tab, int rec, const double *w, const double *v, const double *iS, int nchunk,
                              long pairs_per_chunk, double *part);   // k_psi.hip: d <= 20, k <= 8, else -1
void launch_predict_noisy(hipStream_t st, int kind, int n, long ldx, int m, int d, int de, int k, const double *Xr,
                          const double *Psir, const double *Psi3, const double *tab, int rec, const double *w,
                          const double *v, const double *iS, int nchunk, long pairs_per_chunk, double *part,
                          double *ws = nullptr, int flags = 0);
void launch_predict_noisy_final(hipStream_t st, const double *sums, long ldx, int n, int k, const double *mu,
                                const double *lnbeta, const double *b, double *gamma, double *nu, double *beta_i);
void launch_prior_update(hipStream_t st, const double *colsum, double ns, int m, double *prior, double *keep);
void launch_prior_iter(hipStream_t st, const double *N, int ld, int n, int m, const double *prior, double *colslab,
                       int nwg);

// prediction with missing dimensions, diagonal kinds (predictDiag.m:127-297; k_pmiss.hip).  obs: bit c set = dimension c observed
// (ObsMask: 256 bits, passed by value; the covariance kinds keep a 64-bit mask, d <= 64).
struct ObsMask {
    unsigned long long w[4];
};
#define GPZ_PM_MAXD 256        // bits of the mask
#define GPZ_PM_MAXD_DIAG 144   // what the pair-table kernel's LDS tile (d KB per 64 pairs) allows
static inline __host__ __device__ bool obs_bit(const ObsMask &o, int c) { return (o.w[c >> 6] >> (c & 63)) & 1ull; }
struct ObsFlags {               // any width: one byte per dimension in DEVICE memory (1 = observed); the kernels' wide instantiations
    const unsigned char *f;
};
static inline __device__ bool obs_bit(const ObsFlags &o, int c) { return o.f[c] != 0; }
void launch_pm_no(hipStream_t st, const double *Xr, const double *Psir, int de, int n, long n_pad, int m, int ld, int d,
                  ObsMask obs, const double *P, const double *G, const double *priors, double *No, double *Pio);
void launch_pm_no(hipStream_t st, const double *Xr, const double *Psir, int de, int n, long n_pad, int m, int ld, int d,
                  ObsFlags obs, const double *P, const double *G, const double *priors, double *No, double *Pio);
void launch_pm_pio(hipStream_t st, const double *No, int ld, int n, int m, const double *priors, double *Pio);
// covariance kinds (predictCov.m:134-337; k_pmiss_cov.hip): see launch_pmc for the work buffers
int pmc_rec_len(int d, unsigned long long obs);
void launch_pmc(hipStream_t st, unsigned long long obs, int n, long ldx, int m, int ld, int d, int de, int k, const double *Xr,
                const double *Psi3, const double *P, const double *Sig, const double *iSig, const double *priors,
                const double *w, const double *v, const double *iS, int rows_blk, double *rec, double *tab, double *Ex,
                double *Pio, double *Xhat, double *Phat, int nchunk, long pairs_per_chunk, double *part, double *Phi,
                double *work2 = nullptr /* m * (d(d+1)/2 + d*d + d + 1) doubles: enables the register-resident route */,
                bool tab_ready = false /* the pair table (pattern-independent) is already in `tab`: kept from the previous group */);
// the same for 32 < d <= 64: scratch-resident kernels only (k_pmiss_cov64.hip); work2 is not used
void launch_pmc_wide(hipStream_t st, unsigned long long obs, int n, long ldx, int m, int ld, int d, int de, int k, const double *Xr,
                     const double *Psi3, const double *P, const double *Sig, const double *iSig, const double *priors,
                     const double *w, const double *v, const double *iS, int rows_blk, double *rec, double *tab, double *Ex,
                     double *Pio, double *Xhat, double *Phat, int nchunk, long pairs_per_chunk, double *part, double *Phi,
                     double *work2, bool tab_ready);
bool pmc_fast(int d, int k);   // 2 <= d <= 10, k <= 8: the register-resident kernels (needs rows_blk <= 64)
void launch_pm_nij(hipStream_t st, int m, int ld, int d, int de, ObsMask obs, const double *P, const double *G, double *B);
void launch_pm_phi(hipStream_t st, const double *No, const double *T1, int ld, int n, long n_pad, int m, int d, int de,
                   const double *G, double *Phi);
void launch_pm_pairtab(hipStream_t st, long q0, long npairs, int m, int ld, int width, int d, int de, int k, ObsMask obs,
                       int has_psi, const double *P, const double *G, const double *w, const double *v, const double *iS,
                       double *B, double *rec, int nrec);
void launch_pm_accum(hipStream_t st, const double *Xr, const double *Psir, int de, int n, long n_pad, int ld, int d, int k,
                     ObsMask obs, int npq, const double *T2, const double *rec, int nrec,
                     double *sums /* [nsplit][3k][n_pad] */, int nsplit = 1);
int pm_accum_splits(int n);
// the same four for inputs of any width (d > GPZ_PM_MAXD_DIAG): pattern as device flags, no LDS tiles
void launch_pm_nij(hipStream_t st, int m, int ld, int d, int de, ObsFlags obs, const double *P, const double *G, double *B);
void launch_pm_pairtab(hipStream_t st, long q0, long npairs, int m, int ld, int width, int d, int de, int k, ObsFlags obs,
                       int has_psi, const double *P, const double *G, const double *w, const double *v, const double *iS,
                       double *B, double *rec, int nrec);
void launch_pm_accum(hipStream_t st, const double *Xr, const double *Psir, int de, int n, long n_pad, int ld, int d, int k,
                     ObsFlags obs, int npq, const double *T2, const double *rec, int nrec, double *sums, int nsplit);
// covariance kinds at d > 64 (k_pmiss_covg.hip): the per-thread d x d temporaries live in a workspace in device memory.
//   pat_dev: 3 d ints (observed | missing | unshuffle), filled by the launcher;  ws: ws_threads * pmg_ws_per_thread(d) doubles.
// Work buffers as for launch_pmc (rows_blk = 1 is enough: one launch per row and item range).
size_t pmg_ws_per_thread(int d);
void launch_pmc_generic(hipStream_t st, const unsigned char *obs_host, int n, long ldx, int m, int ld, int d, int de, int k,
                        const double *Xr, const double *Psi3, const double *P, const double *Sig, const double *iSig,
                        const double *priors, const double *w, const double *v, const double *iS, double *rec, double *tab, double *Ex,
                        double *Pio, double *Xhat, double *Phat, int nchunk, long pairs_per_chunk, double *part, double *Phi,
                        bool tab_ready, int *pat_dev, double *ws, long ws_threads);

// N = PHI .* exp(-1/2 ln|Sigma_oo| - 1/2 |o| ln 2pi + 1/2 |u| ln 2)   (getPHI.m:77,87,98,105,114)
struct NormArgs {
    const double *Phi; int ld; int n, m, d, de, kind, gen;
    const double *G;        // diag kinds: gamma [m][de]
    const double *Rc;       // cov kinds, tuned path: QR factor records
    const double *Mr, *ucnt;// diag kinds with missing values (row-major mask, missing count) or nullptr
    const int *gid; const unsigned char *pat; const double *lnS;   // general cov path
    double *N;              // n_pad x ld row-major
};
void launch_phi_norm(hipStream_t st, const NormArgs &a);

// gpz_predict_last_route (gpz_predict.hip): what the one-shot predict entries and the launchers that choose a kernel family note down,
// host side and per thread.  A launcher called outside such an entry notes nothing (predict_route_add is a no-op then).
void predict_route_add(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

// misc
void launch_dxy(hipStream_t st, const double *X, long nx, const double *Y, long ny, int d, double *D);
void launch_transpose_out(hipStream_t st, const double *src, int ld, long n, int m, double *dst /* n x m col-major */,
                          const int *perm = nullptr /* source row i -> destination row perm[i] */);
void launch_nu(hipStream_t st, const double *Phi, const double *T, int ld, int n, int m, double *nu);
