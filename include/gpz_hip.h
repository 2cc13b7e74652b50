/*
 * gpz_hip.h — C ABI of libgpz_hip.so: the MI355X (gfx950) implementation of GPz's
 * marginal-likelihood objective/gradient path.
 *
 * Every entry point replaces one reference interface (paths relative to the
 * OxfordML/GPz tree); INTEGRATION.md shows the MEX / ctypes binding for each.
 *
 *   gpz_ctx_create      the closure  f = @(params) GPz(params,model,X,Y,Psi,omega,training,validation)
 *                       GPz/train.m:40, GPz/init.m:89  (data captured once; row selection of
 *                       GPz/getPHI.m:14-22 is done here, once, instead of on every call)
 *   gpz_eval            [nlogML,grad] = GPz(theta,...)      GPz/GPz.m:1  (nargout<=2 mode, :89-261)
 *                       + globals trainRMSE/trainLL/validRMSE/validLL   GPz/GPz.m:3-7,236-259
 *   gpz_solve           [~,~,w,iSigma_w] = GPz(theta,...)   GPz/GPz.m:84-87 (nargout>2 mode)
 *   gpz_phi             [PHI,Gamma,lnBeta_i,N] = getPHI(X,Psi,theta,model,[]) GPz/getPHI.m:1
 *   gpz_predict_full    predictFull(X,theta,w,iSigma_w,model) GPz/predictDiag.m:58-74, predictCov.m:53-69
 *   gpz_predict_noisy   predictNoisy(X,Psi,...)               GPz/predictDiag.m:75-125, predictCov.m:70-132
 *   gpz_predict_missing predictMissing / predictNoisyMissing  GPz/predictDiag.m:127-297, predictCov.m:134-337
 *   gpz_prior           prior = getPrior(X,Psi,theta,model,set) GPz/getPrior.m:1
 *   gpz_inv_logdet      [Xi,logdet] = inv_logdet(X)         GPz/inv_logdet.m:1
 *   gpz_dxy             D = Dxy(X,Y)                        GPz/Dxy.m:1
 *   gpz_nan_groups      the NaN-pattern grouping loop       GPz/getPHI.m:43-54 (== GPz.m:118-129)
 *   gpz_mgpu_*          the same closure / calls on all GPUs of the node behind one synchronous call
 *                       (minFunc_2012/minFunc/minFunc.m:314 calls funObj once and waits)
 *
 * Limits: none on d, k or the number of NaN patterns for the evaluation, getPHI, predictFull, predictNoisy, getPrior and the
 * NaN grouping (the reference is generic, getPHI.m:60-110, GPz.m:133-213).  d <= 20 and k <= 8 run the instantiated,
 * register-resident kernels; wider inputs / more outputs take runtime-d kernels with the row data in LDS (k_wide.hip) and, for
 * GC/VC with missing values, a workspace-backed form of the general path (DESIGN.md section 7 gives the cost; when a row tile
 * does not fit the 160 KB of LDS - d beyond ~100 for the diagonal kinds with input noise and missing values, ~300 without - the
 * PHI build reads the row data where it uses it, and GC/VC beyond d = 142 factor Gamma_j in a device workspace).  GC/VC with
 * input noise in fp64 runs register-resident up to d = 10 and as a block elimination in f64 MFMA accumulators for
 * 10 < d <= 64 (four pairs per wave up to d = 48), the workspace form beyond.
 * gpz_predict_missing for GC/VC runs register / MFMA kernels up to d = 32 and scratch-resident kernels with 64-wide temporaries for
 * 32 < d <= 64 (correct and slow: 32 KB of scratch per thread and temporary) and, for ANY wider input, the same kernels with their
 * temporaries in a device workspace (k_pmiss_covg.hip: 3 d^2 + 2 d doubles per thread, at most 2 GB per launch; 9 rows of one
 * pattern at d = 100: 0.8 s with m = 4, 2.9 s with m = 16).  The diagonal kinds run tuned to d = 144 (pattern mask by value, d KB of
 * LDS per 64 basis pairs) and LDS-free beyond (pattern as device flags; d = 260, m = 8, 30 rows: 83 ms).  No width is refused.
 * Rows: PHI and T (2 n mp doubles) stay on the device while they fit; beyond that the evaluation streams them in row tiles (PHI built
 * twice per evaluation, +10 % at c4's shape; plain route: no Psi, no missing values on GC/VC) - gpz_ctx_route reports it, gpz_get_phi is
 * refused there.
 * dtype = f32 with d > 20 takes
 * the fp64 kernels (the fp32 pair kernels hold a d <= 20 triangle in registers); gpz_ctx_route says which route a context runs.
 *
 * Conventions (MATLAB's, so a MEX shim is pure marshalling):
 *   - all matrices are column-major double; masks are 1 byte per row (MATLAB logical);
 *     a NULL pointer plays MATLAB's [].
 *   - theta / grad use the reference packing [P(:);Gamma(:);lnAlpha(:);b(:);v(:);lnTau(:)]
 *     (GPz/GPz.m:227-231, GPz/init.m:87-97).
 *   - host pointers are never retained after a call returns; outputs are caller-allocated.
 *   - return value: 0 ok; <0 error (text via gpz_last_error()).  Numerical breakdown
 *     (non-positive-definite or non-finite SIGMA) is NOT an error: f and g come back NaN so the
 *     caller's line search backs off (minFunc/WolfeLineSearch.m:53-70, isLegal.m); this is a
 *     documented deviation — the reference would raise from svd().
 *   - no torch types, no C++ in the signatures.  The library owns its device memory
 *     (hipMalloc) and runs on the HIP stream given at context creation (NULL = the null stream).
 */
#ifndef GPZ_HIP_H
#define GPZ_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPZ_OK               0
#define GPZ_ERR_ARG         -1   /* bad argument / unsupported combination */
#define GPZ_ERR_HIP         -2   /* HIP runtime failure */
#define GPZ_ERR_ALLOC       -3
#define GPZ_ERR_COMM        -4   /* the all-reduce hook failed */
#define GPZ_ERR_UNSUPPORTED -5   /* valid in the reference, not built yet (see DESIGN.md scope table) */

#define GPZ_VERSION 3   /* 3: no limits on d, k, NaN patterns; gpz_release_cached_memory; psi_kind 3 */

typedef struct gpz_ctx gpz_ctx;

/* model.{d,k,m,method,heteroscedastic} (GPz/init.m:16-20) + placement. */
typedef struct gpz_desc {
    int32_t d;                /* input dimension */
    int32_t m;                /* number of basis functions */
    int32_t k;                /* number of outputs */
    char    method[4];        /* "GL","VL","GD","VD","GC","VC" (NUL padded) */
    int32_t heteroscedastic;  /* model.heteroscedastic */
    int32_t device;           /* HIP device ordinal */
    void   *stream;           /* hipStream_t to run on; NULL = null stream */
    int32_t rank;             /* this shard's rank (0 when unsharded) */
    int32_t world;            /* number of row shards (1 when unsharded) */
    int32_t dtype;            /* GPZ_F64 (0, default) or GPZ_F32: precision flag of the path.  f32 applies to
                               * GC/VC with input noise and no missing values (BASELINE config 5): fp32 per-(sample, basis)
                               * factorisations, and the two MFMA contractions on fp32-rounded operands (PHI'W PHI with fp64
                               * master sums, PHI*inv(SIGMA) with fp32 accumulation).  Delta, ln PHI, PHI, every sum over
                               * rows, the m x m stage, theta, f and g stay fp64; every other configuration ignores the
                               * flag and runs the fp64 path bit for bit.  Gates: 1e-4 on f, 1e-3 on g (of max|g|) */
    int32_t omega_cols;       /* columns of omega: 0 or 1 = n_tot x 1, one weight per row for every output; k = n_tot x k,
                               * per-output weights (GPz.m:48 omega(training,:); getOmega.m:19 returns (1+Y).^-2, n x k for a
                               * k-column Y).  The two RMSE statistics read omega(training) = the FIRST column (GPz.m:236,258) */
    int32_t reserved[2];
} gpz_desc;
#define GPZ_F64 0
#define GPZ_F32 1

/* In-place SUM all-reduce over ranks of `count` doubles at device pointer `buf`, ordered on
 * `stream`.  Return 0 on success.  The Python host wires this to torch.distributed (RCCL);
 * a single-process caller leaves it unset. */
typedef int (*gpz_allreduce_fn)(void *user, void *buf, size_t count, void *stream);

/* Build the evaluation context.  X is n_tot x d, Y n_tot x k, omega n_tot x 1 or n_tot x k (desc->omega_cols; NULL = ones),
 * training/validation n_tot x 1 logical (NULL = all rows / no validation), all HOST pointers,
 * column-major.  psi_kind: 0 none; 1 = n_tot x d (after fixPsi, diag kinds); 2 = d x d x n_tot cube (GC/VC);
 * 3 = n_tot x d per-dimension variances for GC/VC, meaning the diagonal cubes fixPsi.m:27-31 builds from them
 * (Psi(:,:,i) = diag(S(i,:))): the library expands them, so the caller never materialises d x d x n (6.4 GB at
 * n = 2e6, d = 20).  Results are identical to passing that cube with psi_kind 2.
 * When world>1 the arrays hold only this rank's row shard. */
int gpz_ctx_create(const gpz_desc *desc, int64_t n_tot,
                   const double *X, const double *Y,
                   const double *Psi, int32_t psi_kind,
                   const double *omega,
                   const uint8_t *training, const uint8_t *validation,
                   gpz_ctx **out);

/* gpz_ctx_create for a row shard of GC/VC data with missing values.  The NaN-pattern groups of getPHI.m:43-54 must be
 * the same on every rank (the second all-reduce carries one record block per pattern): `patterns` is the table of the
 * WHOLE data set, n_patterns x d bytes row-major, 1 = missing (isnan), in first-occurrence order; a rank may hold no
 * row of some pattern.  NULL / 0 behaves like gpz_ctx_create. */
int gpz_ctx_create_sharded(const gpz_desc *desc, int64_t n_tot, const double *X, const double *Y,
                           const double *Psi, int32_t psi_kind, const double *omega,
                           const uint8_t *training, const uint8_t *validation,
                           const uint8_t *patterns, int32_t n_patterns, gpz_ctx **out);
void gpz_ctx_destroy(gpz_ctx *ctx);
int  gpz_ctx_set_allreduce(gpz_ctx *ctx, gpz_allreduce_fn fn, void *user);

/* numel(theta) for this context's model / for a model description (init.m:65-97; -1: bad description). */
int64_t gpz_theta_len(const gpz_ctx *ctx);
int64_t gpz_theta_len_of(const gpz_desc *desc);
/* rows selected by the training / validation mask on this rank. */
int64_t gpz_n_train(const gpz_ctx *ctx);
int64_t gpz_n_valid(const gpz_ctx *ctx);

/* [f,g] = GPz(theta,...).  stats[0..3] = trainRMSE, trainLL, validRMSE, validLL (the last two
 * untouched when there is no validation mask).  diag (optional, may be NULL) receives
 * diag[0] = Cholesky info (0 ok, j>0: pivot j not positive), diag[1] = global n. */
int gpz_eval(gpz_ctx *ctx, const double *theta, double *f, double *g, double stats[4], double diag[2]);

/* [~,~,w,iSigma_w] = GPz(theta,...): w is m x k, iSigma_w m x m x k; nlogML_partial (optional)
 * is the un-normalised 1 x k vector of GPz.m:81-82. */
int gpz_solve(gpz_ctx *ctx, const double *theta, double *w, double *iSigma_w, double *nlogML_partial);

/* gpz_eval for a device-resident caller: theta_dev and g_dev are device pointers on the context's device; only f and
 * the statistics cross PCIe.  Used with the L-BFGS memory below to keep the optimiser's vectors on the GPU. */
int gpz_eval_dev(gpz_ctx *ctx, const double *theta_dev, double *f, double *g_dev, double stats[4], double diag[2]);

/* Copy PHI (n_train x m, column-major) of the last gpz_eval/gpz_solve back to the host
 * (5th output of GPz.m:1). */
int gpz_get_phi(gpz_ctx *ctx, double *PHI);

/* Which branch of inv_logdet.m:7-12 an evaluation takes.  mode 0 (default): the Cholesky inverse, and the
 * rank-truncating SVD pseudo-inverse whenever SIGMA is close enough to singular that the reference might drop
 * singular values (decided on the device from ||SIGMA||_F and ||inv||_F, or a failed pivot); 1: always the
 * SVD route; -1: never (a failed pivot then gives NaN f/g).
 * gpz_ctx_last_pinv: out[0] = 1 if the last gpz_eval/gpz_solve took the SVD route, out[1] = rank kept
 * (minimum over outputs), out[2] = largest singular value, out[3] = Jacobi sweeps. */
int gpz_ctx_set_pinv_mode(gpz_ctx *ctx, int mode);
int gpz_ctx_last_pinv(const gpz_ctx *ctx, double out[4]);
/* Covariance kinds with many basis functions (GC / VC, m + k > 256, d <= 10 padded to 8 or 10, one output, no input noise or missing
 * values) build PHI as a product of centred row features on the f64 MFMA whenever a bound on that product's rounding error over the
 * context's rows, max_j B_j, is at most 2^-33, and with the vector kernel otherwise; the choice is made on the device per evaluation.
 * gpz_ctx_last_phi: out[0] = 1 if the last gpz_eval fell back to the vector kernel, out[1] = max_j B_j (0 on every other route). */
int gpz_ctx_last_phi(const gpz_ctx *ctx, double out[2]);

/* Per-stage GPU time (HIP events on the context's stream).  enable = 1: events around every stage (the evaluation then runs as
 * eager launches); enable = 2: around the dominant stages only (phi_build, syrk, tgemm, moments), the evaluation still replayed as
 * hipGraph segments with the events between them; 0: off.  gpz_ctx_timings copies up to `cap` accumulated stage times in ms and the
 * call counts, returns the number of stages; names are static strings. */
int gpz_ctx_enable_timing(gpz_ctx *ctx, int enable);   /* 3: level 2 plus events around every other segment ("rest") and around the
                                                          * all-reduce hooks ("exchange"): wall time of a call minus the sum of all stage times is then what the device spent BETWEEN
                                                          * segments - the launch-to-launch gaps of a replayed evaluation */
int gpz_ctx_timings(gpz_ctx *ctx, const char **names, double *ms, int64_t *calls, int cap);
int gpz_ctx_reset_timings(gpz_ctx *ctx);
/* Which kernel family this context's rows run on (e.g. dtype = GPZ_F32 with missing values or d > 20 takes the fp64 pair kernels:
 * said here instead of silently), which MFMA operand type the contractions use, and the state of the captured evaluation graph
 * ("replayed" / "eager" / "disabled").  Writes a NUL-terminated description of at most cap bytes; returns its full length. */
int gpz_ctx_route(const gpz_ctx *ctx, char *buf, int cap);

/* [PHI,~,lnBeta_i,N] = getPHI(X,Psi,theta,model,[]) on ns rows: PHI ns x m, lnBeta_i ns x k, N ns x m
 * (column-major, host; any output may be NULL).  Psi / psi_kind as in gpz_ctx_create; X may contain NaN. */
int gpz_phi(const gpz_desc *desc, const double *theta, const double *Xs, int64_t ns,
            const double *Psi, int32_t psi_kind, double *PHI, double *lnBeta_i, double *N);

/* predictFull: mu = PHI*w (muY NOT added, as in predictDiag.m:65), nu, beta_i; PHI optional. */
int gpz_predict_full(const gpz_desc *desc, const double *theta, const double *w, const double *iSigma_w,
                     const double *Xs, int64_t ns,
                     double *mu, double *nu, double *beta_i, double *PHI);

/* predictNoisy (inputs with noise Psi, no missing values): also returns gamma; mu without muY. */
int gpz_predict_noisy(const gpz_desc *desc, const double *theta, const double *w, const double *iSigma_w,
                      const double *Xs, int64_t ns, const double *Psi, int32_t psi_kind,
                      double *mu, double *nu, double *beta_i, double *gamma, double *PHI);

/* predictMissing / predictNoisyMissing (GPz/predictDiag.m:127-297, GPz/predictCov.m:134-337) for ONE group of
 * rows that share a NaN pattern (predict.m:45-69 forms the groups; the pattern is read from the first row,
 * predictDiag.m:3).  priors: 1 x m mixture weights (model.best.priors, train.m:59,74).  Psi: n x d (diagonal
 * kinds) / d x d x n (GC, VC) or NULL. */
int gpz_predict_missing(const gpz_desc *desc, const double *theta, const double *w, const double *iSigma_w,
                        const double *priors, const double *Xs, int64_t ns, const double *Psi, int32_t psi_kind,
                        double *mu, double *nu, double *beta_i, double *gamma, double *PHI);

/* Which kernels the last gpz_predict_full / _noisy / _missing of the CALLING THREAD ran, as one line of text: the entry, the kernel
 * family with its template widths (noisy_diag<8,1>, psi<5,8>, cpsi4<3,8>, cpsi4w<9,1>, gen<20>, gen_rt, pmc_fast<5>, pmc4<12>,
 * pmc_scratch, pmc_wide, pmc_generic, pm_diag, pm_diag_flags, tgemm) and the host-side counts (nchunk, ppc, rows_blk, blocks, width,
 * passes, last, npg, n_pad).  Host bookkeeping for tests and diagnosis; empty before the first call.  Returns the text's full length. */
int gpz_predict_last_route(char *buf, int64_t cap);

/* ---- persistent streaming predictor: predictFull / predictNoisy for any number of rows --------------------------------------------
 * gpz_predictor_create does the once-per-model work on desc->device (theta unpacked, B_o = [inv(Sigma_o) | w | v] laid out for the
 * product) and allocates tile-sized buffers only: afterwards device memory does not depend on how many rows are predicted.  theta, w and
 * iSigma_w as gpz_predict_full takes them; tile_rows = 0 chooses.  Two routes: fused (ceil16(m + 2k) <= 256 and d <= 20, k <= 8: one
 * kernel writes mu, nu and beta, PHI and T never exist) and tiles (PHI kernel + T-GEMM per tile of rows); GPZ_PREDICT_FORCE_TILES takes
 * the tile route where the fused kernel fits.  desc->stream is not used: the handle has streams of its own.
 * gpz_predictor_run: conventions of gpz_predict_full / gpz_predict_noisy - Xs column-major ns x d, normalised; outputs column-major ns x k,
 * mu without muY; gamma = 0 without Psi (predictDiag.m:74); PHI (ns x m) may be NULL, and then never leaves the device.  Rows with NaN are
 * refused (GPZ_ERR_UNSUPPORTED; outputs undefined).  Psi / psi_kind (1, 2, 3) as in gpz_predict_noisy: that branch runs per tile.
 * ns = 0 does nothing.  One thread at a time per handle.
 * gpz_predictor_route: as gpz_ctx_route (returns the description's full length).  gpz_predictor_info: [tile_rows, device bytes held, route (0 fused, 1 tiles), runs]. */
typedef struct gpz_predictor gpz_predictor;
#define GPZ_PREDICT_FORCE_TILES 1   /* flags: take the tile route even where the fused kernel fits (A/B and tests) */
/* flags: complete rows with input noise stay on the handle up to ceil16(m) <= 1024 (without it: 256).  predict_noisy_fits and
 * predict_noisy_cov_fits widen in m only; the entries for rows with missing inputs keep ceil16(m) <= 256.  Nothing is allocated before
 * the first call with Psi, and where ceil16(m) <= 256 the flag changes no kernel, chunk count, byte or bit (except that the draws of a
 * diagonal kind with Psi then also run off the fused route: k_predict_noisy_phi + k_tgemm).  The cost at m = 1024: a pair table of
 * m (m + 1) / 2 = 524 800 records (0.1 to 0.4 GB, and for GC / VC a temporary of 524 800 (1 + d + d d) doubles while it is built) and
 * 524 800 pair densities per row. */
#define GPZ_PREDICT_LARGE_M 2
/* flags: one group of rows with missing inputs stays on the handle up to ceil16(m) <= 1024 for the diagonal kinds (GL, VL, GD, VD),
 * d <= 20, k <= 8.  Read only by the entries that take one NaN-pattern group of such a kind: gpz_predictor_run_missing_dev,
 * _draws_missing_dev, _draws_gamma_missing_dev, _stack_missing_dev and their noisy_missing twins; the covariance kinds' entries
 * (*_missing_cov_dev, *_noisy_missing_cov_dev, *_psi_cube_missing_dev) and every entry for complete rows do not look at it (complete rows
 * with Psi past 256 need GPZ_PREDICT_LARGE_M as well).  Where ceil16(m) <= 256 the flag changes no kernel, chunk count, byte or bit;
 * beyond, the pair product runs in k_pml_pairs / k_pml_gamma (k_predict_group_large_impl.h), whose LDS does not grow with m.  The cost
 * at m = 1024, on the first call for a group: U of 524 800 x 1024 doubles (4.3 GB) and the pair records (0.1 to 0.3 GB), rebuilt in
 * place when the pattern or the priors change; every row costs 524 800 x 1024 multiply-adds on the f64 MFMA.  Past 1024:
 * GPZ_ERR_UNSUPPORTED, naming m and the limit. */
#define GPZ_PREDICT_LARGE_M_MISSING 4
int gpz_predictor_create(const gpz_desc *desc, const double *theta, const double *w, const double *iSigma_w,
                         int64_t tile_rows, int32_t flags, gpz_predictor **out);
void gpz_predictor_destroy(gpz_predictor *p);
int gpz_predictor_run(gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi, int32_t psi_kind,
                      double *mu, double *nu, double *beta_i, double *gamma, double *PHI);
int gpz_predictor_route(const gpz_predictor *p, char *buf, int cap);
int gpz_predictor_info(const gpz_predictor *p, int64_t out[4]);

/* ---- posterior draws of the predictive mean through a predictor handle ---------------------------------------------------------
 * F(i, o, s) = PHI(i, :) (w(:, o) + R_o z(:, s, o)) for the complete rows of Xs: draw s is one realisation of the model's weights
 * w_s ~ N(w, iSigma_w) over the whole catalogue, so the spread of an aggregate across draws is its error from the finite training set.
 * R_o R_o' = (iSigma_w(:,:,o) + iSigma_w(:,:,o)') / 2: its Cholesky factor, or V diag(sqrt(max(lambda, 0))) from its eigendecomposition
 * where the Cholesky breaks down (a failed pivot, or min L_jj^2 <= m eps max S_jj).  z: the caller's Z (m x ndraws x k, column-major) or,
 * Z = NULL, z[j, s, o] = sqrt(-2 ln u1) cos(2 pi u2) from (x0, x1, x2, x3) = Philox4x32-10(counter (j, s, o, 0), key (seed & 0xffffffff,
 * seed >> 32)), u1 = (((x1 << 32 | x0) >> 11) + 1) 2^-53, u2 = ((x3 << 32 | x2) >> 11) 2^-53: draw s of a seed is the same on every call
 * and for every ndraws > s.  A row's draws have the same bits for any tile size, row order or split of the rows into calls.
 * Xs: column-major ns x d, normalised (as gpz_predictor_run); ns = 0 does nothing.  F: column-major ns x k x ndraws, without muY.
 * 1 <= ndraws, ndraws * k <= GPZ_DRAWS_MAX_COLUMNS, else GPZ_ERR_ARG; rows with NaN are refused (GPZ_ERR_UNSUPPORTED).  The factors
 * are formed on the device on the first call; the draws buffers are allocated then too (gpz_predictor_info's bytes include them, its
 * runs count gpz_predictor_run calls only), and gpz_predictor_route appends the draws route and each output's factor (cholesky / eigen). */
#define GPZ_DRAWS_MAX_COLUMNS 16384
int gpz_predictor_draws(gpz_predictor *p, const double *Xs, int64_t ns, int32_t ndraws, uint64_t seed,
                        const double *Z /* NULL or m x ndraws x k */, double *F /* ns x k x ndraws, column-major */);

/* ---- stacked predictive densities through a predictor handle: n(z) per group, for the posterior-mean weights and per draw --------
 * Rows i of Xs (complete, noise-free, as for gpz_predictor_draws), outputs o < k, edges e_0 < .. < e_nbins per output, a label
 * g_i in {-1, 0 .. ngroups-1} per row (-1: the row is left out; group = NULL: every row in group 0), a weight omega_i >= 0 per row
 * (weight = NULL: 1).  Columns c = 0 .. ndraws:
 *   c = 0      mu = gpz_predictor_run's mu, width^2 = nu + beta_i (the predictive variance, gamma = 0 for these rows);
 *   c = 1 + s  mu = gpz_predictor_draws' F(i, o, s) for the same seed / Z, width^2 = beta_i (the weight uncertainty is in the draw).
 *   hist[c, g, o, j]  = sum over the rows of group g of omega_i (Phi((e_{j+1} - mu) / width) - Phi((e_j - mu) / width))
 *   sum_w[g]          = sum omega_i      sum_mu[c, g, o] = sum omega_i mu      sum_mu2[c, g, o] = sum omega_i mu^2
 * edges: k x (nbins + 1), output o's edges at edges[o * (nbins + 1) ..], in the units of mu as this entry sees it: WITHOUT muY, so a
 * caller with edges in the units of y passes e - muY[o]; sum_mu and sum_mu2 are sums of that mu (without muY) too when mu_shift is
 * NULL.  mu_shift (k values, the caller's muY) is added to every mu before it enters sum_mu and sum_mu2, and to nothing else: shifting
 * the finished sums instead (sum mu^2 + 2 muY sum mu + muY^2 sum omega) cancels where a group's mu + muY is small against muY, and a
 * group of a few rows then loses digits that the sums of mu + muY keep.  Mass outside
 * [e_0, e_nbins] is not counted, and a bin further than 9 widths from a row's mu gets none of that row (less than 1.2e-19 omega_i).
 * Layouts, the last index fastest: hist [1 + ndraws][ngroups][k][nbins], sum_w [ngroups], sum_mu and sum_mu2 [1 + ndraws][ngroups][k].
 * Per-row results never leave the device; what comes back does not depend on ns, and the results of several calls add.  The same
 * call on the same handle gives the same bits every time (partial sums per slab of rows, added in a fixed order); another tile size
 * may change the last bits.  ns = 0 returns zeros.
 * GPZ_ERR_ARG: edges not finite or not strictly increasing, nbins < 1, ngroups < 1, a label outside [-1, ngroups), a negative or
 * non-finite weight, ndraws < 0, (1 + ndraws) * k > GPZ_DRAWS_MAX_COLUMNS, ngroups * nbins > GPZ_STACK_MAX_GROUP_BINS (the histogram
 * of one column lives in one workgroup's LDS; with the column limit that is at most 2^26 cells per call).  Rows with NaN:
 * GPZ_ERR_UNSUPPORTED.  ndraws = 0 forms no factors and allocates no draws buffer; the stack buffers are allocated on the first call
 * (gpz_predictor_info's bytes include them) and gpz_predictor_route then appends a stack clause.  A call with a larger shape takes
 * larger accumulator and slab blocks and the handle keeps the outgrown ones until it is destroyed. */
#define GPZ_STACK_MAX_GROUP_BINS 4096
int gpz_predictor_stack(gpz_predictor *p, const double *Xs, int64_t ns, int32_t ndraws, uint64_t seed,
                        const double *Z /* NULL or m x ndraws x k */, const double *edges /* k x (nbins + 1), muY already subtracted */,
                        int32_t nbins, const int32_t *group /* ns or NULL */, int32_t ngroups, const double *weight /* ns or NULL */,
                        double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift /* k or NULL */);

/* ---- device-resident entries of the predictor handle: the catalogue is read from device memory, per-row results stay there ---------
 * The three entries above with the rows, and every per-row result, in the caller's memory on the handle's device: no row and no
 * per-row result crosses the bus.  X_d: element (i, c) of the ns x d rows at X_d[i * row_stride + c * col_stride], strides in elements
 * (a row-major array has (d, 1), a column-major one (1, ns), any view of either its own), x_type GPZ_X_F64 or GPZ_X_F32 (converted to
 * f64, exactly).  muX, sdX (host, d values each): the rows enter the kernels as (x - muX[c]) / sdX[c], one f64 subtraction and one f64
 * division (the bits of the host's normalisation); both NULL: the rows are normalised already.  muY (host, k values or NULL) is added
 * to mu and to the draws.  Every *_d argument is a device pointer; everything else is host memory.
 * gpz_predictor_run_dev: mu_d, nu_d, beta_d (required), sigma_d = nu + beta + gamma, gamma_d = 0 (both optional): column-major ns x k;
 * PHI_d: column-major ns x m or NULL.  gpz_predictor_draws_dev: F_d column-major ns x k x ndraws (with muY when given); Z stays a host
 * array.  gpz_predictor_stack_dev: group_d (ns int32 labels or NULL) and weight_d (ns doubles or NULL) on the device, edges, mu_shift and
 * the results in host memory exactly as gpz_predictor_stack takes and returns them.
 * stream: the caller's hipStream_t (NULL: the legacy default stream).  The call is ordered after everything queued on it so far (an
 * event, not a host synchronisation), runs on the handle's compute stream and returns when its results are complete.  The tile length is
 * the host entry's, and the tile kernels are the host entries' own: the results have the bits of the host entry on the same rows.
 * Before its first tile a call scans all rows (and labels and weights) on the device: rows with NaN -> GPZ_ERR_UNSUPPORTED, a label
 * outside [-1, ngroups) or a negative or non-finite weight -> GPZ_ERR_ARG, in both cases with the outputs untouched.  The argument
 * checks of the host entries apply unchanged; x_type outside {0, 1}, a stride of 0 with ns > 1, or only one of muX / sdX ->
 * GPZ_ERR_ARG.  Input noise has entries of its own below.  gpz_predictor_info's runs count gpz_predictor_run_dev calls too; its bytes
 * grow by one small parameter buffer on the first device call and never with ns; gpz_predictor_route then appends
 * "; device entries: k_pred_stage". */
#define GPZ_X_F64 0
#define GPZ_X_F32 1
int gpz_predictor_run_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                          const double *muX, const double *sdX, const double *muY /* k or NULL */,
                          double *mu_d, double *sigma_d, double *nu_d, double *beta_d, double *gamma_d, double *PHI_d, void *stream);
int gpz_predictor_draws_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                            const double *muX, const double *sdX, const double *muY /* k or NULL */,
                            int32_t ndraws, uint64_t seed, const double *Z /* host: NULL or m x ndraws x k */,
                            double *F_d /* ns x k x ndraws, column-major */, void *stream);
int gpz_predictor_stack_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                            const double *muX, const double *sdX,
                            int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                            const int32_t *group_d /* ns or NULL */, int32_t ngroups, const double *weight_d /* ns or NULL */,
                            double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift /* k or NULL */,
                            void *stream);

/* ---- rows with input noise on the predictor handle --------------------------------------------------------------------------------
 * predictNoisy (predictDiag.m:75-125) and the draws for rows with a variance per input dimension, on the handle's own tiles, where
 * predict_noisy_fits holds: a diagonal kind (GL, VL, GD, VD), d <= 20, k <= 8 and ceil16(m) <= 256 (1024 on a handle with GPZ_PREDICT_LARGE_M).  Any other shape returns
 * GPZ_ERR_UNSUPPORTED and names the condition; gpz_predictor_run takes Psi for every shape on its one-shot route.  Complete rows only.
 * The device entries take what gpz_predictor_run_dev / _draws_dev take, plus Psi_d: element (i, c) of the ns x d variances at
 * Psi_d[i * psi_row_stride + c * psi_col_stride], psi_type GPZ_X_F64 or GPZ_X_F32, a column stride of 0 for one variance per row; and
 * sd2 (host, d values, = sdX squared; NULL with sdX): Psi enters the kernels as double(psi) / sd2[c], one f64 division (the bits of
 * fixPsi).  gpz_predictor_run_noisy_dev: mu_d, nu_d, beta_d (required), gamma_d, sigma_d = (nu + beta) + gamma (optional); there is no
 * PHI argument.  nu reads the lower triangle of iSigma_w(:,:,o) only, as the reference does.  A NaN in the rows -> GPZ_ERR_UNSUPPORTED,
 * an element of Psi that is NaN, negative or (itself or divided by sd2) infinite -> GPZ_ERR_ARG, both found by the scan before the first tile, outputs untouched.
 * gpz_predictor_draws_noisy (host): F(i, o, s) = E_x[PHI](i, :) (w(:, o) + R_o z(:, s, o)), the predictive mean of predictNoisy under
 * weight draw s (it is linear in w); Xs and Psi column-major ns x d, normalised; everything else as gpz_predictor_draws.
 * A row's results have the same bits for any tile size, row order or split of the rows into calls: the pair sum is cut into
 * chunks by the model's shape alone.  The first call with Psi allocates the Psi slots; the first gpz_predictor_run_noisy_dev the pair
 * table (m (m + 1) / 2 records of 1 + 2 d + 3 k doubles), the output slots and the chunk slab (gpz_predictor_info's bytes; a handle that never sees Psi holds what it held), and
 * gpz_predictor_route then ends in "; noise: k_predict_noisy_small (C pair chunks)". */
int gpz_predictor_run_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                const void *Psi_d, int32_t psi_type, int64_t psi_row_stride, int64_t psi_col_stride,
                                const double *muX, const double *sdX, const double *sd2, const double *muY /* k or NULL */,
                                double *mu_d, double *sigma_d, double *nu_d, double *beta_d, double *gamma_d, void *stream);
int gpz_predictor_draws_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                  const void *Psi_d, int32_t psi_type, int64_t psi_row_stride, int64_t psi_col_stride,
                                  const double *muX, const double *sdX, const double *sd2, const double *muY /* k or NULL */,
                                  int32_t ndraws, uint64_t seed, const double *Z /* host: NULL or m x ndraws x k */,
                                  double *F_d /* ns x k x ndraws, column-major */, void *stream);
int gpz_predictor_draws_noisy(gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi /* ns x d, normalised */,
                              int32_t ndraws, uint64_t seed, const double *Z /* NULL or m x ndraws x k */,
                              double *F /* ns x k x ndraws, column-major */);
/* The same two questions for the covariance kinds (predictCov.m:70-132), where predict_noisy_cov_fits holds: GC or VC, 1 <= d <= 10,
 * 1 <= k <= 8 and ceil16(m) <= 256 (1024 on a handle with GPZ_PREDICT_LARGE_M).  Any other shape returns GPZ_ERR_UNSUPPORTED and names the condition.  The arguments are exactly
 * those of gpz_predictor_run_noisy_dev / _draws_noisy_dev: Psi is a variance per input dimension (or one per row), the diagonal that
 * fixPsi puts into the d x d x n cube of these kinds, entering the kernels as double(psi) / sd2[c]; a full Psi cube stays on
 * gpz_predictor_run.  Complete rows only; NaN rows and bad elements of Psi are refused as above, before the first tile, outputs
 * untouched.  Per tile k_predict_noisy_cov_small (a packed Cholesky of Sigma_j + Psi_i and of C_ab + Psi_i per row and record in
 * registers; k_predict_noisy_cov.hip) and the finish kernel of the diagonal kinds; the draws are E_x[PHI] from k_predict_noisy_cov_phi
 * against W on the T-GEMM.  Same bits for any tile size, row order or split of the rows into calls.  The first call writes the basis
 * records (m of 1 + d + d (d + 1) / 2 + 2 k doubles), takes the Psi slots and, for the draws on a fused-route handle, a PHI tile; the
 * first gpz_predictor_run_noisy_cov_dev the pair records (m (m + 1) / 2 of 1 + d + d (d + 1) / 2 + 3 k doubles), the output slots and
 * the chunk slab.  None of it depends on the number of rows, a handle that never calls these holds what it held, and
 * gpz_predictor_route then ends in "; noise: k_predict_noisy_cov_small (C pair chunks)". */
int gpz_predictor_run_noisy_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                    const void *Psi_d, int32_t psi_type, int64_t psi_row_stride, int64_t psi_col_stride,
                                    const double *muX, const double *sdX, const double *sd2, const double *muY /* k or NULL */,
                                    double *mu_d, double *sigma_d, double *nu_d, double *beta_d, double *gamma_d, void *stream);
int gpz_predictor_draws_noisy_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                      int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                      int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                      const double *muY /* k or NULL */, int32_t ndraws, uint64_t seed,
                                      const double *Z /* host: NULL or m x ndraws x k */,
                                      double *F_d /* ns x k x ndraws, column-major */, void *stream);

/* ---- stacked densities of rows with input noise, and gamma under every weight draw ----------------------------------------------------
 * gpz_predictor_stack / _stack_dev for rows with a variance per input dimension, where predict_noisy_fits holds and the handle is on the
 * fused route (GPZ_PREDICT_FORCE_TILES not set); anything else returns GPZ_ERR_UNSUPPORTED and names the condition.  Column 0 (the
 * posterior-mean weights): mu of gpz_predictor_run_noisy_dev, width^2 = (nu + beta) + gamma, the bits of that call's sigma.  Column
 * 1 + s (weight draw s): mu_s of gpz_predictor_draws_noisy_dev, width^2 = beta_i + max(gamma_s,i, 0) with
 *   gamma_s,i = sum_{a >= b} f_ab E[phi_a phi_b](x_i, psi_i) w_s,a w_s,b - mu_s,i^2   (f_ab = 2 off the diagonal, 1 on it),
 * predictNoisy's gamma (predictDiag.m:111-124) under the draw's weights: the variance of PHI(x) w_s over the input noise.  Everything
 * else - edges, groups, weights, mu_shift, layouts, additivity over calls, the 9-width window - is gpz_predictor_stack's.  The host
 * entry takes Psi as gpz_predictor_draws_noisy does (ns x d column-major, normalised), the device entry as gpz_predictor_draws_noisy_dev
 * does (Psi_d, its type and strides, sd2).  An element of Psi that is NaN, negative or infinite -> GPZ_ERR_ARG; rows with NaN ->
 * GPZ_ERR_UNSUPPORTED; in every refusal the outputs are untouched.  Both entries return the same bits for the same rows on the same
 * handle.  ndraws = 0 forms no factors and allocates no draws or gamma buffer.
 * gpz_predictor_draws_gamma_noisy_dev: gpz_predictor_draws_noisy_dev plus Gam_d (ns x k x ndraws column-major, device) <- gamma_s,
 * unclamped.  A row's gamma_s has the same bits for any tile size, row order, split into calls and any ndraws > s.
 * The first of these calls adds to the handle what gpz_predictor_run_noisy_dev adds, plus the chunk slab of the pair sums
 * (predict_gamma_chunks(m) x ndraws k x tile rows doubles) and, for the stacks, the widths ((1 + ndraws) k x tile rows); nothing grows
 * with ns, and gpz_predictor_route then holds "; noise per draw: k_predict_noisy_gamma (C pair chunks)", followed by
 * " + k_stack_tile_w" once one of the stack entries has been called. */
int gpz_predictor_stack_noisy(gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi /* ns x d, normalised */,
                              int32_t ndraws, uint64_t seed, const double *Z /* NULL or m x ndraws x k */,
                              const double *edges /* k x (nbins + 1), muY already subtracted */, int32_t nbins,
                              const int32_t *group /* ns or NULL */, int32_t ngroups, const double *weight /* ns or NULL */,
                              double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift /* k or NULL */);
int gpz_predictor_stack_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                  const void *Psi_d, int32_t psi_type, int64_t psi_row_stride, int64_t psi_col_stride,
                                  const double *muX, const double *sdX, const double *sd2,
                                  int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                  const int32_t *group_d /* ns or NULL */, int32_t ngroups, const double *weight_d /* ns or NULL */,
                                  double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift /* k or NULL */,
                                  void *stream);
int gpz_predictor_draws_gamma_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                        int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                        int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                        const double *muY /* k or NULL */, int32_t ndraws, uint64_t seed,
                                        const double *Z /* host: NULL or m x ndraws x k */, double *F_d /* ns x k x ndraws, column-major */,
                                        double *Gam_d /* ns x k x ndraws, column-major */, void *stream);

/* The same for the covariance kinds: gpz_predictor_stack_noisy_dev and gpz_predictor_draws_gamma_noisy_dev for rows with a variance per
 * input dimension on a GC or VC model, where predict_noisy_cov_fits holds (any other model returns GPZ_ERR_UNSUPPORTED and names that
 * function) and on any route of the handle.  The arguments are exactly those of the two entries above.  Column 0: mu of
 * gpz_predictor_run_noisy_cov_dev, width^2 = (nu + beta) + gamma, the bits of that call's sigma.  Column 1 + s: mu_s of
 * gpz_predictor_draws_noisy_cov_dev, width^2 = beta_i + max(gamma_s,i, 0) with
 *   gamma_s,i = sum_{a >= b} f_ab z_ab(x_i, psi_i) w_s,a w_s,b - mu_s,i^2,   z_ab = exp(lnZ_ab - q / 2) prod_c 1 / L_cc
 * from the Cholesky factor L of C_ab + diag(psi_i): predictNoisy's gamma (predictCov.m:105-119) under the draw's weights.  Per tile
 * k_predict_noisy_cov_gamma (k_predict_noisy_cov_gamma.hip: k_predict_noisy_gamma's f64 MFMA product with k_predict_noisy_cov_small's
 * pair density, on the head of the handle's packed pair records) in front of the same finish and stack kernels.  Rows with NaN ->
 * GPZ_ERR_UNSUPPORTED, a bad element of Psi, label or weight -> GPZ_ERR_ARG, all found before the first tile; in every refusal the
 * outputs are untouched.  Gam_d is unclamped; a row's gamma_s has the same bits for any tile size, row order, split into calls and any
 * ndraws > s.  The first of these calls adds to the handle what gpz_predictor_run_noisy_cov_dev adds and, with draws, what
 * gpz_predictor_draws_noisy_cov_dev adds, plus the chunk slab of the pair sums (predict_gamma_chunks(m) x ndraws k x tile rows doubles)
 * and, for the stack, the widths ((1 + ndraws) k x tile rows); ndraws = 0 forms no factors and takes no draws buffer and no slab.
 * Nothing grows with ns, and gpz_predictor_route then ends in "; noise per draw: k_predict_noisy_cov_gamma (C pair chunks)", followed
 * by " + k_stack_tile_w" once the stack entry has been called. */
int gpz_predictor_stack_noisy_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                      const void *Psi_d, int32_t psi_type, int64_t psi_row_stride, int64_t psi_col_stride,
                                      const double *muX, const double *sdX, const double *sd2,
                                      int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                      const int32_t *group_d /* ns or NULL */, int32_t ngroups, const double *weight_d /* ns or NULL */,
                                      double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift /* k or NULL */,
                                      void *stream);
int gpz_predictor_draws_gamma_noisy_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                            int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                            int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                            const double *muY /* k or NULL */, int32_t ndraws, uint64_t seed,
                                            const double *Z /* host: NULL or m x ndraws x k */, double *F_d /* ns x k x ndraws, column-major */,
                                            double *Gam_d /* ns x k x ndraws, column-major */, void *stream);

/* ---- a full input-noise covariance per row on the predictor handle, covariance kinds --------------------------------------------------
 * The four questions of the *_noisy_cov_dev entries for rows whose Psi is a d x d matrix each, the d x d x n cube that fixPsi.m and
 * predictCov.m:109 take: gpz_predictor_run_psi_cube_dev (the moments), _draws_psi_cube_dev, _draws_gamma_psi_cube_dev and
 * _stack_psi_cube_dev, where predict_noisy_cov_fits holds (any other model returns GPZ_ERR_UNSUPPORTED and names that function).  Each
 * has the arguments of its noisy_cov twin with three Psi strides in place of two - element (r, c) of row i lies at
 * Psi_d[r psi_mrow_stride + c psi_mcol_stride + i psi_row_stride], so the reference's column-major d x d x n cube is (1, d, d d) and an
 * n x d x d array is read where it lies - and div in place of sd2: the d (d + 1) / 2 divisors sdX[r] sdX[c] at r (r + 1) / 2 + c, a host
 * or a device pointer (NULL together with muX / sdX: no normalisation).  Only the lower triangle (r >= c) of a row's matrix is read and
 * scanned; it enters the kernels as double(psi) / div, a plain f64 division (fixPsi.m:36).  An element of a lower triangle that is NaN
 * or infinite, itself or after its division, or a negative diagonal element -> GPZ_ERR_ARG; rows with NaN -> GPZ_ERR_UNSUPPORTED; a bad
 * label or weight -> GPZ_ERR_ARG; all found before the first tile (k_pred_check_psi_cube), outputs untouched.  A matrix that passes the
 * scan but is not positive semidefinite is the caller's error: that row's results are unspecified (NaN where a pivot of
 * S + Psi_i is not positive) and no other row is affected.
 * Per tile k_pred_stage_psi_cube packs the lower triangles into [d (d + 1) / 2][tile rows] and k_predict_psi_cube_small / _phi / _gamma
 * (k_predict_psi_cube.hip, k_predict_psi_cube_gamma.hip) are the noisy_cov kernels with the packed Cholesky of S + Psi_i over the whole
 * triangle, on the same records, chunk counts, finish kernels, T-GEMM and stack kernel.  A cube with zeros off the diagonal returns the
 * bits of the noisy_cov entries on its diagonal.  Same bits for any tile size, row order, split into calls and any ndraws > s.  The
 * first call adds to the handle what the twin adds except the Psi slots, and in their place two slots of d (d + 1) / 2 x tile rows
 * doubles and the divisor triangle; on a handle that has served the twin it adds only these.  Nothing grows with ns, and
 * gpz_predictor_route then holds "; noise cube: k_predict_psi_cube_small (C pair chunks)" and, after gamma per draw or a stack,
 * "; noise cube per draw: k_predict_psi_cube_gamma (C pair chunks)" (" + k_stack_tile_w" once the stack entry has been called). */
int gpz_predictor_run_psi_cube_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                   const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride, int64_t psi_mcol_stride,
                                   int64_t psi_row_stride, const double *muX, const double *sdX,
                                   const double *div /* d (d + 1) / 2, host or device */, const double *muY /* k or NULL */,
                                   double *mu_d, double *sigma_d, double *nu_d, double *beta_d, double *gamma_d, void *stream);
int gpz_predictor_draws_psi_cube_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                     int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                     int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX, const double *sdX,
                                     const double *div, const double *muY /* k or NULL */, int32_t ndraws, uint64_t seed,
                                     const double *Z /* host: NULL or m x ndraws x k */,
                                     double *F_d /* ns x k x ndraws, column-major */, void *stream);
int gpz_predictor_draws_gamma_psi_cube_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                           int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                           int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX, const double *sdX,
                                           const double *div, const double *muY /* k or NULL */, int32_t ndraws, uint64_t seed,
                                           const double *Z /* host: NULL or m x ndraws x k */,
                                           double *F_d /* ns x k x ndraws, column-major */,
                                           double *Gam_d /* ns x k x ndraws, column-major */, void *stream);
int gpz_predictor_stack_psi_cube_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                     const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride, int64_t psi_mcol_stride,
                                     int64_t psi_row_stride, const double *muX, const double *sdX, const double *div,
                                     int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                     const int32_t *group_d /* ns or NULL */, int32_t ngroups, const double *weight_d /* ns or NULL */,
                                     double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift /* k or NULL */,
                                     void *stream);

/* ---- rows with missing inputs on the predictor handle ------------------------------------------------------------------------------
 * predictMissing (predictDiag.m:127-209) and the draws for ONE group of rows that share a NaN pattern, on the handle's own tiles,
 * where predict_missing_fits holds: a diagonal kind (GL, VL, GD, VD), d <= 20, k <= 8 and ceil16(m) <= 256, no Psi.  Any other shape
 * returns GPZ_ERR_UNSUPPORTED and names the condition; gpz_predict_missing takes every shape.  The entries take what
 * gpz_predictor_run_dev / _draws_dev take, plus priors (host, m values; NULL: 1 / m each) and obs_mask, the pattern: bit c is set
 * when dimension c is observed.  A mask with no missing dimension or with a bit at or above d -> GPZ_ERR_ARG; a mask with no observed
 * dimension is valid.  Before the first tile a scan verifies that every row is NaN exactly where the mask says missing; otherwise
 * GPZ_ERR_ARG ("the rows of a group must share one NaN pattern"), outputs untouched.  The caller groups the rows (predict.m:45-57).
 * gpz_predictor_run_missing_dev: mu_d, nu_d, beta_d (required), gamma_d, sigma_d = (nu + beta) + gamma (optional).
 * gpz_predictor_draws_missing_dev: F(i, o, s) = PHI_missing(i, :) (w(:, o) + R_o z(:, s, o)) + muY[o]; ndraws, seed, Z and the weights
 * W as gpz_predictor_draws_dev, so draw s is the same weight draw for the rows of every group and for complete rows.
 * Cost per row: O(m^2) for PHI and 2 ceil16(m) m (m + 1) / 2 flop on the f64 MFMA plus m (m + 1) / 2 exp for the pair sums; the n x pairs
 * product never reaches memory.  Per pattern (kept until the pattern or the priors change): m (m + 1) / 2 x ceil16(m) doubles of U
 * (4.5 MB at m = 100, 67 MB at m = 256), the pair records and an mp x mp factor; per handle three [tile][mp] buffers with tile =
 * min(tile_rows, 16384).  All of it is allocated on the first such call and does not grow with ns or the number of patterns; a
 * handle that never sees such a call holds what it held.  A row's results have the same bits for any tile size, row order or split
 * of the rows into calls.  gpz_predictor_route then ends in "; missing: k_predict_missing_pairs (C pair chunks), T-row tiles".
 * On a handle with GPZ_PREDICT_LARGE_M_MISSING these entries, the stack and gamma-per-draw entries below and their noisy_missing
 * twins take ceil16(m) <= 1024 (predict_missing_large_fits); past 256 the route text then adds "; missing past 256: k_pml_pairs / k_pml_gamma
 * (K panels of 128, 4 groups per batch)", 2 groups where k > 1. */
int gpz_predictor_run_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                  const double *muX, const double *sdX, const double *muY /* k or NULL */,
                                  const double *priors /* m or NULL */, uint32_t obs_mask,
                                  double *mu_d, double *sigma_d, double *nu_d, double *beta_d, double *gamma_d, void *stream);
int gpz_predictor_draws_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                    const double *muX, const double *sdX, const double *muY /* k or NULL */,
                                    const double *priors /* m or NULL */, uint32_t obs_mask,
                                    int32_t ndraws, uint64_t seed, const double *Z /* host: NULL or m x ndraws x k */,
                                    double *F_d /* ns x k x ndraws, column-major */, void *stream);

/* ---- rows with missing inputs on the predictor handle, covariance kinds ----------------------------------------------------------------
 * predictMissing of GC and VC (predictCov.m:134-232) and the draws for ONE group of rows that share a NaN pattern, where
 * predict_missing_cov_fits holds: GC or VC, 1 <= d <= 10, 1 <= k <= 8 and ceil16(m) <= 256, no Psi, device tensors.  Any other shape
 * returns GPZ_ERR_UNSUPPORTED and names the condition (gpz_predict_missing takes every shape); a diagonal kind returns
 * GPZ_ERR_UNSUPPORTED and names gpz_predictor_run_missing_dev.  The two entries take exactly the arguments of
 * gpz_predictor_run_missing_dev / _draws_missing_dev, and priors, obs_mask, the scan of the pattern and every refusal are theirs.
 * With no observed dimensions every density of predictMissing is exp(lnw - 1/2 |U (x_o - a)|^2) in the row's observed inputs x_o alone
 * (a record of 1 + no + no (no + 1) / 2 doubles per centre and component, k_predict_missing_cov.hip), so a row costs
 * m + m^2 + m^2 (m + 1) / 2 densities of no (no + 3) / 2 multiply-adds and one exp each.  Per pattern (kept until the pattern or the
 * priors change): the m + m^2 records of Ex and PHI; per handle the model's Sigma_j and pair records (O(m^2 d^2) doubles), two
 * [tile][mp] buffers with tile = min(tile_rows, 16384), predict_missing_cov_chunks(m) x 3k x tile partial sums and one slab of at most
 * 64 MB through which the m^2 (m + 1) / 2 pair-component records pass, regenerated per tile (kept where they all fit).  All of it is
 * allocated on the first such call, sized for the widest pattern, and does not grow with ns or the number of patterns; a handle that
 * never sees such a call holds what it held.  A row's results have the same bits for any tile size, row order or split of the rows
 * into calls.  gpz_predictor_route then ends in "; missing: k_predict_missing_cov_pairs (C pair chunks)". */
int gpz_predictor_run_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                      int64_t col_stride, const double *muX, const double *sdX, const double *muY /* k or NULL */,
                                      const double *priors /* m or NULL */, uint32_t obs_mask,
                                      double *mu_d, double *sigma_d, double *nu_d, double *beta_d, double *gamma_d, void *stream);
int gpz_predictor_draws_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                        int64_t col_stride, const double *muX, const double *sdX, const double *muY /* k or NULL */,
                                        const double *priors /* m or NULL */, uint32_t obs_mask,
                                        int32_t ndraws, uint64_t seed, const double *Z /* host: NULL or m x ndraws x k */,
                                        double *F_d /* ns x k x ndraws, column-major */, void *stream);

/* ---- stacked densities of rows with missing inputs, and gamma under every weight draw --------------------------------------------------
 * gpz_predictor_stack_dev for ONE group of rows that share a NaN pattern (non-detections), and gpz_predictor_draws_missing_dev with
 * gamma: the scope (predict_missing_fits), priors, obs_mask, the scan of the pattern and its refusals are those of the two entries
 * above; no Psi, no host-array entry.  Column 0 (the posterior-mean weights): mu of gpz_predictor_run_missing_dev, width^2 = (nu + beta)
 * + gamma, the bits of that call's sigma.  Column 1 + s (weight draw s): mu_s of gpz_predictor_draws_missing_dev, width^2 = beta_i +
 * max(gamma_s,i, 0) with
 *   gamma_s,i = sum_{a >= b} f_ab EcC_ab(x_i) w_s,a w_s,b - mu_s,i^2   (f_ab = 2 off the diagonal, 1 on it),
 * predictMissing's gamma (predictDiag.m:172-198, :209) under the draw's weights: the variance of PHI(x) w_s over the missing
 * dimensions; beta_i does not depend on w.  Everything else - edges, groups, weights, mu_shift, layouts, additivity over calls, the
 * 9-width window - is gpz_predictor_stack's, so the results of the groups of a catalogue (and of gpz_predictor_stack_dev on its
 * complete rows) add field by field.  A bad label or weight -> GPZ_ERR_ARG; in every refusal the outputs are untouched.  ndraws = 0
 * forms no factors and allocates no draws or gamma buffer.
 * gpz_predictor_draws_gamma_missing_dev: gpz_predictor_draws_missing_dev plus Gam_d (ns x k x ndraws column-major, device) <- gamma_s,
 * unclamped.  A row's gamma_s has the same bits for any tile size, row order, position among other rows, split into calls and any
 * ndraws > s.  k_predict_missing_gamma forms the pair expectations as gpz_predictor_run_missing_dev's pair kernel does and multiplies
 * them into all draws at once on the f64 MFMA: 2 (ceil16(m) + ceil16(ndraws k)) m (m + 1) / 2 flop per row.
 * The first of these calls adds to the handle what the two entries above add, plus the chunk slab of the pair sums
 * (predict_missing_chunks(m) x ndraws k x tile rows doubles, tile = min(draws tile, 16384)) and, for the stack, the widths ((1 + ndraws)
 * k x tile rows) and gpz_predictor_stack_dev's accumulators and slabs; nothing grows with ns or the number of patterns, and
 * gpz_predictor_route then holds "; missing per draw: k_predict_missing_gamma (C pair chunks)", followed by " + k_stack_tile_w" once
 * the stack entry has been called. */
int gpz_predictor_draws_gamma_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                          int64_t col_stride, const double *muX, const double *sdX, const double *muY /* k or NULL */,
                                          const double *priors /* m or NULL */, uint32_t obs_mask,
                                          int32_t ndraws, uint64_t seed, const double *Z /* host: NULL or m x ndraws x k */,
                                          double *F_d /* ns x k x ndraws, column-major */,
                                          double *Gam_d /* ns x k x ndraws, column-major */, void *stream);
int gpz_predictor_stack_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                    const double *muX, const double *sdX,
                                    const double *priors /* m or NULL */, uint32_t obs_mask,
                                    int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                    const int32_t *group_d /* ns or NULL */, int32_t ngroups, const double *weight_d /* ns or NULL */,
                                    double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift /* k or NULL */,
                                    void *stream);

/* ---- the same for a covariance kind -----------------------------------------------------------------------------------------------------
 * gpz_predictor_stack_missing_dev and gpz_predictor_draws_gamma_missing_dev for ONE group of rows of a GC or VC model that share a NaN
 * pattern, with exactly those entries' arguments; the scope (predict_missing_cov_fits), priors, obs_mask, the scan of the pattern and
 * every refusal are those of gpz_predictor_run_missing_cov_dev / _draws_missing_cov_dev (a diagonal kind is sent to the two entries
 * above by name).  Column 0: mu of gpz_predictor_run_missing_cov_dev, width^2 = (nu + beta) + gamma, the bits of that call's sigma.
 * Column 1 + s: mu_s of gpz_predictor_draws_missing_cov_dev, width^2 = beta_i + max(gamma_s,i, 0) with
 *   gamma_s,i = sum_{a >= b} f_ab z_ab(x_i) w_s,a w_s,b - mu_s,i^2,   z_ab(x) = sum_l Pio_l(x) exp(lnw_abl - 1/2 |U_abl (x_o - a_abl)|^2),
 * predictMissing's gamma (predictCov.m:183-216) under the draw's weights, returned unclamped in Gam_d.  k_predict_missing_cov_gamma
 * forms z from the records of gpz_predictor_run_missing_cov_dev's pair kernel (m exp per pair and row) and multiplies it into all
 * draws at once on the f64 MFMA; a stack therefore forms every z twice, once per kernel.  A row's gamma_s has the same bits for any
 * tile size, row order, position among other rows, split into calls and any ndraws > s.  The first of these calls adds to the handle
 * what the two covariance entries above add, plus the chunk slab of the pair sums (predict_missing_cov_chunks(m) x ndraws k x tile
 * rows doubles) and, for the stack, the widths ((1 + ndraws) k x tile rows) and gpz_predictor_stack_dev's accumulators and slabs;
 * nothing grows with ns or the number of patterns, and gpz_predictor_route then holds "; missing per draw: k_predict_missing_cov_gamma
 * (C pair chunks)", followed by " + k_stack_tile_w" once the stack entry has been called. */
int gpz_predictor_draws_gamma_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                              int64_t col_stride, const double *muX, const double *sdX, const double *muY /* k or NULL */,
                                              const double *priors /* m or NULL */, uint32_t obs_mask,
                                              int32_t ndraws, uint64_t seed, const double *Z /* host: NULL or m x ndraws x k */,
                                              double *F_d /* ns x k x ndraws, column-major */,
                                              double *Gam_d /* ns x k x ndraws, column-major */, void *stream);
int gpz_predictor_stack_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                        const double *muX, const double *sdX,
                                        const double *priors /* m or NULL */, uint32_t obs_mask,
                                        int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                        const int32_t *group_d /* ns or NULL */, int32_t ngroups, const double *weight_d /* ns or NULL */,
                                        double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift /* k or NULL */,
                                        void *stream);

/* ---- rows with input noise AND missing inputs on the predictor handle -------------------------------------------------------------------
 * predictNoisyMissing (predictDiag.m:211-297) and the draws for ONE group of rows that share a NaN pattern and carry a variance per
 * input dimension, on the handle's own tiles, where predict_missing_fits holds (a diagonal kind, d <= 20, k <= 8, ceil16(m) <= 256);
 * any other shape returns GPZ_ERR_UNSUPPORTED and names the condition, and gpz_predict_missing takes every shape.  The entries take
 * what gpz_predictor_run_noisy_dev / _draws_noisy_dev take (Psi_d with its type and strides, sd2), with priors and obs_mask behind muY
 * as the missing entries have them, and the mask rules are theirs.  The scan before the first tile refuses a row whose NaN pattern
 * differs from the mask (GPZ_ERR_ARG, "the rows of a group must share one NaN pattern") and an element of Psi that is NaN, negative or
 * infinite IN AN OBSERVED DIMENSION (GPZ_ERR_ARG, the text of the noisy entries); outputs untouched in both cases.  Psi in a missing
 * dimension is never read, whatever it holds.  Complete rows go to gpz_predictor_run_noisy_dev / _draws_noisy_dev.
 * The tables of the pattern are those of the missing entries (Psi touches the observed dimensions only); a second pair-record table,
 * a function of the model alone, is written on the first call.  Per tile: No and Pio with psi in the widths, PHI through the T-GEMM,
 * and k_predict_noisy_missing_pairs: the f64-MFMA product of the missing pair kernel with the epilogue of k_predict_noisy_small, one
 * (C_q + psi)^-1/2 per (row, pair, observed dimension).  The draws are PHI W + muY with the handle's weight draws, the same draw s for
 * the rows of every group.  The first call allocates what the missing and noisy entries would (where the handle does not hold it yet)
 * plus the second record table; nothing grows with ns or the number of patterns, a handle that never makes such a call holds what it
 * held, and a row's results have the same bits for any tile size, row order or split of the rows into calls.  gpz_predictor_route then
 * holds "; noisy missing: k_predict_noisy_missing_pairs (C pair chunks)".  The stack and gamma per draw follow below; no host-array
 * entry. */
int gpz_predictor_run_noisy_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                        int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                        int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                        const double *muY /* k or NULL */, const double *priors /* m or NULL */, uint32_t obs_mask,
                                        double *mu_d, double *sigma_d, double *nu_d, double *beta_d, double *gamma_d, void *stream);
int gpz_predictor_draws_noisy_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                          int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                          int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                          const double *muY /* k or NULL */, const double *priors /* m or NULL */, uint32_t obs_mask,
                                          int32_t ndraws, uint64_t seed, const double *Z /* host: NULL or m x ndraws x k */,
                                          double *F_d /* ns x k x ndraws, column-major */, void *stream);

/* ---- rows with input noise AND missing inputs on the predictor handle, covariance kinds -------------------------------------------------
 * predictNoisyMissing of predictCov.m:233-337 and the draws of its mean for ONE group of rows that share a NaN pattern and carry a
 * variance per input dimension (entering as psi / sd2[c] on the diagonal of the row's Psi, as fixPsi puts it there; a full d x d x n
 * cube stays on gpz_predict_missing), where predict_missing_cov_fits holds (GC or VC, 1 <= d <= 10, k <= 8, ceil16(m) <= 256); any
 * other shape returns GPZ_ERR_UNSUPPORTED and names the function, a diagonal kind GPZ_ERR_UNSUPPORTED naming
 * gpz_predictor_run_noisy_missing_dev.  The arguments are exactly those of gpz_predictor_run_noisy_missing_dev /
 * _draws_noisy_missing_dev, and the scans before the first tile are theirs: a row whose NaN pattern differs from the mask and an
 * element of Psi that is NaN, negative or infinite IN AN OBSERVED DIMENSION are GPZ_ERR_ARG with their texts, outputs untouched.  Psi
 * in a missing dimension is never read; a group with nothing observed (obs_mask 0) reads no Psi at all and gets the bits of
 * gpz_predictor_run_missing_cov_dev / _draws_missing_cov_dev.  Complete rows go to gpz_predictor_run_noisy_cov_dev /
 * _draws_noisy_cov_dev.
 * Every density of predictNoisyMissing is N(T x_o + s - c ; S + G Psi_oo G') with S, T and s of predictMissing and G the rows of T where
 * predictCov.m:271-273 scatters them through `unshuffle` (kept as written: G = T only where [observed | missing] is its own inverse).
 * Whitened by S and split by a QR of G, the exponent is a sum of d - no squares and one no x no form in (M + Psi_oo)^-1, written once
 * per pattern as a record of 1 + no + no (no + 1) / 2 + no no + (d - no)(no + 1) doubles (k_predict_noisy_missing_cov.hip), so a
 * density costs a packed no x no Cholesky of M + diag(psi_o) and a forward substitution in registers, not a d x d factorisation.
 * The tile buffers, the pattern's [R | CU | off] and coefficients, the chunks and the order of every sum are those of the missing_cov
 * entries, whose own tables stay valid; the first call adds the Psi slots where the handle has none, the Ex and PHI records and a
 * slab of at most 64 MB in this form, sized for the widest pattern of the model.
 * Nothing grows with ns or the number of patterns, a handle that never makes such a call holds what it held, and a row's results
 * have the same bits for any tile size, row order, company or split of the rows into calls.  The draws are PHI W + muY with the
 * handle's weight draws.  gpz_predictor_route then holds "; noisy missing: k_predict_noisy_missing_cov_pairs (C pair chunks)".
 * The stack and gamma per draw of such rows follow at the end of the predictor's entries; host arrays and PHI are not on the handle. */
int gpz_predictor_run_noisy_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                            int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                            int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                            const double *muY /* k or NULL */, const double *priors /* m or NULL */, uint32_t obs_mask,
                                            double *mu_d, double *sigma_d, double *nu_d, double *beta_d, double *gamma_d, void *stream);
int gpz_predictor_draws_noisy_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                              int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                              int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                              const double *muY /* k or NULL */, const double *priors /* m or NULL */, uint32_t obs_mask,
                                              int32_t ndraws, uint64_t seed, const double *Z /* host: NULL or m x ndraws x k */,
                                              double *F_d /* ns x k x ndraws, column-major */, void *stream);

/* ---- stacked densities of rows with input noise AND missing inputs, and gamma under every weight draw ----------------------------------
 * gpz_predictor_stack_noisy_dev for ONE group of rows that share a NaN pattern and carry a variance per input dimension, and
 * gpz_predictor_draws_noisy_missing_dev with gamma: the scope (predict_missing_fits), Psi, priors, obs_mask, the scans of the pattern
 * and of Psi in the observed dimensions and their refusals are those of the two entries above; no host-array entry.  Column 0 (the
 * posterior-mean weights): mu of gpz_predictor_run_noisy_missing_dev, width^2 = (nu + beta) + gamma, the bits of that call's sigma.
 * Column 1 + s (weight draw s): mu_s of gpz_predictor_draws_noisy_missing_dev, width^2 = beta_i + max(gamma_s,i, 0) with
 *   gamma_s,i = sum_{a >= b} f_ab EcC_ab(x_i, psi_i) w_s,a w_s,b - mu_s,i^2   (f_ab = 2 off the diagonal, 1 on it),
 * predictNoisyMissing's gamma (predictDiag.m:257-295) under the draw's weights: the variance of PHI(x) w_s over the input noise and the
 * missing dimensions together; beta_i does not depend on w.  On a complete row gamma_s is gpz_predictor_draws_gamma_noisy_dev's.
 * Everything else - edges, groups, weights, mu_shift, layouts, additivity over calls, the 9-width window - is gpz_predictor_stack's, so
 * the results of the groups of a catalogue (and of gpz_predictor_stack_noisy_dev on its complete rows) add field by field.  A bad
 * label or weight -> GPZ_ERR_ARG; in every refusal the outputs are untouched and the handle gains no byte.
 * gpz_predictor_draws_gamma_noisy_missing_dev: gpz_predictor_draws_noisy_missing_dev plus Gam_d (ns x k x ndraws column-major, device)
 * <- gamma_s, unclamped.  A row's gamma_s has the same bits for any tile size, row order, position among other rows, split into calls
 * and any ndraws > s.  k_predict_noisy_missing_gamma forms the pair expectations as k_predict_noisy_missing_pairs does and multiplies
 * them into all draws at once on the f64 MFMA, up to 128 columns per launch.  The first of these calls adds to the handle what the two
 * entries above add, plus the chunk slab of the pair sums and, for the stack, the widths and gpz_predictor_stack_dev's accumulators
 * and slabs; nothing grows with ns or the number of patterns, and gpz_predictor_route then holds
 * "; noisy missing per draw: k_predict_noisy_missing_gamma (C pair chunks)", followed by " + k_stack_tile_w" once the stack entry has
 * been called. */
int gpz_predictor_draws_gamma_noisy_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                const double *muY /* k or NULL */, const double *priors /* m or NULL */,
                                                uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                const double *Z /* host: NULL or m x ndraws x k */,
                                                double *F_d /* ns x k x ndraws, column-major */,
                                                double *Gam_d /* ns x k x ndraws, column-major */, void *stream);
int gpz_predictor_stack_noisy_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                          int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                          int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                          const double *priors /* m or NULL */, uint32_t obs_mask,
                                          int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                          const int32_t *group_d /* ns or NULL */, int32_t ngroups, const double *weight_d /* ns or NULL */,
                                          double *hist, double *sum_w, double *sum_mu, double *sum_mu2,
                                          const double *mu_shift /* k or NULL */, void *stream);

/* ---- stacked densities of rows with input noise AND missing inputs on a covariance kind, and gamma under every weight draw -------------
 * gpz_predictor_stack_noisy_missing_dev and gpz_predictor_draws_gamma_noisy_missing_dev for a covariance kind: the arguments are exactly
 * theirs; the scope (predict_missing_cov_fits), Psi, priors, obs_mask, the scans of the pattern and of Psi in the observed dimensions and
 * every refusal are those of gpz_predictor_run_noisy_missing_cov_dev / _draws_noisy_missing_cov_dev (a diagonal kind is sent to the two
 * entries above by name), made before the first tile with the outputs untouched; no host-array entry.  Column 0: mu of
 * gpz_predictor_run_noisy_missing_cov_dev, width^2 = (nu + beta) + gamma, the bits of that call's sigma.  Column 1 + s: mu_s of
 * gpz_predictor_draws_noisy_missing_cov_dev, width^2 = beta_i + max(gamma_s,i, 0) with
 *   gamma_s,i = sum_{a >= b} f_ab z_ab(x_i, psi_i) w_s,a w_s,b - mu_s,i^2   (f_ab = 2 off the diagonal, 1 on it),
 * predictNoisyMissing's gamma of predictCov.m:308-320 under the draw's weights, z_ab the pair quantity of
 * k_predict_noisy_missing_cov_pairs.  k_predict_noisy_missing_cov_gamma forms z from that kernel's slab records and the tile's Pio (m
 * densities per pair and row, each a packed no x no Cholesky of M + diag(psi_o)) and multiplies it into all draws at once on the f64
 * MFMA, up to 128 columns per pass (64 with seven observed dimensions).  A table of one slab is kept on the handle, whichever kernel
 * filled it; with several slabs they are generated again per tile behind the pair kernel's own pass.  A group with nothing observed
 * (obs_mask 0) reads no Psi and gets the bits of gpz_predictor_draws_gamma_missing_cov_dev / _stack_missing_cov_dev.  Complete rows go
 * to gpz_predictor_draws_gamma_noisy_cov_dev / _stack_noisy_cov_dev.  Everything else - edges, groups, weights, mu_shift, layouts,
 * additivity over calls - is gpz_predictor_stack's.  gpz_predictor_draws_gamma_noisy_missing_cov_dev: Gam_d (ns x k x ndraws
 * column-major, device) <- gamma_s, unclamped; F_d has the bits of gpz_predictor_draws_noisy_missing_cov_dev.  A row's gamma_s has the
 * same bits for any tile size, row order, position among other rows, split into calls and any ndraws > s.  The first of these calls
 * adds to the handle what the two entries above add, plus the chunk slab of the pair sums and, for the stack, the widths and
 * gpz_predictor_stack_dev's accumulators and slabs; nothing grows with ns or the number of patterns, and gpz_predictor_route then
 * holds "; noisy missing per draw: k_predict_noisy_missing_cov_gamma (C pair chunks)", followed by " + k_stack_tile_w" once the stack
 * entry has been called. */
int gpz_predictor_draws_gamma_noisy_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                    int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                    int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                    const double *muY /* k or NULL */, const double *priors /* m or NULL */,
                                                    uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                    const double *Z /* host: NULL or m x ndraws x k */,
                                                    double *F_d /* ns x k x ndraws, column-major */,
                                                    double *Gam_d /* ns x k x ndraws, column-major */, void *stream);
int gpz_predictor_stack_noisy_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                              int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                              int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                              const double *priors /* m or NULL */, uint32_t obs_mask,
                                              int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                              const int32_t *group_d /* ns or NULL */, int32_t ngroups, const double *weight_d /* ns or NULL */,
                                              double *hist, double *sum_w, double *sum_mu, double *sum_mu2,
                                              const double *mu_shift /* k or NULL */, void *stream);

/* ---- rows with a full input-noise covariance AND missing inputs on a covariance kind: all four questions ------------------------------
 * One group of rows that share a NaN pattern and carry a d x d matrix Psi each (the cube of fixPsi.m:36, which predictCov.m takes):
 * gpz_predictor_run_psi_cube_missing_dev (the moments), _draws_psi_cube_missing_dev, _draws_gamma_psi_cube_missing_dev and
 * _stack_psi_cube_missing_dev, where predict_missing_cov_fits holds (GC or VC, 1 <= d <= 10, 1 <= k <= 8, ceil16(m) <= 256; any other
 * model returns GPZ_ERR_UNSUPPORTED and names that function; a diagonal kind is sent to gpz_predictor_run_noisy_missing_dev /
 * _draws_noisy_missing_dev with the cube's diagonal).  Each takes the arguments of its noisy_missing_cov twin with Psi passed as the
 * psi_cube entries pass it: element (r, c) of row i at Psi_d[r psi_mrow_stride + c psi_mcol_stride + i psi_row_stride], f64 or f32, and
 * div, the d (d + 1) / 2 divisors sdX[r] sdX[c] at r (r + 1) / 2 + c (host or device; NULL exactly when sdX is), in place of sd2.
 * Element (r, c) enters as double(Psi) / div.  Only the lower triangle of the observed x observed block of a row's matrix is read,
 * scanned and staged: Psi in a missing row or column is never read and may be NaN.  An element there that is NaN or infinite, itself
 * or after its division, or a negative diagonal element -> GPZ_ERR_ARG; a row off the mask -> GPZ_ERR_ARG; all found before the first
 * tile (k_pmd_check, k_pcm_check_psi), outputs untouched.  A matrix that passes the scan but is not positive semidefinite is the
 * caller's error: a non-positive pivot gives that row NaN and no other row is touched.  Complete rows go to the psi_cube entries
 * (obs_mask without a missing dimension -> GPZ_ERR_ARG); a group with nothing observed (obs_mask 0) reads no Psi and gets the bits of
 * the missing_cov entries.  Per tile k_pcm_stage_psi packs the observed triangles into [no (no + 1) / 2][tile rows] and k_pcm_ex,
 * k_pcm_phi, k_predict_psi_cube_missing_pairs and k_predict_psi_cube_missing_gamma (k_predict_psi_cube_missing.hip,
 * k_predict_psi_cube_missing_gamma.hip) are the noisy_missing_cov kernels with the packed Cholesky of M + Psi_oo over the whole
 * triangle, on that group's records, slabs, chunks and tile buffers: a handle that has served that group on the same pattern builds
 * nothing twice.  A cube with zeros off the diagonal returns the bits of the noisy_missing_cov entries.  A row's results have the same
 * bits for any tile size, row order, company, split into calls and (gamma_s) any ndraws > s.  The first such call adds to the handle
 * what its twin adds, with the psi_cube entries' triangle slots in place of the Psi slots; nothing grows with ns or the number of
 * patterns.  gpz_predictor_route then holds "; noise cube missing: k_predict_psi_cube_missing_pairs (C pair chunks)" and, after gamma
 * per draw or a stack, "; noise cube missing per draw: k_predict_psi_cube_missing_gamma (C pair chunks)" (" + k_stack_tile_w" once
 * the stack entry has been called). */
int gpz_predictor_run_psi_cube_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                           int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                           int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX, const double *sdX,
                                           const double *div, const double *muY /* k or NULL */, const double *priors /* m or NULL */,
                                           uint32_t obs_mask, double *mu_d, double *sigma_d /* or NULL */, double *nu_d, double *beta_d,
                                           double *gamma_d /* or NULL */, void *stream);
int gpz_predictor_draws_psi_cube_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                             int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                             int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX, const double *sdX,
                                             const double *div, const double *muY /* k or NULL */, const double *priors /* m or NULL */,
                                             uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                             const double *Z /* host: NULL or m x ndraws x k */,
                                             double *F_d /* ns x k x ndraws, column-major */, void *stream);
int gpz_predictor_draws_gamma_psi_cube_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                   int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                                   int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX, const double *sdX,
                                                   const double *div, const double *muY /* k or NULL */,
                                                   const double *priors /* m or NULL */, uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                   const double *Z /* host: NULL or m x ndraws x k */,
                                                   double *F_d /* ns x k x ndraws, column-major */,
                                                   double *Gam_d /* ns x k x ndraws, column-major */, void *stream);
int gpz_predictor_stack_psi_cube_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                             int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                             int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX, const double *sdX,
                                             const double *div, const double *priors /* m or NULL */, uint32_t obs_mask,
                                             int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                             const int32_t *group_d /* ns or NULL */, int32_t ngroups, const double *weight_d /* ns or NULL */,
                                             double *hist, double *sum_w, double *sum_mu, double *sum_mu2,
                                             const double *mu_shift /* k or NULL */, void *stream);

/* ---- device-resident L-BFGS memory: minFunc's lbfgsAdd.m / lbfgsProd.m (mex/lbfgsAddC.c, mex/lbfgsProdC.c) ----
 * S and Y (p x corrections) live on the device; all vector arguments are device pointers.
 * gpz_lbfgs_add:        y = g - g_old, s = t*d; skipped (added = 0) when y's <= 1e-10        (lbfgsAdd.m:2-4)
 * gpz_lbfgs_direction:  d = -H*g with Hdiag = y's/y'y of the newest pair                      (lbfgsProd.m, minFunc.m:553-578)
 *                       g_dev = NULL stands for the g of the gpz_lbfgs_add just before (minFunc's order): the products [S Y]'g of that
 *                       pass and its pointer are used, one pass over the memory less; GPZ_ERR_ARG when no gpz_lbfgs_add precedes the
 *                       call or another gpz_lbfgs_direction has come between.  A non-NULL g_dev always forms [S Y]'g itself - the
 *                       address is never compared with an earlier one, the buffer may hold another vector by now
 * gpz_vec_stats:        out = [g.d, max|g|, sum|g|, max|d|] (NaN-propagating), the scalars of minFunc's tests
 * gpz_vec_axpy:         out = x + t*d */
typedef struct gpz_lbfgs gpz_lbfgs;
int gpz_lbfgs_create(int64_t p, int32_t corrections, int32_t device, void *stream, gpz_lbfgs **out);
void gpz_lbfgs_destroy(gpz_lbfgs *h);
int gpz_lbfgs_add(gpz_lbfgs *h, const double *g_dev, const double *g_old_dev, double t, const double *d_dev, int32_t *added);
int gpz_lbfgs_direction(gpz_lbfgs *h, const double *g_dev, double *d_dev);
const char *gpz_lbfgs_last_error(void);
int gpz_vec_stats(const double *g_dev, const double *d_dev, int64_t p, int32_t device, void *stream, double out[4]);
int gpz_vec_axpy(double *out_dev, const double *x_dev, double t, const double *d_dev, int64_t p, int32_t device, void *stream);

/* prior = getPrior(X,Psi,theta,model,[]): mixture weights (1 x m) of the normalised basis densities;
 * iterations (optional) receives the number of fixed-point iterations used (<= 100). */
int gpz_prior(const gpz_desc *desc, const double *theta, const double *Xs, int64_t ns,
              const double *Psi, int32_t psi_kind, double *prior, int32_t *iterations);

/* [Xi,logdet] = inv_logdet(X) for a symmetric m x m matrix (GPz/inv_logdet.m:1-15).  A comfortably
 * positive-definite X goes through the Cholesky inverse; a numerically singular or indefinite one
 * through a Jacobi SVD with the reference's truncation (singular values <= m*eps(max s) dropped from
 * both Xi and logdet).  info (optional): number of singular values dropped (0 = none), -1 = X is not
 * finite (Xi, logdet are NaN then; MATLAB's svd raises). */
int gpz_inv_logdet(const double *A, int32_t m, int32_t device, double *Xi, double *logdet, int32_t *info);

/* D = | |x|^2 + |y|^2 - 2 x y' |, X nx x d, Y ny x d, D nx x ny. */
int gpz_dxy(const double *X, int64_t nx, const double *Y, int64_t ny, int32_t d, int32_t device, double *D);

/* Group id per row = rank (by first occurrence) of the row's NaN pattern; returns the number of
 * groups in *n_groups.  Bit-exact with the greedy loop of getPHI.m:43-54. */
int gpz_nan_groups(const double *X, int64_t n, int32_t d, int32_t device, int32_t *group_id, int32_t *n_groups);

/* ---- all GPUs of the node behind ONE synchronous call (SURVEY.md 8b "threading", 8e) -------------------------------
 * The reference calls [f,g] = funObj(x) from one MATLAB process and blocks on it (minFunc/minFunc.m:314,
 * WolfeLineSearch.m:34,114,194; closure at GPz/train.m:40).  gpz_mgpu_create takes the same arguments as gpz_ctx_create
 * (the whole, unsharded data set), splits the training-selected rows and the validation rows into contiguous balanced
 * blocks, one per device, and keeps one context per device; gpz_mgpu_eval / gpz_mgpu_solve then have the semantics of
 * gpz_eval / gpz_solve.  Inside, one host thread per device drives that device's stream and the two all-reduces of an
 * evaluation are RCCL calls (ncclCommInitAll communicators) on the library's device buffers: only m x m and
 * m x (d^2+d) partials cross xGMI.  desc->device / stream / rank / world are ignored.
 *   n_gpus   <= 0: every device of the node (hipGetDeviceCount)
 *   devices  NULL: 0 .. n_gpus-1 (loopback: all 0)
 *   reducer  GPZ_REDUCER_RCCL, or GPZ_REDUCER_LOOPBACK: an in-library rank-ordered reducer for shards that share one
 *            device (RCCL refuses duplicate devices) - the way the sharded path is tested on single-GPU machines. */
#define GPZ_REDUCER_RCCL     0
#define GPZ_REDUCER_LOOPBACK 1
typedef struct gpz_mgpu gpz_mgpu;
int gpz_mgpu_create(const gpz_desc *desc, int32_t n_gpus, const int32_t *devices, int32_t reducer, int64_t n_tot,
                    const double *X, const double *Y, const double *Psi, int32_t psi_kind, const double *omega,
                    const uint8_t *training, const uint8_t *validation, gpz_mgpu **out);
void gpz_mgpu_destroy(gpz_mgpu *h);
int gpz_mgpu_eval(gpz_mgpu *h, const double *theta, double *f, double *g, double stats[4], double diag[2]);
int gpz_mgpu_solve(gpz_mgpu *h, const double *theta, double *w, double *iSigma_w, double *nlogML_partial);
int32_t gpz_mgpu_size(const gpz_mgpu *h);
/* Failure of one rank inside a call (HIP error, allocation failure, a failed exchange): with GPZ_REDUCER_RCCL the other ranks would
 * wait inside ncclAllReduce for ever, so the failing rank aborts every communicator of the handle (ncclCommAbort); the call returns
 * that rank's error and the handle is DEAD: gpz_mgpu_alive returns 0 and every later gpz_mgpu_eval / _solve returns GPZ_ERR_COMM until
 * the handle is destroyed and re-created.  (The loopback reducer releases its barrier instead and stays usable.)
 * gpz_mgpu_debug_fail_at: test hook - the next call fails on `rank` at its exchange point `exchange` (1 or 2), once. */
int32_t gpz_mgpu_alive(const gpz_mgpu *h);
int gpz_mgpu_debug_fail_at(gpz_mgpu *h, int32_t rank, int32_t exchange);
int64_t gpz_mgpu_theta_len(const gpz_mgpu *h);
/* the context of one rank, for gpz_n_train / gpz_ctx_enable_timing / gpz_ctx_timings / gpz_ctx_set_pinv_mode (apply
 * settings to every rank); owned by the handle - never destroy it. */
gpz_ctx *gpz_mgpu_ctx(gpz_mgpu *h, int32_t rank);
int gpz_device_count(void);
/* Prediction of ONE NaN-pattern group (predict.m:60-69) over several GPUs: the rows are independent, so contiguous row blocks go
 * to the devices, each through the single-device entry its content selects — gpz_predict_full / _noisy / _missing, the choice
 * predictDiag.m:39-55 makes from X (pattern of the first row) and Psi.  Arguments as in those entries (priors and gamma may be
 * NULL when the group has neither missing values nor input noise: gamma is then not written / written as 0); results equal the
 * single-device call row for row.  n_gpus <= 0: every device; devices NULL: 0 .. n_gpus-1 (cyclic when n_gpus exceeds the node:
 * several blocks per device, which is how single-GPU machines exercise the path). */
int gpz_mgpu_predict(const gpz_desc *desc, int32_t n_gpus, const int32_t *devices, const double *theta, const double *w,
                     const double *iSigma_w, const double *priors, const double *Xs, int64_t ns, const double *Psi,
                     int32_t psi_kind, double *mu, double *nu, double *beta_i, double *gamma, double *PHI);

/* ---- one rank per PROCESS (torchrun / mpirun launchers): RCCL inside the library instead of a caller-supplied hook.
 * Rank 0 calls gpz_rccl_unique_id and ships the 128 bytes to the other ranks by any out-of-band means; every rank then
 * calls gpz_ctx_init_rccl on its sharded context (collective: returns when all `world` ranks have called).  The
 * communicator is destroyed with the context.  gpz_rccl_origin: which RCCL the library bound to (dlopen at first use:
 * one the process already carries, else librccl.so.1 from the library path). */
#define GPZ_RCCL_ID_BYTES 128
int gpz_rccl_unique_id(void *id128);
int gpz_ctx_init_rccl(gpz_ctx *ctx, const void *id128, int32_t rank, int32_t world, int32_t device);
const char *gpz_rccl_origin(void);
/* What the communicator behind a context's (a rank's) all-reduce reports about itself, so that a multi-GPU run can prove N ranks on N
 * devices from its own output: info[0] = ncclCommCount, info[1] = ncclCommUserRank, info[2] = ncclCommCuDevice (-1 each when there is
 * no in-library RCCL communicator: single rank, loopback reducer, a caller-supplied hook), info[3] = the HIP device ordinal of the
 * context; bus_id (optional, cap bytes) = that device's PCI bus id.  No reference counterpart. */
int gpz_ctx_comm_info(const gpz_ctx *ctx, int32_t info[4], char *bus_id, int32_t cap);
int gpz_mgpu_comm_info(const gpz_mgpu *h, int32_t rank, int32_t info[4], char *bus_id, int32_t cap);

/* Text of the calling thread's last failure - or of a NEWER failure on another thread (work that failed on one of the library's
 * worker threads); "" when nothing has failed.  The return code of the call is the authority, this is its text.  Valid until the
 * thread's next library call. */
const char *gpz_last_error(void);
int gpz_version(void);

/* Device buffers released by contexts and stand-alone calls are kept (up to 4 GiB per device) for the next call instead of
 * being returned to the runtime one hipFree at a time, and gpz_predict_missing (GC/VC) keeps the last model's covariance and
 * basis-pair tables on the device for the next NaN-pattern group; this hands all of that back.  No reference counterpart. */
void gpz_release_cached_memory(void);

/* Test hook: the kth device allocation from now on (kth >= 1; 0 disarms) reports out-of-memory once, so the release-and-retry
 * path of the allocator can be exercised without exhausting 288 GB.  Process-wide.  No reference counterpart. */
void gpz_debug_fail_alloc(int64_t kth);

#ifdef __cplusplus
}
#endif
#endif /* GPZ_HIP_H */
