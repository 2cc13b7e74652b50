// The streaming predictor's device-resident entries (gpz_predictor_run_dev, _draws_dev, _stack_dev and their _noisy_, _noisy_cov_ and
// _missing_ kin): the rows are read from the caller's device memory and the per-row results are left there.  The handle, the tile functions of
// every kind of rows and the file's place among the predictor's units: gpz_predictor.h and the comment at the top of gpz_predictor.hip.
#include "gpz_predictor.h"

namespace gpzi {
// the caller's rows: element (i, c) at X[i rs + c cs], type GPZ_X_F64 or GPZ_X_F32
struct DevRows {
    const void *X;
    int32_t type;
    int64_t ns, rs, cs;
    int f32() const { return type == GPZ_X_F32; }
};

// What every device entry takes: the rows, their kind (with Psi and sd2 for rows with input noise), the normalisation and the caller's
// stream; and, once predictor_dev_begin has run, where the normalisation lies on the device.
struct DevCall {
    DevRows x;
    const double *muX, *sdX, *muY;
    void *stream;
    Rows rows;
    DevRows psi;
    const double *sd2;
    int64_t psi_mr;      // a cube: the stride between the rows of a matrix (psi.cs: between its columns, psi.rs: between catalogue rows)
    const double *div;   // a cube: the divisors sdX[r] sdX[c] in LT order, host or device (nullptr with sdX: none)
    const double *muX_d, *sdX_d, *muY_d, *sd2_d, *div_d;
};

static DevCall dev_call(const void *X_d, int32_t x_type, int64_t ns, int64_t rs, int64_t cs, const double *muX, const double *sdX,
                        const double *muY, void *stream) {
    DevCall c{};
    c.x = DevRows{X_d, x_type, ns, rs, cs};
    c.muX = muX; c.sdX = sdX; c.muY = muY; c.stream = stream;
    return c;
}

static DevCall with_psi(DevCall c, const void *Psi_d, int32_t psi_type, int64_t rs, int64_t cs, const double *sd2) {
    c.rows.kind = ROWS_NOISY;
    c.psi = DevRows{Psi_d, psi_type, c.x.ns, rs, cs};
    c.sd2 = sd2;
    return c;
}

// complete rows of a covariance kind with a full d x d Psi each: element (r, c) of row i at Psi[r mr + c mc + i rs]
static DevCall with_cube(DevCall c, const void *Psi_d, int32_t psi_type, int64_t mr, int64_t mc, int64_t rs, const double *div) {
    c.rows.kind = ROWS_PSI_CUBE;
    c.psi = DevRows{Psi_d, psi_type, c.x.ns, rs, mc};
    c.psi_mr = mr;
    c.div = div;
    return c;
}

// rows with Psi of a covariance kind: with_psi first
static DevCall with_cov(DevCall c) {
    c.rows.kind = ROWS_NOISY_COV;
    return c;
}

static DevCall with_pattern(DevCall c, const double *priors, uint32_t obs_mask) {
    c.rows = Rows{ROWS_MISSING, obs_mask, priors};
    return c;
}

// such a group on a covariance kind
static DevCall with_cov_pattern(DevCall c, const double *priors, uint32_t obs_mask) {
    c.rows = Rows{ROWS_MISSING_COV, obs_mask, priors};
    return c;
}

// a group whose rows have Psi too: with_psi first, then the pattern
static DevCall with_noisy_pattern(DevCall c, const double *priors, uint32_t obs_mask) {
    c.rows = Rows{ROWS_NOISY_MISSING, obs_mask, priors};
    return c;
}

// such a group with Psi on a covariance kind: with_psi first, then the pattern
static DevCall with_noisy_cov_pattern(DevCall c, const double *priors, uint32_t obs_mask) {
    c.rows = Rows{ROWS_NOISY_MISSING_COV, obs_mask, priors};
    return c;
}

// such a group whose rows have a full d x d Psi each: with_cube first, then the pattern
static DevCall with_cube_pattern(DevCall c, const double *priors, uint32_t obs_mask) {
    c.rows = Rows{ROWS_PSI_CUBE_MISSING, obs_mask, priors};
    return c;
}

static int predictor_dev_args(const char *who, const gpz_predictor *p, const DevRows &x, const double *muX, const double *sdX) {
    if (x.type != GPZ_X_F64 && x.type != GPZ_X_F32)
        return gpz_fail(GPZ_ERR_ARG, "%s: x_type %d is neither GPZ_X_F64 nor GPZ_X_F32", who, (int)x.type);
    if ((muX != nullptr) != (sdX != nullptr)) return gpz_fail(GPZ_ERR_ARG, "%s: muX and sdX go together (both or neither)", who);
    if (x.ns > 0 && !x.X) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    if (x.rs < 0 || x.cs < 0 || (x.ns > 1 && (x.rs == 0 || (x.cs == 0 && p->d > 1))))
        return gpz_fail(GPZ_ERR_ARG, "%s: strides (%lld, %lld) of %lld rows: a stride must be positive", who, (long long)x.rs,
                        (long long)x.cs, (long long)x.ns);
    return 0;
}

// the caller's Psi: as X, and a column stride of 0 broadcasts an n x 1 Psi
static int predictor_dev_psi_args(const char *who, const DevRows &psi, const double *sdX, const double *sd2) {
    if (psi.type != GPZ_X_F64 && psi.type != GPZ_X_F32)
        return gpz_fail(GPZ_ERR_ARG, "%s: psi_type %d is neither GPZ_X_F64 nor GPZ_X_F32", who, (int)psi.type);
    if ((sdX != nullptr) != (sd2 != nullptr)) return gpz_fail(GPZ_ERR_ARG, "%s: sdX and sd2 go together (both or neither)", who);
    if (psi.ns > 0 && !psi.X) return gpz_fail(GPZ_ERR_ARG, "%s: null Psi", who);
    if (psi.rs < 0 || psi.cs < 0 || (psi.ns > 1 && psi.rs == 0))
        return gpz_fail(GPZ_ERR_ARG, "%s: Psi strides (%lld, %lld) of %lld rows: the row stride must be positive", who, (long long)psi.rs,
                        (long long)psi.cs, (long long)psi.ns);
    return 0;
}

// the caller's cube: only the lower triangle is read, so a 1 x 1 matrix needs no matrix stride
static int predictor_dev_cube_args(const char *who, const gpz_predictor *p, const DevCall &c) {
    const DevRows &psi = c.psi;
    if (psi.type != GPZ_X_F64 && psi.type != GPZ_X_F32)
        return gpz_fail(GPZ_ERR_ARG, "%s: psi_type %d is neither GPZ_X_F64 nor GPZ_X_F32", who, (int)psi.type);
    if ((c.sdX != nullptr) != (c.div != nullptr))
        return gpz_fail(GPZ_ERR_ARG, "%s: sdX and the divisor triangle go together (both or neither)", who);
    if (psi.ns > 0 && !psi.X) return gpz_fail(GPZ_ERR_ARG, "%s: null Psi", who);
    if (c.psi_mr < 0 || psi.cs < 0 || psi.rs < 0 || (psi.ns > 1 && psi.rs == 0) || (p->d > 1 && (c.psi_mr == 0 || psi.cs == 0)))
        return gpz_fail(GPZ_ERR_ARG, "%s: Psi strides (%lld, %lld, %lld) of %lld matrices: a stride must be positive", who,
                        (long long)c.psi_mr, (long long)psi.cs, (long long)psi.rs, (long long)psi.ns);
    return 0;
}

static int predictor_dev_check(const char *who, const gpz_predictor *p, const DevCall &c) {
    if (int rc = predictor_dev_args(who, p, c.x, c.muX, c.sdX)) return rc;
    if (c.rows.cube() || c.rows.cube_obs()) return predictor_dev_cube_args(who, p, c);   // (nothing observed: no Psi is read)
    return c.rows.psi() ? predictor_dev_psi_args(who, c.psi, c.sdX, c.sd2) : 0;
}

// the end of every device entry once it has prepared anything after predictor_dev_begin, failed or not: copies from the caller's memory
// (Z, the edges) may be in flight
static int predictor_dev_sync(gpz_predictor *p, const char *who, int rc) {
    if (hipStreamSynchronize(p->s_cmp) != hipSuccess && !rc) rc = gpz_fail(GPZ_ERR_HIP, "%s: sync failed", who);
    return rc;
}

// What a device call does before its first tile: the parameter buffer (once per handle), muX, sdX and muY up, the compute stream after
// everything queued on the caller's stream, and k_pred_check_dev over all rows with its verdict.  nan_text: the host entry's refusal of
// rows with NaN.  What the kind needs on the handle (rows_prepare with pairs) comes before the scan for rows with Psi - a call that the
// scan refuses leaves it there - and after it for a group with missing inputs: a refused group adds no byte to the handle.  A group with
// Psi too has its Psi scanned in the observed dimensions only (k_pnm_check_psi needs no device copy of sd2, which goes up behind
// rows_prepare).  A refusal leaves the caller's outputs untouched.
static int predictor_dev_begin(gpz_predictor *p, const char *who, DevCall &c, const int *lab, int G, const double *wt, const char *nan_text,
                               bool pairs) {
    const size_t d = p->d, k = p->k;
    const DevRows &x = c.x, *psi = c.rows.psi() ? &c.psi : nullptr;
    const double *muX = c.muX, *sdX = c.sdX, *muY = c.muY, *sd2 = c.sd2;
    const unsigned obs = c.rows.obs, *pattern = c.rows.group() ? &obs : nullptr;
    if (!pattern)   // (the scan below needs sd2_d and the Psi slots)
        if (int rc = rows_prepare(p, who, c.rows, pairs)) return rc;
    hipStream_t st = p->s_cmp;
    if (!p->par_d)
        if (int rc = p->ar.alloc(&p->par_d, 2 * d + k + 2)) return rc;
    if (c.rows.cube_obs() && !p->div_d)   // (the scan of such a group divides on the device: the one table it takes before its verdict)
        if (int rc = p->ar.alloc(&p->div_d, d * (d + 1) / 2)) return rc;
    if (!p->ev_dev) HIPCHK(hipEventCreateWithFlags(&p->ev_dev, hipEventDisableTiming));
    p->dev_used = true;
    unsigned *rec = (unsigned *)(p->par_d + 2 * d + k);
    unsigned verdict[4] = {0, 0, 0, 0};
    int rc = 0;
    // from here on every failure leaves through the synchronisation below: copies from the caller's memory may be in flight
    if (hipEventRecord(p->ev_dev, (hipStream_t)c.stream) != hipSuccess || hipStreamWaitEvent(st, p->ev_dev, 0) != hipSuccess)
        rc = gpz_fail(GPZ_ERR_HIP, "%s: cannot order the call after the caller's stream", who);
    if (!rc &&
        ((muX && (hipMemcpyAsync(p->par_d, muX, d * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
                  hipMemcpyAsync(p->par_d + d, sdX, d * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)) ||
         (muY && hipMemcpyAsync(p->par_d + 2 * d, muY, k * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) ||
         hipMemsetAsync(rec, 0, 4 * sizeof(unsigned), st) != hipSuccess))
        rc = gpz_fail(GPZ_ERR_HIP, "%s: copy failed", who);
    // pattern (the entries for one group of rows with missing inputs): word 0 says that a row does not have exactly that NaN pattern
    if (!rc && (pattern ? launch_pmd_check(st, x.X, x.f32(), x.ns, p->d, x.rs, x.cs, *pattern, rec)
                        : launch_pred_check_dev(st, x.X, x.f32(), x.ns, p->d, x.rs, x.cs, lab, G, wt, rec)))
        rc = gpz_fail(GPZ_ERR_HIP, "%s: k_pred_check_dev launch failed", who);
    // the labels and weights of a stack of such a group: k_pred_check_dev over no columns (words 1 and 2 only, X is not read)
    if (!rc && pattern && (lab || wt) && launch_pred_check_dev(st, nullptr, 0, x.ns, 0, 0, 0, lab, G, wt, rec))
        rc = gpz_fail(GPZ_ERR_HIP, "%s: k_pred_check_dev launch failed", who);
    if (!rc && psi && pattern &&
        launch_pnm_check_psi(st, psi->X, psi->f32(), psi->ns, p->d, psi->rs, psi->cs, obs, sd2 ? *std::min_element(sd2, sd2 + d) : 1.0, rec))
        rc = gpz_fail(GPZ_ERR_HIP, "%s: k_pred_check_psi launch failed", who);
    if (!rc && psi && !pattern &&
        ((sd2 && hipMemcpyAsync(p->sd2_d, sd2, d * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) ||
         launch_pred_check_psi(st, psi->X, psi->f32(), psi->ns, p->d, psi->rs, psi->cs, sd2 ? *std::min_element(sd2, sd2 + d) : 1.0, rec)))
        rc = gpz_fail(GPZ_ERR_HIP, "%s: k_pred_check_psi launch failed", who);
    // a full Psi per row: the divisor triangle up (from the host or the device), then the scan of every lower triangle
    if (!rc && c.rows.cube() &&
        ((c.div && hipMemcpyAsync(p->div_d, c.div, d * (d + 1) / 2 * sizeof(double), hipMemcpyDefault, st) != hipSuccess) ||
         launch_pred_check_psi_cube(st, c.psi.X, c.psi.f32(), c.psi.ns, p->d, c.psi_mr, c.psi.cs, c.psi.rs, c.div ? p->div_d : nullptr, rec)))
        rc = gpz_fail(GPZ_ERR_HIP, "%s: k_pred_check_psi_cube launch failed", who);
    // such a group with a full Psi per row: the same, over the lower triangle of the observed x observed block only
    if (!rc && c.rows.cube_obs() &&
        ((c.div && hipMemcpyAsync(p->div_d, c.div, d * (d + 1) / 2 * sizeof(double), hipMemcpyDefault, st) != hipSuccess) ||
         launch_pcm_check_psi(st, c.psi.X, c.psi.f32(), c.psi.ns, p->d, obs, c.psi_mr, c.psi.cs, c.psi.rs, c.div ? p->div_d : nullptr, rec)))
        rc = gpz_fail(GPZ_ERR_HIP, "%s: k_pcm_check_psi launch failed", who);
    if (!rc && hipMemcpyAsync(verdict, rec, sizeof verdict, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = gpz_fail(GPZ_ERR_HIP, "%s: copy failed", who);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = gpz_fail(GPZ_ERR_HIP, "%s: sync failed", who);
    if (rc) return rc;
    if (verdict[1]) return gpz_fail(GPZ_ERR_ARG, "%s: a label is outside [-1, %d)", who, G);
    if (verdict[2]) return gpz_fail(GPZ_ERR_ARG, "%s: a weight is negative or not finite", who);
    if (verdict[0] && pattern)
        return gpz_fail(GPZ_ERR_ARG, "%s: the rows of a group must share one NaN pattern, the one of the mask", who);
    if (verdict[0]) return gpz_fail(GPZ_ERR_UNSUPPORTED, "%s: %s", who, nan_text);
    if (verdict[3] && c.rows.cube())
        return gpz_fail(GPZ_ERR_ARG, "%s: the lower triangle of Psi has an element that is NaN or infinite, or a negative diagonal element",
                        who);
    if (verdict[3] && c.rows.cube_obs())
        return gpz_fail(GPZ_ERR_ARG,
                        "%s: the lower triangle of Psi over the observed dimensions has an element that is NaN or infinite, or a negative "
                        "diagonal element",
                        who);
    if (verdict[3]) return gpz_fail(GPZ_ERR_ARG, "%s: Psi has an element that is NaN, infinite or negative", who);
    c.muX_d = muX ? p->par_d : nullptr;
    c.sdX_d = muX ? p->par_d + d : nullptr;
    c.muY_d = muY ? p->par_d + 2 * d : nullptr;
    if (pattern) {
        if (int rc = rows_prepare(p, who, c.rows, pairs)) return predictor_dev_sync(p, who, rc);
        if (psi && sd2 && hipMemcpyAsync(p->sd2_d, sd2, d * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
            return predictor_dev_sync(p, who, gpz_fail(GPZ_ERR_HIP, "%s: copy failed", who));
    }
    c.sd2_d = sd2 ? p->sd2_d : nullptr;   // (a group's first call with Psi has it from rows_prepare only)
    c.div_d = c.div ? p->div_d : nullptr;
    return 0;
}

// The tiles of a device entry, all on the compute stream: k_pred_stage (and, with Psi, k_pred_stage_psi into Psic[s]) from the caller's
// memory into slot s, then body(s, r0, nt), the entry's kernels down to the one that writes into the caller's arrays.
template <class Body>
static int predictor_dev_tiles(gpz_predictor *p, const char *who, const DevCall &c, int64_t T, Body body) {
    hipStream_t st = p->s_cmp;
    const DevRows &x = c.x, &psi = c.psi;
    for (int64_t r0 = 0, t = 0; r0 < x.ns; r0 += T, ++t) {
        const int s = (int)(t & 1), nt = (int)std::min<int64_t>(T, x.ns - r0);
        if (launch_pred_stage(st, x.X, x.f32(), x.rs, x.cs, r0, nt, p->d, c.muX_d, c.sdX_d, p->Xc[s], p->tile_pad))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_pred_stage launch failed", who);
        if (c.rows.psi() &&
            launch_pred_stage_psi(st, psi.X, psi.f32(), psi.rs, psi.cs, r0, nt, p->d, c.sd2_d, p->Psic[s], p->tile_pad))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_pred_stage_psi launch failed", who);
        if (c.rows.cube() && launch_pred_stage_psi_cube(st, psi.X, psi.f32(), c.psi_mr, psi.cs, psi.rs, r0, nt, p->d, c.div_d, p->Psiq[s],
                                                        p->tile_pad))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_pred_stage_psi_cube launch failed", who);
        if (c.rows.cube_obs() && launch_pcm_stage_psi(st, psi.X, psi.f32(), c.psi_mr, psi.cs, psi.rs, r0, nt, p->d, c.rows.obs, c.div_d,
                                                      p->Psiq[s], p->tile_pad))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_pcm_stage_psi launch failed", who);
        if (int rc = body(s, r0, nt)) return rc;
    }
    return 0;
}

// ---- one runner and one check ladder per question, for every kind of rows -------------------------------------------------------------
// the moments of every tile, each with its finish kernel into the caller's arrays
static int predictor_run_dev(gpz_predictor *p, const char *who, DevCall &c, double *mu, double *sigma, double *nu, double *beta,
                             double *gamma, double *PHI) {
    hipStream_t st = p->s_cmp;
    const Rows &r = c.rows;
    const int64_t ns = c.x.ns;
    int rc = PHI ? predictor_want_phi(p, false) : 0;
    if (!rc)
        rc = predictor_dev_begin(p, who, c, nullptr, 0, nullptr,
                                 r.psi() || r.cube()
                                     ? "the rows have missing values (NaN): input noise on the handle is for complete rows"
                                     : "the rows have missing values (NaN): group them by pattern and call gpz_predict_missing (predict.m:45-69)",
                                 true);
    if (rc) return rc;
    rc = predictor_dev_tiles(p, who, c, rows_tile(p, r, p->tile_rows), [&](int s, int64_t r0, int nt) {
        if (int rc = rows_moments_tile(p, who, r, s, nt, PHI != nullptr)) return rc;
        if (r.kind == ROWS_CLEAN
                ? launch_pred_finish_dev(st, p->out[s], nt, p->k, c.muY_d, ns, r0, mu, sigma, nu, beta, gamma) ||
                      (PHI && launch_pred_phi_dev(st, p->phi_d[s], nt, p->m, ns, r0, PHI))
                : launch_pred_finish_noisy_dev(st, rows_moments(p, r, s), nt, p->k, c.muY_d, ns, r0, mu, sigma, nu, beta, gamma))
            return gpz_fail(GPZ_ERR_HIP, "%s: finish kernel launch failed", who);
        return 0;
    });
    rc = predictor_dev_sync(p, who, rc);
    if (!rc) ++p->runs;
    return rc;
}

// gpz_predictor_run_dev, _run_noisy_dev, _run_noisy_cov_dev, _run_psi_cube_dev, _run_missing_dev, _run_missing_cov_dev, _run_noisy_missing_dev and
// _run_noisy_missing_cov_dev
static int run_dev_entry(const char *who, gpz_predictor *p, DevCall c, double *mu_d, double *sigma_d, double *nu_d, double *beta_d,
                         double *gamma_d, double *PHI_d) {
    if (int rc = predictor_check_call(who, p, c.x.ns)) return rc;
    if (int rc = rows_check(who, p, c.rows, false)) return rc;
    if (int rc = predictor_dev_check(who, p, c)) return rc;
    if (c.x.ns == 0) return 0;
    if (!mu_d || !nu_d || !beta_d) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    return predictor_call(p, who, [&] { return predictor_run_dev(p, who, c, mu_d, sigma_d, nu_d, beta_d, gamma_d, PHI_d); });
}

// The draws of every tile, F = PHI W + muY (for a group PHI_missing: mu is linear in w).  Gam (rows with Psi or a group; nullptr: none):
// gamma under every draw too, gamma_s = the pair sum under draw s - mu_s^2 with mu_s as dout[s] holds it (without muY)
static int predictor_run_draws_dev(gpz_predictor *p, const char *who, DevCall &c, int nd, unsigned long long seed, const double *Z,
                                   double *F, double *Gam) {
    hipStream_t st = p->s_cmp;
    const Rows &r = c.rows;
    const int ncol = nd * p->k, ldw = rup(ncol, 16);
    int64_t T = 0;
    int rc = predictor_dev_begin(p, who, c, nullptr, 0, nullptr, "the rows have missing values (NaN): draws are for complete rows",
                                 Gam != nullptr);   // gamma reads the pair tables
    if (rc) return rc;
    rc = rows_draws_prepare(p, r, nd, seed, Z, false, &T);
    if (!rc && Gam) rc = rows_gamma_prepare(p, r, ncol, 0, T);
    if (!rc)
        rc = predictor_dev_tiles(p, who, c, T, [&](int s, int64_t r0, int nt) {
            if (int rc = rows_draws_tile(p, who, r, s, nt, ncol, ldw, false)) return rc;
            if (Gam) {
                if (int rc = rows_gamma_tile(p, who, r, s, nt, ncol, ldw)) return rc;
                if (launch_gamma_finish_dev(st, p->gpart, rows_chunks(p, r), nt, p->dout[s], nt, p->k, nd, c.x.ns, r0, Gam))
                    return gpz_fail(GPZ_ERR_HIP, "%s: k_gamma_finish_dev launch failed", who);
            }
            if (launch_draws_finish_dev(st, p->dout[s], nt, p->k, nd, c.muY_d, c.x.ns, r0, F))
                return gpz_fail(GPZ_ERR_HIP, "%s: k_draws_finish_dev launch failed", who);
            return 0;
        });
    return predictor_dev_sync(p, who, rc);
}

// gpz_predictor_draws_dev, _draws_noisy_dev, _draws_noisy_cov_dev, _draws_missing_dev, _draws_missing_cov_dev, _draws_noisy_missing_dev and, with want_gamma, _draws_gamma_noisy_dev, _draws_gamma_noisy_cov_dev, _draws_gamma_missing_dev, _draws_gamma_missing_cov_dev, _draws_gamma_noisy_missing_dev and _draws_gamma_noisy_missing_cov_dev
static int draws_dev_entry(const char *who, gpz_predictor *p, DevCall c, int32_t ndraws, uint64_t seed, const double *Z, double *F_d,
                           double *Gam_d = nullptr, bool want_gamma = false) {
    if (int rc = predictor_check_call(who, p, c.x.ns)) return rc;
    if (int rc = predictor_check_ndraws(who, p, ndraws, 1)) return rc;
    if (int rc = rows_check(who, p, c.rows, true)) return rc;
    if (int rc = predictor_dev_check(who, p, c)) return rc;
    if (c.x.ns == 0) return 0;
    if (!F_d || (want_gamma && !Gam_d)) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    return predictor_call(p, who, [&] {
        return predictor_run_draws_dev(p, who, c, (int)ndraws, (unsigned long long)seed, Z, F_d, want_gamma ? Gam_d : nullptr);
    });
}

// The stack with the rows, labels and weights (and Psi) where the caller has them: the tile kernels read lab + r0 and wt + r0 directly.
// The scan stands for the host entry's loops over labels and weights and for its staging loop over the rows, before any tile.
static int predictor_run_stack_dev(gpz_predictor *p, const char *who, DevCall &c, const StackArgs &a, double *res) {
    StackCall sc{};
    int rc = predictor_dev_begin(p, who, c, a.group, a.ngroups, a.weight, "the rows have missing values (NaN): stacks are for complete rows",
                                 true);
    if (rc) return rc;
    rc = predictor_stack_prepare(p, who, c.rows, a, false, &sc);
    if (!rc)
        rc = predictor_dev_tiles(p, who, c, sc.T, [&](int s, int64_t r0, int nt) {
            return predictor_stack_tile(p, who, c.rows, sc, s, nt, a.group ? a.group + r0 : nullptr, a.weight ? a.weight + r0 : nullptr);
        });
    if (!rc) rc = predictor_stack_result(p, who, sc, res);
    return predictor_dev_sync(p, who, rc);
}

// gpz_predictor_stack_dev, _stack_noisy_dev, _stack_noisy_cov_dev, _stack_missing_dev, _stack_missing_cov_dev, _stack_noisy_missing_dev and _stack_noisy_missing_cov_dev
static int stack_dev_entry(const char *who, gpz_predictor *p, DevCall c, const StackArgs &a) {
    return stack_entry(
        who, p, c.x.ns, c.x.X, a, false,
        [&] {
            if (int rc = rows_check(who, p, c.rows, true)) return rc;
            return predictor_dev_check(who, p, c);
        },
        [] { return 0; }, [&](double *res) { return predictor_run_stack_dev(p, who, c, a, res); });
}
}   // namespace gpzi

extern "C" int gpz_predictor_run_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                     const double *muX, const double *sdX, const double *muY, double *mu_d, double *sigma_d, double *nu_d,
                                     double *beta_d, double *gamma_d, double *PHI_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return run_dev_entry("gpz_predictor_run_dev", p, x, mu_d, sigma_d, nu_d, beta_d, gamma_d, PHI_d);
}

extern "C" int gpz_predictor_run_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                           int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                           int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                           const double *muY, double *mu_d, double *sigma_d, double *nu_d, double *beta_d,
                                           double *gamma_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return run_dev_entry("gpz_predictor_run_noisy_dev", p, with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), mu_d,
                         sigma_d, nu_d, beta_d, gamma_d, nullptr);
}

extern "C" int gpz_predictor_draws_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                       int64_t col_stride, const double *muX, const double *sdX, const double *muY, int32_t ndraws,
                                       uint64_t seed, const double *Z, double *F_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_dev", p, x, ndraws, seed, Z, F_d);
}

extern "C" int gpz_predictor_draws_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                             int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                             int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                             const double *muY, int32_t ndraws, uint64_t seed, const double *Z, double *F_d,
                                             void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_noisy_dev", p, with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), ndraws,
                           seed, Z, F_d);
}

extern "C" int gpz_predictor_run_noisy_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                               int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                               int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                               const double *muY, double *mu_d, double *sigma_d, double *nu_d, double *beta_d,
                                               double *gamma_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return run_dev_entry("gpz_predictor_run_noisy_cov_dev", p,
                         with_cov(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2)), mu_d, sigma_d, nu_d, beta_d, gamma_d,
                         nullptr);
}

extern "C" int gpz_predictor_draws_noisy_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                 int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                 int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                 const double *muY, int32_t ndraws, uint64_t seed, const double *Z, double *F_d,
                                                 void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_noisy_cov_dev", p,
                           with_cov(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2)), ndraws, seed, Z, F_d);
}

extern "C" int gpz_predictor_draws_gamma_noisy_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                       int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                       int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                       const double *muY, int32_t ndraws, uint64_t seed, const double *Z, double *F_d,
                                                       double *Gam_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_gamma_noisy_cov_dev", p,
                           with_cov(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2)), ndraws, seed, Z, F_d, Gam_d, true);
}

extern "C" int gpz_predictor_stack_noisy_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                 int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                 int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                 int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                                 const int32_t *group_d, int32_t ngroups, const double *weight_d, double *hist,
                                                 double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, nullptr, stream);
    const StackArgs a{ndraws, seed, Z, edges, nbins, group_d, ngroups, weight_d, hist, sum_w, sum_mu, sum_mu2, mu_shift};
    return stack_dev_entry("gpz_predictor_stack_noisy_cov_dev", p,
                           with_cov(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2)), a);
}

extern "C" int gpz_predictor_run_psi_cube_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                              int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                              int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX, const double *sdX,
                                              const double *div, const double *muY, double *mu_d, double *sigma_d, double *nu_d,
                                              double *beta_d, double *gamma_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return run_dev_entry("gpz_predictor_run_psi_cube_dev", p,
                         with_cube(x, Psi_d, psi_type, psi_mrow_stride, psi_mcol_stride, psi_row_stride, div), mu_d, sigma_d, nu_d, beta_d,
                         gamma_d, nullptr);
}

extern "C" int gpz_predictor_draws_psi_cube_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                                int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX, const double *sdX,
                                                const double *div, const double *muY, int32_t ndraws, uint64_t seed, const double *Z,
                                                double *F_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_psi_cube_dev", p,
                           with_cube(x, Psi_d, psi_type, psi_mrow_stride, psi_mcol_stride, psi_row_stride, div), ndraws, seed, Z, F_d);
}

extern "C" int gpz_predictor_draws_gamma_psi_cube_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                      int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                                      int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX,
                                                      const double *sdX, const double *div, const double *muY, int32_t ndraws,
                                                      uint64_t seed, const double *Z, double *F_d, double *Gam_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_gamma_psi_cube_dev", p,
                           with_cube(x, Psi_d, psi_type, psi_mrow_stride, psi_mcol_stride, psi_row_stride, div), ndraws, seed, Z, F_d,
                           Gam_d, true);
}

extern "C" int gpz_predictor_stack_psi_cube_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                                int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX, const double *sdX,
                                                const double *div, int32_t ndraws, uint64_t seed, const double *Z, const double *edges,
                                                int32_t nbins, const int32_t *group_d, int32_t ngroups, const double *weight_d,
                                                double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift,
                                                void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, nullptr, stream);
    const StackArgs a{ndraws, seed, Z, edges, nbins, group_d, ngroups, weight_d, hist, sum_w, sum_mu, sum_mu2, mu_shift};
    return stack_dev_entry("gpz_predictor_stack_psi_cube_dev", p,
                           with_cube(x, Psi_d, psi_type, psi_mrow_stride, psi_mcol_stride, psi_row_stride, div), a);
}

extern "C" int gpz_predictor_run_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                             int64_t col_stride, const double *muX, const double *sdX, const double *muY,
                                             const double *priors, uint32_t obs_mask, double *mu_d, double *sigma_d, double *nu_d,
                                             double *beta_d, double *gamma_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return run_dev_entry("gpz_predictor_run_missing_dev", p, with_pattern(x, priors, obs_mask), mu_d, sigma_d, nu_d, beta_d, gamma_d,
                         nullptr);
}

extern "C" int gpz_predictor_draws_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                               int64_t col_stride, const double *muX, const double *sdX, const double *muY,
                                               const double *priors, uint32_t obs_mask, int32_t ndraws, uint64_t seed, const double *Z,
                                               double *F_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_missing_dev", p, with_pattern(x, priors, obs_mask), ndraws, seed, Z, F_d);
}

extern "C" int gpz_predictor_run_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                 int64_t col_stride, const double *muX, const double *sdX, const double *muY,
                                                 const double *priors, uint32_t obs_mask, double *mu_d, double *sigma_d, double *nu_d,
                                                 double *beta_d, double *gamma_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return run_dev_entry("gpz_predictor_run_missing_cov_dev", p, with_cov_pattern(x, priors, obs_mask), mu_d, sigma_d, nu_d, beta_d,
                         gamma_d, nullptr);
}

extern "C" int gpz_predictor_draws_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                   int64_t col_stride, const double *muX, const double *sdX, const double *muY,
                                                   const double *priors, uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                   const double *Z, double *F_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_missing_cov_dev", p, with_cov_pattern(x, priors, obs_mask), ndraws, seed, Z, F_d);
}

extern "C" int gpz_predictor_draws_gamma_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                         int64_t col_stride, const double *muX, const double *sdX, const double *muY,
                                                         const double *priors, uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                         const double *Z, double *F_d, double *Gam_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_gamma_missing_cov_dev", p, with_cov_pattern(x, priors, obs_mask), ndraws, seed, Z, F_d,
                           Gam_d, true);
}

extern "C" int gpz_predictor_stack_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                   int64_t col_stride, const double *muX, const double *sdX, const double *priors,
                                                   uint32_t obs_mask, int32_t ndraws, uint64_t seed, const double *Z, const double *edges,
                                                   int32_t nbins, const int32_t *group_d, int32_t ngroups, const double *weight_d,
                                                   double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift,
                                                   void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, nullptr, stream);
    const StackArgs a{ndraws, seed, Z, edges, nbins, group_d, ngroups, weight_d, hist, sum_w, sum_mu, sum_mu2, mu_shift};
    return stack_dev_entry("gpz_predictor_stack_missing_cov_dev", p, with_cov_pattern(x, priors, obs_mask), a);
}

extern "C" int gpz_predictor_run_noisy_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                   int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                   int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                   const double *muY, const double *priors, uint32_t obs_mask, double *mu_d,
                                                   double *sigma_d, double *nu_d, double *beta_d, double *gamma_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return run_dev_entry("gpz_predictor_run_noisy_missing_dev", p,
                         with_noisy_pattern(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), priors, obs_mask), mu_d,
                         sigma_d, nu_d, beta_d, gamma_d, nullptr);
}

extern "C" int gpz_predictor_draws_noisy_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                     int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                     int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                     const double *muY, const double *priors, uint32_t obs_mask, int32_t ndraws,
                                                     uint64_t seed, const double *Z, double *F_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_noisy_missing_dev", p,
                           with_noisy_pattern(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), priors, obs_mask), ndraws,
                           seed, Z, F_d);
}

extern "C" int gpz_predictor_run_noisy_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                       int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                       int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                       const double *muY, const double *priors, uint32_t obs_mask, double *mu_d,
                                                       double *sigma_d, double *nu_d, double *beta_d, double *gamma_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return run_dev_entry("gpz_predictor_run_noisy_missing_cov_dev", p,
                         with_noisy_cov_pattern(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), priors, obs_mask), mu_d,
                         sigma_d, nu_d, beta_d, gamma_d, nullptr);
}

extern "C" int gpz_predictor_draws_noisy_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                         int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                         int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                         const double *muY, const double *priors, uint32_t obs_mask, int32_t ndraws,
                                                         uint64_t seed, const double *Z, double *F_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_noisy_missing_cov_dev", p,
                           with_noisy_cov_pattern(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), priors, obs_mask),
                           ndraws, seed, Z, F_d);
}

extern "C" int gpz_predictor_stack_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                       int64_t col_stride, const double *muX, const double *sdX, int32_t ndraws, uint64_t seed,
                                       const double *Z, const double *edges, int32_t nbins, const int32_t *group_d, int32_t ngroups,
                                       const double *weight_d, double *hist, double *sum_w, double *sum_mu, double *sum_mu2,
                                       const double *mu_shift, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, nullptr, stream);
    const StackArgs a{ndraws, seed, Z, edges, nbins, group_d, ngroups, weight_d, hist, sum_w, sum_mu, sum_mu2, mu_shift};
    return stack_dev_entry("gpz_predictor_stack_dev", p, x, a);
}

extern "C" int gpz_predictor_draws_gamma_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                   int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                   int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                   const double *muY, int32_t ndraws, uint64_t seed, const double *Z, double *F_d,
                                                   double *Gam_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_gamma_noisy_dev", p, with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2),
                           ndraws, seed, Z, F_d, Gam_d, true);
}

extern "C" int gpz_predictor_stack_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                             int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                             int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                             int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                             const int32_t *group_d, int32_t ngroups, const double *weight_d, double *hist, double *sum_w,
                                             double *sum_mu, double *sum_mu2, const double *mu_shift, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, nullptr, stream);
    const StackArgs a{ndraws, seed, Z, edges, nbins, group_d, ngroups, weight_d, hist, sum_w, sum_mu, sum_mu2, mu_shift};
    return stack_dev_entry("gpz_predictor_stack_noisy_dev", p, with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), a);
}

extern "C" int gpz_predictor_draws_gamma_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                     int64_t col_stride, const double *muX, const double *sdX, const double *muY,
                                                     const double *priors, uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                     const double *Z, double *F_d, double *Gam_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_gamma_missing_dev", p, with_pattern(x, priors, obs_mask), ndraws, seed, Z, F_d, Gam_d,
                           true);
}

extern "C" int gpz_predictor_stack_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                               int64_t col_stride, const double *muX, const double *sdX, const double *priors,
                                               uint32_t obs_mask, int32_t ndraws, uint64_t seed, const double *Z, const double *edges,
                                               int32_t nbins, const int32_t *group_d, int32_t ngroups, const double *weight_d,
                                               double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift,
                                               void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, nullptr, stream);
    const StackArgs a{ndraws, seed, Z, edges, nbins, group_d, ngroups, weight_d, hist, sum_w, sum_mu, sum_mu2, mu_shift};
    return stack_dev_entry("gpz_predictor_stack_missing_dev", p, with_pattern(x, priors, obs_mask), a);
}

extern "C" int gpz_predictor_draws_gamma_noisy_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                           int64_t col_stride, const void *Psi_d, int32_t psi_type,
                                                           int64_t psi_row_stride, int64_t psi_col_stride, const double *muX,
                                                           const double *sdX, const double *sd2, const double *muY, const double *priors,
                                                           uint32_t obs_mask, int32_t ndraws, uint64_t seed, const double *Z, double *F_d,
                                                           double *Gam_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_gamma_noisy_missing_dev", p,
                           with_noisy_pattern(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), priors, obs_mask), ndraws,
                           seed, Z, F_d, Gam_d, true);
}

extern "C" int gpz_predictor_stack_noisy_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                     int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                     int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                     const double *priors, uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                     const double *Z, const double *edges, int32_t nbins, const int32_t *group_d,
                                                     int32_t ngroups, const double *weight_d, double *hist, double *sum_w, double *sum_mu,
                                                     double *sum_mu2, const double *mu_shift, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, nullptr, stream);
    const StackArgs a{ndraws, seed, Z, edges, nbins, group_d, ngroups, weight_d, hist, sum_w, sum_mu, sum_mu2, mu_shift};
    return stack_dev_entry("gpz_predictor_stack_noisy_missing_dev", p,
                           with_noisy_pattern(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), priors, obs_mask), a);
}

extern "C" int gpz_predictor_draws_gamma_noisy_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns,
                                                               int64_t row_stride, int64_t col_stride, const void *Psi_d, int32_t psi_type,
                                                               int64_t psi_row_stride, int64_t psi_col_stride, const double *muX,
                                                               const double *sdX, const double *sd2, const double *muY,
                                                               const double *priors, uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                               const double *Z, double *F_d, double *Gam_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_gamma_noisy_missing_cov_dev", p,
                           with_noisy_cov_pattern(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), priors, obs_mask),
                           ndraws, seed, Z, F_d, Gam_d, true);
}

extern "C" int gpz_predictor_stack_noisy_missing_cov_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                         int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                         int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                         const double *priors, uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                         const double *Z, const double *edges, int32_t nbins, const int32_t *group_d,
                                                         int32_t ngroups, const double *weight_d, double *hist, double *sum_w,
                                                         double *sum_mu, double *sum_mu2, const double *mu_shift, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, nullptr, stream);
    const StackArgs a{ndraws, seed, Z, edges, nbins, group_d, ngroups, weight_d, hist, sum_w, sum_mu, sum_mu2, mu_shift};
    return stack_dev_entry("gpz_predictor_stack_noisy_missing_cov_dev", p,
                           with_noisy_cov_pattern(with_psi(x, Psi_d, psi_type, psi_row_stride, psi_col_stride, sd2), priors, obs_mask), a);
}

extern "C" int gpz_predictor_run_psi_cube_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                      int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                                      int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX,
                                                      const double *sdX, const double *div, const double *muY, const double *priors,
                                                      uint32_t obs_mask, double *mu_d, double *sigma_d, double *nu_d, double *beta_d,
                                                      double *gamma_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return run_dev_entry("gpz_predictor_run_psi_cube_missing_dev", p,
                         with_cube_pattern(with_cube(x, Psi_d, psi_type, psi_mrow_stride, psi_mcol_stride, psi_row_stride, div), priors,
                                           obs_mask),
                         mu_d, sigma_d, nu_d, beta_d, gamma_d, nullptr);
}

extern "C" int gpz_predictor_draws_psi_cube_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                        int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                                        int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX,
                                                        const double *sdX, const double *div, const double *muY, const double *priors,
                                                        uint32_t obs_mask, int32_t ndraws, uint64_t seed, const double *Z, double *F_d,
                                                        void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_psi_cube_missing_dev", p,
                           with_cube_pattern(with_cube(x, Psi_d, psi_type, psi_mrow_stride, psi_mcol_stride, psi_row_stride, div), priors,
                                             obs_mask),
                           ndraws, seed, Z, F_d);
}

extern "C" int gpz_predictor_draws_gamma_psi_cube_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns,
                                                              int64_t row_stride, int64_t col_stride, const void *Psi_d, int32_t psi_type,
                                                              int64_t psi_mrow_stride, int64_t psi_mcol_stride, int64_t psi_row_stride,
                                                              const double *muX, const double *sdX, const double *div, const double *muY,
                                                              const double *priors, uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                              const double *Z, double *F_d, double *Gam_d, void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, muY, stream);
    return draws_dev_entry("gpz_predictor_draws_gamma_psi_cube_missing_dev", p,
                           with_cube_pattern(with_cube(x, Psi_d, psi_type, psi_mrow_stride, psi_mcol_stride, psi_row_stride, div), priors,
                                             obs_mask),
                           ndraws, seed, Z, F_d, Gam_d, true);
}

extern "C" int gpz_predictor_stack_psi_cube_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                        int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_mrow_stride,
                                                        int64_t psi_mcol_stride, int64_t psi_row_stride, const double *muX,
                                                        const double *sdX, const double *div, const double *priors, uint32_t obs_mask,
                                                        int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                                        const int32_t *group_d, int32_t ngroups, const double *weight_d, double *hist,
                                                        double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift,
                                                        void *stream) {
    const DevCall x = dev_call(X_d, x_type, ns, row_stride, col_stride, muX, sdX, nullptr, stream);
    const StackArgs a{ndraws, seed, Z, edges, nbins, group_d, ngroups, weight_d, hist, sum_w, sum_mu, sum_mu2, mu_shift};
    return stack_dev_entry("gpz_predictor_stack_psi_cube_missing_dev", p,
                           with_cube_pattern(with_cube(x, Psi_d, psi_type, psi_mrow_stride, psi_mcol_stride, psi_row_stride, div), priors,
                                             obs_mask),
                           a);
}
