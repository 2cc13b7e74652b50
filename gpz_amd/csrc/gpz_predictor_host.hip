// The streaming predictor's host entries (gpz_predictor_run, _draws, _draws_noisy, _stack, _stack_noisy): the rows come from host arrays
// through pinned slots and the results go home the same way.  The handle, the tile functions of every kind of rows and the file's place
// among the predictor's units: gpz_predictor.h and the comment at the top of gpz_predictor.hip.
#include "gpz_predictor.h"

namespace gpzi {
// ---- the host pipeline --------------------------------------------------------------------------------------------------------------
// columns [r0, r0 + nt) of the column-major ns x d array A into a pinned slot ([d][tp], the layout of Xc); true if hit(v) held for an element
template <class Hit>
static bool predictor_stage(const double *A, int64_t ns, int d, int64_t r0, int64_t nt, double *slot, size_t tp, Hit hit) {
    bool bad = false;
    for (int c = 0; c < d; ++c) {
        const double *src = A + (size_t)c * ns + r0;
        double *dst = slot + (size_t)c * tp;
        int any = 0;
        for (int64_t i = 0; i < nt; ++i) { const double v = src[i]; dst[i] = v; any |= hit(v); }
        bad |= any != 0;
    }
    return bad;
}

// The tiles of a host entry: three streams - copies in, compute, copies out - and the two slots.  The driver owns the loop and every event
// and stream call; a job says what one tile in slot s (nt rows from row r0, T rows per tile) is made of:
//   who, nan_text     the entry's name in the messages, and its refusal of rows with missing values
//   downloads         false: nothing comes home per tile (the stack), so there is no work on s_out and no tile to wait for at the end
//   stage(s, r0, nt)  what goes into the pinned slots beside the rows: 0, or the refusal
//   upload(s, nt)     the copies that ride s_in behind the rows; true: one failed (so too download)
//   kernels(s, nt)    the tile's kernels on s_cmp: 0, or the failure
//   download(s, nt)   the copies home on s_out;  scatter(s, r0, nt): the pinned results into the caller's arrays, two tiles later
// Failures return at once: the caller drains the streams (predictor_drain) whatever the result.
template <class Job>
static int predictor_pipeline(gpz_predictor *p, const double *Xs, int64_t ns, int64_t T, Job &job) {
    const size_t tp = (size_t)p->tile_pad;
    const int64_t ntiles = (ns + T - 1) / T;
    int64_t nt_of[2] = {0, 0}, r0_of[2] = {0, 0};
    for (int64_t t = 0; t < ntiles + (Job::downloads ? 2 : 0); ++t) {
        const int s = (int)(t & 1);
        if (t >= 2) {   // slot s is free for tile t: tile t - 2 is home (into the caller's arrays) or, with no download, its upload has left the pinned slot
            if (hipEventSynchronize(Job::downloads ? p->ev_out[s] : p->ev_in[s]) != hipSuccess)
                return gpz_fail(GPZ_ERR_HIP, "%s: tile failed", job.who);
            if constexpr (Job::downloads) job.scatter(s, r0_of[s], nt_of[s]);
        }
        if (t >= ntiles) continue;
        const int64_t r0 = t * T, nt = std::min<int64_t>(T, ns - r0);
        nt_of[s] = nt; r0_of[s] = r0;
        // stage the tile's rows and look for missing values on the way
        if (predictor_stage(Xs, ns, p->d, r0, nt, p->hin[s], tp, [](double v) { return v != v; }))
            return gpz_fail(GPZ_ERR_UNSUPPORTED, "%s: %s", job.who, job.nan_text);
        if (int rc = job.stage(s, r0, nt)) return rc;
        // copies in (after tile t - 2's kernels are done with the slot); kernels (after the copies, and after tile t - 2's download of the
        // slot's outputs); copies out
        if (hipStreamWaitEvent(p->s_in, p->ev_cmp[s], 0) != hipSuccess ||
            hipMemcpy2DAsync(p->Xc[s], tp * sizeof(double), p->hin[s], tp * sizeof(double), (size_t)nt * sizeof(double), p->d,
                             hipMemcpyHostToDevice, p->s_in) != hipSuccess ||
            job.upload(s, nt) || hipEventRecord(p->ev_in[s], p->s_in) != hipSuccess ||
            hipStreamWaitEvent(p->s_cmp, p->ev_in[s], 0) != hipSuccess ||
            (Job::downloads && hipStreamWaitEvent(p->s_cmp, p->ev_out[s], 0) != hipSuccess))
            return gpz_fail(GPZ_ERR_HIP, "%s: copy failed", job.who);
        if (int rc = job.kernels(s, nt)) return rc;
        if (hipEventRecord(p->ev_cmp[s], p->s_cmp) != hipSuccess)
            return gpz_fail(GPZ_ERR_HIP, "%s: %s failed", job.who, Job::downloads ? "copy" : "event");
        if constexpr (Job::downloads)
            if (hipStreamWaitEvent(p->s_out, p->ev_cmp[s], 0) != hipSuccess || job.download(s, nt) ||
                hipEventRecord(p->ev_out[s], p->s_out) != hipSuccess)
                return gpz_fail(GPZ_ERR_HIP, "%s: copy failed", job.who);
    }
    return 0;
}

// the end of every host entry, failed or not: nothing of the call is in flight when it returns
static int predictor_drain(gpz_predictor *p, const char *who, int rc) {
    for (hipStream_t st : {p->s_in, p->s_cmp, p->s_out})
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = gpz_fail(GPZ_ERR_HIP, "%s: sync failed", who);
    return rc;
}

// gpz_predictor_run (full branch): mu, nu, beta and, when asked, PHI of every tile come home
struct RunJob {
    gpz_predictor *p;
    int64_t ns;
    double *mu, *nu, *beta_i, *PHI;
    const char *who = "gpz_predictor_run";
    const char *nan_text = "the rows have missing values (NaN): group them by pattern and call gpz_predict_missing (predict.m:45-69)";
    static constexpr bool downloads = true;
    int stage(int, int64_t, int64_t) { return 0; }
    bool upload(int, int64_t) { return false; }
    int kernels(int s, int64_t nt) { return rows_moments_tile(p, who, Rows{}, s, (int)nt, PHI != nullptr); }
    bool download(int s, int64_t nt) {
        return hipMemcpyAsync(p->hout[s], p->out[s], 3 * (size_t)p->k * nt * sizeof(double), hipMemcpyDeviceToHost, p->s_out) != hipSuccess ||
               (PHI && hipMemcpyAsync(p->hphi[s], p->phi_d[s], (size_t)p->m * nt * sizeof(double), hipMemcpyDeviceToHost, p->s_out) != hipSuccess);
    }
    void scatter(int s, int64_t r0, int64_t nt) {
        double *dst[3] = {mu, nu, beta_i};
        for (int q = 0; q < 3; ++q)
            for (int o = 0; o < p->k; ++o)
                memcpy(dst[q] + (size_t)o * ns + r0, p->hout[s] + (size_t)(q * p->k + o) * nt, (size_t)nt * sizeof(double));
        if (PHI)
            for (int j = 0; j < p->m; ++j) memcpy(PHI + (size_t)j * ns + r0, p->hphi[s] + (size_t)j * nt, (size_t)nt * sizeof(double));
    }
};

static int predictor_run_full(gpz_predictor *p, const double *Xs, int64_t ns, double *mu, double *nu, double *beta_i, double *PHI) {
    RunJob job{p, ns, mu, nu, beta_i, PHI};
    return predictor_drain(p, job.who, predictor_pipeline(p, Xs, ns, p->tile_rows, job));
}

// input noise: gpz_predict_noisy on one tile of rows at a time (its buffers are sized by the tile)
static int predictor_run_noisy(gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi, int32_t psi_kind, double *mu,
                               double *nu, double *beta_i, double *gamma, double *PHI) {
    const int k = p->k, d = p->d, m = p->m;
    const int64_t T = p->tile_rows;
    const size_t pr = psi_kind == 2 ? (size_t)d * d : (size_t)d;   // Psi doubles per row
    std::vector<double> xt, pt, o4, ph;
    for (int64_t r0 = 0; r0 < ns; r0 += T) {
        const int64_t nt = std::min<int64_t>(T, ns - r0);
        xt.resize((size_t)nt * d);
        pt.resize((size_t)nt * pr);
        o4.resize((size_t)nt * k * 4);
        for (int c = 0; c < d; ++c) memcpy(xt.data() + (size_t)c * nt, Xs + (size_t)c * ns + r0, (size_t)nt * sizeof(double));
        if (psi_kind == 2)
            memcpy(pt.data(), Psi + (size_t)r0 * pr, (size_t)nt * pr * sizeof(double));
        else
            for (int c = 0; c < d; ++c) memcpy(pt.data() + (size_t)c * nt, Psi + (size_t)c * ns + r0, (size_t)nt * sizeof(double));
        if (PHI) ph.resize((size_t)nt * m);
        double *o = o4.data();
        const size_t ok = (size_t)nt * k;
        if (int rc = gpz_predict_noisy(&p->desc, p->theta_h.data(), p->w_h.data(), p->iS_h.data(), xt.data(), nt, pt.data(), psi_kind, o,
                                       o + ok, o + 2 * ok, o + 3 * ok, PHI ? ph.data() : nullptr))
            return rc;
        double *dst[4] = {mu, nu, beta_i, gamma};
        for (int q = 0; q < 4; ++q)
            for (int oo = 0; oo < k; ++oo)
                memcpy(dst[q] + (size_t)oo * ns + r0, o + q * ok + (size_t)oo * nt, (size_t)nt * sizeof(double));
        if (PHI)
            for (int j = 0; j < m; ++j) memcpy(PHI + (size_t)j * ns + r0, ph.data() + (size_t)j * nt, (size_t)nt * sizeof(double));
    }
    return 0;
}

// ---- Psi beside the rows (gpz_predictor_draws_noisy, _stack_noisy) ----------------------------------------------------------------------
// Psi: normalised ns x d column-major, staged into a second pair of pinned slots and uploaded with X's tile
static int predictor_psi_pinned(gpz_predictor *p) {
    for (int s = 0; s < 2; ++s)
        if (!p->hpsi[s]) HIPCHK(hipHostMalloc((void **)&p->hpsi[s], (size_t)p->d * p->tile_pad * sizeof(double), hipHostMallocDefault));
    return 0;
}

// Psi's tile into hpsi[s]: 0, or the refusal in the name of who
static int predictor_stage_psi(gpz_predictor *p, const char *who, const double *Psi, int64_t ns, int s, int64_t r0, int64_t nt) {
    if (predictor_stage(Psi, ns, p->d, r0, nt, p->hpsi[s], (size_t)p->tile_pad,
                        [](double v) { return !(v >= 0.0) || !(v <= 1.7976931348623157e308); }))
        return gpz_fail(GPZ_ERR_ARG, "%s: Psi has an element that is NaN, infinite or negative", who);
    return 0;
}

static bool predictor_upload_psi(gpz_predictor *p, int s, int64_t nt) {
    const size_t tp = (size_t)p->tile_pad;
    return hipMemcpy2DAsync(p->Psic[s], tp * sizeof(double), p->hpsi[s], tp * sizeof(double), (size_t)nt * sizeof(double), p->d,
                            hipMemcpyHostToDevice, p->s_in) != hipSuccess;
}

// ---- draws ------------------------------------------------------------------------------------------------------------------------
// gpz_predictor_draws: the draws of every tile come home.  Psi (gpz_predictor_draws_noisy; nullptr: noise-free rows) rides with the rows.
// (The refusal of rows with NaN says gpz_predictor_draws for either entry, as it always has.)
struct DrawsJob {
    gpz_predictor *p;
    int64_t ns;
    int nd, ncol, ldw;
    const double *Psi;
    double *F;
    Rows rows{Psi ? ROWS_NOISY : ROWS_CLEAN};
    const char *who = "gpz_predictor_draws";
    const char *nan_text = "the rows have missing values (NaN): draws are for complete rows";
    static constexpr bool downloads = true;
    int stage(int s, int64_t r0, int64_t nt) { return Psi ? predictor_stage_psi(p, "gpz_predictor_draws_noisy", Psi, ns, s, r0, nt) : 0; }
    bool upload(int s, int64_t nt) { return Psi && predictor_upload_psi(p, s, nt); }
    int kernels(int s, int64_t nt) { return rows_draws_tile(p, who, rows, s, (int)nt, ncol, ldw, false); }
    bool download(int s, int64_t nt) {
        return hipMemcpyAsync(p->hdout[s], p->dout[s], (size_t)ncol * nt * sizeof(double), hipMemcpyDeviceToHost, p->s_out) != hipSuccess;
    }
    void scatter(int s, int64_t r0, int64_t nt) {   // column c = o nd + q of the slot -> F(:, o, q)
        for (int c = 0; c < ncol; ++c) {
            const int o = c / nd, q = c % nd;
            memcpy(F + (size_t)(o + (size_t)p->k * q) * ns + r0, p->hdout[s] + (size_t)c * nt, (size_t)nt * sizeof(double));
        }
    }
};

static int predictor_run_draws(gpz_predictor *p, const double *Xs, int64_t ns, int nd, unsigned long long seed, const double *Z,
                               double *F, const double *Psi) {
    int rc = 0;
    int64_t T = 0;
    if (Psi && ((rc = predictor_psi_slots(p)) || (rc = predictor_psi_pinned(p)))) return rc;
    if ((rc = rows_draws_prepare(p, Rows{}, nd, seed, Z, true, &T))) return rc;
    if (Psi && p->large_m && rup(p->m, 16) > 256) p->large_seen = true;
    if (Psi && p->droute != 0 && !p->large_m) return gpz_fail(GPZ_ERR_UNSUPPORTED, "gpz_predictor_draws_noisy: input noise needs the fused draws route");
    DrawsJob job{p, ns, nd, nd * p->k, rup(nd * p->k, 16), Psi, F};
    return predictor_drain(p, job.who, predictor_pipeline(p, Xs, ns, T, job));   // on tiles of T rows
}

// gpz_predictor_draws and, with noisy, gpz_predictor_draws_noisy
static int draws_entry(const char *who, bool noisy, gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi, int32_t ndraws,
                       uint64_t seed, const double *Z, double *F) {
    if (int rc = predictor_check_call(who, p, ns)) return rc;
    if (int rc = predictor_check_ndraws(who, p, ndraws, 1)) return rc;
    if (int rc = rows_check(who, p, Rows{noisy ? ROWS_NOISY : ROWS_CLEAN}, true)) return rc;
    if (ns == 0) return 0;
    if (!Xs || (noisy && !Psi) || !F) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    return predictor_call(p, who, [&] { return predictor_run_draws(p, Xs, ns, (int)ndraws, (unsigned long long)seed, Z, F, Psi); });
}

// ---- stack ------------------------------------------------------------------------------------------------------------------------
// gpz_predictor_stack and, with Psi, gpz_predictor_stack_noisy: the tile's labels and weights (and Psi) ride up with its rows, nothing
// comes home
struct StackJob {
    gpz_predictor *p;
    const char *who;
    const Rows &rows;
    const StackCall &c;
    int64_t ns;
    const double *Psi;
    const int32_t *group;
    const double *weight;
    const char *nan_text = "the rows have missing values (NaN): stacks are for complete rows";
    static constexpr bool downloads = false;
    int stage(int s, int64_t r0, int64_t nt) {
        if (Psi)
            if (int rc = predictor_stage_psi(p, who, Psi, ns, s, r0, nt)) return rc;
        if (group) memcpy(p->hlab[s], group + r0, (size_t)nt * sizeof(int));
        if (weight) memcpy(p->hwt[s], weight + r0, (size_t)nt * sizeof(double));
        return 0;
    }
    bool upload(int s, int64_t nt) {
        return (Psi && predictor_upload_psi(p, s, nt)) ||
               (group && hipMemcpyAsync(p->lab_d[s], p->hlab[s], (size_t)nt * sizeof(int), hipMemcpyHostToDevice, p->s_in) != hipSuccess) ||
               (weight && hipMemcpyAsync(p->wt_d[s], p->hwt[s], (size_t)nt * sizeof(double), hipMemcpyHostToDevice, p->s_in) != hipSuccess);
    }
    int kernels(int s, int64_t nt) {
        return predictor_stack_tile(p, who, rows, c, s, nt, group ? p->lab_d[s] : nullptr, weight ? p->wt_d[s] : nullptr);
    }
};

static int predictor_run_stack(gpz_predictor *p, const char *who, const double *Xs, int64_t ns, const double *Psi, const StackArgs &a,
                               double *res) {
    const Rows rows{Psi ? ROWS_NOISY : ROWS_CLEAN};
    StackCall c{};
    int rc = rows_prepare(p, who, rows, true);
    if (!rc && Psi) rc = predictor_psi_pinned(p);
    if (rc) return rc;   // nothing of the call is queued yet
    rc = predictor_stack_prepare(p, who, rows, a, true, &c);
    if (!rc) {
        StackJob job{p, who, rows, c, ns, Psi, a.group, a.weight};
        rc = predictor_pipeline(p, Xs, ns, c.T, job);
    }
    if (!rc) rc = predictor_stack_result(p, who, c, res);
    return predictor_drain(p, who, rc);
}

// gpz_predictor_stack and, with noisy, gpz_predictor_stack_noisy.  The first one alone clears its outputs before it runs (stack_entry).
static int stack_host_entry(const char *who, bool noisy, gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi,
                            const StackArgs &a) {
    return stack_entry(
        who, p, ns, Xs, a, !noisy,
        [&] {
            if (int rc = rows_check(who, p, Rows{noisy ? ROWS_NOISY : ROWS_CLEAN}, true)) return rc;
            if (noisy && ns > 0 && !Psi) return gpz_fail(GPZ_ERR_ARG, "%s: null Psi", who);
            for (int64_t i = 0; a.group && i < ns; ++i)
                if (a.group[i] < -1 || a.group[i] >= a.ngroups)
                    return gpz_fail(GPZ_ERR_ARG, "%s: label %d of row %lld is outside [-1, %d)", who, (int)a.group[i], (long long)i,
                                    (int)a.ngroups);
            return 0;
        },
        [&] {
            for (int64_t i = 0; a.weight && i < ns; ++i)
                if (!(a.weight[i] >= 0.0) || !std::isfinite(a.weight[i]))
                    return gpz_fail(GPZ_ERR_ARG, "%s: the weight of row %lld is negative or not finite", who, (long long)i);
            return 0;
        },
        [&](double *res) { return predictor_run_stack(p, who, Xs, ns, Psi, a, res); });
}
}   // namespace gpzi

extern "C" int gpz_predictor_run(gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi, int32_t psi_kind, double *mu,
                                 double *nu, double *beta_i, double *gamma, double *PHI) {
    const char *who = "gpz_predictor_run";
    if (int rc = predictor_check_call(who, p, ns)) return rc;
    if (ns == 0) return 0;
    if (!Xs || !mu || !nu || !beta_i || !gamma) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_run: null argument");
    if (psi_kind < 0 || psi_kind > 3 || (psi_kind != 0) != (Psi != nullptr))
        return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_run: psi_kind %d does not match Psi", (int)psi_kind);
    if ((psi_kind == 2 || psi_kind == 3) && p->kind != GPZ_KIND_COV)
        return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_run: psi_kind %d is for the covariance kinds", (int)psi_kind);
    return predictor_call(p, who, [&] {
        int rc = 0;
        if (Psi) {
            rc = predictor_run_noisy(p, Xs, ns, Psi, psi_kind, mu, nu, beta_i, gamma, PHI);
        } else {
            memset(gamma, 0, (size_t)ns * p->k * sizeof(double));   // predictDiag.m:74
            if (PHI) rc = predictor_want_phi(p);
            if (!rc) rc = predictor_run_full(p, Xs, ns, mu, nu, beta_i, PHI);
        }
        if (!rc) ++p->runs;
        return rc;
    });
}

extern "C" int gpz_predictor_draws(gpz_predictor *p, const double *Xs, int64_t ns, int32_t ndraws, uint64_t seed, const double *Z,
                                   double *F) {
    return draws_entry("gpz_predictor_draws", false, p, Xs, ns, nullptr, ndraws, seed, Z, F);
}

extern "C" int gpz_predictor_draws_noisy(gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi, int32_t ndraws, uint64_t seed,
                                         const double *Z, double *F) {
    return draws_entry("gpz_predictor_draws_noisy", true, p, Xs, ns, Psi, ndraws, seed, Z, F);
}

extern "C" int gpz_predictor_stack(gpz_predictor *p, const double *Xs, int64_t ns, int32_t ndraws, uint64_t seed, const double *Z,
                                   const double *edges, int32_t nbins, const int32_t *group, int32_t ngroups, const double *weight,
                                   double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift) {
    return stack_host_entry("gpz_predictor_stack", false, p, Xs, ns, nullptr,
                            StackArgs{ndraws, seed, Z, edges, nbins, group, ngroups, weight, hist, sum_w, sum_mu, sum_mu2, mu_shift});
}

extern "C" int gpz_predictor_stack_noisy(gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi, int32_t ndraws, uint64_t seed,
                                         const double *Z, const double *edges, int32_t nbins, const int32_t *group, int32_t ngroups,
                                         const double *weight, double *hist, double *sum_w, double *sum_mu, double *sum_mu2,
                                         const double *mu_shift) {
    return stack_host_entry("gpz_predictor_stack_noisy", true, p, Xs, ns, Psi,
                            StackArgs{ndraws, seed, Z, edges, nbins, group, ngroups, weight, hist, sum_w, sum_mu, sum_mu2, mu_shift});
}
