// Host side of libgpz_hip.so: the persistent streaming predictor (gpz_predictor_*, include/gpz_hip.h).
//
// gpz_predict_full is a one-shot: per call it builds a context, uploads and scans all rows, transposes inv(Sigma_o) on the host, and holds
// PHI and T for every row on the device.  A predictor does the once-per-model work once (theta unpacked, the QR factors of the covariance
// kinds, B_o = [inv(Sigma_o) | w | v] laid out for the product) and then streams any number of rows through tile-sized buffers:
//   * route 0, fused: ceil16(m + 2k) <= 256 and an instantiated d - k_predict_small writes mu, nu and beta only (PHI and T never exist);
//   * route 1, tiles: the existing k_phi_* + k_tgemm (nu and PHI w from its epilogue) on one tile of rows at a time, k_pred_tile_finish.
// Rows with input noise go through gpz_predict_noisy one tile at a time.  Device memory does not depend on the number of rows: the
// buffers are sized by the tile at creation (PHI's own tile buffers are added on the first call that asks for PHI).
//
// Pipeline of gpz_predictor_run (full branch): three streams - copies in, compute, copies out - and two slots of pinned staging and device
// buffers.  Tile t's upload, tile t-1's kernels and tile t-2's download are in flight together while the host thread stages tile t+1's
// rows and scatters tile t-2's results into the caller's column-major arrays.
//
// gpz_predictor_draws (posterior draws of the mean, F_s = PHI W_s with W_s = w + R z_s) runs the same pipeline on a tile of its own, sized
// so that one slot's output is at most 256 MiB.  Its buffers, the factors R_o and W are allocated on the first draws call, so a
// predict-only handle holds what it held before:
//   * draws route 0, fused: ceil16(m) <= 256 and an instantiated d - k_predict_draws writes the draws only (PHI never leaves LDS);
//   * draws route 1, tiles: k_phi_* + k_tgemm with B = W (all n_draws * k columns in one product) + a transpose into the slot.
// gpz_predictor_stack (stacked predictive densities per group, for the posterior-mean weights and per draw) runs predictor_tile and, with
// draws, their kernels on the draws tile without any download, then k_stack_tile / k_stack_accum (k_predict_stack.hip); the accumulators
// come home once at the end.  Its buffers (labels, weights, edges, accumulators, slabs) are allocated on the first stack call.
// R_o is the Cholesky factor of the symmetric part S_o of iSigma_w(:, :, o) (k_chol_step); where it breaks down (a failed pivot, or
// min L_jj^2 <= m eps max S_jj) it is V diag(sqrt(max(lambda, 0))) from the one-sided Jacobi sweeps of k_pinv.hip.
// The device-resident entries (gpz_predictor_run_dev / _draws_dev / _stack_dev) take the rows from the caller's device memory and leave
// the per-row results there: per tile k_pred_stage -> the same predictor_tile / predictor_draws_tile / k_stack_tile -> a finish kernel
// (k_predict_dev.hip), all on the compute stream, which waits for an event on the caller's stream first.  No pinned slot, no copy
// stream; one scan of all rows (k_pred_check_dev) before the first tile stands for the host entries' NaN, label and weight loops.
// Rows with per-dimension input noise stay on the handle where predict_noisy_fits holds (a diagonal kind, d <= 20, k <= 8, m <= 256):
// gpz_predictor_run_noisy_dev runs k_predict_noisy_small per tile (predictNoisy as one kernel + a finish, k_predict_noisy.hip), and
// gpz_predictor_draws_noisy / _draws_noisy_dev the draws kernel behind a PHI block built from X and Psi.  The pair table (which depends on
// the model only), the Psi slots, the 4k-row outputs and the chunk slab are allocated on the first such call (predictor_noisy_prepare).
// gpz_predictor_run with Psi keeps the one-shot route above.
// On a handle created with GPZ_PREDICT_LARGE_M the complete rows with Psi (this paragraph, the covariance kinds' and the cube's below;
// not the groups with missing inputs) stay on the handle up to ceil16(m) <= 1024: the same kernels and chunk counts on a larger pair
// table, and off the fused draws route the draws of a diagonal kind as E_x[PHI] of the tile (k_predict_noisy_phi) against W on k_tgemm.
// The covariance kinds (GC, VC) have the same two questions where predict_noisy_cov_fits holds (1 <= d <= 10, k <= 8, m <= 256), for a
// variance per input dimension: gpz_predictor_run_noisy_cov_dev runs k_predict_noisy_cov_small per tile (k_predict_noisy_cov.hip: a
// packed Cholesky per row and record in registers) with the same finish, and gpz_predictor_draws_noisy_cov_dev E_x[PHI] of the tile
// (k_predict_noisy_cov_phi) against W on k_tgemm.  Their record tables are written on the first such call (predictor_noisy_cov_prepare)
// from Sigma_j, ln|Sigma_j| and the raw pair records of predictor_cov_model_tables, which the missing-input entries below keep on the handle.
// gpz_predictor_stack_noisy_cov_dev / _draws_gamma_noisy_cov_dev answer the other two questions for them as the entries of the next
// paragraph do for the diagonal kinds, with gamma under every draw from k_predict_noisy_cov_gamma.hip (the same frame,
// k_predict_gamma_impl.h, with k_predict_noisy_cov_small's pair density) on the handle's packed pair records.
// gpz_predictor_stack_noisy / _stack_noisy_dev stack rows with Psi of a diagonal kind: per tile predictNoisy, the draws with Psi, gamma under every draw
// (k_predict_noisy_gamma.hip: predict_gamma_body of k_predict_gamma_impl.h, an f64 MFMA product of pair densities and weight products,
// with k_predict_noisy_small's pair density), and k_stack_tile_w with a width per (column,
// row); gpz_predictor_draws_gamma_noisy_dev returns that gamma beside the draws.  Their buffers are allocated on their first call.
// gpz_predictor_stack_missing_dev stacks one group of rows with missing inputs in the same way, with gamma under every draw from
// k_predict_missing_gamma.hip (the pair kernel's product chained into a second f64 MFMA against the weight products);
// gpz_predictor_draws_gamma_missing_dev returns that gamma beside the draws.  Their buffers are allocated on their first call.
// Rows with missing inputs, one group of a NaN pattern per call, stay on the handle too where predict_missing_fits holds (the same
// shapes): gpz_predictor_run_missing_dev / _draws_missing_dev run predictMissing on tiles of at most GPZ_PREDICTOR_TILE_MISSING rows
// (k_predict_missing.hip): No and Pio, PHI through k_tgemm, then the fused pair kernel, or for the draws k_tgemm against W.  The tables
// of a pattern (NijS, the pair records, U) are kept until the pattern or the priors change; all of it is allocated on the first such call.
// On a handle created with GPZ_PREDICT_LARGE_M_MISSING these groups (and those with Psi below, their stacks and gamma per draw) stay on
// the handle up to ceil16(m) <= 1024 (predict_missing_large_fits): the same tables, tiles, chunk count, slabs and finish, with the pair
// product past 256 in k_pml_pairs / k_pml_gamma (k_predict_group_large_impl.h), whose LDS does not grow with m.
// The covariance kinds have these two entries as gpz_predictor_run_missing_cov_dev / _draws_missing_cov_dev where
// predict_missing_cov_fits holds (1 <= d <= 10, k <= 8, m <= 256; k_predict_missing_cov.hip): every density of predictMissing of
// predictCov.m is a quadratic in the row's observed inputs, written once per pattern as a record; Ex, Pio and PHI per tile from the m
// and m^2 records of the pattern, the pair sums from the m^2 (m + 1) / 2 pair-component records, which pass through a slab of at most
// 64 MB (predictor_missing_cov_prepare, predictor_missing_cov_tile); the finish and the draws are the diagonal kinds'.
// A group whose rows have Psi as well goes through gpz_predictor_run_noisy_missing_dev / _draws_noisy_missing_dev (predictNoisyMissing,
// k_predict_noisy_missing.hip): the same tiles and tables with No widened by psi and a pair kernel whose epilogue is predictNoisy's, on a
// second record table that is the model's alone.  gpz_predictor_stack_noisy_missing_dev stacks such a group as the two stacks above,
// with gamma under every draw from k_predict_noisy_missing_gamma.hip (k_predict_missing_gamma's two chained products with that
// epilogue between them); gpz_predictor_draws_gamma_noisy_missing_dev returns that gamma beside the draws.
// The covariance kinds have the first two of these as gpz_predictor_run_noisy_missing_cov_dev / _draws_noisy_missing_cov_dev
// (k_predict_noisy_missing_cov.hip): the frame, tile buffers and pattern tables of the missing_cov entries, with record tables of
// their own whose density is a packed no x no Cholesky of M + diag(psi_o) per row (predictor_noisy_missing_cov_prepare), and the other
// two as gpz_predictor_stack_noisy_missing_cov_dev / _draws_gamma_noisy_missing_cov_dev, with gamma under every draw from
// k_predict_noisy_missing_cov_gamma.hip (k_predict_missing_cov_gamma's frame on those records and that slab).
// Such a group whose rows have a full d x d Psi each has all four as gpz_predictor_run_psi_cube_missing_dev / _draws_ / _draws_gamma_ /
// _stack_psi_cube_missing_dev (k_predict_psi_cube_missing.hip, k_predict_psi_cube_missing_gamma.hip): the same records, slabs and tile
// buffers, the packed Cholesky of M + Psi_oo over the observed triangle of the row's matrix, which k_pcm_stage_psi packs into Psiq.
// Layout: gpz_predictor.h holds the handle and what the three units share.  This unit holds the handle's life and setup, what a tile is
// made of for each kind of rows (clean, with Psi, one NaN-pattern group: the rows_* functions), draws preparation and factorisation, the
// stack's preparation and tile, the checks the entries share, route and info.  gpz_predictor_host.hip holds the host pipeline, its jobs
// and the entries that take host arrays; gpz_predictor_dev.hip the device-resident entries.  Every entry is one check ladder and one
// runner per question (moments, draws with or without gamma, stack) for every kind of rows.  What two kinds of rows both need is
// written once: predictor_phi_times_w (PHI W of the draws on k_tgemm), predictor_noisy_slots, predictor_cov_model_tables, PER_DRAW.
#include <string>

#include "gpz_predictor.h"

namespace gpzi {
static void predictor_free(gpz_predictor *p) {
    if (!p) return;
    if (p->s_cmp) (void)hipSetDevice(p->device);
    for (hipStream_t s : {p->s_in, p->s_cmp, p->s_out})
        if (s) (void)hipStreamSynchronize(s);
    for (int s = 0; s < 2; ++s) {
        if (p->hin[s]) (void)hipHostFree(p->hin[s]);
        if (p->hout[s]) (void)hipHostFree(p->hout[s]);
        if (p->hphi[s]) (void)hipHostFree(p->hphi[s]);
        if (p->hdout[s]) (void)hipHostFree(p->hdout[s]);
        if (p->hlab[s]) (void)hipHostFree(p->hlab[s]);
        if (p->hwt[s]) (void)hipHostFree(p->hwt[s]);
        if (p->hpsi[s]) (void)hipHostFree(p->hpsi[s]);
        if (p->ev_in[s]) (void)hipEventDestroy(p->ev_in[s]);
        if (p->ev_cmp[s]) (void)hipEventDestroy(p->ev_cmp[s]);
        if (p->ev_out[s]) (void)hipEventDestroy(p->ev_out[s]);
    }
    if (p->ev_dev) (void)hipEventDestroy(p->ev_dev);
    p->ar.release();
    for (hipStream_t s : {p->s_in, p->s_cmp, p->s_out})
        if (s) (void)hipStreamDestroy(s);
    delete p;
}

static int predictor_setup(gpz_predictor *p, const double *theta, const double *w, const double *iSigma_w, int64_t tile_rows,
                           int32_t flags) {
    const size_t m = p->m, de = p->de, k = p->k;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamCreateWithFlags(&p->s_in, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&p->s_cmp, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&p->s_out, hipStreamNonBlocking));
    for (int s = 0; s < 2; ++s) {
        HIPCHK(hipEventCreateWithFlags(&p->ev_in[s], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&p->ev_cmp[s], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&p->ev_out[s], hipEventDisableTiming));
        HIPCHK(hipEventRecord(p->ev_cmp[s], p->s_cmp));   // recorded once, so that the first waits of gpz_predictor_run have an event
        HIPCHK(hipEventRecord(p->ev_out[s], p->s_out));
    }
    p->force_tiles = (flags & GPZ_PREDICT_FORCE_TILES) != 0;
    p->large_m = (flags & GPZ_PREDICT_LARGE_M) != 0;
    p->large_m_missing = (flags & GPZ_PREDICT_LARGE_M_MISSING) != 0;
    p->route = (!p->force_tiles && predict_small_fits(p->de, p->m, p->k)) ? 0 : 1;
    if (tile_rows <= 0) {
        if (p->route == 0) tile_rows = GPZ_PREDICTOR_TILE_FUSED;
        else {   // PHI + T of a tile within about 1 GiB
            tile_rows = (1L << 30) / (16L * p->mp);
            tile_rows = std::max<int64_t>(1024, std::min<int64_t>(GPZ_PREDICTOR_TILE_FUSED, tile_rows / 1024 * 1024));
        }
    }
    if (tile_rows > (1L << 24)) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_create: tile_rows %lld above 2^24", (long long)tile_rows);
    p->tile_rows = tile_rows;
    p->tile_pad = rup(tile_rows, 1024);
    const size_t tp = (size_t)p->tile_pad;
    // ---- parameters: k_unpack (+ the QR factors of the covariance kinds), as run_phi_only does
    auto &ar = p->ar;
    int rc = 0;
    if ((rc = ar.alloc(&p->theta_d, (size_t)p->p))) return rc;
    if ((rc = ar.alloc(&p->pr.P, m * de))) return rc;
    if ((rc = ar.alloc(&p->pr.G, p->kind == GPZ_KIND_COV ? m * de * de : m * de))) return rc;
    if ((rc = ar.alloc(&p->pr.G2, m * de))) return rc;
    if ((rc = ar.alloc(&p->pr.Rc, m * (de * (de + 1) / 2 + de)))) return rc;
    if (const size_t wl = p->kind == GPZ_KIND_COV ? prep_cov_ws_len(p->m, p->de) : 0)
        if ((rc = ar.alloc(&p->prep_ws, wl))) return rc;
    if ((rc = ar.alloc(&p->pr.lnAlpha, m * k))) return rc;
    if ((rc = ar.alloc(&p->pr.alpha, m * k))) return rc;
    if ((rc = ar.alloc(&p->pr.b, k))) return rc;
    if ((rc = ar.alloc(&p->pr.v, m * k))) return rc;
    if ((rc = ar.alloc(&p->pr.lnTau, m * k))) return rc;
    if ((rc = ar.alloc(&p->pr.tau, m * k))) return rc;
    if ((rc = ar.alloc(&p->iS_d, m * m * k))) return rc;
    if ((rc = ar.alloc(&p->w_d, m * k))) return rc;
    hipStream_t st = p->s_cmp;
    HIPCHK(hipMemcpyAsync(p->theta_d, theta, (size_t)p->p * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(p->iS_d, iSigma_w, m * m * k * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(p->w_d, w, m * k * sizeof(double), hipMemcpyHostToDevice, st));
    launch_unpack(st, p->theta_d, p->mid, p->m, p->d, p->de, p->k, p->hetero, p->pr);
    if (p->kind == GPZ_KIND_COV) launch_prep_cov(st, p->pr.G, p->pr.P, p->m, p->de, p->pr.Rc, p->prep_ws);
    // ---- B_o and the tile buffers
    for (int s = 0; s < 2; ++s) {
        if ((rc = ar.alloc(&p->Xc[s], de * tp))) return rc;
        if ((rc = ar.alloc(&p->out[s], 3 * k * tp))) return rc;
        HIPCHK(hipMemsetAsync(p->Xc[s], 0, de * tp * sizeof(double), st));   // dimensions d .. de - 1 stay zero
    }
    const double *vsrc = p->hetero ? p->pr.v : nullptr;
    if (p->route == 0) {
        p->nk = rup(p->m, 16);
        p->ldb = rup(p->m + 2 * p->k, 16);
        const size_t bs = (size_t)p->nk * p->ldb;
        if ((rc = ar.alloc(&p->B, bs * k))) return rc;
        for (int o = 0; o < p->k; ++o)   // [inv(Sigma_o) | w | v]: mu_o = T(:, m + o), ln beta_o - b_o = T(:, m + k + o)
            launch_pred_fill_b(st, p->iS_d + (size_t)o * m * m, p->w_d, p->k, p->m, vsrc, p->k, p->m + p->k, p->m, p->nk, p->ldb,
                               p->B + (size_t)o * bs);
    } else {
        const size_t mp = (size_t)p->mp, bs = mp * mp;
        p->nslots = gpz_gemm_wave_cols() * (int)((mp + 127) / 128);
        if ((rc = ar.alloc(&p->B, bs * k))) return rc;
        for (int o = 0; o < p->k; ++o)   // gpz_predict_full's Bext: [inv(Sigma_o) | 0 .. w_o at column m + o .. 0]
            launch_pred_fill_b(st, p->iS_d + (size_t)o * m * m, p->w_d + (size_t)o * m, 1, p->m + o, nullptr, 0, 0, p->m, p->mp, p->mp,
                               p->B + (size_t)o * bs);
        if ((rc = ar.alloc(&p->Phi, tp * mp))) return rc;
        if ((rc = ar.alloc(&p->T, tp * mp))) return rc;
        if ((rc = ar.alloc(&p->nupart, (size_t)p->nslots * k * tp))) return rc;
        if ((rc = ar.alloc(&p->phiw, k * tp))) return rc;
        if ((rc = ar.alloc(&p->lnbeta, k * tp))) return rc;
    }
    for (int s = 0; s < 2; ++s) {
        HIPCHK(hipHostMalloc((void **)&p->hin[s], (size_t)p->d * tp * sizeof(double), hipHostMallocDefault));
        HIPCHK(hipHostMalloc((void **)&p->hout[s], 3 * k * tp * sizeof(double), hipHostMallocDefault));
        memset(p->hin[s], 0, (size_t)p->d * tp * sizeof(double));
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    p->theta_h.assign(theta, theta + p->p);
    p->w_h.assign(w, w + m * k);
    p->iS_h.assign(iSigma_w, iSigma_w + m * m * k);
    return 0;
}

// launch_phi's arguments for the nt rows in Xc[s] on the tile route: PHI into p->Phi, ln beta into p->lnbeta
static PhiArgs predictor_phi_args(const gpz_predictor *p, int s, int nt) {
    PhiArgs a{};
    a.Xc = p->Xc[s]; a.ldx = p->tile_pad; a.n = nt; a.n_pad = (int)rup(nt, 1024);
    a.m = p->m; a.mp = p->mp; a.d = p->de; a.k = p->k; a.kind = p->kind;
    a.P = p->pr.P; a.G = p->kind == GPZ_KIND_COV ? p->pr.Rc : p->pr.G2;
    a.v = p->hetero ? p->pr.v : nullptr; a.b = p->pr.b;
    a.Phi = p->Phi; a.lnbeta = p->lnbeta;
    return a;
}

// the kernels of one tile of nt rows: Xc[s] -> out[s] ([3k][nt]) and, when asked, phi_d[s] ([m][nt])
static int predictor_tile(gpz_predictor *p, int s, int nt, bool want_phi) {
    hipStream_t st = p->s_cmp;
    const int k = p->k;
    if (p->route == 0) {
        if (launch_predict_small(st, p->kind, p->de, p->Xc[s], p->tile_pad, nt, p->m, k, p->pr.P,
                                 p->kind == GPZ_KIND_COV ? p->pr.Rc : p->pr.G2, p->B, p->ldb, (long)p->nk * p->ldb, p->pr.b, p->out[s],
                                 nt, want_phi ? p->phi_d[s] : nullptr, nt))
            return gpz_fail(GPZ_ERR_HIP, "gpz_predictor_run: k_predict_small launch failed");
        return 0;
    }
    const long np = rup(nt, 1024);
    if (launch_phi(st, predictor_phi_args(p, s, nt)))
        return gpz_fail(GPZ_ERR_UNSUPPORTED, "gpz_predictor_run: PHI kernel not instantiated for d=%d", p->de);
    const size_t mp = (size_t)p->mp;
    for (int o = 0; o < k; ++o)
        launch_tgemm(st, p->Phi, p->mp, p->B + (size_t)o * mp * mp, p->mp, p->T, (int)np, p->mp,
                     p->nupart + (size_t)o * p->nslots * p->tile_pad, p->phiw + (size_t)o * p->tile_pad, p->m, p->m + o);
    launch_pred_tile_finish(st, p->phiw, p->nupart, p->nslots, np, (long)p->nslots * p->tile_pad, p->lnbeta, p->tile_pad, nt, k,
                            p->out[s], nt);
    if (want_phi) launch_transpose_out(st, p->Phi, p->mp, nt, p->m, p->phi_d[s]);
    if (hipGetLastError() != hipSuccess) return gpz_fail(GPZ_ERR_HIP, "gpz_predictor_run: kernel launch failed");
    return 0;
}

// PHI's tile buffers, each one where it is missing; the pinned ones only for a call that takes PHI home (pinned)
int predictor_want_phi(gpz_predictor *p, bool pinned) {
    const size_t n = (size_t)p->m * p->tile_pad;
    for (int s = 0; s < 2; ++s) {
        if (!p->phi_d[s])
            if (int rc = p->ar.alloc(&p->phi_d[s], n)) return rc;
        if (pinned && !p->hphi[s]) HIPCHK(hipHostMalloc((void **)&p->hphi[s], n * sizeof(double), hipHostMallocDefault));
    }
    return 0;
}

// ---- input noise on the handle ----------------------------------------------------------------------------------------------------
static int predictor_noisy_check(const char *who, const gpz_predictor *p) {
    if (p->large_m && !predict_noisy_fits(p->kind, p->de, p->m, p->k, true))
        return gpz_fail(GPZ_ERR_UNSUPPORTED,
                        "%s: input noise on the handle needs predict_noisy_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, k <= 8 and, "
                        "with GPZ_PREDICT_LARGE_M, ceil16(m) <= %d (method %.2s, d %d, m %d, k %d); gpz_predictor_run takes Psi for every "
                        "shape",
                        who, GPZ_PREDICT_LARGE_M_MAX, p->desc.method, p->d, p->m, p->k);
    if (!p->large_m && !predict_noisy_fits(p->kind, p->de, p->m, p->k))
        return gpz_fail(GPZ_ERR_UNSUPPORTED,
                        "%s: input noise on the handle needs predict_noisy_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, k <= 8 and "
                        "ceil16(m) <= 256 (method %.2s, d %d, m %d, k %d); gpz_predictor_run takes Psi for every shape",
                        who, p->desc.method, p->d, p->m, p->k);
    return 0;
}

// What every call with Psi needs, the draws included: Psic[2] and sd2.  Each one where it is missing.
int predictor_psi_slots(gpz_predictor *p) {
    const size_t tp = (size_t)p->tile_pad;
    int rc = 0;
    for (int s = 0; s < 2; ++s)
        if (!p->Psic[s]) {
            if ((rc = p->ar.alloc(&p->Psic[s], (size_t)p->de * tp))) return rc;
            HIPCHK(hipMemsetAsync(p->Psic[s], 0, (size_t)p->de * tp * sizeof(double), p->s_cmp));   // dimensions d .. de - 1 stay zero
        }
    if (!p->sd2_d && (rc = p->ar.alloc(&p->sd2_d, (size_t)p->d))) return rc;
    return 0;
}

// What a call with a full Psi per row needs in their place: the packed triangles of a tile, Psiq[2], and the divisor triangle
static int predictor_cube_slots(gpz_predictor *p) {
    const size_t np = (size_t)p->d * (p->d + 1) / 2;
    int rc = 0;
    for (int s = 0; s < 2; ++s)
        if (!p->Psiq[s] && (rc = p->ar.alloc(&p->Psiq[s], np * (size_t)p->tile_pad))) return rc;
    if (!p->div_d && (rc = p->ar.alloc(&p->div_d, np))) return rc;
    return 0;
}

// a handle with GPZ_PREDICT_LARGE_M whose model is past the limit without it
static bool predictor_is_large(const gpz_predictor *p) { return p->large_m && rup(p->m, 16) > 256; }

// the row stride of the chunk slab npart: the handle's padded tile, or that of the shrunk tile ntile of a large model
static long predictor_npart_ld(const gpz_predictor *p) { return p->ntile ? (long)rup(p->ntile, 1024) : (long)p->tile_pad; }

// The 4k-row output slots and the chunk slab of predictNoisy's moments over nchunks pair chunks, each where it is missing.  On a large
// model the calls that fill the slab run on tiles of ntile rows: the handle's tile, shrunk in whole granules of 1024 rows so that the
// slab is at most 1 GiB (rows_tile); everywhere else ntile stays 0 and the slab has the handle's tile, as it always had.
static int predictor_noisy_slots(gpz_predictor *p, int nchunks) {
    const size_t k = p->k, tp = (size_t)p->tile_pad;
    int rc = 0;
    for (int s = 0; s < 2; ++s)
        if (!p->nout[s] && (rc = p->ar.alloc(&p->nout[s], 4 * k * tp))) return rc;
    if (p->npart) return 0;
    if (predictor_is_large(p)) {
        const int64_t most = std::max<int64_t>(1024, (int64_t)((1L << 27) / ((long)nchunks * 5 * p->k)) / 1024 * 1024);
        p->ntile = std::min<int64_t>(p->tile_rows, most);
    }
    return p->ar.alloc(&p->npart, (size_t)nchunks * 5 * k * (size_t)predictor_npart_ld(p));
}

// What the first predictNoisy call adds to the handle beyond that: the pair table [lnZ | c_ab | C_ab | coefficients] (the model's alone:
// launch_pair_table needs only pr.P and pr.G for a diagonal kind), the 4k-row output slots and the chunk slab.  The draws read none of
// these and do not come here.
static int predictor_noisy_prepare(gpz_predictor *p) {
    if (p->noisy_ready) return 0;
    const size_t m = p->m, npair = m * (m + 1) / 2;
    hipStream_t st = p->s_cmp;
    int rc = 0;
    if ((rc = predictor_psi_slots(p))) return rc;
    p->nchunks = predict_noisy_chunks(p->m, p->d, p->k);
    p->nrec = predict_noisy_rec(p->d, p->k);
    if (!p->ptab && (rc = p->ar.alloc(&p->ptab, npair * p->nrec))) return rc;
    if ((rc = predictor_noisy_slots(p, p->nchunks))) return rc;
    launch_pair_table(st, GPZ_KIND_DIAG, p->m, p->d, p->de, p->pr.P, p->pr.G, nullptr, nullptr, p->ptab, p->nrec, nullptr);
    if (hipGetLastError() != hipSuccess ||
        launch_noisy_pair_coef(st, p->m, p->k, p->d, p->w_d, p->hetero ? p->pr.v : nullptr, p->iS_d, p->ptab, p->nrec))
        return gpz_fail(GPZ_ERR_HIP, "gpz_predictor: pair table launch failed");
    HIPCHK(hipStreamSynchronize(st));
    p->noisy_ready = true;
    return 0;
}

// predictNoisy of one tile of nt rows: Xc[s], Psic[s] -> nout[s] ([4k][nt] = mu | nu | beta | gamma)
static int predictor_noisy_tile(gpz_predictor *p, const char *who, int s, int nt) {
    if (launch_predict_noisy_small(p->s_cmp, p->d, p->de, p->Xc[s], p->Psic[s], p->tile_pad, nt, p->m, p->k, p->pr.P, p->pr.G2, p->w_d,
                                   p->hetero ? p->pr.v : nullptr, p->pr.b, p->ptab, p->nchunks, p->npart, predictor_npart_ld(p), p->nout[s]))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_noisy_small launch failed", who);
    return 0;
}

// ---- input noise on the handle, covariance kinds --------------------------------------------------------------------------------------
static int predictor_noisy_cov_check(const char *who, const gpz_predictor *p) {
    if (p->large_m && !predict_noisy_cov_fits(p->kind, p->d, p->m, p->k, true))
        return gpz_fail(GPZ_ERR_UNSUPPORTED,
                        "%s: input noise for a covariance kind on the handle needs predict_noisy_cov_fits: GC or VC, 1 <= d <= 10, "
                        "1 <= k <= 8 and, with GPZ_PREDICT_LARGE_M, ceil16(m) <= %d (method %.2s, d %d, m %d, k %d); a diagonal kind goes "
                        "to gpz_predictor_run_noisy_dev / _draws_noisy_dev, and gpz_predictor_run takes Psi for every shape",
                        who, GPZ_PREDICT_LARGE_M_MAX, p->desc.method, p->d, p->m, p->k);
    if (!p->large_m && !predict_noisy_cov_fits(p->kind, p->d, p->m, p->k))
        return gpz_fail(GPZ_ERR_UNSUPPORTED,
                        "%s: input noise for a covariance kind on the handle needs predict_noisy_cov_fits: GC or VC, 1 <= d <= 10, "
                        "1 <= k <= 8 and ceil16(m) <= 256 (method %.2s, d %d, m %d, k %d); a diagonal kind goes to "
                        "gpz_predictor_run_noisy_dev / _draws_noisy_dev, and gpz_predictor_run takes Psi for every shape",
                        who, p->desc.method, p->d, p->m, p->k);
    return 0;
}

// The model's own tables of a covariance kind, into the caller's blocks: Sigma_j (m d d doubles) and ln|Sigma_j| (m) from Gamma_j
// (launch_gen_prep, as the evaluation has them) and, where raw is given, launch_pair_table's records [lnZ | c_ab | C_ab] (1 + d + d d a
// pair).  inv(Sigma_j) and the pattern "every dimension observed" are temporaries of this call; it returns with the stream synchronised.
static int predictor_cov_model_tables(gpz_predictor *p, double *Sig, double *lnS, double *raw) {
    const size_t d = p->d, nsig = (size_t)p->m * d * d;
    hipStream_t st = p->s_cmp;
    double *iSig = nullptr;
    if (hipMalloc((void **)&iSig, (nsig + (d + 7) / 8) * sizeof(double)) != hipSuccess)
        return gpz_fail(GPZ_ERR_ALLOC, "gpz_predictor: out of device memory");
    unsigned char *pat = (unsigned char *)(iSig + nsig);
    int rc = 0;
    if (hipMemsetAsync(pat, 1, d, st) != hipSuccess) rc = gpz_fail(GPZ_ERR_HIP, "gpz_predictor: memset failed");
    if (!rc) {
        launch_gen_prep(st, p->pr.G, p->m, p->d, p->de, Sig, iSig, pat, 1, lnS, nullptr);
        if (raw) launch_pair_table(st, GPZ_KIND_COV, p->m, p->d, p->de, p->pr.P, p->pr.G, Sig, iSig, raw, (int)(1 + d + d * d), nullptr);
        if (hipGetLastError() != hipSuccess) rc = gpz_fail(GPZ_ERR_HIP, "gpz_predictor: table launch failed");
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = gpz_fail(GPZ_ERR_HIP, "gpz_predictor: sync failed");
    (void)hipFree(iSig);
    return rc;
}

// The record tables of rows with input noise on a covariance kind: predictor_cov_model_tables (with pairs, its pair records too) into
// temporaries of this call, repacked by k_noisy_cov_records into the handle's basis records and, with pairs, pair records.
static int predictor_noisy_cov_tables(gpz_predictor *p, bool pairs) {
    const size_t m = p->m, d = p->d, nsig = m * d * d, nraw = pairs ? m * (m + 1) / 2 * (1 + d + d * d) : 0;
    double *tmp = nullptr;
    if (hipMalloc((void **)&tmp, (nsig + m + nraw) * sizeof(double)) != hipSuccess) return gpz_fail(GPZ_ERR_ALLOC, "gpz_predictor: out of device memory");
    double *Sig = tmp, *lnS = Sig + nsig, *raw = pairs ? lnS + m : nullptr;
    int rc = predictor_cov_model_tables(p, Sig, lnS, raw);
    if (!rc && launch_noisy_cov_records(p->s_cmp, p->m, p->d, p->de, p->k, p->pr.P, Sig, lnS, raw, p->w_d, p->hetero ? p->pr.v : nullptr,
                                        p->iS_d, p->cbrec, pairs ? p->cprec : nullptr))
        rc = gpz_fail(GPZ_ERR_HIP, "gpz_predictor: record table launch failed");
    if (hipStreamSynchronize(p->s_cmp) != hipSuccess && !rc) rc = gpz_fail(GPZ_ERR_HIP, "gpz_predictor: sync failed");
    (void)hipFree(tmp);
    return rc;
}

// the PHI tile of the draws of such rows, on a handle whose own route has none
static int predictor_noisy_cov_phi_tile(gpz_predictor *p) {
    if (p->cphi) return 0;
    if (p->Phi) {   // the tile route's PHI, [tile_pad][mp]: a tile's kernels are done with it before the next one's
        p->cphi = p->Phi;
        return 0;
    }
    return p->ar.alloc(&p->cphi, (size_t)p->tile_pad * p->mp);
}

// What a call for such rows adds to the handle, each thing where it is missing: the Psi slots and the basis records (every call); with
// pairs (the moments, gamma per draw, the stack) the pair records, the 4k-row output slots and the chunk slab of predictor_noisy_prepare,
// which a covariance kind has from nowhere else; without (the draws) the PHI tile, which a call with pairs and draws takes in
// rows_fit_tile.
static int predictor_noisy_cov_prepare(gpz_predictor *p, const Rows &r, bool pairs) {
    const size_t m = p->m, npair = m * (m + 1) / 2;
    auto &ar = p->ar;
    int rc = 0;
    if ((rc = r.cube() ? predictor_cube_slots(p) : predictor_psi_slots(p))) return rc;
    p->cchunks = predict_noisy_cov_chunks(p->m, p->d, p->k);
    const bool basis = !p->cbrec, table = pairs && !p->ncov_ready;
    if (basis && (rc = ar.alloc(&p->cbrec, m * predict_noisy_cov_brec(p->d, p->k)))) return rc;
    if (!pairs) {
        if ((rc = predictor_noisy_cov_phi_tile(p))) return rc;
    } else {
        if (!p->cprec && (rc = ar.alloc(&p->cprec, npair * predict_noisy_cov_prec(p->d, p->k)))) return rc;
        if ((rc = predictor_noisy_slots(p, p->cchunks))) return rc;
    }
    if (basis || table)
        if ((rc = predictor_noisy_cov_tables(p, table))) return rc;
    if (table) p->ncov_ready = true;
    return 0;
}

// The two forms of Psi on complete rows of a covariance kind (Rows::ncov()) differ on the host in the tile's Psi slot, in the launchers of
// their three kernels (the same signatures: k_predict_noisy_cov*.hip and k_predict_psi_cube*.hip) and in the names of those kernels
struct NcovForm {
    double *const *Psi;               // Psic: a variance per dimension; Psiq: the packed triangle of a full matrix per row
    decltype(&launch_predict_noisy_cov_small) small;
    decltype(&launch_predict_noisy_cov_phi) phi;
    decltype(&launch_predict_noisy_cov_gamma) gamma;
    const char *name;                 // k_predict_<name>_small, _phi, _gamma
};
static NcovForm ncov_form(const gpz_predictor *p, const Rows &r) {
    if (r.cube()) return {p->Psiq, launch_predict_psi_cube_small, launch_predict_psi_cube_phi, launch_predict_psi_cube_gamma, "psi_cube"};
    return {p->Psic, launch_predict_noisy_cov_small, launch_predict_noisy_cov_phi, launch_predict_noisy_cov_gamma, "noisy_cov"};
}

// predictNoisy of one tile of nt rows: Xc[s] and the form's Psi slot -> nout[s] ([4k][nt] = mu | nu | beta | gamma)
static int predictor_noisy_cov_tile(gpz_predictor *p, const char *who, const Rows &r, int s, int nt) {
    const NcovForm f = ncov_form(p, r);
    if (f.small(p->s_cmp, p->d, p->mid == 4, p->Xc[s], f.Psi[s], p->tile_pad, nt, p->m, p->k, p->cbrec, p->cprec, p->pr.b, p->cchunks,
                p->npart, predictor_npart_ld(p), p->nout[s]))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_%s_small launch failed", who, f.name);
    return 0;
}

// ---- draws ------------------------------------------------------------------------------------------------------------------------
// R_o for every output, once per handle: the blocked Cholesky steps of k_chol.hip on S_o (padded to a multiple of 32 with the identity),
// the eigen-factor of k_pinv.hip's sweeps where that breaks down.
static int predictor_factor(gpz_predictor *p) {
    const int m = p->m, k = p->k, mq = rup(m, GPZ_CH_NB);
    hipStream_t st = p->s_cmp;
    auto &ar = p->ar;
    double *S = nullptr, *A = nullptr, *Lm = nullptr, *logdet = nullptr, *Gt = nullptr, *Vt = nullptr;
    int *info = nullptr;
    unsigned long long *word = nullptr;
    int rc = 0;
    if ((rc = ar.alloc(&p->R, (size_t)m * m * k))) return rc;
    if ((rc = ar.alloc(&S, (size_t)m * m))) return rc;
    if ((rc = ar.alloc(&A, (size_t)mq * mq))) return rc;
    if ((rc = ar.alloc(&Lm, (size_t)mq * mq))) return rc;
    if ((rc = ar.alloc(&logdet, 1))) return rc;
    if ((rc = ar.alloc(&info, 4 + (size_t)k))) return rc;   // [pivot failure, -, -, -, ok_0 .. ok_{k-1}]
    p->fkind.assign(k, 0);
    for (int o = 0; o < k; ++o) {
        launch_draws_sym(st, p->iS_d + (size_t)o * m * m, m, mq, S, A);
        HIPCHK(hipMemsetAsync(info, 0, 4 * sizeof(int), st));
        for (int k0 = 0; k0 < mq; k0 += GPZ_CH_NB) launch_chol_step(st, A, Lm, nullptr, mq, mq, k0, logdet, info, false);
        launch_draws_chol_check(st, Lm, mq, S, m, info, p->R + (size_t)o * m * m, info + 4 + o);
        int ok = 0;
        HIPCHK(hipMemcpyAsync(&ok, info + 4 + o, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (ok) continue;
        p->fkind[o] = 1;   // semidefinite (or numerically so): R_o = V diag(sqrt(max(lambda, 0)))
        if (!Gt) {
            if ((rc = ar.alloc(&Gt, (size_t)m * m))) return rc;
            if ((rc = ar.alloc(&Vt, (size_t)m * m))) return rc;
            if ((rc = ar.alloc(&word, 2))) return rc;
        }
        if (run_jacobi_sqrt(st, S, m, m, Gt, Vt, m, word, p->R + (size_t)o * m * m, m) < 0)
            return gpz_fail(GPZ_ERR_HIP, "gpz_predictor_draws: Jacobi sweeps failed");
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return 0;
}

// a device buffer of at least need doubles (a larger request takes a new block; the handle holds its blocks until it is destroyed, the
// outgrown one too: calls with ever larger shapes keep every earlier block, and the stack's accumulators and slabs can be 128 MiB each)
static int predictor_grow(gpz_predictor *p, double **buf, size_t *cap, size_t need) {
    if (*buf && *cap >= need) return 0;
    if (int rc = p->ar.alloc(buf, need)) return rc;
    *cap = need;
    return 0;
}

// the rows of W, K of a product against it (once the draws route is known)
static int predictor_wrows(const gpz_predictor *p) { return p->droute == 0 ? rup(p->m, 16) : p->mp; }

// what a call with nd draws needs before its first tile: the factors (once per handle), W for (seed, Z), the draws tile *Tout and the
// device buffers of that tile; the pinned slots too when the draws themselves go home (pinned)
static int predictor_draws_prepare(gpz_predictor *p, int nd, unsigned long long seed, const double *Z, bool pinned, int64_t *Tout) {
    const int k = p->k, m = p->m, ncol = nd * k, ldw = rup(ncol, 16);
    hipStream_t st = p->s_cmp;
    int rc = 0;
    if (p->droute < 0) {
        const int r = (!p->force_tiles && predict_draws_fits(p->de, p->m)) ? 0 : 1;
        if (r == 1 && !p->Phi)   // (not reached: a shape outside the fused draws kernel is outside k_predict_small too)
            return gpz_fail(GPZ_ERR_UNSUPPORTED, "gpz_predictor_draws: no PHI tile buffers on a fused-route handle");
        if ((rc = predictor_factor(p))) return rc;
        p->droute = r;
    }
    // ---- W = [W_0 | W_1 | ...] for this call (kept while the seed and the number of draws stay the same and Z is NULL)
    const int wrows = predictor_wrows(p);
    if (Z || !p->w_seeded || p->w_seed != seed || p->w_nd != nd || p->w_cap < (size_t)wrows * ldw) {
        if ((rc = predictor_grow(p, &p->Wd, &p->w_cap, (size_t)wrows * ldw))) return rc;
        if (Z) {
            if ((rc = predictor_grow(p, &p->Zd, &p->z_cap, (size_t)m * ncol))) return rc;
            HIPCHK(hipMemcpyAsync(p->Zd, Z, (size_t)m * ncol * sizeof(double), hipMemcpyHostToDevice, st));
        }
        launch_draws_weights(st, p->w_d, p->R, Z ? p->Zd : nullptr, seed, m, nd, k, wrows, ldw, p->Wd);
        HIPCHK(hipGetLastError());
        p->w_seeded = Z == nullptr;
        p->w_seed = seed;
        p->w_nd = nd;
    }
    // ---- the draws tile: the handle's, shrunk so that a slot's output is <= 256 MiB, in whole granules of the route
    const int64_t gran = p->droute == 0 ? 32 : 1024;
    int64_t T = std::min<int64_t>(p->tile_rows, (256L << 20) / (8L * ncol)) / gran * gran;
    if (T < gran) T = gran;   // <= tile_pad (a multiple of 1024)
    p->dtile = T;
    const size_t slot = (size_t)ncol * T;
    if (p->dout_cap < slot) {
        for (int s = 0; s < 2; ++s)
            if ((rc = p->ar.alloc(&p->dout[s], slot))) return rc;
        p->dout_cap = slot;
    }
    if (pinned && p->hdout_cap < slot) {
        for (int s = 0; s < 2; ++s) {
            if (p->hdout[s]) (void)hipHostFree(p->hdout[s]);
            p->hdout[s] = nullptr;
        }
        p->hdout_cap = 0;
        for (int s = 0; s < 2; ++s) HIPCHK(hipHostMalloc((void **)&p->hdout[s], slot * sizeof(double), hipHostMallocDefault));
        p->hdout_cap = slot;
    }
    if (p->droute == 1 && (rc = predictor_grow(p, &p->Td, &p->t_cap, (size_t)rup(T, 1024) * ldw))) return rc;
    *Tout = T;
    return 0;
}

// PHI of nt rows (np rows of mp doubles, the rows of k_tgemm's tile) against the handle's W on k_tgemm -> dout[s] ([ncol][nt], without
// muY): T = PHI W with K = the rows of W (those >= m are zero) and ldw output columns, then transposed into the slot
static int predictor_phi_times_w(gpz_predictor *p, const char *who, const double *Phi, long np, int s, int64_t nt, int ncol, int ldw) {
    launch_tgemm(p->s_cmp, Phi, p->mp, p->Wd, ldw, p->Td, (int)np, ldw, nullptr, nullptr, p->m, 0, false, predictor_wrows(p), ldw);
    launch_transpose_out(p->s_cmp, p->Td, ldw, nt, ncol, p->dout[s]);
    if (hipGetLastError() != hipSuccess) return gpz_fail(GPZ_ERR_HIP, "%s: kernel launch failed", who);
    return 0;
}

// the draws kernels of one tile of nt rows: Xc[s] -> dout[s] ([nd k][nt]).  phi_built: predictor_tile has just run on the same slot and
// rows on the tile route, so p->Phi already holds this tile's PHI (the same launch_phi with the same arguments; launch_tgemm only reads it)
// Psic: the tile's Psi slot for rows with input noise (diagonal kinds), else nullptr.  Off the fused route such rows need a handle with
// GPZ_PREDICT_LARGE_M: E_x[PHI] of the tile (k_predict_noisy_phi) into the tile route's PHI, which a handle off the fused draws route
// always has (predictor_draws_prepare), then the product against W as for every other kind
static int predictor_draws_tile(gpz_predictor *p, int s, int64_t nt, int ncol, int ldw, bool phi_built = false,
                                const double *Psic = nullptr) {
    const int m = p->m;
    hipStream_t st = p->s_cmp;
    const double *G = p->kind == GPZ_KIND_COV ? p->pr.Rc : p->pr.G2;
    if (Psic) {
        if (p->droute != 0 && p->large_m) {
            const int np = (int)rup(nt, 1024);   // <= tile_pad: zeros in the rows of the last partial block, as launch_tgemm takes them
            if (launch_predict_noisy_phi(st, p->d, p->de, p->Xc[s], Psic, p->tile_pad, (int)nt, np, m, p->mp, p->pr.P, p->pr.G2,
                                         predict_noisy_chunks(m, p->d, p->k), p->Phi))
                return gpz_fail(GPZ_ERR_HIP, "gpz_predictor_draws: k_predict_noisy_phi launch failed");
            return predictor_phi_times_w(p, "gpz_predictor_draws", p->Phi, np, s, nt, ncol, ldw);
        }
        if (p->droute != 0) return gpz_fail(GPZ_ERR_UNSUPPORTED, "gpz_predictor_draws: input noise needs the fused draws route");
        if (launch_predict_draws_psi(st, p->de, p->Xc[s], Psic, p->tile_pad, (int)nt, m, p->pr.P, G, p->Wd, ldw, ncol, p->dout[s], nt))
            return gpz_fail(GPZ_ERR_HIP, "gpz_predictor_draws: k_predict_draws_psi launch failed");
        return 0;
    }
    if (p->droute == 0) {
        if (launch_predict_draws(st, p->kind, p->de, p->Xc[s], p->tile_pad, (int)nt, m, p->pr.P, G, p->Wd, ldw, ncol, p->dout[s], nt))
            return gpz_fail(GPZ_ERR_HIP, "gpz_predictor_draws: k_predict_draws launch failed");
        return 0;
    }
    if (!phi_built && launch_phi(st, predictor_phi_args(p, s, (int)nt)))
        return gpz_fail(GPZ_ERR_UNSUPPORTED, "gpz_predictor_draws: PHI kernel not instantiated for d=%d", p->de);
    return predictor_phi_times_w(p, "gpz_predictor_draws", p->Phi, rup(nt, 1024), s, nt, ncol, ldw);   // (K = mp on this route)
}

// ---- rows with missing inputs on the handle -----------------------------------------------------------------------------------------
// cov: the entries of the covariance kinds (ROWS_MISSING_COV); each of the two refuses the other's kinds and names their entry
// noisy (with cov): the entries for such a group with Psi (ROWS_NOISY_MISSING_COV), whose diagonal kinds have gpz_predictor_*_noisy_missing_dev
// a handle with GPZ_PREDICT_LARGE_M_MISSING whose model is past the limit without it: its groups run the panelled pair kernels
static bool predictor_missing_is_large(const gpz_predictor *p) { return p->large_m_missing && rup(p->m, 16) > 256; }

static int predictor_missing_check(const char *who, const gpz_predictor *p, uint32_t obs, bool cov, bool noisy = false) {
    if (cov && noisy && p->kind != GPZ_KIND_COV)
        return gpz_fail(GPZ_ERR_UNSUPPORTED,
                        "%s: method %.2s is a diagonal kind: its rows with input noise and missing inputs go to "
                        "gpz_predictor_run_noisy_missing_dev / _draws_noisy_missing_dev",
                        who, p->desc.method);
    if (cov && p->kind != GPZ_KIND_COV)
        return gpz_fail(GPZ_ERR_UNSUPPORTED,
                        "%s: method %.2s is a diagonal kind: its rows with missing inputs go to gpz_predictor_run_missing_dev / "
                        "_draws_missing_dev / _draws_gamma_missing_dev / _stack_missing_dev",
                        who, p->desc.method);
    if (cov && !predict_missing_cov_fits(p->kind, p->d, p->m, p->k))
        return gpz_fail(GPZ_ERR_UNSUPPORTED,
                        "%s: missing inputs for a covariance kind on the handle need predict_missing_cov_fits: GC or VC, 1 <= d <= 10, "
                        "1 <= k <= 8 and ceil16(m) <= 256 (method %.2s, d %d, m %d, k %d); gpz_predict_missing takes every shape",
                        who, p->desc.method, p->d, p->m, p->k);
    if (!cov && predictor_missing_is_large(p)) {   // (GPZ_PREDICT_LARGE_M_MISSING past 256: the limit in m alone is wider)
        if (!predict_missing_large_fits(p->kind, p->de, p->m, p->k))
            return gpz_fail(GPZ_ERR_UNSUPPORTED,
                            "%s: missing inputs on the handle need predict_missing_large_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, "
                            "k <= 8 and, with GPZ_PREDICT_LARGE_M_MISSING, ceil16(m) <= %d (method %.2s, d %d, m %d, k %d); "
                            "gpz_predict_missing takes every shape",
                            who, GPZ_PREDICT_LARGE_M_MAX, p->desc.method, p->d, p->m, p->k);
    } else if (!cov && !predict_missing_fits(p->kind, p->de, p->m, p->k))
        return gpz_fail(GPZ_ERR_UNSUPPORTED,
                        "%s: missing inputs on the handle need predict_missing_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, k <= 8 and "
                        "ceil16(m) <= 256 (method %.2s, d %d, m %d, k %d); gpz_predict_missing takes every shape",
                        who, p->desc.method, p->d, p->m, p->k);
    const uint32_t full = p->d >= 32 ? 0xffffffffu : ((1u << p->d) - 1u);
    if (obs & ~full) return gpz_fail(GPZ_ERR_ARG, "%s: the mask %#x has a bit at or above d = %d", who, (unsigned)obs, p->d);
    if (obs == full)
        return gpz_fail(GPZ_ERR_ARG, "%s: no dimension is missing in the mask (complete rows go to gpz_predictor_run_dev / _draws_dev)", who);
    return 0;
}

// What a call for a group needs before its first tile: the tile buffers (on the first call; with pairs the pair tables, the chunk slab
// and the output slot too) and the tables of (obs, priors), rebuilt where the handle holds another pattern's.  priors: m values or
// nullptr for 1 / m.
// noisy: the rows have Psi too (ROWS_NOISY_MISSING) - the Psi slots and, with pairs, the second record table, which is the model's
// alone and written once; the tables of the pattern are the same ones.
static int predictor_missing_prepare(gpz_predictor *p, const char *who, uint32_t obs, const double *priors, bool pairs, bool noisy) {
    const size_t m = p->m, k = p->k, mp = p->mp, nk = rup(p->m, 16);
    auto &ar = p->ar;
    hipStream_t st = p->s_cmp;
    int rc = 0;
    if (noisy) {
        if ((rc = predictor_psi_slots(p))) return rc;
        if (pairs && !p->nmrec) {
            double *rec = nullptr;
            if ((rc = ar.alloc(&rec, (size_t)predict_missing_groups(p->m) * 64 * (size_t)predict_missing_rec(p->d, p->k)))) return rc;
            if (launch_pnm_records(st, p->m, p->d, p->de, p->k, p->pr.P, p->pr.G2, p->w_d, p->hetero ? p->pr.v : nullptr, p->iS_d, rec))
                return gpz_fail(GPZ_ERR_HIP, "%s: record kernel launch failed", who);
            p->nmrec = rec;
        }
        p->nm_used = true;
    }
    if (!p->mtile) p->mtile = std::min<int64_t>(p->tile_rows, GPZ_PREDICTOR_TILE_MISSING);
    const size_t mtp = (size_t)rup(p->mtile, 1024), npad = (size_t)predict_missing_groups(p->m) * 64;
    p->mchunks = predict_missing_chunks(p->m);
    if (!p->mNo && (rc = ar.alloc(&p->mNo, mtp * mp))) return rc;
    if (!p->mPio && (rc = ar.alloc(&p->mPio, mtp * mp))) return rc;
    if (!p->mT && (rc = ar.alloc(&p->mT, mtp * mp))) return rc;
    if (!p->mbt && (rc = ar.alloc(&p->mbt, 2 * mp))) return rc;
    if (!p->mNij && (rc = ar.alloc(&p->mNij, mp * mp))) return rc;
    if (!p->mpri && (rc = ar.alloc(&p->mpri, m))) return rc;
    if (!p->mhd && (rc = ar.alloc(&p->mhd, 2 * k * mtp))) return rc;
    if (pairs) {
        if (!p->mU && (rc = ar.alloc(&p->mU, npad * nk))) return rc;
        if (!p->mrec && (rc = ar.alloc(&p->mrec, npad * (size_t)predict_missing_rec(p->d, p->k)))) return rc;
        if (!p->mpart && (rc = ar.alloc(&p->mpart, (size_t)p->mchunks * 3 * k * mtp))) return rc;
        if (!p->mout && (rc = ar.alloc(&p->mout, 4 * k * mtp))) return rc;
    }
    if (!noisy) p->miss_used = true;
    if (predictor_missing_is_large(p)) p->mlarge_seen = true;
    const bool same_pri = priors ? (!p->mtab_uniform && p->mtab_pri.size() == m && std::equal(priors, priors + m, p->mtab_pri.begin()))
                                 : p->mtab_uniform;
    if (p->mtab_valid && p->mtab_obs == obs && same_pri && (p->mtab_pairs || !pairs)) return 0;
    p->mtab_valid = false;
    p->mtab_uniform = priors == nullptr;
    if (priors) {   // the handle's own copy: the upload may still be in flight when the caller has its memory back
        p->mtab_pri.assign(priors, priors + m);
        if (hipMemcpyAsync(p->mpri, p->mtab_pri.data(), m * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
            return gpz_fail(GPZ_ERR_HIP, "%s: copy failed", who);
    }
    if (launch_pmd_tables(st, p->m, p->mp, p->d, p->de, p->k, obs, p->pr.P, p->pr.G2, priors ? p->mpri : nullptr, p->w_d,
                          p->hetero ? p->pr.v : nullptr, p->iS_d, p->mbt, p->mNij, p->mU, p->mrec, pairs))
        return gpz_fail(GPZ_ERR_HIP, "%s: table kernel launch failed", who);
    p->mtab_obs = obs;
    p->mtab_pairs = pairs;
    p->mtab_valid = true;
    return 0;
}

// predictMissing of one tile of nt rows of the group: Xc[s] -> PHI in mNo, mu | ElnS - b in mhd and, with pairs, mout ([4k][nt] = mu | nu |
// beta | gamma).  Psic: the tile's Psi slot for a group with input noise too (predictNoisyMissing: No widened by psi, and the pair kernel
// of k_predict_noisy_missing.hip on the second record table), else nullptr
static int predictor_missing_tile(gpz_predictor *p, const char *who, int s, int nt, uint32_t obs, bool pairs, const double *Psic = nullptr) {
    hipStream_t st = p->s_cmp;
    const int np = rup(nt, 128);   // the rows of the product: k_tgemm's row tile
    const long mtp = rup(p->mtile, 1024);
    const double *v = p->hetero ? p->pr.v : nullptr;
    if (launch_pmd_no(st, p->Xc[s], Psic, p->tile_pad, nt, np, p->m, p->mp, p->d, p->de, obs, p->pr.P, p->pr.G2, p->mbt, p->mNo, p->mPio))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_%s_no launch failed", who, Psic ? "pnm" : "pmd");
    launch_tgemm(st, p->mPio, p->mp, p->mNij, p->mp, p->mT, np, p->mp, nullptr, nullptr, p->m, -1);
    if (hipGetLastError() != hipSuccess) return gpz_fail(GPZ_ERR_HIP, "%s: k_tgemm launch failed", who);
    if (launch_pmd_phi(st, p->mNo, p->mT, nt, p->m, p->mp, p->k, p->w_d, v, p->mhd, mtp))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_pmd_phi launch failed", who);
    // with Psi: the second record table (C, not 1 / C, and lnZ without the determinant, which depends on the row's Psi)
    if (pairs && predictor_missing_is_large(p)) {   // the same tables, slab and finish behind the panelled kernel
        if (launch_predict_missing_large_pairs(st, p->Xc[s], Psic, p->tile_pad, nt, p->mPio, p->mp, p->m, p->d, p->k, obs, p->mU,
                                               Psic ? p->nmrec : p->mrec, p->mchunks, p->mpart, mtp, p->mhd, mtp, p->pr.b, p->mout))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_pml_pairs%s launch failed", who, Psic ? "_psi" : "");
        return 0;
    }
    if (pairs && launch_predict_missing_pairs(st, p->Xc[s], Psic, p->tile_pad, nt, p->mPio, p->mp, p->m, p->d, p->k, obs, p->mU,
                                              Psic ? p->nmrec : p->mrec, p->mchunks, p->mpart, mtp, p->mhd, mtp, p->pr.b, p->mout))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_%smissing_pairs launch failed", who, Psic ? "noisy_" : "");
    return 0;
}

// the draws of one tile of the group behind predictor_missing_tile: PHI_missing (mNo) against the handle's W on k_tgemm -> dout[s]
// ([ncol][nt], without muY)
static int predictor_missing_draws_tile(gpz_predictor *p, const char *who, int s, int nt, int ncol, int ldw) {
    return predictor_phi_times_w(p, who, p->mNo, rup(nt, 128), s, nt, ncol, ldw);
}

// the draws of one tile of nt rows with Psi, covariance kinds: E_x[PHI] (k_predict_noisy_cov_phi or k_predict_psi_cube_phi, rows of the
// product padded with zeros) against the handle's W on k_tgemm -> dout[s] ([ncol][nt], without muY)
static int predictor_noisy_cov_draws_tile(gpz_predictor *p, const char *who, const Rows &r, int s, int nt, int ncol, int ldw) {
    const int np = rup(nt, 128);   // the rows of the product: k_tgemm's row tile
    const NcovForm f = ncov_form(p, r);
    if (f.phi(p->s_cmp, p->d, p->mid == 4, p->Xc[s], f.Psi[s], p->tile_pad, nt, np, p->m, p->mp, p->k, p->cbrec, p->cchunks, p->cphi))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_%s_phi launch failed", who, f.name);
    return predictor_phi_times_w(p, who, p->cphi, np, s, nt, ncol, ldw);
}

// ---- rows with missing inputs on the handle, covariance kinds -------------------------------------------------------------------------
// The model's own tables on the handle, each where it is missing: Sigma_j and ln|Sigma_j| and, with pairs, the raw pair records
// (predictor_cov_model_tables)
static int predictor_missing_cov_model(gpz_predictor *p, bool pairs) {
    const size_t m = p->m, d = p->d;
    const bool sig = !p->mcSig, raw = pairs && !p->mcraw;
    if (!sig && !raw) return 0;
    int rc = 0;
    double *Sig = p->mcSig, *lnS = p->mclnS, *rawt = nullptr;   // (where only raw is missing they are written again: the same values)
    if (sig && ((rc = p->ar.alloc(&Sig, m * d * d)) || (rc = p->ar.alloc(&lnS, m)))) return rc;
    if (raw && (rc = p->ar.alloc(&rawt, m * (m + 1) / 2 * (1 + d + d * d)))) return rc;
    if ((rc = predictor_cov_model_tables(p, Sig, lnS, rawt))) return rc;
    if (sig) { p->mcSig = Sig; p->mclnS = lnS; }
    if (raw) p->mcraw = rawt;
    return 0;
}

// What a call for a group needs before its first tile, as predictor_missing_prepare: the tile buffers and the record tables sized for
// the widest pattern of the model (so nothing grows with the patterns a handle sees), with pairs the pair records, coefficients, slab,
// chunk partials and the output slot too; then the tables of (obs, priors), rebuilt where the handle holds another pattern's.
static int predictor_missing_cov_prepare(gpz_predictor *p, const char *who, uint32_t obs, const double *priors, bool pairs) {
    const size_t m = p->m, k = p->k, mp = p->mp, npair = m * (m + 1) / 2;
    auto &ar = p->ar;
    hipStream_t st = p->s_cmp;
    int rc = 0;
    if ((rc = predictor_missing_cov_model(p, pairs))) return rc;
    if (!p->mtile) p->mtile = std::min<int64_t>(p->tile_rows, GPZ_PREDICTOR_TILE_MISSING);
    const size_t mtp = (size_t)rup(p->mtile, 1024);
    size_t rlmax = 0, nbmax = 0, slabmax = 0;   // over no = 0 .. d - 1
    for (int no = 0; no < p->d; ++no) {
        const size_t rl = (size_t)predict_missing_cov_rec(no);
        rlmax = std::max(rlmax, rl);
        nbmax = std::max(nbmax, (size_t)predict_missing_cov_bas(p->d, no));
        slabmax = std::max(slabmax, (size_t)predict_missing_cov_slab_pairs(p->m, no) * m * rl);
    }
    p->mchunks = predict_missing_cov_chunks(p->m);
    if (!p->mNo && (rc = ar.alloc(&p->mNo, mtp * mp))) return rc;
    if (!p->mPio && (rc = ar.alloc(&p->mPio, mtp * mp))) return rc;
    if (!p->mpri && (rc = ar.alloc(&p->mpri, m))) return rc;
    if (!p->mhd && (rc = ar.alloc(&p->mhd, 2 * k * mtp))) return rc;
    if (!p->mcbas && (rc = ar.alloc(&p->mcbas, m * nbmax))) return rc;
    if (!p->mcex && (rc = ar.alloc(&p->mcex, m * rlmax))) return rc;
    if (!p->mcphi && (rc = ar.alloc(&p->mcphi, m * m * rlmax))) return rc;
    if (pairs) {
        if (!p->mccoef && (rc = ar.alloc(&p->mccoef, npair * 3 * k))) return rc;
        if (!p->mcslab && (rc = ar.alloc(&p->mcslab, slabmax))) return rc;
        if (!p->mpart && (rc = ar.alloc(&p->mpart, (size_t)p->mchunks * 3 * k * mtp))) return rc;
        if (!p->mout && (rc = ar.alloc(&p->mout, 4 * k * mtp))) return rc;
    }
    p->mcov_used = true;
    const bool same_pri = priors ? (!p->mtab_uniform && p->mtab_pri.size() == m && std::equal(priors, priors + m, p->mtab_pri.begin()))
                                 : p->mtab_uniform;
    if (p->mtab_valid && p->mtab_obs == obs && same_pri && (p->mtab_pairs || !pairs)) return 0;
    p->mtab_valid = false;
    p->mcslab_kept = false;
    p->nmtab_valid = false;   // the records of k_predict_noisy_missing_cov.hip are made from these tables
    p->nmcslab_kept = false;
    p->mtab_uniform = priors == nullptr;
    if (priors) {   // the handle's own copy: the upload may still be in flight when the caller has its memory back
        p->mtab_pri.assign(priors, priors + m);
        if (hipMemcpyAsync(p->mpri, p->mtab_pri.data(), m * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
            return gpz_fail(GPZ_ERR_HIP, "%s: copy failed", who);
    }
    if (launch_pmcv_tables(st, p->m, p->d, p->de, p->k, obs, p->pr.P, p->mcSig, p->mclnS, priors ? p->mpri : nullptr, p->w_d,
                           p->hetero ? p->pr.v : nullptr, p->iS_d, p->mcbas, p->mcex, p->mcphi, pairs ? p->mccoef : nullptr))
        return gpz_fail(GPZ_ERR_HIP, "%s: table kernel launch failed", who);
    p->mtab_obs = obs;
    p->mtab_pairs = pairs;
    p->mtab_valid = true;
    return 0;
}

// Such a group whose rows have Psi too (ROWS_NOISY_MISSING_COV with something observed): the Psi slots, everything above (the tile
// buffers, [R | CU | off] and the coefficients of the pattern are shared, and the tables above stay valid for the entries that read
// them), and the Ex and PHI records and the slab in the form of k_predict_noisy_missing_cov.hip, sized for the widest pattern of the
// model and kept until the tables above are written again.
// A full Psi per row (ROWS_PSI_CUBE_MISSING) takes the cube kind's slots in place of the Psi slots and nothing else of its own: the
// records do not depend on Psi, so the two forms share nmcex, nmcphi, nmcslab and their flags.
static int predictor_noisy_missing_cov_prepare(gpz_predictor *p, const char *who, const Rows &r, bool pairs) {
    const size_t m = p->m;
    const uint32_t obs = r.obs;
    const double *priors = r.priors;
    int rc = 0;
    if ((rc = r.cube_obs() ? predictor_cube_slots(p) : predictor_psi_slots(p))) return rc;
    const bool had = p->mcov_used;   // (the route text of the entries without Psi is theirs)
    rc = predictor_missing_cov_prepare(p, who, obs, priors, pairs);
    p->mcov_used = had;
    if (rc) return rc;
    size_t rlmax = 0, slabmax = 0;   // over no = 1 .. d - 1
    for (int no = 1; no < p->d; ++no) {
        const size_t rl = (size_t)predict_noisy_missing_cov_rec(p->d, no);
        rlmax = std::max(rlmax, rl);
        slabmax = std::max(slabmax, (size_t)predict_noisy_missing_cov_slab_pairs(p->m, p->d, no) * m * rl);
    }
    if (!p->nmcex && (rc = p->ar.alloc(&p->nmcex, m * rlmax))) return rc;
    if (!p->nmcphi && (rc = p->ar.alloc(&p->nmcphi, m * m * rlmax))) return rc;
    if (pairs && !p->nmcslab && (rc = p->ar.alloc(&p->nmcslab, slabmax))) return rc;
    if (p->nmtab_valid) return 0;
    p->nmcslab_kept = false;
    if (launch_pnmc_tables(p->s_cmp, p->m, p->d, p->de, obs, p->pr.P, p->mcSig, p->mclnS, priors ? p->mpri : nullptr, p->mcbas, p->nmcex,
                           p->nmcphi))
        return gpz_fail(GPZ_ERR_HIP, "%s: table kernel launch failed", who);
    p->nmtab_valid = true;
    return 0;
}

// The two forms of Psi on a group of a covariance kind (Rows::group_psi()) differ on the host as NcovForm's do: in the tile's Psi slot
// (Psic in Xc's layout, or Psiq with the observed triangles), in the launchers of their four kernels (the same signatures:
// k_predict_noisy_missing_cov*.hip and k_predict_psi_cube_missing*.hip) and in the names the failure texts give those kernels
struct GroupPsiForm {
    double *const *Psi;
    decltype(&launch_pnmc_rows) rows;
    decltype(&launch_predict_noisy_missing_cov_pairs) pairs;
    decltype(&launch_predict_noisy_missing_cov_gamma) gamma;
    const char *rows_name, *name;     // rows_name, k_predict_<name>_pairs, _gamma
};
static GroupPsiForm group_psi_form(const gpz_predictor *p, const Rows &r) {
    if (r.kind == ROWS_PSI_CUBE_MISSING)
        return {p->Psiq, launch_pcm_rows, launch_predict_psi_cube_missing_pairs, launch_predict_psi_cube_missing_gamma, "k_pcm",
                "psi_cube_missing"};
    return {p->Psic, launch_pnmc_rows, launch_predict_noisy_missing_cov_pairs, launch_predict_noisy_missing_cov_gamma, "k_pnmc",
            "noisy_missing_cov"};
}

// predictMissing of one tile of nt rows of the group, covariance kinds: Xc[s] -> Pio in mPio ([m][tile]), PHI in mNo, mu | ElnS - b in mhd
// and, with pairs, mout ([4k][nt] = mu | nu | beta | gamma)
// A group with input noise too (predictNoisyMissing) runs its form's kernels on their own record tables with the form's Psi slot
static int predictor_missing_cov_tile(gpz_predictor *p, const char *who, const Rows &r, int s, int nt, bool pairs) {
    hipStream_t st = p->s_cmp;
    const int np = rup(nt, 128);   // the rows of the draws' product: k_tgemm's row tile
    const long mtp = rup(p->mtile, 1024);
    const uint32_t obs = r.obs;
    if (r.group_psi()) {
        const GroupPsiForm f = group_psi_form(p, r);
        if (f.rows(st, p->Xc[s], f.Psi[s], p->tile_pad, nt, np, p->m, p->mp, p->d, p->k, obs, p->nmcex, p->nmcphi, p->w_d,
                   p->hetero ? p->pr.v : nullptr, p->mPio, mtp, p->mNo, p->mhd, mtp))
            return gpz_fail(GPZ_ERR_HIP, "%s: %s launch failed", who, f.rows_name);
        if (pairs && f.pairs(st, p->Xc[s], f.Psi[s], p->tile_pad, nt, p->mPio, mtp, p->m, p->d, p->k, obs, p->mcraw, p->mcbas, p->mccoef,
                             p->nmcslab, &p->nmcslab_kept, p->mchunks, p->mpart, mtp, p->mhd, mtp, p->pr.b, p->mout))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_%s_pairs launch failed", who, f.name);
        return 0;
    }
    if (launch_pmcv_rows(st, p->Xc[s], p->tile_pad, nt, np, p->m, p->mp, p->d, p->k, obs, p->mcex, p->mcphi, p->w_d,
                         p->hetero ? p->pr.v : nullptr, p->mPio, mtp, p->mNo, p->mhd, mtp))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_pmcv launch failed", who);
    if (pairs && launch_predict_missing_cov_pairs(st, p->Xc[s], p->tile_pad, nt, p->mPio, mtp, p->m, p->d, p->k, obs, p->mcraw, p->mcbas,
                                                  p->mccoef, p->mcslab, &p->mcslab_kept, p->mchunks, p->mpart, mtp, p->mhd, mtp, p->pr.b,
                                                  p->mout))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_missing_cov_pairs launch failed", who);
    return 0;
}

// ---- what a kind of rows is made of ---------------------------------------------------------------------------------------------------
// the kind's refusal of the model and, for a group, of its mask.  draws: the call has draws, which with Psi need the fused draws route
int rows_check(const char *who, const gpz_predictor *p, const Rows &r, bool draws) {
    if (r.kind == ROWS_PSI_CUBE_MISSING && p->kind != GPZ_KIND_COV)
        return gpz_fail(GPZ_ERR_UNSUPPORTED,
                        "%s: method %.2s is a diagonal kind: fixPsi gives it the cube's diagonal, and its rows with input noise and "
                        "missing inputs go to gpz_predictor_run_noisy_missing_dev / _draws_noisy_missing_dev",
                        who, p->desc.method);
    if (r.group())   // (with Psi too: its product against W needs no fused draws route)
        return predictor_missing_check(who, p, r.obs, r.cov_group(), r.kind == ROWS_NOISY_MISSING_COV);
    if (r.kind == ROWS_CLEAN) return 0;
    if (r.ncov()) return predictor_noisy_cov_check(who, p);   // (its draws are a product on the T-GEMM: any route)
    if (int rc = predictor_noisy_check(who, p)) return rc;
    if (draws && p->force_tiles && !p->large_m)   // (with GPZ_PREDICT_LARGE_M: k_predict_noisy_phi + k_tgemm)
        return gpz_fail(GPZ_ERR_UNSUPPORTED, "%s: input noise needs the fused draws route (GPZ_PREDICT_FORCE_TILES is set)", who);
    return 0;
}

// What the call needs on the handle before its first tile.  pairs: it reads the kind's pair tables (the moments, gamma per draw, the
// stack); the draws alone do not, and take the Psi slots or the group's tables without them.
int rows_prepare(gpz_predictor *p, const char *who, const Rows &r, bool pairs) {
    if (r.cov_group()) {
        if (int rc = r.group_psi() ? predictor_noisy_missing_cov_prepare(p, who, r, pairs)
                                   : predictor_missing_cov_prepare(p, who, r.obs, r.priors, pairs))
            return rc;
        if (r.kind == ROWS_NOISY_MISSING_COV) p->nmcov_used = true;
        if (r.kind == ROWS_PSI_CUBE_MISSING) p->pcm_used = true;
        return 0;
    }
    if (r.group()) return predictor_missing_prepare(p, who, r.obs, r.priors, pairs, r.kind == ROWS_NOISY_MISSING);
    if ((r.kind == ROWS_NOISY || r.ncov()) && predictor_is_large(p)) p->large_seen = true;
    if (r.kind == ROWS_NOISY) return pairs ? predictor_noisy_prepare(p) : predictor_psi_slots(p);
    if (r.ncov()) {
        if (int rc = predictor_noisy_cov_prepare(p, r, pairs)) return rc;
        if (pairs) (r.cube() ? p->cube_used : p->ncov_used) = true;   // (two flags: the route text has a line for each form)
    }
    return 0;
}

// the rows per tile of a call that would take T: No, Pio and T of a group hold mtile rows; complete rows with Psi on a large model take
// at most the ntile rows of their chunk slab (predictor_noisy_slots; 0 before the first call that reads the pairs)
int64_t rows_tile(const gpz_predictor *p, const Rows &r, int64_t T) {
    if (r.group()) return std::min<int64_t>(T, p->mtile);
    return (r.kind == ROWS_NOISY || r.ncov()) && p->ntile ? std::min<int64_t>(T, p->ntile) : T;
}

// the moments of one tile of nt rows in slot s -> rows_moments: [3k][nt] = mu | nu | beta for clean rows (and PHI when asked), else
// [4k][nt] = mu | nu | beta | gamma
int rows_moments_tile(gpz_predictor *p, const char *who, const Rows &r, int s, int nt, bool want_phi) {
    if (r.cov_group()) return predictor_missing_cov_tile(p, who, r, s, nt, true);
    if (r.group()) return predictor_missing_tile(p, who, s, nt, r.obs, true, r.psi() ? p->Psic[s] : nullptr);
    if (r.kind == ROWS_NOISY) return predictor_noisy_tile(p, who, s, nt);
    if (r.ncov()) return predictor_noisy_cov_tile(p, who, r, s, nt);
    return predictor_tile(p, s, nt, want_phi);
}

const double *rows_moments(const gpz_predictor *p, const Rows &r, int s) {
    return r.group() ? p->mout : r.psi() || r.cube() ? p->nout[s] : p->out[s];
}

// the kind's tile for a call whose draws (or stack) would take *T rows, and for a group the output tile of its product PHI_missing W:
// the tile route of the draws has one already, the fused route does not
static int rows_fit_tile(gpz_predictor *p, const Rows &r, int ncol, int ldw, int64_t *T) {
    *T = rows_tile(p, r, *T);   // (ROWS_MISSING_COV is a group: its PHI_missing W takes the same output tile)
    if ((!r.group() && !r.ncov()) || ncol == 0) return 0;   // (a covariance kind with Psi: the output tile of E_x[PHI] W)
    if (r.ncov())   // (a call that reads the pairs too - gamma per draw, a stack with draws - has no PHI tile from rows_prepare)
        if (int rc = predictor_noisy_cov_phi_tile(p)) return rc;
    return predictor_grow(p, &p->Td, &p->t_cap, (size_t)rup(*T, 1024) * ldw);
}

// predictor_draws_prepare and the kind's tile
int rows_draws_prepare(gpz_predictor *p, const Rows &r, int nd, unsigned long long seed, const double *Z, bool pinned, int64_t *Tout) {
    if (int rc = predictor_draws_prepare(p, nd, seed, Z, pinned, Tout)) return rc;
    return rows_fit_tile(p, r, nd * p->k, rup(nd * p->k, 16), Tout);
}

// The draws of one tile of nt rows in slot s -> dout[s] ([ncol][nt], without muY).  after_moments: rows_moments_tile has just run on the
// same slot and rows, so PHI of the tile route (p->Phi) or of the group (mNo) is built already; else a group builds it here, without pairs.
int rows_draws_tile(gpz_predictor *p, const char *who, const Rows &r, int s, int nt, int ncol, int ldw, bool after_moments) {
    if (r.kind == ROWS_CLEAN) return predictor_draws_tile(p, s, nt, ncol, ldw, after_moments && p->route == 1);
    if (r.kind == ROWS_NOISY) return predictor_draws_tile(p, s, nt, ncol, ldw, false, p->Psic[s]);
    if (r.ncov()) return predictor_noisy_cov_draws_tile(p, who, r, s, nt, ncol, ldw);
    if (!after_moments)   // (a covariance kind's PHI_missing lies in mNo as the diagonal kinds' does)
        if (int rc = r.cov_group() ? predictor_missing_cov_tile(p, who, r, s, nt, false)
                                   : predictor_missing_tile(p, who, s, nt, r.obs, false, r.psi() ? p->Psic[s] : nullptr))
            return rc;
    return predictor_missing_draws_tile(p, who, s, nt, ncol, ldw);
}

int rows_chunks(const gpz_predictor *p, const Rows &r) { return r.group() ? p->mchunks : p->gchunks; }

// What a call that needs gamma under nd draws on tiles of T rows adds to the handle (after rows_prepare with pairs: the pair table, or U
// and the records): the chunk slab of the pair sums and, for a stack of Q column-outputs, the kind's widths.  nd = 0 takes no slab.
int rows_gamma_prepare(gpz_predictor *p, const Rows &r, int ncol, int Q, int64_t T) {
    gpz_predictor::PerDraw &g = p->gam[r.kind - 1];
    int rc = 0;
    if (r.kind == ROWS_NOISY || r.ncov()) p->gchunks = predict_gamma_chunks(p->m);   // (a handle has one of the two kinds)
    if (ncol > 0 && (rc = predictor_grow(p, &p->gpart, &p->gpart_cap, (size_t)rows_chunks(p, r) * ncol * T))) return rc;
    if (Q > 0 && (rc = predictor_grow(p, &g.s2_d, &g.s2_cap, (size_t)Q * T))) return rc;
    g.used = true;
    return 0;
}

// the pair sums under every draw of one tile of nt rows (a group: after predictor_missing_tile, mPio): -> gpart ([chunks][ncol][nt])
int rows_gamma_tile(gpz_predictor *p, const char *who, const Rows &r, int s, int nt, int ncol, int ldw) {
    if (r.ncov()) {   // the head of the packed pair records, read with the table's stride; Psi in the form's slot
        const NcovForm f = ncov_form(p, r);
        if (f.gamma(p->s_cmp, p->d, p->mid == 4, p->Xc[s], f.Psi[s], p->tile_pad, nt, p->m, p->cprec, predict_noisy_cov_prec(p->d, p->k),
                    p->Wd, ldw, ncol, p->gchunks, p->gpart, nt))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_%s_gamma launch failed", who, f.name);
        return 0;
    }
    if (r.cov_group()) {   // the slab of the pattern's pair records: kept, or written here as the pair kernel writes it.  With Psi: the
        // form's own records and slab; with nothing observed there is no Psi to read and the group runs the kernel without Psi
        const long mtp = rup(p->mtile, 1024);
        if (r.group_psi()) {
            const GroupPsiForm g = group_psi_form(p, r);
            if (g.gamma(p->s_cmp, p->Xc[s], g.Psi[s], p->tile_pad, nt, p->mPio, mtp, p->m, p->d, r.obs, p->mcraw, p->mcbas,
                        p->nmcslab, &p->nmcslab_kept, p->Wd, ldw, ncol, p->mchunks, p->gpart, nt))
                return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_%s_gamma launch failed", who, g.name);
            return 0;
        }
        if (launch_predict_missing_cov_gamma(p->s_cmp, p->Xc[s], p->tile_pad, nt, p->mPio, mtp, p->m, p->d, r.obs, p->mcraw, p->mcbas,
                                             p->mcslab, &p->mcslab_kept, p->Wd, ldw, ncol, p->mchunks, p->gpart, nt))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_%s_gamma launch failed", who,   // (a group of the two Psi kinds with nothing observed
                            r.kind == ROWS_MISSING_COV ? "missing_cov" : group_psi_form(p, r).name);   //  keeps its own kind's name)
        return 0;
    }
    if (r.group() && predictor_missing_is_large(p)) {   // a group with Psi: the second record table
        if (launch_predict_missing_large_gamma(p->s_cmp, p->Xc[s], r.psi() ? p->Psic[s] : nullptr, p->tile_pad, nt, p->mPio, p->mp, p->m,
                                               p->d, p->k, r.obs, p->mU, r.psi() ? p->nmrec : p->mrec, p->Wd, ldw, ncol, p->mchunks,
                                               p->gpart, nt))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_pml_gamma%s launch failed", who, r.psi() ? "_psi" : "");
        return 0;
    }
    // a group with Psi: the second record table
    if (r.kind == ROWS_NOISY
            ? launch_predict_noisy_gamma(p->s_cmp, p->d, p->Xc[s], p->Psic[s], p->tile_pad, nt, p->m, p->ptab, p->nrec, p->Wd, ldw, ncol,
                                         p->gchunks, p->gpart, nt)
            : launch_predict_missing_gamma(p->s_cmp, p->Xc[s], r.psi() ? p->Psic[s] : nullptr, p->tile_pad, nt, p->mPio, p->mp, p->m, p->d,
                                           p->k, r.obs, p->mU, r.psi() ? p->nmrec : p->mrec, p->Wd, ldw, ncol, p->mchunks, p->gpart, nt))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_%s_gamma launch failed", who,
                        r.kind == ROWS_NOISY ? "noisy" : r.kind == ROWS_MISSING ? "missing" : "noisy_missing");
    return 0;
}

// ---- stack ------------------------------------------------------------------------------------------------------------------------
// Per tile: rows, labels and weights up; predictor_tile (mu, nu, beta stay in out[s]); with draws, their kernels (F stays in dout[s]);
// k_stack_tile writes the tile's row slabs and k_stack_accum adds them to the running accumulators, all on the compute stream, so the
// tiles add in their order.  Nothing comes back before the accumulators at the end.  Both kernels run on the draws tile, so that out[s]
// and dout[s] describe the same rows.  res: (1 + nd) k records of G B + 3 G doubles (k_predict_stack.hip).
// For rows with Psi or a group with missing inputs the moments are [4k][nt] with gamma, the pair sums under every draw follow the draws,
// and the stack kernel reads a width per (column, row): column 0 (nu + beta) + gamma, draw s beta + max(gamma_s, 0) (k_gamma_finish_s2).
//
// What a stack call does before its first tile (after rows_prepare with pairs): with draws, what they need; the label and weight slots of
// the host entry (pinned); the edges, accumulators and slabs; the kind's tile (a group's is at most mtile rows; the slabs allocated for
// the call's own tile hold its fewer slabs) and what gamma under every draw needs; then the edges and shifts go up and the accumulators
// are cleared.  Once this has been called the entry leaves through its stream synchronisation, failed or not: copies from the caller's
// memory may be in flight.
int predictor_stack_prepare(gpz_predictor *p, const char *who, const Rows &r, const StackArgs &a, bool pinned, StackCall *c) {
    const int k = p->k, nd = a.ndraws, B = a.nbins, G = a.ngroups, Q = (1 + nd) * k;
    const size_t tp = (size_t)p->tile_pad, rec = (size_t)G * B + 3 * (size_t)G;
    hipStream_t st = p->s_cmp;
    int rc = 0;
    int64_t T = p->tile_rows;
    if (nd > 0 && (rc = predictor_draws_prepare(p, nd, (unsigned long long)a.seed, a.Z, false, &T))) return rc;
    for (int s = 0; s < 2 && pinned; ++s) {   // each one where it is missing: a call that failed half-way here leaves the next one its rest
        if (!p->lab_d[s] && (rc = p->ar.alloc(&p->lab_d[s], tp))) return rc;
        if (!p->wt_d[s] && (rc = p->ar.alloc(&p->wt_d[s], tp))) return rc;
        if (!p->hlab[s]) HIPCHK(hipHostMalloc((void **)&p->hlab[s], tp * sizeof(int), hipHostMallocDefault));
        if (!p->hwt[s]) HIPCHK(hipHostMalloc((void **)&p->hwt[s], tp * sizeof(double), hipHostMallocDefault));
    }
    *c = StackCall{nd, B, G, nd * k, rup(nd * k, 16), predict_stack_slabs(Q, (long)rec, T), (size_t)k * (B + 1), (size_t)Q * rec, T};
    if ((rc = predictor_grow(p, &p->edges_d, &p->edges_cap, c->ne + k))) return rc;
    if ((rc = predictor_grow(p, &p->acc_d, &p->acc_cap, c->count))) return rc;
    if ((rc = predictor_grow(p, &p->slab_d, &p->slab_cap, c->count * c->R))) return rc;
    if ((rc = rows_fit_tile(p, r, c->ncol, c->ldw, &c->T))) return rc;
    c->R = predict_stack_slabs(Q, (long)rec, c->T);   // <= the slabs that were allocated
    p->stile = c->T;   // (the route text prints them)
    p->sslabs = c->R;
    if (r.kind != ROWS_CLEAN && (rc = rows_gamma_prepare(p, r, c->ncol, Q, c->T))) return rc;
    if (hipMemcpyAsync(p->edges_d, a.edges, c->ne * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
        (a.mu_shift ? hipMemcpyAsync(p->edges_d + c->ne, a.mu_shift, (size_t)k * sizeof(double), hipMemcpyHostToDevice, st)
                    : hipMemsetAsync(p->edges_d + c->ne, 0, (size_t)k * sizeof(double), st)) != hipSuccess ||
        hipMemsetAsync(p->acc_d, 0, c->count * sizeof(double), st) != hipSuccess)
        return gpz_fail(GPZ_ERR_HIP, "%s: copy failed", who);
    return 0;
}

// the kernels of one stack tile of nt rows in slot s; lab, wt: the tile's labels and weights on the device (nullptr: one group, weight 1)
int predictor_stack_tile(gpz_predictor *p, const char *who, const Rows &r, const StackCall &c, int s, int64_t nt, const int *lab,
                         const double *wt) {
    hipStream_t st = p->s_cmp;
    const double *mom = rows_moments(p, r, s), *F = c.nd > 0 ? p->dout[s] : nullptr, *sh = p->edges_d + c.ne;
    int rc = 0, bad = 0;
    if ((rc = rows_moments_tile(p, who, r, s, (int)nt, false))) return rc;
    if (c.nd > 0 && (rc = rows_draws_tile(p, who, r, s, (int)nt, c.ncol, c.ldw, true))) return rc;
    if (r.kind == ROWS_CLEAN) {
        bad = launch_stack_tile(st, mom, F, lab, wt, p->edges_d, sh, nt, p->k, c.nd, c.B, c.G, c.R, p->slab_d);
    } else {
        double *s2 = p->gam[r.kind - 1].s2_d;
        if (c.nd > 0 && (rc = rows_gamma_tile(p, who, r, s, (int)nt, c.ncol, c.ldw))) return rc;
        if (launch_gamma_finish_s2(st, p->gpart, rows_chunks(p, r), nt, mom, F, (int)nt, p->k, c.nd, s2))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_gamma_finish_s2 launch failed", who);
        bad = launch_stack_tile_w(st, mom, s2, F, lab, wt, p->edges_d, sh, nt, p->k, c.nd, c.B, c.G, c.R, p->slab_d);
    }
    if (bad || launch_stack_accum(st, p->slab_d, c.R, c.count, p->acc_d))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_stack_tile%s launch failed", who, r.kind == ROWS_CLEAN ? "" : "_w");
    return 0;
}

// the accumulators come home behind the last tile
int predictor_stack_result(gpz_predictor *p, const char *who, const StackCall &c, double *res) {
    if (hipMemcpyAsync(res, p->acc_d, c.count * sizeof(double), hipMemcpyDeviceToHost, p->s_cmp) != hipSuccess)
        return gpz_fail(GPZ_ERR_HIP, "%s: copy failed", who);
    return 0;
}

// ---- what the entries share ---------------------------------------------------------------------------------------------------------
int predictor_check_call(const char *who, const gpz_predictor *p, int64_t ns) {
    if (!p) return gpz_fail(GPZ_ERR_ARG, "%s: null handle", who);
    if (ns < 0) return gpz_fail(GPZ_ERR_ARG, "%s: ns < 0", who);
    return 0;
}

// least: 1 for the draws; 0 for the stack, whose column 0 is the posterior mean
int predictor_check_ndraws(const char *who, const gpz_predictor *p, int32_t ndraws, int least) {
    if (ndraws < least || (1 - least + (int64_t)ndraws) * p->k > GPZ_DRAWS_MAX_COLUMNS)
        return gpz_fail(GPZ_ERR_ARG, "%s: need %d <= ndraws and %s * k <= %d (ndraws %d, k %d)", who, least,
                        least ? "ndraws" : "(1 + ndraws)", GPZ_DRAWS_MAX_COLUMNS, (int)ndraws, p->k);
    return 0;
}

// the shape checks of a stack call, in the order gpz_predictor_stack has always made them (who: the entry's name in the message)
int stack_check_shape(const char *who, const gpz_predictor *p, int64_t ns, const StackArgs &a, const void *Xs) {
    const int32_t nbins = a.nbins, ngroups = a.ngroups;
    const double *edges = a.edges;
    if (int rc = predictor_check_call(who, p, ns)) return rc;
    if (int rc = predictor_check_ndraws(who, p, a.ndraws, 0)) return rc;
    if (nbins < 1 || ngroups < 1) return gpz_fail(GPZ_ERR_ARG, "%s: need nbins >= 1 and ngroups >= 1", who);
    if ((int64_t)nbins * ngroups > GPZ_STACK_MAX_GROUP_BINS)
        return gpz_fail(GPZ_ERR_ARG, "%s: ngroups * nbins = %lld is over GPZ_STACK_MAX_GROUP_BINS = %d", who, (long long)nbins * ngroups,
                        GPZ_STACK_MAX_GROUP_BINS);
    const int k = p->k, B = nbins;
    if (!edges || !a.hist || !a.sum_w || !a.sum_mu || !a.sum_mu2) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    for (int o = 0; o < k; ++o)
        for (int j = 0; j <= B; ++j) {
            const double e = edges[(size_t)o * (B + 1) + j];
            if (!std::isfinite(e) || (j > 0 && !(e > edges[(size_t)o * (B + 1) + j - 1])))
                return gpz_fail(GPZ_ERR_ARG, "%s: the edges must be finite and strictly increasing (output %d, edge %d)", who, o, j);
        }
    if (ns > 0 && !Xs) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    return 0;
}

// records [c][o][G B + 3 G] -> hist [c][g][o][B], sums [c][g][o]; the sum of the weights is the same in every record
void stack_unpack(const gpz_predictor *p, const StackArgs &a, const double *res) {
    const int C = 1 + a.ndraws, k = p->k, G = a.ngroups, B = a.nbins;
    const size_t GB = (size_t)G * B, rec = GB + 3 * (size_t)G;
    for (int c = 0; c < C; ++c)
        for (int o = 0; o < k; ++o) {
            const double *r = res + ((size_t)c * k + o) * rec;
            for (int g = 0; g < G; ++g) {
                const size_t at = ((size_t)c * G + g) * k + o;
                memcpy(a.hist + at * B, r + (size_t)g * B, (size_t)B * sizeof(double));
                a.sum_mu[at] = r[GB + 3 * (size_t)g + 1];
                a.sum_mu2[at] = r[GB + 3 * (size_t)g + 2];
                if (c == 0 && o == 0) a.sum_w[g] = r[GB + 3 * (size_t)g];
            }
        }
}

void stack_zero(const gpz_predictor *p, const StackArgs &a) {
    const size_t Q = (size_t)(1 + a.ndraws) * p->k, G = a.ngroups;
    memset(a.hist, 0, Q * G * a.nbins * sizeof(double));
    memset(a.sum_w, 0, G * sizeof(double));
    memset(a.sum_mu, 0, Q * G * sizeof(double));
    memset(a.sum_mu2, 0, Q * G * sizeof(double));
}

int stack_check_shift(const char *who, const gpz_predictor *p, const double *mu_shift) {
    for (int o = 0; mu_shift && o < p->k; ++o)
        if (!std::isfinite(mu_shift[o])) return gpz_fail(GPZ_ERR_ARG, "%s: mu_shift must be finite", who);
    return 0;
}
}   // namespace gpzi

extern "C" int gpz_predictor_create(const gpz_desc *desc, const double *theta, const double *w, const double *iSigma_w,
                                    int64_t tile_rows, int32_t flags, gpz_predictor **out) {
    if (!out) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_create: null argument");
    *out = nullptr;
    if (!desc || !theta || !w || !iSigma_w) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_create: null argument");
    if (desc->dtype != GPZ_F64) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_create: fp64 only");
    if (flags & ~(GPZ_PREDICT_FORCE_TILES | GPZ_PREDICT_LARGE_M) & ~GPZ_PREDICT_LARGE_M_MISSING) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_create: unknown flags %d", (int)flags);
    gpz_predictor *p = new gpz_predictor();
    p->desc = *desc;
    p->desc.world = 1;
    p->desc.rank = 0;
    p->mid = method_id_of(desc->method);
    if (p->mid < 0) { delete p; return gpz_fail(GPZ_ERR_ARG, "unknown method '%.2s'", desc->method); }
    if (desc->d < 1 || desc->m < 1 || desc->k < 1) { delete p; return gpz_fail(GPZ_ERR_ARG, "d, m, k must be >= 1"); }
    p->kind = p->mid >= 4 ? GPZ_KIND_COV : GPZ_KIND_DIAG;
    p->d = desc->d;
    p->de = pad_dim(desc->d);
    p->m = desc->m;
    p->k = desc->k;
    p->hetero = desc->heteroscedastic ? 1 : 0;
    p->p = (long)p->m * p->d + g_dim_of(p->mid, p->m, p->d) + (long)p->m * p->k + p->k + (p->hetero ? 2L * p->m * p->k : 0);
    p->mp = rup(p->m + p->k, 16);
    p->device = desc->device;
    int prev = 0;
    (void)hipGetDevice(&prev);
    gpz_opts_scope opts_scope(&p->opt);
    int rc = predictor_setup(p, theta, w, iSigma_w, tile_rows, flags);
    if (rc) predictor_free(p);
    else *out = p;
    (void)hipSetDevice(prev);
    return rc;
}

extern "C" void gpz_predictor_destroy(gpz_predictor *p) {
    if (!p) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    predictor_free(p);
    (void)hipSetDevice(prev);
}

extern "C" int gpz_predictor_route(const gpz_predictor *p, char *buf, int cap) {
    if (!p || !buf || cap < 1) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_route: null argument");
    char tmp[160];
    if (p->route == 0)
        snprintf(tmp, sizeof tmp, "fused: k_predict_small, %lld-row tiles", (long long)p->tile_rows);
    else
        snprintf(tmp, sizeof tmp, "tiles: k_phi + k_tgemm, %lld-row tiles", (long long)p->tile_rows);
    std::string r = tmp;
    // after the first stack or gamma-per-draw call for a kind of rows (gam[kind - 1]): its kernel and chunks (a group's: mchunks)
    static const struct { const char *fmt; bool group; } PER_DRAW[8] = {
        {"; noise per draw: k_predict_noisy_gamma (%d pair chunks)", false},
        {"; missing per draw: k_predict_missing_gamma (%d pair chunks)", true},
        {"; noisy missing per draw: k_predict_noisy_missing_gamma (%d pair chunks)", true},
        {"; noise per draw: k_predict_noisy_cov_gamma (%d pair chunks)", false},
        {"; missing per draw: k_predict_missing_cov_gamma (%d pair chunks)", true},
        {"; noisy missing per draw: k_predict_noisy_missing_cov_gamma (%d pair chunks)", true},
        {"; noise cube per draw: k_predict_psi_cube_gamma (%d pair chunks)", false},
        {"; noise cube missing per draw: k_predict_psi_cube_missing_gamma (%d pair chunks)", true}};
    auto gamma_line = [&](int i) {
        const gpz_predictor::PerDraw &g = p->gam[i];
        if (!g.used) return;
        if (p->mlarge_seen && (i == 1 || i == 2))   // a diagonal kind's group past 256: the panelled kernels
            snprintf(tmp, sizeof tmp, i == 1 ? "; missing per draw: k_pml_gamma (%d pair chunks)" : "; noisy missing per draw: k_pml_gamma_psi (%d pair chunks)",
                     p->mchunks);
        else
            snprintf(tmp, sizeof tmp, PER_DRAW[i].fmt, PER_DRAW[i].group ? p->mchunks : p->gchunks);
        r += tmp;
        if (g.s2_d) r += " + k_stack_tile_w";   // the widths exist: a stack call was among them
    };
    if (p->droute >= 0) {   // after a draws call: its route and each output's factor
        snprintf(tmp, sizeof tmp, "; draws: %s, %lld-row tiles, factors:", p->droute == 0 ? "fused k_predict_draws" : "tiles k_phi + k_tgemm",
                 (long long)p->dtile);
        r += tmp;
        for (size_t o = 0; o < p->fkind.size(); ++o) r += p->fkind[o] ? " eigen" : " cholesky";
    }
    if (p->stile > 0) {   // after a stack call
        snprintf(tmp, sizeof tmp, "; stack: k_stack_tile + k_stack_accum, %lld-row tiles, %d row slabs", (long long)p->stile, p->sslabs);
        r += tmp;
    }
    if (p->dev_used) r += "; device entries: k_pred_stage";
    if (p->noisy_ready) {   // after the first call with input noise on the handle
        snprintf(tmp, sizeof tmp, "; noise: k_predict_noisy_small (%d pair chunks)", p->nchunks);
        r += tmp;
    }
    if (p->ncov_used) {   // after the first call with input noise on a covariance kind that reads the pairs
        snprintf(tmp, sizeof tmp, "; noise: k_predict_noisy_cov_small (%d pair chunks)", p->cchunks);
        r += tmp;
    }
    gamma_line(3);
    if (p->cube_used) {   // after the first call with a full Psi per row that reads the pairs
        snprintf(tmp, sizeof tmp, "; noise cube: k_predict_psi_cube_small (%d pair chunks)", p->cchunks);
        r += tmp;
    }
    gamma_line(6);
    gamma_line(0);
    if (p->large_seen) {   // a handle with GPZ_PREDICT_LARGE_M past ceil16(m) = 256, after its first call with Psi
        snprintf(tmp, sizeof tmp, "; noisy large-m: tiles, %d chunks", predict_noisy_chunks(p->m, p->d, p->k));
        r += tmp;
    }
    if (p->mlarge_seen) {   // a handle with GPZ_PREDICT_LARGE_M_MISSING past ceil16(m) = 256, after its first call for a group: the kernels
        snprintf(tmp, sizeof tmp, "; missing past 256: k_pml_pairs / k_pml_gamma (K panels of %d, %d groups per batch)", GPZ_PML_KP,   // behind
                 p->k == 1 ? GPZ_PML_GB : GPZ_PML_GB8);                                                                          // the lines below
        r += tmp;
    }
    if (p->miss_used) {   // after the first call for a group of rows with missing inputs
        snprintf(tmp, sizeof tmp, "; missing: %s (%d pair chunks), %lld-row tiles", p->mlarge_seen ? "k_pml_pairs" : "k_predict_missing_pairs",
                 p->mchunks, (long long)p->mtile);
        r += tmp;
    }
    if (p->mcov_used) {   // after the first call for a group of rows with missing inputs on a covariance kind
        snprintf(tmp, sizeof tmp, "; missing: k_predict_missing_cov_pairs (%d pair chunks)", p->mchunks);
        r += tmp;
    }
    gamma_line(4);
    gamma_line(1);
    if (p->nm_used) {   // after the first call for a group of rows with input noise and missing inputs
        snprintf(tmp, sizeof tmp, "; noisy missing: %s (%d pair chunks)", p->mlarge_seen ? "k_pml_pairs_psi" : "k_predict_noisy_missing_pairs",
                 p->mchunks);
        r += tmp;
    }
    gamma_line(2);
    if (p->nmcov_used) {   // after the first call for such a group on a covariance kind
        snprintf(tmp, sizeof tmp, "; noisy missing: k_predict_noisy_missing_cov_pairs (%d pair chunks)", p->mchunks);
        r += tmp;
    }
    gamma_line(5);
    if (p->pcm_used) {   // after the first call for such a group with a full Psi per row
        snprintf(tmp, sizeof tmp, "; noise cube missing: k_predict_psi_cube_missing_pairs (%d pair chunks)", p->mchunks);
        r += tmp;
    }
    gamma_line(7);
    snprintf(buf, (size_t)cap, "%s", r.c_str());
    return (int)r.size();
}

extern "C" int gpz_predictor_info(const gpz_predictor *p, int64_t out[4]) {
    if (!p || !out) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_info: null argument");
    out[0] = p->tile_rows;
    out[1] = (int64_t)p->ar.bytes;
    out[2] = p->route;
    out[3] = p->runs;
    return 0;
}
