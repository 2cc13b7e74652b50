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
// gpz_predictor_stack_noisy / _stack_noisy_dev stack such rows: per tile predictNoisy, the draws with Psi, gamma under every draw
// (k_predict_noisy_gamma.hip, an f64 MFMA product of pair densities and weight products), and k_stack_tile_w with a width per (column,
// row); gpz_predictor_draws_gamma_noisy_dev returns that gamma beside the draws.  Their buffers are allocated on their first call.
// gpz_predictor_stack_missing_dev stacks one group of rows with missing inputs in the same way, with gamma under every draw from
// k_predict_missing_gamma.hip (the pair kernel's product chained into a second f64 MFMA against the weight products);
// gpz_predictor_draws_gamma_missing_dev returns that gamma beside the draws.  Their buffers are allocated on their first call.
// Rows with missing inputs, one group of a NaN pattern per call, stay on the handle too where predict_missing_fits holds (the same
// shapes): gpz_predictor_run_missing_dev / _draws_missing_dev run predictMissing on tiles of at most GPZ_PREDICTOR_TILE_MISSING rows
// (k_predict_missing.hip): No and Pio, PHI through k_tgemm, then the fused pair kernel, or for the draws k_tgemm against W.  The tables
// of a pattern (NijS, the pair records, U) are kept until the pattern or the priors change; all of it is allocated on the first such call.
#include <string>

#include "gpz_ctx.h"

#define GPZ_PREDICTOR_TILE_FUSED (1L << 17)   // default rows per tile, fused route: 4096 blocks of 32 rows = 8 rounds of 512 workgroups
#define GPZ_PREDICTOR_TILE_MISSING (1L << 14) // most rows per tile of a group with missing inputs: No, Pio and T are [tile][mp] each

struct gpz_predictor {
    gpz_desc desc;
    gpz_options opt = gpz_options_load();
    int mid = 0, kind = 0, d = 0, de = 0, m = 0, k = 1, hetero = 0, mp = 0;
    long p = 0;
    int device = 0;
    int route = 0;                 // 0 fused, 1 tiles
    bool force_tiles = false;      // GPZ_PREDICT_FORCE_TILES
    int64_t tile_rows = 0, tile_pad = 0, runs = 0;
    int nk = 0, ldb = 0;           // fused: B_o is nk x ldb
    int nslots = 0;                // tiles: nu partial slots per output
    Arena ar;
    hipStream_t s_in = nullptr, s_cmp = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = {}, ev_cmp[2] = {}, ev_out[2] = {};
    double *theta_d = nullptr, *iS_d = nullptr, *w_d = nullptr, *prep_ws = nullptr;
    GpzParams pr{};
    double *B = nullptr;           // fused: k x [nk][ldb];  tiles: k x [mp][mp]
    double *Xc[2] = {}, *out[2] = {}, *phi_d[2] = {};
    double *Phi = nullptr, *T = nullptr, *nupart = nullptr, *phiw = nullptr, *lnbeta = nullptr;   // tiles
    double *hin[2] = {}, *hout[2] = {}, *hphi[2] = {};   // pinned
    std::vector<double> theta_h, w_h, iS_h;              // the model, for the input-noise branch (gpz_predict_noisy per tile)
    // ---- draws (gpz_predictor_draws): nothing of this exists before the first draws call
    int droute = -1;               // -1 no draws call yet, 0 fused (k_predict_draws), 1 tiles (k_phi + k_tgemm)
    std::vector<int> fkind;        // per output: 0 Cholesky, 1 eigendecomposition
    double *R = nullptr;           // m x m x k column-major: R_o R_o' = S_o
    double *Wd = nullptr, *Zd = nullptr, *Td = nullptr, *dout[2] = {}, *hdout[2] = {};
    size_t w_cap = 0, z_cap = 0, t_cap = 0, dout_cap = 0, hdout_cap = 0;   // doubles
    int64_t dtile = 0;             // rows per draws tile (last call)
    bool w_seeded = false;         // Wd holds the draws of (w_seed, w_nd)
    unsigned long long w_seed = 0;
    int w_nd = 0;
    // ---- stack (gpz_predictor_stack): nothing of this exists before the first stack call
    int *lab_d[2] = {}, *hlab[2] = {};      // the tile's labels: device, pinned
    double *wt_d[2] = {}, *hwt[2] = {};     // the tile's weights
    double *edges_d = nullptr, *acc_d = nullptr, *slab_d = nullptr;
    size_t edges_cap = 0, acc_cap = 0, slab_cap = 0;   // doubles
    int64_t stile = 0;             // rows per stack tile (last call; 0: no stack call yet)
    int sslabs = 0;                // row slabs per tile (last call)
    // ---- device-resident entries: nothing of this exists before the first of their calls
    double *par_d = nullptr;       // [muX d | sdX d | muY k | the record of k_pred_check_dev, 4 words]
    hipEvent_t ev_dev = nullptr;   // recorded on the caller's stream, waited for by s_cmp
    bool dev_used = false;
    // ---- input noise on the handle (gpz_predictor_*_noisy*): nothing of this exists before the first of their calls
    bool noisy_ready = false;
    int nchunks = 0, nrec = 0;     // predict_noisy_chunks, predict_noisy_rec of the model
    double *ptab = nullptr;        // m (m + 1) / 2 pair records
    double *Psic[2] = {}, *nout[2] = {}, *npart = nullptr;   // Psi in the layout of Xc; [4k][tile_pad]; [nchunks][5k][tile_pad]
    double *sd2_d = nullptr;       // sdX ** 2 of the device entries
    double *hpsi[2] = {};          // pinned, gpz_predictor_draws_noisy only
    // ---- gamma per draw and stacks of rows with input noise (gpz_predictor_stack_noisy*, _draws_gamma_noisy_dev): nothing before their first call
    bool gam_used = false;
    int gchunks = 0;               // predict_gamma_chunks of the model
    double *gpart = nullptr, *s2_d = nullptr;   // [gchunks][nd k][tile] pair sums per chunk; [(1 + nd) k][tile] widths^2 of the stack
    size_t gpart_cap = 0, s2_cap = 0;           // doubles
    // ---- gamma per draw and stacks of rows with missing inputs (gpz_predictor_stack_missing_dev, _draws_gamma_missing_dev): nothing before
    // their first call.  The chunk slab of the pair sums is gpart above ([mchunks][nd k][tile] here).
    bool mgam_used = false;
    double *ms2_d = nullptr;       // [(1 + nd) k][tile] widths^2 of the stack
    size_t ms2_cap = 0;            // doubles
    // ---- rows with missing inputs on the handle (gpz_predictor_*_missing_dev): nothing of this exists before the first of their calls
    bool miss_used = false;
    int64_t mtile = 0;             // rows per tile of a group: min(tile_rows, GPZ_PREDICTOR_TILE_MISSING)
    int mchunks = 0;               // predict_missing_chunks of the model
    double *mNo = nullptr, *mPio = nullptr, *mT = nullptr;   // [rup(mtile, 1024)][mp]: No (then PHI), Pio, T = Pio NijS
    double *mbt = nullptr, *mNij = nullptr, *mpri = nullptr, *mhd = nullptr;   // [2][mp]; [mp][mp]; the priors; [2k][rup(mtile, 1024)]
    double *mU = nullptr, *mrec = nullptr, *mpart = nullptr, *mout = nullptr;  // the pair tables, chunk slab and [4k] outputs (not for draws)
    bool mtab_valid = false, mtab_pairs = false, mtab_uniform = false;         // the tables hold (mtab_obs, mtab_pri); U and records too
    unsigned mtab_obs = 0;
    std::vector<double> mtab_pri;
};

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
static int predictor_want_phi(gpz_predictor *p, bool pinned = true) {
    const size_t n = (size_t)p->m * p->tile_pad;
    for (int s = 0; s < 2; ++s) {
        if (!p->phi_d[s])
            if (int rc = p->ar.alloc(&p->phi_d[s], n)) return rc;
        if (pinned && !p->hphi[s]) HIPCHK(hipHostMalloc((void **)&p->hphi[s], n * sizeof(double), hipHostMallocDefault));
    }
    return 0;
}

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
    int kernels(int s, int64_t nt) { return predictor_tile(p, s, (int)nt, PHI != nullptr); }
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

// ---- input noise on the handle ----------------------------------------------------------------------------------------------------
static int predictor_noisy_check(const char *who, const gpz_predictor *p) {
    if (!predict_noisy_fits(p->kind, p->de, p->m, p->k))
        return gpz_fail(GPZ_ERR_UNSUPPORTED,
                        "%s: input noise on the handle needs predict_noisy_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, k <= 8 and "
                        "ceil16(m) <= 256 (method %.2s, d %d, m %d, k %d); gpz_predictor_run takes Psi for every shape",
                        who, p->desc.method, p->d, p->m, p->k);
    return 0;
}

// What every call with Psi needs, the draws included: Psic[2] and sd2.  Each one where it is missing.
static int predictor_psi_slots(gpz_predictor *p) {
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

// What the first predictNoisy call adds to the handle beyond that: the pair table [lnZ | c_ab | C_ab | coefficients] (the model's alone:
// launch_pair_table needs only pr.P and pr.G for a diagonal kind), the 4k-row output slots and the chunk slab.  The draws read none of
// these and do not come here.
static int predictor_noisy_prepare(gpz_predictor *p) {
    if (p->noisy_ready) return 0;
    const size_t m = p->m, k = p->k, tp = (size_t)p->tile_pad, npair = m * (m + 1) / 2;
    hipStream_t st = p->s_cmp;
    auto &ar = p->ar;
    int rc = 0;
    if ((rc = predictor_psi_slots(p))) return rc;
    p->nchunks = predict_noisy_chunks(p->m, p->d, p->k);
    p->nrec = predict_noisy_rec(p->d, p->k);
    if (!p->ptab && (rc = ar.alloc(&p->ptab, npair * p->nrec))) return rc;
    for (int s = 0; s < 2; ++s)
        if (!p->nout[s] && (rc = ar.alloc(&p->nout[s], 4 * k * tp))) return rc;
    if (!p->npart && (rc = ar.alloc(&p->npart, (size_t)p->nchunks * 5 * k * tp))) return rc;
    launch_pair_table(st, GPZ_KIND_DIAG, p->m, p->d, p->de, p->pr.P, p->pr.G, nullptr, nullptr, p->ptab, p->nrec, nullptr);
    if (hipGetLastError() != hipSuccess ||
        launch_noisy_pair_coef(st, p->m, p->k, p->d, p->w_d, p->hetero ? p->pr.v : nullptr, p->iS_d, p->ptab, p->nrec))
        return gpz_fail(GPZ_ERR_HIP, "gpz_predictor: pair table launch failed");
    HIPCHK(hipStreamSynchronize(st));
    p->noisy_ready = true;
    return 0;
}

// predictNoisy of one tile of nt rows: Xc[s], Psic[s] -> nout[s] ([4k][nt] = mu | nu | beta | gamma)
static int predictor_noisy_tile(gpz_predictor *p, int s, int nt) {
    if (launch_predict_noisy_small(p->s_cmp, p->d, p->de, p->Xc[s], p->Psic[s], p->tile_pad, nt, p->m, p->k, p->pr.P, p->pr.G2, p->w_d,
                                   p->hetero ? p->pr.v : nullptr, p->pr.b, p->ptab, p->nchunks, p->npart, p->tile_pad, p->nout[s]))
        return gpz_fail(GPZ_ERR_HIP, "gpz_predictor_run_noisy_dev: k_predict_noisy_small launch failed");
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
    const int wrows = p->droute == 0 ? rup(m, 16) : p->mp;
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

// the draws kernels of one tile of nt rows: Xc[s] -> dout[s] ([nd k][nt]).  phi_built: predictor_tile has just run on the same slot and
// rows on the tile route, so p->Phi already holds this tile's PHI (the same launch_phi with the same arguments; launch_tgemm only reads it)
// Psic: the tile's Psi slot for rows with input noise (fused route, diagonal kinds), else nullptr
static int predictor_draws_tile(gpz_predictor *p, int s, int64_t nt, int ncol, int ldw, bool phi_built = false,
                                const double *Psic = nullptr) {
    const int m = p->m;
    hipStream_t st = p->s_cmp;
    const double *G = p->kind == GPZ_KIND_COV ? p->pr.Rc : p->pr.G2;
    if (Psic) {
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
    const long np = rup(nt, 1024);
    if (!phi_built && launch_phi(st, predictor_phi_args(p, s, (int)nt)))
        return gpz_fail(GPZ_ERR_UNSUPPORTED, "gpz_predictor_draws: PHI kernel not instantiated for d=%d", p->de);
    // T = PHI W: K = mp (rows >= m of W are zero), ldw output columns
    launch_tgemm(st, p->Phi, p->mp, p->Wd, ldw, p->Td, (int)np, ldw, nullptr, nullptr, m, 0, false, p->mp, ldw);
    launch_transpose_out(st, p->Td, ldw, nt, ncol, p->dout[s]);
    if (hipGetLastError() != hipSuccess) return gpz_fail(GPZ_ERR_HIP, "gpz_predictor_draws: kernel launch failed");
    return 0;
}

// What a call that needs gamma under nd draws on tiles of T rows adds to the handle (after predictor_noisy_prepare: the pair table): the
// chunk slab of the pair sums and, for a stack of Q column-outputs, the widths.  nd = 0 takes no slab.
static int predictor_gamma_prepare(gpz_predictor *p, int ncol, int Q, int64_t T) {
    int rc = 0;
    p->gchunks = predict_gamma_chunks(p->m);
    if (ncol > 0 && (rc = predictor_grow(p, &p->gpart, &p->gpart_cap, (size_t)p->gchunks * ncol * T))) return rc;
    if (Q > 0 && (rc = predictor_grow(p, &p->s2_d, &p->s2_cap, (size_t)Q * T))) return rc;
    p->gam_used = true;
    return 0;
}

// the pair sums under every draw of one tile of nt rows: Xc[s], Psic[s], W -> gpart ([gchunks][ncol][nt])
static int predictor_gamma_tile(gpz_predictor *p, const char *who, int s, int nt, int ncol, int ldw) {
    if (launch_predict_noisy_gamma(p->s_cmp, p->d, p->Xc[s], p->Psic[s], p->tile_pad, nt, p->m, p->ptab, p->nrec, p->Wd, ldw, ncol,
                                   p->gchunks, p->gpart, nt))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_noisy_gamma launch failed", who);
    return 0;
}

// gpz_predictor_draws: the draws of every tile come home.  Psi (gpz_predictor_draws_noisy; nullptr: noise-free rows): normalised ns x d
// column-major, staged into a second pair of pinned slots and uploaded with X's tile
struct DrawsJob {
    gpz_predictor *p;
    int64_t ns;
    int nd, ncol, ldw;
    const double *Psi;
    double *F;
    const char *who = "gpz_predictor_draws";
    const char *nan_text = "the rows have missing values (NaN): draws are for complete rows";
    static constexpr bool downloads = true;
    int stage(int s, int64_t r0, int64_t nt) {
        if (Psi && predictor_stage(Psi, ns, p->d, r0, nt, p->hpsi[s], (size_t)p->tile_pad,
                                   [](double v) { return !(v >= 0.0) || !(v <= 1.7976931348623157e308); }))
            return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_draws_noisy: Psi has an element that is NaN, infinite or negative");
        return 0;
    }
    bool upload(int s, int64_t nt) {
        const size_t tp = (size_t)p->tile_pad;
        return Psi && hipMemcpy2DAsync(p->Psic[s], tp * sizeof(double), p->hpsi[s], tp * sizeof(double), (size_t)nt * sizeof(double), p->d,
                                       hipMemcpyHostToDevice, p->s_in) != hipSuccess;
    }
    int kernels(int s, int64_t nt) { return predictor_draws_tile(p, s, nt, ncol, ldw, false, Psi ? p->Psic[s] : nullptr); }
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
    if (Psi) {
        if ((rc = predictor_psi_slots(p))) return rc;
        for (int s = 0; s < 2; ++s)
            if (!p->hpsi[s])
                HIPCHK(hipHostMalloc((void **)&p->hpsi[s], (size_t)p->d * p->tile_pad * sizeof(double), hipHostMallocDefault));
    }
    if ((rc = predictor_draws_prepare(p, nd, seed, Z, true, &T))) return rc;
    if (Psi && p->droute != 0) return gpz_fail(GPZ_ERR_UNSUPPORTED, "gpz_predictor_draws_noisy: input noise needs the fused draws route");
    DrawsJob job{p, ns, nd, nd * p->k, rup(nd * p->k, 16), Psi, F};
    return predictor_drain(p, job.who, predictor_pipeline(p, Xs, ns, T, job));   // on tiles of T rows
}

// ---- stack ------------------------------------------------------------------------------------------------------------------------
// Per tile: rows, labels and weights up; predictor_tile (mu, nu, beta stay in out[s]); with draws, their kernels (F stays in dout[s]);
// k_stack_tile writes the tile's row slabs and k_stack_accum adds them to the running accumulators, all on the compute stream, so the
// tiles add in their order.  Nothing comes back before the accumulators at the end.  Both kernels run on the draws tile, so that out[s]
// and dout[s] describe the same rows.  res: (1 + nd) k records of G B + 3 G doubles (k_predict_stack.hip).
struct StackCall {
    int nd, B, G, ncol, ldw;
    int R;           // row slabs per tile
    size_t ne;       // the edges; behind them in edges_d, the k shifts of the sums
    size_t count;    // doubles in the accumulators
    int64_t T;       // rows per tile
};

// What a stack call does before its first tile: with draws, what they need; the label and weight slots of the host entry (pinned); the
// edges, accumulators and slabs; then the edges and shifts go up and the accumulators are cleared.  Once this has been called the entry
// leaves through its stream synchronisation, failed or not: copies from the caller's memory may be in flight.
static int predictor_stack_prepare(gpz_predictor *p, const char *who, int nd, unsigned long long seed, const double *Z, const double *edges,
                         const double *shift, int B, int G, bool pinned, StackCall *c) {
    const int k = p->k, Q = (1 + nd) * k;
    const size_t tp = (size_t)p->tile_pad, rec = (size_t)G * B + 3 * (size_t)G;
    hipStream_t st = p->s_cmp;
    int rc = 0;
    int64_t T = p->tile_rows;
    if (nd > 0 && (rc = predictor_draws_prepare(p, nd, seed, Z, false, &T))) return rc;
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
    p->stile = T;
    p->sslabs = c->R;
    if (hipMemcpyAsync(p->edges_d, edges, c->ne * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
        (shift ? hipMemcpyAsync(p->edges_d + c->ne, shift, (size_t)k * sizeof(double), hipMemcpyHostToDevice, st)
               : hipMemsetAsync(p->edges_d + c->ne, 0, (size_t)k * sizeof(double), st)) != hipSuccess ||
        hipMemsetAsync(p->acc_d, 0, c->count * sizeof(double), st) != hipSuccess)
        return gpz_fail(GPZ_ERR_HIP, "%s: copy failed", who);
    return 0;
}

// the kernels of one stack tile of nt rows in slot s; lab, wt: the tile's labels and weights on the device (nullptr: one group, weight 1)
static int predictor_stack_tile(gpz_predictor *p, const char *who, const StackCall &c, int s, int64_t nt, const int *lab, const double *wt) {
    int rc = 0;
    if ((rc = predictor_tile(p, s, (int)nt, false))) return rc;
    if (c.nd > 0 && (rc = predictor_draws_tile(p, s, nt, c.ncol, c.ldw, p->route == 1))) return rc;
    if (launch_stack_tile(p->s_cmp, p->out[s], c.nd > 0 ? p->dout[s] : nullptr, lab, wt, p->edges_d, p->edges_d + c.ne, nt, p->k, c.nd, c.B,
                          c.G, c.R, p->slab_d) ||
        launch_stack_accum(p->s_cmp, p->slab_d, c.R, c.count, p->acc_d))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_stack_tile launch failed", who);
    return 0;
}

// the accumulators come home behind the last tile
static int predictor_stack_result(gpz_predictor *p, const char *who, const StackCall &c, double *res) {
    if (hipMemcpyAsync(res, p->acc_d, c.count * sizeof(double), hipMemcpyDeviceToHost, p->s_cmp) != hipSuccess)
        return gpz_fail(GPZ_ERR_HIP, "%s: copy failed", who);
    return 0;
}

// gpz_predictor_stack: the tile's labels and weights ride up with its rows, nothing comes home
struct StackJob {
    gpz_predictor *p;
    const StackCall &c;
    const int32_t *group;
    const double *weight;
    const char *who = "gpz_predictor_stack";
    const char *nan_text = "the rows have missing values (NaN): stacks are for complete rows";
    static constexpr bool downloads = false;
    int stage(int s, int64_t r0, int64_t nt) {
        if (group) memcpy(p->hlab[s], group + r0, (size_t)nt * sizeof(int));
        if (weight) memcpy(p->hwt[s], weight + r0, (size_t)nt * sizeof(double));
        return 0;
    }
    bool upload(int s, int64_t nt) {
        return (group && hipMemcpyAsync(p->lab_d[s], p->hlab[s], (size_t)nt * sizeof(int), hipMemcpyHostToDevice, p->s_in) != hipSuccess) ||
               (weight && hipMemcpyAsync(p->wt_d[s], p->hwt[s], (size_t)nt * sizeof(double), hipMemcpyHostToDevice, p->s_in) != hipSuccess);
    }
    int kernels(int s, int64_t nt) { return predictor_stack_tile(p, who, c, s, nt, group ? p->lab_d[s] : nullptr, weight ? p->wt_d[s] : nullptr); }
};

static int predictor_run_stack(gpz_predictor *p, const double *Xs, int64_t ns, int nd, unsigned long long seed, const double *Z,
                               const double *edges, const double *shift, int B, const int32_t *group, int G, const double *weight,
                               double *res) {
    const char *who = "gpz_predictor_stack";
    StackCall c{};
    int rc = predictor_stack_prepare(p, who, nd, seed, Z, edges, shift, B, G, true, &c);
    if (!rc) {
        StackJob job{p, c, group, weight};
        rc = predictor_pipeline(p, Xs, ns, c.T, job);
    }
    if (!rc) rc = predictor_stack_result(p, who, c, res);
    return predictor_drain(p, who, rc);
}

// ---- stack of rows with input noise --------------------------------------------------------------------------------------------
// predictor_stack_tile for rows with Psi in Psic[s]: predictNoisy (nout[s]), with draws their kernel behind PHI of (X, Psi) (dout[s]) and
// the pair sums under every draw, the widths (column 0: (nu + beta) + gamma, draw s: beta + max(gamma_s, 0)), then the stack kernel that
// reads them and k_stack_accum
static int predictor_stack_noisy_tile(gpz_predictor *p, const char *who, const StackCall &c, int s, int64_t nt, const int *lab,
                                      const double *wt) {
    int rc = 0;
    if ((rc = predictor_noisy_tile(p, s, (int)nt))) return rc;
    if (c.nd > 0) {
        if ((rc = predictor_draws_tile(p, s, nt, c.ncol, c.ldw, false, p->Psic[s]))) return rc;
        if ((rc = predictor_gamma_tile(p, who, s, (int)nt, c.ncol, c.ldw))) return rc;
    }
    if (launch_gamma_finish_s2(p->s_cmp, p->gpart, p->gchunks, nt, p->nout[s], c.nd > 0 ? p->dout[s] : nullptr, (int)nt, p->k, c.nd, p->s2_d))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_gamma_finish_s2 launch failed", who);
    if (launch_stack_tile_w(p->s_cmp, p->nout[s], p->s2_d, c.nd > 0 ? p->dout[s] : nullptr, lab, wt, p->edges_d, p->edges_d + c.ne, nt, p->k,
                            c.nd, c.B, c.G, c.R, p->slab_d) ||
        launch_stack_accum(p->s_cmp, p->slab_d, c.R, c.count, p->acc_d))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_stack_tile_w launch failed", who);
    return 0;
}

// gpz_predictor_stack_noisy: StackJob with Psi's tile staged into the hpsi slots and uploaded with X's, as DrawsJob does
struct StackNoisyJob {
    gpz_predictor *p;
    const StackCall &c;
    int64_t ns;
    const double *Psi;
    const int32_t *group;
    const double *weight;
    const char *who = "gpz_predictor_stack_noisy";
    const char *nan_text = "the rows have missing values (NaN): stacks are for complete rows";
    static constexpr bool downloads = false;
    int stage(int s, int64_t r0, int64_t nt) {
        if (predictor_stage(Psi, ns, p->d, r0, nt, p->hpsi[s], (size_t)p->tile_pad,
                            [](double v) { return !(v >= 0.0) || !(v <= 1.7976931348623157e308); }))
            return gpz_fail(GPZ_ERR_ARG, "%s: Psi has an element that is NaN, infinite or negative", who);
        if (group) memcpy(p->hlab[s], group + r0, (size_t)nt * sizeof(int));
        if (weight) memcpy(p->hwt[s], weight + r0, (size_t)nt * sizeof(double));
        return 0;
    }
    bool upload(int s, int64_t nt) {
        const size_t tp = (size_t)p->tile_pad;
        return hipMemcpy2DAsync(p->Psic[s], tp * sizeof(double), p->hpsi[s], tp * sizeof(double), (size_t)nt * sizeof(double), p->d,
                                hipMemcpyHostToDevice, p->s_in) != hipSuccess ||
               (group && hipMemcpyAsync(p->lab_d[s], p->hlab[s], (size_t)nt * sizeof(int), hipMemcpyHostToDevice, p->s_in) != hipSuccess) ||
               (weight && hipMemcpyAsync(p->wt_d[s], p->hwt[s], (size_t)nt * sizeof(double), hipMemcpyHostToDevice, p->s_in) != hipSuccess);
    }
    int kernels(int s, int64_t nt) {
        return predictor_stack_noisy_tile(p, who, c, s, nt, group ? p->lab_d[s] : nullptr, weight ? p->wt_d[s] : nullptr);
    }
};

static int predictor_run_stack_noisy(gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi, int nd, unsigned long long seed,
                                     const double *Z, const double *edges, const double *shift, int B, const int32_t *group, int G,
                                     const double *weight, double *res) {
    const char *who = "gpz_predictor_stack_noisy";
    StackCall c{};
    int rc = predictor_noisy_prepare(p);
    for (int s = 0; s < 2 && !rc; ++s)
        if (!p->hpsi[s]) HIPCHK(hipHostMalloc((void **)&p->hpsi[s], (size_t)p->d * p->tile_pad * sizeof(double), hipHostMallocDefault));
    if (!rc) rc = predictor_stack_prepare(p, who, nd, seed, Z, edges, shift, B, G, true, &c);
    if (!rc) rc = predictor_gamma_prepare(p, c.ncol, (1 + nd) * p->k, c.T);
    if (!rc) {
        StackNoisyJob job{p, c, ns, Psi, group, weight};
        rc = predictor_pipeline(p, Xs, ns, c.T, job);
    }
    if (!rc) rc = predictor_stack_result(p, who, c, res);
    return predictor_drain(p, who, rc);
}

// ---- device-resident entries -------------------------------------------------------------------------------------------------------
// the caller's rows: element (i, c) at X[i rs + c cs], type GPZ_X_F64 or GPZ_X_F32
struct DevRows {
    const void *X;
    int32_t type;
    int64_t ns, rs, cs;
    int f32() const { return type == GPZ_X_F32; }
};

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

// What a device call does before its first tile: the parameter buffer (once per handle), muX, sdX and muY up, the compute stream after
// everything queued on the caller's stream, and k_pred_check_dev over all rows with its verdict.  nan_text: the host entry's refusal.
static int predictor_dev_begin(gpz_predictor *p, const char *who, const DevRows &x, const double *muX, const double *sdX, const double *muY,
                               const int *lab, int G, const double *wt, void *stream, const char *nan_text, const double **muX_d,
                               const double **sdX_d, const double **muY_d, const DevRows *psi = nullptr, const double *sd2 = nullptr,
                               const unsigned *pattern = nullptr) {
    const size_t d = p->d, k = p->k;
    hipStream_t st = p->s_cmp;
    if (!p->par_d)
        if (int rc = p->ar.alloc(&p->par_d, 2 * d + k + 2)) return rc;
    if (!p->ev_dev) HIPCHK(hipEventCreateWithFlags(&p->ev_dev, hipEventDisableTiming));
    p->dev_used = true;
    unsigned *rec = (unsigned *)(p->par_d + 2 * d + k);
    unsigned verdict[4] = {0, 0, 0, 0};
    int rc = 0;
    // from here on every failure leaves through the synchronisation below: copies from the caller's memory may be in flight
    if (hipEventRecord(p->ev_dev, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent(st, p->ev_dev, 0) != hipSuccess)
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
    if (!rc && psi &&   // (predictor_psi_slots has run: sd2_d exists)
        ((sd2 && hipMemcpyAsync(p->sd2_d, sd2, d * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) ||
         launch_pred_check_psi(st, psi->X, psi->f32(), psi->ns, p->d, psi->rs, psi->cs, sd2 ? *std::min_element(sd2, sd2 + d) : 1.0, rec)))
        rc = gpz_fail(GPZ_ERR_HIP, "%s: k_pred_check_psi launch failed", who);
    if (!rc && hipMemcpyAsync(verdict, rec, sizeof verdict, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = gpz_fail(GPZ_ERR_HIP, "%s: copy failed", who);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = gpz_fail(GPZ_ERR_HIP, "%s: sync failed", who);
    if (rc) return rc;
    if (verdict[1]) return gpz_fail(GPZ_ERR_ARG, "%s: a label is outside [-1, %d)", who, G);
    if (verdict[2]) return gpz_fail(GPZ_ERR_ARG, "%s: a weight is negative or not finite", who);
    if (verdict[0] && pattern) return gpz_fail(GPZ_ERR_ARG, "%s: %s", who, nan_text);
    if (verdict[0]) return gpz_fail(GPZ_ERR_UNSUPPORTED, "%s: %s", who, nan_text);
    if (verdict[3]) return gpz_fail(GPZ_ERR_ARG, "%s: Psi has an element that is NaN, infinite or negative", who);
    *muX_d = muX ? p->par_d : nullptr;
    *sdX_d = muX ? p->par_d + d : nullptr;
    *muY_d = muY ? p->par_d + 2 * d : nullptr;
    return 0;
}

// The tiles of a device entry, all on the compute stream: k_pred_stage (and, with psi, k_pred_stage_psi into Psic[s]) from the caller's
// memory into slot s, then body(s, r0, nt), the entry's kernels down to the one that writes into the caller's arrays.
template <class Body>
static int predictor_dev_tiles(gpz_predictor *p, const char *who, const DevRows &x, const double *muX_d, const double *sdX_d,
                               const DevRows *psi, const double *sd2_d, int64_t T, Body body) {
    hipStream_t st = p->s_cmp;
    for (int64_t r0 = 0, t = 0; r0 < x.ns; r0 += T, ++t) {
        const int s = (int)(t & 1), nt = (int)std::min<int64_t>(T, x.ns - r0);
        if (launch_pred_stage(st, x.X, x.f32(), x.rs, x.cs, r0, nt, p->d, muX_d, sdX_d, p->Xc[s], p->tile_pad))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_pred_stage launch failed", who);
        if (psi && launch_pred_stage_psi(st, psi->X, psi->f32(), psi->rs, psi->cs, r0, nt, p->d, sd2_d, p->Psic[s], p->tile_pad))
            return gpz_fail(GPZ_ERR_HIP, "%s: k_pred_stage_psi launch failed", who);
        if (int rc = body(s, r0, nt)) return rc;
    }
    return 0;
}

// the end of every device entry once it has prepared anything after predictor_dev_begin, failed or not: copies from the caller's memory
// (Z, the edges) may be in flight
static int predictor_dev_sync(gpz_predictor *p, const char *who, int rc) {
    if (hipStreamSynchronize(p->s_cmp) != hipSuccess && !rc) rc = gpz_fail(GPZ_ERR_HIP, "%s: sync failed", who);
    return rc;
}

// gpz_predictor_run_dev and, with psi, gpz_predictor_run_noisy_dev (predictNoisy per tile: Xc[s], Psic[s] -> nout[s]), each with its
// finish kernel into the caller's arrays
static int predictor_run_dev(gpz_predictor *p, const char *who, const DevRows &x, const DevRows *psi, const double *muX_d,
                             const double *sdX_d, const double *sd2_d, const double *muY_d, double *mu, double *sigma, double *nu,
                             double *beta, double *gamma, double *PHI) {
    hipStream_t st = p->s_cmp;
    const int64_t ns = x.ns;
    int rc = 0;
    if (psi)
        rc = predictor_dev_tiles(p, who, x, muX_d, sdX_d, psi, sd2_d, p->tile_rows, [&](int s, int64_t r0, int nt) {
            if (int rc = predictor_noisy_tile(p, s, nt)) return rc;
            if (launch_pred_finish_noisy_dev(st, p->nout[s], nt, p->k, muY_d, ns, r0, mu, sigma, nu, beta, gamma))
                return gpz_fail(GPZ_ERR_HIP, "%s: finish kernel launch failed", who);
            return 0;
        });
    else
        rc = predictor_dev_tiles(p, who, x, muX_d, sdX_d, nullptr, nullptr, p->tile_rows, [&](int s, int64_t r0, int nt) {
            if (int rc = predictor_tile(p, s, nt, PHI != nullptr)) return rc;
            if (launch_pred_finish_dev(st, p->out[s], nt, p->k, muY_d, ns, r0, mu, sigma, nu, beta, gamma) ||
                (PHI && launch_pred_phi_dev(st, p->phi_d[s], nt, p->m, ns, r0, PHI)))
                return gpz_fail(GPZ_ERR_HIP, "%s: finish kernel launch failed", who);
            return 0;
        });
    return predictor_dev_sync(p, who, rc);
}

// psi (gpz_predictor_draws_noisy_dev; nullptr: noise-free rows) with sd2_d
static int predictor_run_draws_dev(gpz_predictor *p, const DevRows &x, const double *muX_d, const double *sdX_d, const double *muY_d, int nd,
                                   unsigned long long seed, const double *Z, double *F, const DevRows *psi, const double *sd2_d,
                                   double *Gam = nullptr) {
    const char *who = Gam ? "gpz_predictor_draws_gamma_noisy_dev" : "gpz_predictor_draws_dev";
    const int ncol = nd * p->k, ldw = rup(ncol, 16);
    int64_t T = 0;
    int rc = predictor_draws_prepare(p, nd, seed, Z, false, &T);
    if (!rc && Gam) rc = predictor_gamma_prepare(p, ncol, 0, T);
    if (!rc)
        rc = predictor_dev_tiles(p, who, x, muX_d, sdX_d, psi, sd2_d, T, [&](int s, int64_t r0, int nt) {
            if (int rc = predictor_draws_tile(p, s, nt, ncol, ldw, false, psi ? p->Psic[s] : nullptr)) return rc;
            if (Gam) {   // gamma_s = the pair sum under draw s - mu_s^2, mu_s as dout[s] holds it (without muY)
                if (int rc = predictor_gamma_tile(p, who, s, nt, ncol, ldw)) return rc;
                if (launch_gamma_finish_dev(p->s_cmp, p->gpart, p->gchunks, nt, p->dout[s], nt, p->k, nd, x.ns, r0, Gam))
                    return gpz_fail(GPZ_ERR_HIP, "%s: k_gamma_finish_dev launch failed", who);
            }
            if (launch_draws_finish_dev(p->s_cmp, p->dout[s], nt, p->k, nd, muY_d, x.ns, r0, F))
                return gpz_fail(GPZ_ERR_HIP, "%s: k_draws_finish_dev launch failed", who);
            return 0;
        });
    return predictor_dev_sync(p, who, rc);
}

// predictor_run_stack with the rows, labels and weights where the caller has them: the tile kernels read lab + r0 and wt + r0 directly
static int predictor_run_stack_dev(gpz_predictor *p, const DevRows &x, const double *muX_d, const double *sdX_d, int nd,
                                   unsigned long long seed, const double *Z, const double *edges, const double *shift, int B,
                                   const int32_t *group, int G, const double *weight, double *res) {
    const char *who = "gpz_predictor_stack_dev";
    StackCall c{};
    int rc = predictor_stack_prepare(p, who, nd, seed, Z, edges, shift, B, G, false, &c);
    if (!rc)
        rc = predictor_dev_tiles(p, who, x, muX_d, sdX_d, nullptr, nullptr, c.T, [&](int s, int64_t r0, int nt) {
            return predictor_stack_tile(p, who, c, s, nt, group ? group + r0 : nullptr, weight ? weight + r0 : nullptr);
        });
    if (!rc) rc = predictor_stack_result(p, who, c, res);
    return predictor_dev_sync(p, who, rc);
}

// predictor_run_stack_noisy with the rows, Psi, labels and weights where the caller has them
static int predictor_run_stack_noisy_dev(gpz_predictor *p, const DevRows &x, const DevRows &psi, const double *muX_d, const double *sdX_d,
                                         const double *sd2_d, int nd, unsigned long long seed, const double *Z, const double *edges,
                                         const double *shift, int B, const int32_t *group, int G, const double *weight, double *res) {
    const char *who = "gpz_predictor_stack_noisy_dev";
    StackCall c{};
    int rc = predictor_stack_prepare(p, who, nd, seed, Z, edges, shift, B, G, false, &c);
    if (!rc) rc = predictor_gamma_prepare(p, c.ncol, (1 + nd) * p->k, c.T);
    if (!rc)
        rc = predictor_dev_tiles(p, who, x, muX_d, sdX_d, &psi, sd2_d, c.T, [&](int s, int64_t r0, int nt) {
            return predictor_stack_noisy_tile(p, who, c, s, nt, group ? group + r0 : nullptr, weight ? weight + r0 : nullptr);
        });
    if (!rc) rc = predictor_stack_result(p, who, c, res);
    return predictor_dev_sync(p, who, rc);
}

// ---- rows with missing inputs on the handle -----------------------------------------------------------------------------------------
static int predictor_missing_check(const char *who, const gpz_predictor *p, uint32_t obs) {
    if (!predict_missing_fits(p->kind, p->de, p->m, p->k))
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
static int predictor_missing_prepare(gpz_predictor *p, const char *who, uint32_t obs, const double *priors, bool pairs) {
    const size_t m = p->m, k = p->k, mp = p->mp, nk = rup(p->m, 16);
    auto &ar = p->ar;
    hipStream_t st = p->s_cmp;
    int rc = 0;
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
    p->miss_used = true;
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
// beta | gamma)
static int predictor_missing_tile(gpz_predictor *p, const char *who, int s, int nt, uint32_t obs, bool pairs) {
    hipStream_t st = p->s_cmp;
    const int np = rup(nt, 128);   // the rows of the product: k_tgemm's row tile
    const long mtp = rup(p->mtile, 1024);
    const double *v = p->hetero ? p->pr.v : nullptr;
    if (launch_pmd_no(st, p->Xc[s], p->tile_pad, nt, np, p->m, p->mp, p->d, p->de, obs, p->pr.P, p->pr.G2, p->mbt, p->mNo, p->mPio))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_pmd_no launch failed", who);
    launch_tgemm(st, p->mPio, p->mp, p->mNij, p->mp, p->mT, np, p->mp, nullptr, nullptr, p->m, -1);
    if (hipGetLastError() != hipSuccess) return gpz_fail(GPZ_ERR_HIP, "%s: k_tgemm launch failed", who);
    if (launch_pmd_phi(st, p->mNo, p->mT, nt, p->m, p->mp, p->k, p->w_d, v, p->mhd, mtp))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_pmd_phi launch failed", who);
    if (pairs && launch_predict_missing_pairs(st, p->Xc[s], p->tile_pad, nt, p->mPio, p->mp, p->m, p->d, p->k, obs, p->mU, p->mrec, p->mchunks,
                                              p->mpart, mtp, p->mhd, mtp, p->pr.b, p->mout))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_missing_pairs launch failed", who);
    return 0;
}

// the draws of one tile of the group behind predictor_missing_tile: PHI_missing (mNo) against the handle's W on k_tgemm -> dout[s]
// ([ncol][nt], without muY).  wrows: the rows of W (predictor_draws_prepare), K of the product
static int predictor_missing_draws_tile(gpz_predictor *p, const char *who, int s, int nt, int ncol, int ldw, int wrows) {
    launch_tgemm(p->s_cmp, p->mNo, p->mp, p->Wd, ldw, p->Td, rup(nt, 128), ldw, nullptr, nullptr, p->m, 0, false, wrows, ldw);
    launch_transpose_out(p->s_cmp, p->Td, ldw, nt, ncol, p->dout[s]);
    if (hipGetLastError() != hipSuccess) return gpz_fail(GPZ_ERR_HIP, "%s: kernel launch failed", who);
    return 0;
}

// What a call that needs gamma under nd draws for a group on tiles of T rows adds to the handle (after predictor_missing_prepare with
// pairs: U and the records): the chunk slab of the pair sums and, for a stack of Q column-outputs, the widths.  nd = 0 takes no slab.
static int predictor_missing_gamma_prepare(gpz_predictor *p, int ncol, int Q, int64_t T) {
    int rc = 0;
    if (ncol > 0 && (rc = predictor_grow(p, &p->gpart, &p->gpart_cap, (size_t)p->mchunks * ncol * T))) return rc;
    if (Q > 0 && (rc = predictor_grow(p, &p->ms2_d, &p->ms2_cap, (size_t)Q * T))) return rc;
    p->mgam_used = true;
    return 0;
}

// the pair sums under every draw of one tile of nt rows of the group, after predictor_missing_tile (mPio): -> gpart ([mchunks][ncol][nt])
static int predictor_missing_gamma_tile(gpz_predictor *p, const char *who, int s, int nt, uint32_t obs, int ncol, int ldw) {
    if (launch_predict_missing_gamma(p->s_cmp, p->Xc[s], p->tile_pad, nt, p->mPio, p->mp, p->m, p->d, p->k, obs, p->mU, p->mrec, p->Wd, ldw,
                                     ncol, p->mchunks, p->gpart, nt))
        return gpz_fail(GPZ_ERR_HIP, "%s: k_predict_missing_gamma launch failed", who);
    return 0;
}

// ---- what the entries share ---------------------------------------------------------------------------------------------------------
static int predictor_check_call(const char *who, const gpz_predictor *p, int64_t ns) {
    if (!p) return gpz_fail(GPZ_ERR_ARG, "%s: null handle", who);
    if (ns < 0) return gpz_fail(GPZ_ERR_ARG, "%s: ns < 0", who);
    return 0;
}

// least: 1 for the draws; 0 for the stack, whose column 0 is the posterior mean
static int predictor_check_ndraws(const char *who, const gpz_predictor *p, int32_t ndraws, int least) {
    if (ndraws < least || (1 - least + (int64_t)ndraws) * p->k > GPZ_DRAWS_MAX_COLUMNS)
        return gpz_fail(GPZ_ERR_ARG, "%s: need %d <= ndraws and %s * k <= %d (ndraws %d, k %d)", who, least,
                        least ? "ndraws" : "(1 + ndraws)", GPZ_DRAWS_MAX_COLUMNS, (int)ndraws, p->k);
    return 0;
}

// draws with input noise: a model inside predict_noisy_fits, on the fused draws route
static int predictor_check_noisy_draws(const char *who, const gpz_predictor *p) {
    if (int rc = predictor_noisy_check(who, p)) return rc;
    if (p->force_tiles) return gpz_fail(GPZ_ERR_UNSUPPORTED, "%s: input noise needs the fused draws route (GPZ_PREDICT_FORCE_TILES is set)", who);
    return 0;
}

// Every entry after create runs its body through here: the handle's options and device for the length of the call, the caller's device
// again on every way out.
template <class Body>
static int predictor_call(gpz_predictor *p, const char *who, Body body) {
    int prev = 0;
    (void)hipGetDevice(&prev);
    gpz_opts_scope opts_scope(&p->opt);
    int rc = 0;
    if (hipSetDevice(p->device) != hipSuccess) rc = gpz_fail(GPZ_ERR_HIP, "%s: hipSetDevice failed", who);
    if (!rc) rc = body();
    (void)hipSetDevice(prev);
    return rc;
}

// the shape checks of a stack call, in the order gpz_predictor_stack has always made them (who: the entry's name in the message)
static int stack_check_shape(const char *who, const gpz_predictor *p, int64_t ns, int32_t ndraws, int32_t nbins, int32_t ngroups,
                             const double *edges, const double *hist, const double *sum_w, const double *sum_mu, const double *sum_mu2,
                             const void *Xs) {
    if (int rc = predictor_check_call(who, p, ns)) return rc;
    if (int rc = predictor_check_ndraws(who, p, ndraws, 0)) return rc;
    if (nbins < 1 || ngroups < 1) return gpz_fail(GPZ_ERR_ARG, "%s: need nbins >= 1 and ngroups >= 1", who);
    if ((int64_t)nbins * ngroups > GPZ_STACK_MAX_GROUP_BINS)
        return gpz_fail(GPZ_ERR_ARG, "%s: ngroups * nbins = %lld is over GPZ_STACK_MAX_GROUP_BINS = %d", who, (long long)nbins * ngroups,
                        GPZ_STACK_MAX_GROUP_BINS);
    const int k = p->k, B = nbins;
    if (!edges || !hist || !sum_w || !sum_mu || !sum_mu2) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
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
static void stack_unpack(const double *res, int C, int k, int G, int B, double *hist, double *sum_w, double *sum_mu, double *sum_mu2) {
    const size_t GB = (size_t)G * B, rec = GB + 3 * (size_t)G;
    for (int c = 0; c < C; ++c)
        for (int o = 0; o < k; ++o) {
            const double *r = res + ((size_t)c * k + o) * rec;
            for (int g = 0; g < G; ++g) {
                const size_t at = ((size_t)c * G + g) * k + o;
                memcpy(hist + at * B, r + (size_t)g * B, (size_t)B * sizeof(double));
                sum_mu[at] = r[GB + 3 * (size_t)g + 1];
                sum_mu2[at] = r[GB + 3 * (size_t)g + 2];
                if (c == 0 && o == 0) sum_w[g] = r[GB + 3 * (size_t)g];
            }
        }
}

static void stack_zero(int C, int k, int G, int B, double *hist, double *sum_w, double *sum_mu, double *sum_mu2) {
    const size_t Q = (size_t)C * k;
    memset(hist, 0, Q * G * B * sizeof(double));
    memset(sum_w, 0, (size_t)G * sizeof(double));
    memset(sum_mu, 0, Q * G * sizeof(double));
    memset(sum_mu2, 0, Q * G * sizeof(double));
}

static int stack_check_shift(const char *who, const gpz_predictor *p, const double *mu_shift) {
    for (int o = 0; mu_shift && o < p->k; ++o)
        if (!std::isfinite(mu_shift[o])) return gpz_fail(GPZ_ERR_ARG, "%s: mu_shift must be finite", who);
    return 0;
}

// gpz_predictor_draws and, with noisy, gpz_predictor_draws_noisy
static int draws_entry(const char *who, bool noisy, gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi, int32_t ndraws,
                       uint64_t seed, const double *Z, double *F) {
    if (int rc = predictor_check_call(who, p, ns)) return rc;
    if (int rc = predictor_check_ndraws(who, p, ndraws, 1)) return rc;
    if (noisy)
        if (int rc = predictor_check_noisy_draws(who, p)) return rc;
    if (ns == 0) return 0;
    if (!Xs || (noisy && !Psi) || !F) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    return predictor_call(p, who, [&] { return predictor_run_draws(p, Xs, ns, (int)ndraws, (unsigned long long)seed, Z, F, Psi); });
}

// gpz_predictor_run_dev and, with psi, gpz_predictor_run_noisy_dev
static int run_dev_entry(const char *who, gpz_predictor *p, const DevRows &x, const DevRows *psi, const double *muX, const double *sdX,
                         const double *sd2, const double *muY, double *mu_d, double *sigma_d, double *nu_d, double *beta_d, double *gamma_d,
                         double *PHI_d, void *stream) {
    if (int rc = predictor_check_call(who, p, x.ns)) return rc;
    if (psi)
        if (int rc = predictor_noisy_check(who, p)) return rc;
    if (int rc = predictor_dev_args(who, p, x, muX, sdX)) return rc;
    if (psi)
        if (int rc = predictor_dev_psi_args(who, *psi, sdX, sd2)) return rc;
    if (x.ns == 0) return 0;
    if (!mu_d || !nu_d || !beta_d) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    return predictor_call(p, who, [&] {
        const double *mx = nullptr, *sx = nullptr, *my = nullptr;
        int rc = psi ? predictor_noisy_prepare(p) : PHI_d ? predictor_want_phi(p, false) : 0;
        if (!rc)
            rc = predictor_dev_begin(p, who, x, muX, sdX, muY, nullptr, 0, nullptr, stream,
                                     psi ? "the rows have missing values (NaN): input noise on the handle is for complete rows"
                                         : "the rows have missing values (NaN): group them by pattern and call gpz_predict_missing (predict.m:45-69)",
                                     &mx, &sx, &my, psi, sd2);
        if (!rc) rc = predictor_run_dev(p, who, x, psi, mx, sx, sd2 ? p->sd2_d : nullptr, my, mu_d, sigma_d, nu_d, beta_d, gamma_d, PHI_d);
        if (!rc) ++p->runs;
        return rc;
    });
}

// gpz_predictor_draws_dev and, with psi, gpz_predictor_draws_noisy_dev
static int draws_dev_entry(const char *who, gpz_predictor *p, const DevRows &x, const DevRows *psi, const double *muX, const double *sdX,
                           const double *sd2, const double *muY, int32_t ndraws, uint64_t seed, const double *Z, double *F_d,
                           void *stream, double *Gam_d = nullptr, bool want_gamma = false) {
    if (int rc = predictor_check_call(who, p, x.ns)) return rc;
    if (int rc = predictor_check_ndraws(who, p, ndraws, 1)) return rc;
    if (psi)
        if (int rc = predictor_check_noisy_draws(who, p)) return rc;
    if (int rc = predictor_dev_args(who, p, x, muX, sdX)) return rc;
    if (psi)
        if (int rc = predictor_dev_psi_args(who, *psi, sdX, sd2)) return rc;
    if (x.ns == 0) return 0;
    if (!F_d || (want_gamma && !Gam_d)) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    return predictor_call(p, who, [&] {
        const double *mx = nullptr, *sx = nullptr, *my = nullptr;
        int rc = want_gamma ? predictor_noisy_prepare(p) : psi ? predictor_psi_slots(p) : 0;   // gamma reads the pair table
        if (!rc)
            rc = predictor_dev_begin(p, who, x, muX, sdX, muY, nullptr, 0, nullptr, stream,
                                     "the rows have missing values (NaN): draws are for complete rows", &mx, &sx, &my, psi, sd2);
        if (!rc)
            rc = predictor_run_draws_dev(p, x, mx, sx, my, (int)ndraws, (unsigned long long)seed, Z, F_d, psi, sd2 ? p->sd2_d : nullptr,
                                         want_gamma ? Gam_d : nullptr);
        return rc;
    });
}

static const char *const kMissingPatternText = "the rows of a group must share one NaN pattern, the one of the mask";

// gpz_predictor_run_missing_dev
static int run_missing_dev_entry(const char *who, gpz_predictor *p, const DevRows &x, const double *muX, const double *sdX, const double *muY,
                                 const double *priors, uint32_t obs, double *mu_d, double *sigma_d, double *nu_d, double *beta_d,
                                 double *gamma_d, void *stream) {
    if (int rc = predictor_check_call(who, p, x.ns)) return rc;
    if (int rc = predictor_missing_check(who, p, obs)) return rc;
    if (int rc = predictor_dev_args(who, p, x, muX, sdX)) return rc;
    if (x.ns == 0) return 0;
    if (!mu_d || !nu_d || !beta_d) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    return predictor_call(p, who, [&] {
        const double *mx = nullptr, *sx = nullptr, *my = nullptr;
        const unsigned pat = obs;
        int rc = predictor_dev_begin(p, who, x, muX, sdX, muY, nullptr, 0, nullptr, stream, kMissingPatternText, &mx, &sx, &my, nullptr,
                                     nullptr, &pat);
        if (rc) return rc;   // the outputs are untouched
        rc = predictor_missing_prepare(p, who, obs, priors, true);
        if (!rc)
            rc = predictor_dev_tiles(p, who, x, mx, sx, nullptr, nullptr, p->mtile, [&](int s, int64_t r0, int nt) {
                if (int rc = predictor_missing_tile(p, who, s, nt, obs, true)) return rc;
                if (launch_pred_finish_noisy_dev(p->s_cmp, p->mout, nt, p->k, my, x.ns, r0, mu_d, sigma_d, nu_d, beta_d, gamma_d))
                    return gpz_fail(GPZ_ERR_HIP, "%s: finish kernel launch failed", who);
                return 0;
            });
        rc = predictor_dev_sync(p, who, rc);
        if (!rc) ++p->runs;
        return rc;
    });
}

// gpz_predictor_draws_missing_dev: F = PHI_missing W + muY (mu is linear in w), PHI of the tile against the handle's W on k_tgemm; with
// want_gamma (gpz_predictor_draws_gamma_missing_dev) gamma under every draw into Gam_d too
static int draws_missing_dev_entry(const char *who, gpz_predictor *p, const DevRows &x, const double *muX, const double *sdX,
                                   const double *muY, const double *priors, uint32_t obs, int32_t ndraws, uint64_t seed, const double *Z,
                                   double *F_d, void *stream, double *Gam_d = nullptr, bool want_gamma = false) {
    if (int rc = predictor_check_call(who, p, x.ns)) return rc;
    if (int rc = predictor_check_ndraws(who, p, ndraws, 1)) return rc;
    if (int rc = predictor_missing_check(who, p, obs)) return rc;
    if (int rc = predictor_dev_args(who, p, x, muX, sdX)) return rc;
    if (x.ns == 0) return 0;
    if (!F_d || (want_gamma && !Gam_d)) return gpz_fail(GPZ_ERR_ARG, "%s: null argument", who);
    return predictor_call(p, who, [&] {
        const double *mx = nullptr, *sx = nullptr, *my = nullptr;
        const unsigned pat = obs;
        const int nd = (int)ndraws, ncol = nd * p->k, ldw = rup(ncol, 16);
        int rc = predictor_dev_begin(p, who, x, muX, sdX, muY, nullptr, 0, nullptr, stream, kMissingPatternText, &mx, &sx, &my, nullptr,
                                     nullptr, &pat);
        if (rc) return rc;   // the output is untouched
        int64_t T = 0;
        rc = predictor_missing_prepare(p, who, obs, priors, want_gamma);   // gamma reads U and the records
        if (!rc) rc = predictor_draws_prepare(p, nd, (unsigned long long)seed, Z, false, &T);
        T = std::min<int64_t>(T, p->mtile);
        if (!rc && want_gamma) rc = predictor_missing_gamma_prepare(p, ncol, 0, T);
        // the product's output tile: the tile route of the draws has one already, the fused route does not
        if (!rc) rc = predictor_grow(p, &p->Td, &p->t_cap, (size_t)rup(T, 1024) * ldw);
        const int wrows = p->droute == 0 ? rup(p->m, 16) : p->mp;   // the rows of W (predictor_draws_prepare): K of the product
        if (!rc)
            rc = predictor_dev_tiles(p, who, x, mx, sx, nullptr, nullptr, T, [&](int s, int64_t r0, int nt) {
                if (int rc = predictor_missing_tile(p, who, s, nt, obs, false)) return rc;
                if (int rc = predictor_missing_draws_tile(p, who, s, nt, ncol, ldw, wrows)) return rc;
                if (want_gamma) {   // gamma_s = the pair sum under draw s - mu_s^2, mu_s as dout[s] holds it (without muY)
                    if (int rc = predictor_missing_gamma_tile(p, who, s, nt, obs, ncol, ldw)) return rc;
                    if (launch_gamma_finish_dev(p->s_cmp, p->gpart, p->mchunks, nt, p->dout[s], nt, p->k, nd, x.ns, r0, Gam_d))
                        return gpz_fail(GPZ_ERR_HIP, "%s: k_gamma_finish_dev launch failed", who);
                }
                if (launch_draws_finish_dev(p->s_cmp, p->dout[s], nt, p->k, nd, my, x.ns, r0, F_d))
                    return gpz_fail(GPZ_ERR_HIP, "%s: k_draws_finish_dev launch failed", who);
                return 0;
            });
        return predictor_dev_sync(p, who, rc);
    });
}

// gpz_predictor_stack_missing_dev after its checks: predictor_run_stack_noisy_dev for one group of rows with missing inputs.  Per tile
// of min(stack tile, mtile) rows: predictMissing (mout), with draws PHI_missing W (dout[s]) and the pair sums under every draw, the
// widths (column 0: (nu + beta) + gamma, draw s: beta + max(gamma_s, 0)), k_stack_tile_w and k_stack_accum
static int predictor_run_stack_missing_dev(gpz_predictor *p, const char *who, const DevRows &x, const double *muX_d, const double *sdX_d,
                                           const double *priors, uint32_t obs, int nd, unsigned long long seed, const double *Z,
                                           const double *edges, const double *shift, int B, const int32_t *group, int G,
                                           const double *weight, double *res) {
    const int k = p->k, Q = (1 + nd) * k;
    StackCall c{};
    int rc = predictor_missing_prepare(p, who, obs, priors, true);
    if (!rc) rc = predictor_stack_prepare(p, who, nd, seed, Z, edges, shift, B, G, false, &c);
    if (!rc) {   // the group's tile: No, Pio and T hold mtile rows
        c.T = std::min<int64_t>(c.T, p->mtile);
        c.R = predict_stack_slabs(Q, (long)((size_t)G * B + 3 * (size_t)G), c.T);   // <= the slabs that were allocated
        p->stile = c.T;
        p->sslabs = c.R;
    }
    // the product's output tile: the tile route of the draws has one already, the fused route does not
    if (!rc && nd > 0) rc = predictor_grow(p, &p->Td, &p->t_cap, (size_t)rup(c.T, 1024) * c.ldw);
    if (!rc) rc = predictor_missing_gamma_prepare(p, c.ncol, Q, c.T);
    const int wrows = p->droute == 0 ? rup(p->m, 16) : p->mp;
    if (!rc)
        rc = predictor_dev_tiles(p, who, x, muX_d, sdX_d, nullptr, nullptr, c.T, [&](int s, int64_t r0, int nt) {
            if (int rc = predictor_missing_tile(p, who, s, nt, obs, true)) return rc;
            if (nd > 0) {
                if (int rc = predictor_missing_draws_tile(p, who, s, nt, c.ncol, c.ldw, wrows)) return rc;
                if (int rc = predictor_missing_gamma_tile(p, who, s, nt, obs, c.ncol, c.ldw)) return rc;
            }
            if (launch_gamma_finish_s2(p->s_cmp, p->gpart, p->mchunks, nt, p->mout, nd > 0 ? p->dout[s] : nullptr, nt, k, nd, p->ms2_d))
                return gpz_fail(GPZ_ERR_HIP, "%s: k_gamma_finish_s2 launch failed", who);
            if (launch_stack_tile_w(p->s_cmp, p->mout, p->ms2_d, nd > 0 ? p->dout[s] : nullptr, group ? group + r0 : nullptr,
                                    weight ? weight + r0 : nullptr, p->edges_d, p->edges_d + c.ne, nt, k, nd, c.B, c.G, c.R, p->slab_d) ||
                launch_stack_accum(p->s_cmp, p->slab_d, c.R, c.count, p->acc_d))
                return gpz_fail(GPZ_ERR_HIP, "%s: k_stack_tile_w launch failed", who);
            return 0;
        });
    if (!rc) rc = predictor_stack_result(p, who, c, res);
    return predictor_dev_sync(p, who, rc);
}
}   // namespace gpzi

extern "C" int gpz_predictor_create(const gpz_desc *desc, const double *theta, const double *w, const double *iSigma_w,
                                    int64_t tile_rows, int32_t flags, gpz_predictor **out) {
    if (!out) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_create: null argument");
    *out = nullptr;
    if (!desc || !theta || !w || !iSigma_w) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_create: null argument");
    if (desc->dtype != GPZ_F64) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_create: fp64 only");
    if (flags & ~GPZ_PREDICT_FORCE_TILES) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_create: unknown flags %d", (int)flags);
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
    const char *who = "gpz_predictor_stack";
    if (int rc = stack_check_shape(who, p, ns, ndraws, nbins, ngroups, edges, hist, sum_w, sum_mu, sum_mu2, Xs)) return rc;
    const int k = p->k, B = nbins, G = ngroups, C = 1 + ndraws;
    if (group)
        for (int64_t i = 0; i < ns; ++i)
            if (group[i] < -1 || group[i] >= G)
                return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_stack: label %d of row %lld is outside [-1, %d)", (int)group[i], (long long)i, G);
    if (int rc = stack_check_shift(who, p, mu_shift)) return rc;
    if (weight)
        for (int64_t i = 0; i < ns; ++i)
            if (!(weight[i] >= 0.0) || !std::isfinite(weight[i]))
                return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_stack: the weight of row %lld is negative or not finite", (long long)i);
    stack_zero(C, k, G, B, hist, sum_w, sum_mu, sum_mu2);
    if (ns == 0) return 0;
    std::vector<double> res((size_t)C * k * ((size_t)G * B + 3 * (size_t)G));
    if (int rc = predictor_call(p, who, [&] {
            return predictor_run_stack(p, Xs, ns, (int)ndraws, (unsigned long long)seed, Z, edges, mu_shift, B, group, G, weight, res.data());
        }))
        return rc;
    stack_unpack(res.data(), C, k, G, B, hist, sum_w, sum_mu, sum_mu2);
    return 0;
}

extern "C" int gpz_predictor_run_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, int64_t col_stride,
                                     const double *muX, const double *sdX, const double *muY, double *mu_d, double *sigma_d, double *nu_d,
                                     double *beta_d, double *gamma_d, double *PHI_d, void *stream) {
    return run_dev_entry("gpz_predictor_run_dev", p, DevRows{X_d, x_type, ns, row_stride, col_stride}, nullptr, muX, sdX, nullptr, muY, mu_d,
                         sigma_d, nu_d, beta_d, gamma_d, PHI_d, stream);
}

extern "C" int gpz_predictor_run_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                           int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                           int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                           const double *muY, double *mu_d, double *sigma_d, double *nu_d, double *beta_d,
                                           double *gamma_d, void *stream) {
    const DevRows psi{Psi_d, psi_type, ns, psi_row_stride, psi_col_stride};
    return run_dev_entry("gpz_predictor_run_noisy_dev", p, DevRows{X_d, x_type, ns, row_stride, col_stride}, &psi, muX, sdX, sd2, muY, mu_d,
                         sigma_d, nu_d, beta_d, gamma_d, nullptr, stream);
}

extern "C" int gpz_predictor_draws_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                       int64_t col_stride, const double *muX, const double *sdX, const double *muY, int32_t ndraws,
                                       uint64_t seed, const double *Z, double *F_d, void *stream) {
    return draws_dev_entry("gpz_predictor_draws_dev", p, DevRows{X_d, x_type, ns, row_stride, col_stride}, nullptr, muX, sdX, nullptr, muY,
                           ndraws, seed, Z, F_d, stream);
}

extern "C" int gpz_predictor_draws_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                             int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                             int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                             const double *muY, int32_t ndraws, uint64_t seed, const double *Z, double *F_d,
                                             void *stream) {
    const DevRows psi{Psi_d, psi_type, ns, psi_row_stride, psi_col_stride};
    return draws_dev_entry("gpz_predictor_draws_noisy_dev", p, DevRows{X_d, x_type, ns, row_stride, col_stride}, &psi, muX, sdX, sd2, muY,
                           ndraws, seed, Z, F_d, stream);
}

extern "C" int gpz_predictor_run_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                             int64_t col_stride, const double *muX, const double *sdX, const double *muY,
                                             const double *priors, uint32_t obs_mask, double *mu_d, double *sigma_d, double *nu_d,
                                             double *beta_d, double *gamma_d, void *stream) {
    return run_missing_dev_entry("gpz_predictor_run_missing_dev", p, DevRows{X_d, x_type, ns, row_stride, col_stride}, muX, sdX, muY, priors,
                                 obs_mask, mu_d, sigma_d, nu_d, beta_d, gamma_d, stream);
}

extern "C" int gpz_predictor_draws_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                               int64_t col_stride, const double *muX, const double *sdX, const double *muY,
                                               const double *priors, uint32_t obs_mask, int32_t ndraws, uint64_t seed, const double *Z,
                                               double *F_d, void *stream) {
    return draws_missing_dev_entry("gpz_predictor_draws_missing_dev", p, DevRows{X_d, x_type, ns, row_stride, col_stride}, muX, sdX, muY,
                                   priors, obs_mask, ndraws, seed, Z, F_d, stream);
}

extern "C" int gpz_predictor_stack_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                       int64_t col_stride, const double *muX, const double *sdX, int32_t ndraws, uint64_t seed,
                                       const double *Z, const double *edges, int32_t nbins, const int32_t *group_d, int32_t ngroups,
                                       const double *weight_d, double *hist, double *sum_w, double *sum_mu, double *sum_mu2,
                                       const double *mu_shift, void *stream) {
    const char *who = "gpz_predictor_stack_dev";
    const DevRows x{X_d, x_type, ns, row_stride, col_stride};
    if (int rc = stack_check_shape(who, p, ns, ndraws, nbins, ngroups, edges, hist, sum_w, sum_mu, sum_mu2, X_d)) return rc;
    if (int rc = predictor_dev_args(who, p, x, muX, sdX)) return rc;
    if (int rc = stack_check_shift(who, p, mu_shift)) return rc;
    const int k = p->k, B = nbins, G = ngroups, C = 1 + ndraws;
    if (ns == 0) {
        stack_zero(C, k, G, B, hist, sum_w, sum_mu, sum_mu2);
        return 0;
    }
    std::vector<double> res((size_t)C * k * ((size_t)G * B + 3 * (size_t)G));
    if (int rc = predictor_call(p, who, [&] {
            const double *mx = nullptr, *sx = nullptr, *my = nullptr;
            // the refusals of the host entry's loops over labels and weights, and of its staging loop over the rows, before any tile
            int rc = predictor_dev_begin(p, who, x, muX, sdX, nullptr, group_d, G, weight_d, stream,
                                         "the rows have missing values (NaN): stacks are for complete rows", &mx, &sx, &my);
            if (!rc)
                rc = predictor_run_stack_dev(p, x, mx, sx, (int)ndraws, (unsigned long long)seed, Z, edges, mu_shift, B, group_d, G,
                                             weight_d, res.data());
            return rc;
        }))
        return rc;   // the outputs are untouched
    stack_unpack(res.data(), C, k, G, B, hist, sum_w, sum_mu, sum_mu2);
    return 0;
}

extern "C" int gpz_predictor_draws_gamma_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                   int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                                   int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                                   const double *muY, int32_t ndraws, uint64_t seed, const double *Z, double *F_d,
                                                   double *Gam_d, void *stream) {
    const DevRows psi{Psi_d, psi_type, ns, psi_row_stride, psi_col_stride};
    return draws_dev_entry("gpz_predictor_draws_gamma_noisy_dev", p, DevRows{X_d, x_type, ns, row_stride, col_stride}, &psi, muX, sdX, sd2,
                           muY, ndraws, seed, Z, F_d, stream, Gam_d, true);
}

extern "C" int gpz_predictor_stack_noisy(gpz_predictor *p, const double *Xs, int64_t ns, const double *Psi, int32_t ndraws, uint64_t seed,
                                         const double *Z, const double *edges, int32_t nbins, const int32_t *group, int32_t ngroups,
                                         const double *weight, double *hist, double *sum_w, double *sum_mu, double *sum_mu2,
                                         const double *mu_shift) {
    const char *who = "gpz_predictor_stack_noisy";
    if (int rc = stack_check_shape(who, p, ns, ndraws, nbins, ngroups, edges, hist, sum_w, sum_mu, sum_mu2, Xs)) return rc;
    if (int rc = predictor_check_noisy_draws(who, p)) return rc;
    if (ns > 0 && !Psi) return gpz_fail(GPZ_ERR_ARG, "%s: null Psi", who);
    const int k = p->k, B = nbins, G = ngroups, C = 1 + ndraws;
    if (group)
        for (int64_t i = 0; i < ns; ++i)
            if (group[i] < -1 || group[i] >= G)
                return gpz_fail(GPZ_ERR_ARG, "%s: label %d of row %lld is outside [-1, %d)", who, (int)group[i], (long long)i, G);
    if (int rc = stack_check_shift(who, p, mu_shift)) return rc;
    if (weight)
        for (int64_t i = 0; i < ns; ++i)
            if (!(weight[i] >= 0.0) || !std::isfinite(weight[i]))
                return gpz_fail(GPZ_ERR_ARG, "%s: the weight of row %lld is negative or not finite", who, (long long)i);
    if (ns == 0) {
        stack_zero(C, k, G, B, hist, sum_w, sum_mu, sum_mu2);
        return 0;
    }
    std::vector<double> res((size_t)C * k * ((size_t)G * B + 3 * (size_t)G));
    if (int rc = predictor_call(p, who, [&] {
            return predictor_run_stack_noisy(p, Xs, ns, Psi, (int)ndraws, (unsigned long long)seed, Z, edges, mu_shift, B, group, G, weight,
                                             res.data());
        }))
        return rc;   // the outputs are untouched
    stack_unpack(res.data(), C, k, G, B, hist, sum_w, sum_mu, sum_mu2);
    return 0;
}

extern "C" int gpz_predictor_stack_noisy_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                             int64_t col_stride, const void *Psi_d, int32_t psi_type, int64_t psi_row_stride,
                                             int64_t psi_col_stride, const double *muX, const double *sdX, const double *sd2,
                                             int32_t ndraws, uint64_t seed, const double *Z, const double *edges, int32_t nbins,
                                             const int32_t *group_d, int32_t ngroups, const double *weight_d, double *hist, double *sum_w,
                                             double *sum_mu, double *sum_mu2, const double *mu_shift, void *stream) {
    const char *who = "gpz_predictor_stack_noisy_dev";
    const DevRows x{X_d, x_type, ns, row_stride, col_stride}, psi{Psi_d, psi_type, ns, psi_row_stride, psi_col_stride};
    if (int rc = stack_check_shape(who, p, ns, ndraws, nbins, ngroups, edges, hist, sum_w, sum_mu, sum_mu2, X_d)) return rc;
    if (int rc = predictor_check_noisy_draws(who, p)) return rc;
    if (int rc = predictor_dev_args(who, p, x, muX, sdX)) return rc;
    if (int rc = predictor_dev_psi_args(who, psi, sdX, sd2)) return rc;
    if (int rc = stack_check_shift(who, p, mu_shift)) return rc;
    const int k = p->k, B = nbins, G = ngroups, C = 1 + ndraws;
    if (ns == 0) {
        stack_zero(C, k, G, B, hist, sum_w, sum_mu, sum_mu2);
        return 0;
    }
    std::vector<double> res((size_t)C * k * ((size_t)G * B + 3 * (size_t)G));
    if (int rc = predictor_call(p, who, [&] {
            const double *mx = nullptr, *sx = nullptr, *my = nullptr;
            int rc = predictor_noisy_prepare(p);
            if (!rc)   // the refusals of rows, Psi, labels and weights before any tile
                rc = predictor_dev_begin(p, who, x, muX, sdX, nullptr, group_d, G, weight_d, stream,
                                         "the rows have missing values (NaN): stacks are for complete rows", &mx, &sx, &my, &psi, sd2);
            if (!rc)
                rc = predictor_run_stack_noisy_dev(p, x, psi, mx, sx, sd2 ? p->sd2_d : nullptr, (int)ndraws, (unsigned long long)seed, Z,
                                                   edges, mu_shift, B, group_d, G, weight_d, res.data());
            return rc;
        }))
        return rc;   // the outputs are untouched
    stack_unpack(res.data(), C, k, G, B, hist, sum_w, sum_mu, sum_mu2);
    return 0;
}

extern "C" int gpz_predictor_draws_gamma_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                                     int64_t col_stride, const double *muX, const double *sdX, const double *muY,
                                                     const double *priors, uint32_t obs_mask, int32_t ndraws, uint64_t seed,
                                                     const double *Z, double *F_d, double *Gam_d, void *stream) {
    return draws_missing_dev_entry("gpz_predictor_draws_gamma_missing_dev", p, DevRows{X_d, x_type, ns, row_stride, col_stride}, muX, sdX,
                                   muY, priors, obs_mask, ndraws, seed, Z, F_d, stream, Gam_d, true);
}

extern "C" int gpz_predictor_stack_missing_dev(gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride,
                                               int64_t col_stride, const double *muX, const double *sdX, const double *priors,
                                               uint32_t obs_mask, int32_t ndraws, uint64_t seed, const double *Z, const double *edges,
                                               int32_t nbins, const int32_t *group_d, int32_t ngroups, const double *weight_d,
                                               double *hist, double *sum_w, double *sum_mu, double *sum_mu2, const double *mu_shift,
                                               void *stream) {
    const char *who = "gpz_predictor_stack_missing_dev";
    const DevRows x{X_d, x_type, ns, row_stride, col_stride};
    if (int rc = stack_check_shape(who, p, ns, ndraws, nbins, ngroups, edges, hist, sum_w, sum_mu, sum_mu2, X_d)) return rc;
    if (int rc = predictor_missing_check(who, p, obs_mask)) return rc;
    if (int rc = predictor_dev_args(who, p, x, muX, sdX)) return rc;
    if (int rc = stack_check_shift(who, p, mu_shift)) return rc;
    const int k = p->k, B = nbins, G = ngroups, C = 1 + ndraws;
    if (ns == 0) {
        stack_zero(C, k, G, B, hist, sum_w, sum_mu, sum_mu2);
        return 0;
    }
    std::vector<double> res((size_t)C * k * ((size_t)G * B + 3 * (size_t)G));
    if (int rc = predictor_call(p, who, [&] {
            const double *mx = nullptr, *sx = nullptr, *my = nullptr;
            const unsigned pat = obs_mask;
            // the refusals of rows, labels and weights before any tile
            int rc = predictor_dev_begin(p, who, x, muX, sdX, nullptr, group_d, G, weight_d, stream, kMissingPatternText, &mx, &sx, &my,
                                         nullptr, nullptr, &pat);
            if (rc) return rc;
            return predictor_run_stack_missing_dev(p, who, x, mx, sx, priors, obs_mask, (int)ndraws, (unsigned long long)seed, Z, edges,
                                                   mu_shift, B, group_d, G, weight_d, res.data());
        }))
        return rc;   // the outputs are untouched
    stack_unpack(res.data(), C, k, G, B, hist, sum_w, sum_mu, sum_mu2);
    return 0;
}

extern "C" int gpz_predictor_route(const gpz_predictor *p, char *buf, int cap) {
    if (!p || !buf || cap < 1) return gpz_fail(GPZ_ERR_ARG, "gpz_predictor_route: null argument");
    char tmp[160];
    if (p->route == 0)
        snprintf(tmp, sizeof tmp, "fused: k_predict_small, %lld-row tiles", (long long)p->tile_rows);
    else
        snprintf(tmp, sizeof tmp, "tiles: k_phi + k_tgemm, %lld-row tiles", (long long)p->tile_rows);
    std::string r = tmp;
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
    if (p->gam_used) {   // after the first stack or gamma-per-draw call for rows with input noise
        snprintf(tmp, sizeof tmp, "; noise per draw: k_predict_noisy_gamma (%d pair chunks)", p->gchunks);
        r += tmp;
        if (p->s2_d) r += " + k_stack_tile_w";   // the widths exist: a stack call was among them
    }
    if (p->miss_used) {   // after the first call for a group of rows with missing inputs
        snprintf(tmp, sizeof tmp, "; missing: k_predict_missing_pairs (%d pair chunks), %lld-row tiles", p->mchunks, (long long)p->mtile);
        r += tmp;
    }
    if (p->mgam_used) {   // after the first stack or gamma-per-draw call for such a group
        snprintf(tmp, sizeof tmp, "; missing per draw: k_predict_missing_gamma (%d pair chunks)", p->mchunks);
        r += tmp;
        if (p->ms2_d) r += " + k_stack_tile_w";   // the widths exist: a stack call was among them
    }
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
