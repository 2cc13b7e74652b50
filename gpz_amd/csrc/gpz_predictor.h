// Internal header of the streaming predictor (gpz_predictor_*): the handle and what its three translation units share.
//   gpz_predictor.hip       handle life and setup, the prepare and tile functions of every kind of rows, draws preparation and
//                           factorisation, what a stack call prepares and its tile, the checks the entries share, route and info
//   gpz_predictor_host.hip  the host pipeline (predictor_stage, predictor_pipeline), its jobs and the entries that take host arrays
//   gpz_predictor_dev.hip   the device-resident entries: DevRows, predictor_dev_begin, predictor_dev_tiles, predictor_dev_sync
#pragma once
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
    bool large_m = false;          // GPZ_PREDICT_LARGE_M: complete rows with Psi up to ceil16(m) <= 1024
    bool large_seen = false;       // such a handle past ceil16(m) = 256 has had a call with Psi (the route text)
    bool large_m_missing = false;  // GPZ_PREDICT_LARGE_M_MISSING: a group with missing inputs (diagonal kinds) up to ceil16(m) <= 1024
    bool mlarge_seen = false;      // such a handle past ceil16(m) = 256 has had a call for a group (the route text)
    int64_t ntile = 0;             // rows per tile of the calls that fill npart (the handle's tile, shrunk so that the slab is <= 1 GiB)
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
    // ---- gamma per draw and stacks of rows with input noise (gpz_predictor_stack_noisy*, _draws_gamma_noisy_dev) and of rows with missing
    // inputs (gpz_predictor_stack_missing_dev, _draws_gamma_missing_dev), of rows with both (gpz_predictor_stack_noisy_missing_dev,
    // _draws_gamma_noisy_missing_dev), and of rows with input noise on a covariance kind (gpz_predictor_stack_noisy_cov_dev,
    // _draws_gamma_noisy_cov_dev), and of rows with missing inputs on a covariance kind (gpz_predictor_stack_missing_cov_dev,
    // _draws_gamma_missing_cov_dev), and of such rows with input noise too (gpz_predictor_stack_noisy_missing_cov_dev,
    // _draws_gamma_noisy_missing_cov_dev): nothing of a kind before its first such call
    int gchunks = 0;               // predict_gamma_chunks of the model (input noise, either kind; a group with missing inputs has mchunks)
    double *gpart = nullptr;       // [chunks][nd k][tile] pair sums per chunk, of either kind
    size_t gpart_cap = 0;          // doubles
    struct PerDraw {
        bool used = false;
        double *s2_d = nullptr;    // [(1 + nd) k][tile] widths^2 of the stack
        size_t s2_cap = 0;         // doubles
    } gam[8];                      // [kind - 1] of the call's RowKind: ROWS_NOISY .. ROWS_PSI_CUBE_MISSING (clean rows have no gamma per draw)
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
    // ---- rows with input noise and missing inputs (gpz_predictor_*_noisy_missing_dev): beyond the buffers above and the Psi slots, which
    // such a call takes where the handle does not hold them yet, only this exists, and not before the first of their calls
    bool nm_used = false;
    double *nmrec = nullptr;       // the second pair-record table (k_pnm_records): the model's alone, written once
    // ---- input noise for the covariance kinds (gpz_predictor_*_noisy_cov_dev): beyond the Psi slots and, for the moments, nout and npart
    // (which a covariance kind has from nowhere else), only this exists, and not before the first of their calls
    bool ncov_ready = false;       // the pair records, the output slots and the chunk slab exist (the first call that reads the pairs)
    bool ncov_used = false;        // such a call (a variance per dimension) was the one that read them (the route text)
    int cchunks = 0;               // predict_noisy_cov_chunks of the model
    double *cbrec = nullptr, *cprec = nullptr;   // the basis and pair records (k_noisy_cov_records): the model's alone, written once
    double *cphi = nullptr;        // the draws (and a stack with draws): E_x[PHI] of a tile, [tile_pad][mp] (the tile route's own Phi where there is one)
    // ---- a full input-noise covariance per row for the covariance kinds (gpz_predictor_*_psi_cube_dev): the records, output slots, chunk
    // slab and PHI tile are the group's above, each taken where the handle does not hold it yet (the Psi slots of that group are not
    // needed and not taken).  Beyond them only this exists, and not before the first of their calls
    bool cube_used = false;        // a call that reads the pairs has run (the route text)
    double *Psiq[2] = {};          // the tile's packed lower triangles, [d (d + 1) / 2][tile_pad]
    double *div_d = nullptr;       // the divisors sdX[r] sdX[c] in LT order, d (d + 1) / 2
    // ---- rows with missing inputs for the covariance kinds (gpz_predictor_*_missing_cov_dev): the tile buffers, the priors and the
    // cache keys are the fields of the diagonal kinds' group above (mtile, mNo = PHI, mPio = [m][tile], mhd, mpart, mout, mpri, mtab_*;
    // mchunks = predict_missing_cov_chunks), which a covariance handle has from nowhere else.  Beyond them only this exists, and not
    // before the first of their calls
    bool mcov_used = false;
    double *mcSig = nullptr, *mclnS = nullptr, *mcraw = nullptr;   // the model's alone: Sigma_j, ln|Sigma_j|; with pairs launch_pair_table's records
    double *mcbas = nullptr, *mcex = nullptr, *mcphi = nullptr;    // the pattern's: [R | CU | off] per basis function, the Ex and PHI records
    double *mccoef = nullptr, *mcslab = nullptr;                   // with pairs: the 3k coefficients per pair, the slab of pair-component records
    bool mcslab_kept = false;      // the slab holds the whole table of (mtab_obs, mtab_pri)
    // ---- rows with input noise and missing inputs for the covariance kinds (gpz_predictor_*_noisy_missing_cov_dev): everything of the
    // group above and the Psi slots, each taken where the handle does not hold it yet.  Beyond them only this exists, and not before the
    // first of their calls
    bool nmcov_used = false;
    double *nmcex = nullptr, *nmcphi = nullptr, *nmcslab = nullptr;   // the Ex and PHI records and the slab in the form of k_predict_noisy_missing_cov.hip
    bool nmtab_valid = false;      // nmcex and nmcphi hold the records of (mtab_obs, mtab_pri); cleared where the tables above are written
    bool nmcslab_kept = false;     // nmcslab holds the whole pair-component table of (mtab_obs, mtab_pri)
    // ---- such rows with a full input-noise covariance each (gpz_predictor_*_psi_cube_missing_dev): everything of the group above but its
    // Psi slots (the records do not depend on Psi: a handle that has served that group on the same pattern builds nothing twice), and
    // Psiq and div_d of the cube kind, whose first no (no + 1) / 2 columns hold the observed triangles.  Beyond them only this exists
    bool pcm_used = false;         // such a call has run (the route text)
};

namespace gpzi {
// The kind of rows of a call.  Clean: complete rows.  Noisy: rows with Psi in Psic[s] beside Xc[s].  Missing: one group of rows that
// share the NaN pattern obs (the bit mask of the observed dimensions), with the priors of the set (m values, or nullptr for 1 / m).
// Noisy missing: such a group with Psi in Psic[s] too (read in the observed dimensions only).  Noisy cov: complete rows with Psi of a
// covariance kind (a handle has either this kind or the diagonal noisy one, never both).  What a tile is made of for a kind is answered by the rows_* functions below; the runners of every entry go through them.
// Missing cov: a group without Psi on a covariance kind.  Noisy missing cov: such a group with Psi in Psic[s] too; with nothing observed
// (obs = 0) there is no Psi to read and the group is the missing cov kind's in all but the name of its entry.
// Psi cube: complete rows of a covariance kind with a full d x d Psi each, its packed lower triangle in Psiq[s] beside Xc[s]; the tables
// are the noisy cov kind's.  Psi cube missing: a group on a covariance kind whose rows have a full d x d Psi each; the lower triangle of
// its observed x observed block lies packed in Psiq[s] (no (no + 1) / 2 columns), the tables are the noisy missing cov kind's, and with
// nothing observed there is no Psi to read and the group is the missing cov kind's, as for that kind.
enum RowKind {
    ROWS_CLEAN = 0, ROWS_NOISY = 1, ROWS_MISSING = 2, ROWS_NOISY_MISSING = 3, ROWS_NOISY_COV = 4, ROWS_MISSING_COV = 5,
    ROWS_NOISY_MISSING_COV = 6, ROWS_PSI_CUBE = 7, ROWS_PSI_CUBE_MISSING = 8
};
struct Rows {
    RowKind kind = ROWS_CLEAN;
    uint32_t obs = 0;
    const double *priors = nullptr;
    bool psi() const {   // Psic[s] is staged beside Xc[s]
        return kind == ROWS_NOISY || kind == ROWS_NOISY_MISSING || kind == ROWS_NOISY_COV || (kind == ROWS_NOISY_MISSING_COV && obs != 0);
    }
    bool group() const {   // one NaN pattern, tiles of at most mtile rows
        return kind == ROWS_MISSING || kind == ROWS_NOISY_MISSING || kind == ROWS_MISSING_COV || kind == ROWS_NOISY_MISSING_COV ||
               kind == ROWS_PSI_CUBE_MISSING;
    }
    bool cube() const { return kind == ROWS_PSI_CUBE; }   // Psiq[s] is staged beside Xc[s]
    bool ncov() const { return kind == ROWS_NOISY_COV || kind == ROWS_PSI_CUBE; }   // complete rows of a covariance kind with Psi, either form
    bool cov_group() const {   // such a group on a covariance kind
        return kind == ROWS_MISSING_COV || kind == ROWS_NOISY_MISSING_COV || kind == ROWS_PSI_CUBE_MISSING;
    }
    bool cube_obs() const { return kind == ROWS_PSI_CUBE_MISSING && obs != 0; }   // Psiq[s] holds the observed sub-triangle of each row's Psi
    bool group_psi() const { return cube_obs() || (kind == ROWS_NOISY_MISSING_COV && obs != 0); }   // a covariance group with Psi, either form
};

// ---- what a kind of rows is made of (gpz_predictor.hip) ------------------------------------------------------------------------------
int rows_check(const char *who, const gpz_predictor *p, const Rows &r, bool draws);
int rows_prepare(gpz_predictor *p, const char *who, const Rows &r, bool pairs);
int64_t rows_tile(const gpz_predictor *p, const Rows &r, int64_t T);
int rows_moments_tile(gpz_predictor *p, const char *who, const Rows &r, int s, int nt, bool want_phi);
const double *rows_moments(const gpz_predictor *p, const Rows &r, int s);
int rows_draws_prepare(gpz_predictor *p, const Rows &r, int nd, unsigned long long seed, const double *Z, bool pinned, int64_t *Tout);
int rows_draws_tile(gpz_predictor *p, const char *who, const Rows &r, int s, int nt, int ncol, int ldw, bool after_moments);
int rows_gamma_prepare(gpz_predictor *p, const Rows &r, int ncol, int Q, int64_t T);
int rows_gamma_tile(gpz_predictor *p, const char *who, const Rows &r, int s, int nt, int ncol, int ldw);
int rows_chunks(const gpz_predictor *p, const Rows &r);

int predictor_want_phi(gpz_predictor *p, bool pinned = true);
int predictor_psi_slots(gpz_predictor *p);

// ---- stack ---------------------------------------------------------------------------------------------------------------------------
struct StackCall {
    int nd, B, G, ncol, ldw;
    int R;           // row slabs per tile
    size_t ne;       // the edges; behind them in edges_d, the k shifts of the sums
    size_t count;    // doubles in the accumulators
    int64_t T;       // rows per tile
};
// the arguments of every stack entry behind its rows
struct StackArgs {
    int32_t ndraws;
    uint64_t seed;
    const double *Z, *edges;
    int32_t nbins;
    const int32_t *group;
    int32_t ngroups;
    const double *weight;
    double *hist, *sum_w, *sum_mu, *sum_mu2;
    const double *mu_shift;
};
int predictor_stack_prepare(gpz_predictor *p, const char *who, const Rows &r, const StackArgs &a, bool pinned, StackCall *c);
int predictor_stack_tile(gpz_predictor *p, const char *who, const Rows &r, const StackCall &c, int s, int64_t nt, const int *lab,
                         const double *wt);
int predictor_stack_result(gpz_predictor *p, const char *who, const StackCall &c, double *res);

// ---- what the entries share ----------------------------------------------------------------------------------------------------------
int predictor_check_call(const char *who, const gpz_predictor *p, int64_t ns);
int predictor_check_ndraws(const char *who, const gpz_predictor *p, int32_t ndraws, int least);
int stack_check_shape(const char *who, const gpz_predictor *p, int64_t ns, const StackArgs &a, const void *Xs);
int stack_check_shift(const char *who, const gpz_predictor *p, const double *mu_shift);
void stack_zero(const gpz_predictor *p, const StackArgs &a);
void stack_unpack(const gpz_predictor *p, const StackArgs &a, const double *res);

// Every entry after create runs its body through here: the handle's options and device for the length of the call, the caller's device
// again on every way out.
template <class Body>
int predictor_call(gpz_predictor *p, const char *who, Body body) {
    int prev = 0;
    (void)hipGetDevice(&prev);
    gpz_opts_scope opts_scope(&p->opt);
    int rc = 0;
    if (hipSetDevice(p->device) != hipSuccess) rc = gpz_fail(GPZ_ERR_HIP, "%s: hipSetDevice failed", who);
    if (!rc) rc = body();
    (void)hipSetDevice(prev);
    return rc;
}

// Every stack entry: the shape checks in the order gpz_predictor_stack has always made them, the entry's own (check: the kind's, then
// the host loop over the labels or the layout of the device rows), the shift, what the entry checks behind it (late: the host loop over
// the weights), the empty call, and run(res) inside predictor_call with the records that stack_unpack takes apart.
// zero_first: gpz_predictor_stack alone clears its outputs once its arguments have passed, so a refusal of its rows leaves zeros; the
// entries added after it leave their outputs untouched on every refusal.  Callers rely on either, so both stay.
template <class Check, class Late, class Run>
int stack_entry(const char *who, gpz_predictor *p, int64_t ns, const void *Xs, const StackArgs &a, bool zero_first, Check check, Late late,
                Run run) {
    if (int rc = stack_check_shape(who, p, ns, a, Xs)) return rc;
    if (int rc = check()) return rc;
    if (int rc = stack_check_shift(who, p, a.mu_shift)) return rc;
    if (int rc = late()) return rc;
    if (zero_first || ns == 0) stack_zero(p, a);
    if (ns == 0) return 0;
    std::vector<double> res((size_t)(1 + a.ndraws) * p->k * ((size_t)a.ngroups * a.nbins + 3 * (size_t)a.ngroups));
    if (int rc = predictor_call(p, who, [&] { return run(res.data()); })) return rc;
    stack_unpack(p, a, res.data());
    return 0;
}
}   // namespace gpzi
