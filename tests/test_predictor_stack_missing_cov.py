"""The stacked n(z) and gamma under every weight draw for rows with missing inputs on a covariance kind (Predictor.stack_missing_cov_dev /
draws_missing_cov_dev(..., return_gamma=True); k_predict_missing_cov_gamma.hip) against the existing entries of the handle,
``gpz_amd.predict`` and the oracle: gamma_s against predict_missing_cov_dev's gamma of the model whose weights are the draw's at every
pair-count, chunk, slab and column edge and every number of observed dimensions, the same bits over tiles, orders, company, splits and
layouts, the stack against a torch reduction of the device's own per-row numbers, the state of the slab, a handle shared with the
noisy entries, the refusals of the C entries and constant memory.

Gates.  gamma_s with exact weights: ten times the largest nrel against predict_missing_cov_dev of the w := w_s model seen on an MI355X
over the cases of test 1 and test 3, rounded up to a power of ten and never looser than 1e-9 (GATE_GAMMA; the largest values seen:
GATE_SEEN), and rel <= 1e-8 against the oracle.  With a general iSigma_w: max(1e-11, 10 x the spread of the parent's two routes).  The
stack: the derived tolerances of tests/test_predictor_stack_missing.py, unchanged, with s_min taken over the new widths."""
import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, nrel, synth_model
from test_predictor_draws_cpu import philox_normals
from test_predictor_missing import knock_out, model_with_priors
from test_predictor_missing_cov_cpu import chunks_rule, slabs_rule
from test_predictor_noisy import noise
from test_predictor_stack import EPS, assert_close, setting, stack_slabs
from test_predictor_stack_noisy import with_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COV = ("GC", "VC")
NAN = float("nan")
# the largest nrel of gamma_s against predict_missing_cov_dev of the w_s model seen on an MI355X: over the 28 cases of test 1, over the 9
# of test 3; the largest rel against the oracle (m <= 7, 60 rows)
GATE_SEEN = {"exact weights": 1.08e-14, "column edges": 6.62e-14, "oracle": 7.94e-15}
GATE_GAMMA = 1e-12


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def gamma_of(model, X, tile_rows=256):
    """predict_missing_cov_dev's gamma on a handle of its own: existing code."""
    with gpz_amd.Predictor(model, tile_rows=tile_rows) as q:
        return host(q.predict_missing_cov_dev(dev(X))[4])


def exact_model(method, m, d, k, hetero, seed):
    """iSigma_w = 2^-10 I: its Cholesky factor is exactly 2^-5 I, so w_s = w + 2^-5 z_s is the same double on host and device."""
    model = model_with_priors(method, m, d, k, hetero, seed=seed)
    model.sets["best"]["iSigma_w"] = np.stack([2.0 ** -10 * np.eye(m)] * k, axis=2)
    return model


def exact_weights(model, Z):
    return model.sets["best"]["w"][:, None, :] + 2.0 ** -5 * Z             # (m, nd, k)


def route_tail(m, stack=False):
    return f"; missing per draw: k_predict_missing_cov_gamma ({chunks_rule(m)} pair chunks)" + (" + k_stack_tile_w" if stack else "")


def gam(p, x, nd, **kw):
    return p.draws_missing_cov_dev(x, nd, return_gamma=True, **kw)[1]


# ---- 1. gamma_s with exact weights --------------------------------------------------------------------------------------------------------
# (m, d, k, n_draws): the pair-count and chunk edges in m at d = 3 with dimension 1 missing (NO = 2); m = 140 | 141 one slab | two;
# then d = 1 .. 10 with the last dimension missing, NO = 0 .. 9, at m = 20.  64 draws only where m <= 33; k = 8 with 17 draws is 136
# columns, a second pass of one block.
M_CASES = [(1, 3, 1, 17), (2, 3, 3, 5), (7, 3, 8, 5), (10, 3, 1, 64), (11, 3, 1, 5), (15, 3, 3, 1), (16, 3, 1, 17), (22, 3, 8, 17),
           (23, 3, 1, 5), (31, 3, 1, 64), (32, 3, 3, 5), (33, 3, 1, 17), (250, 3, 1, 5), (140, 3, 1, 1), (141, 3, 1, 5),
           (7, 5, 1, 64), (5, 10, 3, 1), (7, 1, 8, 17)]
NO_CASES = [(20, d, (1, 3, 8)[d % 3], (5, 1, 17)[d % 3]) for d in range(1, 11)]
CASES = M_CASES + NO_CASES


@pytest.mark.parametrize("m,d,k,nd", CASES)
def test_gamma_per_draw_with_exact_weights(m, d, k, nd):
    """The reference is predict_missing_cov_dev's gamma of the model with w := w_s on a handle of its own (the same quantity by
    definition, existing code), per draw, over the rows with missing values.  300 rows of one pattern on 256-row tiles: a full tile and
    a partial one, and a last workgroup of 44 rows; behind them ten rows with nothing observed (NO = 0; at d = 1 they are the same
    pattern, the only input missing).  m = 1, 2, 7 are 1, 3 and 28 pairs: a partial K step; 10 | 11, 15 | 16, 22 | 23, 31 | 32 are the
    chunk counts 1 | 2, 2 | 4, 4 | 8, 8 | 16; m = 33 has components past two 16-record stages; m = 250 passes eight slabs.  Where
    m <= 7, the first 60 rows against the oracle's gamma of the w_s model at rel <= 1e-8, on the first, the middle and the last draw."""
    assert slabs_rule(140, 2) == 1 and slabs_rule(141, 2) == 2 and slabs_rule(250, 2) == 8
    ns = 310
    model = exact_model(COV[(m + d) % 2], m, d, k, bool((m + k) % 2), seed=12000 + 100 * d + 10 * k + m)
    X = catalogue(model, ns, seed=m + d)
    X[:300, 1 if (d == 3 and (m, d, k, nd) in M_CASES) else d - 1] = NAN
    X[300:, :] = NAN
    Z = np.random.default_rng(nd + m).standard_normal((m, nd, k))
    W = exact_weights(model, Z)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F, Gam = p.draws_missing_cov_dev(dev(X), nd, Z=Z, return_gamma=True)
        assert p.route.endswith(route_tail(m)), p.route
        assert "k_stack_tile" not in p.route                             # no stack call on this handle
        assert torch.equal(F, p.draws_missing_cov_dev(dev(X), nd, Z=Z))
    assert Gam.shape == (nd, ns, k) and Gam.dtype == torch.float64
    Gam = host(Gam)
    worst, worst_orc = 0.0, 0.0
    for s in range(nd):
        ms = with_weights(model, W[:, s, :])
        worst = max(worst, nrel(Gam[s], gamma_of(ms, X)))
        if m <= 7 and s in {0, nd // 2, nd - 1}:
            worst_orc = max(worst_orc, rel(Gam[s, :60], O.predict_any(X[:60], ms)[4]))
    print(f"m={m} d={d} k={k} nd={nd}: worst nrel of gamma_s against predict_missing_cov_dev of the w_s model {worst:.3g}; "
          f"worst rel against the oracle {worst_orc:.3g}")
    assert worst <= GATE_GAMMA, worst
    assert worst_orc <= 1e-8, worst_orc


# ---- 2. gamma_s with a general iSigma_w ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
def test_gamma_per_draw_with_seeded_draws(method):
    """Seeded draws of a general iSigma_w; w_s formed on the host as w + chol(sym(iSigma_w)) z_s with the Philox normals of the seed.
    Yardstick: the disagreement of two routes of the parent, gamma of the w := w_s model from the handle's predict_missing_cov_dev
    against gpz_amd.predict.  Gate: max(1e-11, 10 x that spread) - the factor 10 for a third summation order and the host-formed w_s."""
    m, d, k, nd, ns, seed = 60, 5, 2, 6, 600, 31
    model = model_with_priors(method, m, d, k, True, seed=77)
    X = knock_out(catalogue(model, ns, seed=78), seed=79)
    miss = np.isnan(X).any(axis=1)
    z = philox_normals(seed, m, nd, k)
    iS = model.sets["best"]["iSigma_w"]
    L = [np.linalg.cholesky(0.5 * (iS[:, :, o] + iS[:, :, o].T)) for o in range(k)]
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        Gam = host(gam(p, dev(X), nd, seed=seed))
    figures = []
    for s in range(nd):
        ws = np.stack([model.sets["best"]["w"][:, o] + L[o] @ z[:, s, o] for o in range(k)], axis=1)
        ms = with_weights(model, ws)
        a = gamma_of(ms, X)
        b = np.array(gpz_amd.predict(X, ms)[4])
        figures.append((nrel(Gam[s][miss], a[miss]), nrel(a[miss], b[miss])))
        print(f"{method} draw {s}: nrel(gamma_s, predict_missing_cov_dev of w_s) {figures[-1][0]:.3g}; spread of the parent's two routes "
              f"{figures[-1][1]:.3g}")
        assert np.all(Gam[s][~miss] == 0.0)
    for s, (got, spread) in enumerate(figures):
        assert got <= max(1e-11, 10 * spread), (s, got, spread)


# ---- 3. column edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncol,k", [(1, 1), (15, 3), (16, 1), (17, 1), (64, 8), (65, 1), (128, 8), (129, 1), (257, 1)])
def test_column_edges(ncol, k):
    """m = 17, d = 3, VC: n_draws k at a partial block, a full block, the pass edge on gridDim.z (8 blocks, 128 columns) and one column
    past two full passes; rows at the edges of a wave's 16 rows and a workgroup's 64.  Each case against test 1's reference on the
    first, the middle and the last draw."""
    m, d, nmax, nd = 17, 3, 300, ncol // k
    model = exact_model("VC", m, d, k, True, seed=1300 + ncol)
    X = catalogue(model, nmax, seed=ncol)
    X[:, 2] = NAN
    Z = np.random.default_rng(ncol).standard_normal((m, nd, k))
    W = exact_weights(model, Z)
    draws = sorted({0, nd // 2, nd - 1})
    ref = {s: gamma_of(with_weights(model, W[:, s, :]), X) for s in draws}
    Xd = dev(X)
    worst = 0.0
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        for n in (1, 15, 16, 17, 63, 64, 65, 300):
            Gam = gam(p, Xd[:n], nd, Z=Z)
            assert Gam.shape == (nd, n, k) and bool(torch.isfinite(Gam).all())
            for s in draws:
                worst = max(worst, nrel(host(Gam[s]), ref[s][:n]))
    print(f"ncol={ncol} k={k}: worst nrel {worst:.3g}")
    assert worst <= GATE_GAMMA, worst


# ---- 4. the same bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,m,k", [("VC", 40, 2), ("GC", 23, 1)])
def test_same_bits_over_tiles_orders_company_splits_layouts_and_draws(method, m, k):
    n, d, nd = 1400, 5, 5
    model = model_with_priors(method, m, d, k, True, seed=181 + m)
    X32 = knock_out(catalogue(model, n, seed=82), seed=83).astype(np.float32)
    X = X32.astype(np.float64)
    Xd = dev(X)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    Z17 = np.random.default_rng(2).standard_normal((m, 17, k))
    codes = np.isnan(X) @ (1 << np.arange(d))
    full = torch.from_numpy(codes == 0).to(DEV)

    def both(q, x, ndr=nd, **kw):
        return q.draws_missing_cov_dev(x, ndr, Z=Z17[:, :ndr], return_gamma=True, **kw)

    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F5, G5 = both(p, Xd)
        assert torch.equal(p.draws_missing_cov_dev(Xd, nd, Z=Z17[:, :nd]), F5), "F against the call without return_gamma"
        assert bool((G5[:, full] == 0.0).all()) and bool((G5[:, ~full] != 0.0).all())
        assert torch.equal(F5[:, full], p.draws_dev(Xd[full], nd, Z=Z17[:, :nd])), "complete rows: draws_dev's"
        F17, G17 = both(p, Xd, 17)
        assert torch.equal(G17[:nd], G5) and torch.equal(F17[:nd], F5), "the first 5 of 17 draws"
        Fp, Gp = both(p, Xd[perm])
        assert torch.equal(Gp, G5[:, perm]) and torch.equal(Fp, F5[:, perm]), "a row permutation"
        halves = [both(p, Xd[:333]), both(p, Xd[333:])]
        assert torch.equal(torch.cat([h[1] for h in halves], dim=1), G5), "a split into two calls"
        for code in np.unique(codes):                                      # a row alone, a row among its group only
            rows = np.flatnonzero(codes == code)
            r = int(rows[len(rows) // 2])
            assert torch.equal(both(p, Xd[r:r + 1])[1], G5[:, r:r + 1]), ("alone", code)
            assert torch.equal(both(p, Xd[torch.from_numpy(rows).to(DEV)])[1], G5[:, rows]), ("its group", code)
        X2 = dev(np.repeat(X, 2, axis=0))
        wide = torch.full((n, 2 * d), 3.0, dtype=torch.float64, device=DEV)
        wide[:, ::2] = Xd
        for x, what in ((dev(X32, torch.float32), "float32"), (Xd.T.contiguous().T, "transposed"), (X2[::2], "row-sliced"),
                        (dev(X32, torch.float32).T.contiguous().T, "float32 transposed"), (wide[:, ::2], "column-strided")):
            Fx, Gx = both(p, x)
            assert torch.equal(Gx, G5) and torch.equal(Fx, F5), what
        sel = torch.zeros(n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        assert torch.equal(both(p, Xd, selection=sel)[1], G5[:, ::2]), "selection"
    for T in (64, 1024, None):
        with gpz_amd.Predictor(model, tile_rows=T) as q:
            Fq, Gq = both(q, Xd)
            assert torch.equal(Gq, G5) and torch.equal(Fq, F5), T


# ---- 5. stack parity --------------------------------------------------------------------------------------------------------------------
def torch_reference(mu0, s2_0, F, S2, edges, lab, wt, G):
    """The stack's definition as a torch reduction on the device: column 0 N(mu0, s2_0), column 1 + s N(F[s], S2[s]); hist (1 + S, G, k,
    B), sum_w (G,), sum_mu and sum_mu2 (1 + S, G, k) as NumPy arrays.  lab (n,) int64 in [-1, G), wt (n,), edges (B + 1,)."""
    cols = [(mu0, s2_0)] + ([] if F is None else [(F[s], S2[s]) for s in range(F.shape[0])])
    keep = lab >= 0
    n, k = mu0.shape
    B = edges.numel() - 1
    hist = torch.zeros((len(cols), G, k, B), dtype=torch.float64, device=mu0.device)
    sum_mu = torch.zeros((len(cols), G, k), dtype=torch.float64, device=mu0.device)
    sum_mu2 = torch.zeros_like(sum_mu)
    sum_w = torch.zeros(G, dtype=torch.float64, device=mu0.device).index_add_(0, lab[keep], wt[keep])
    for c, (mc, vc) in enumerate(cols):
        cdf = torch.special.ndtr((edges[None, None, :] - mc[:, :, None]) / torch.sqrt(vc)[:, :, None])
        mass = (cdf[:, :, 1:] - cdf[:, :, :-1]) * wt[:, None, None]
        hist[c].index_add_(0, lab[keep], mass[keep])
        sum_mu[c].index_add_(0, lab[keep], (wt[:, None] * mc)[keep])
        sum_mu2[c].index_add_(0, lab[keep], (wt[:, None] * mc * mc)[keep])
    return tuple(host(t) for t in (hist, sum_w, sum_mu, sum_mu2))


def stack_inputs(p, model, Xd, edges, n_draws, draw_kw, groups, weights, G):
    """torch_reference fed with the device's own per-row numbers (predict_missing_cov_dev and draws_missing_cov_dev(return_gamma=True)),
    and the tolerances of test_predictor_stack_missing.py's stack_inputs with s_min over the new widths."""
    mu_t, sigma_t, _, beta_t = p.predict_missing_cov_dev(Xd)[:4]
    Ft = S2t = None
    if n_draws:
        Ft, Gt = p.draws_missing_cov_dev(Xd, n_draws, return_gamma=True, **draw_kw)
        Ft, S2t = Ft.contiguous(), beta_t[None] + torch.clamp(Gt, min=0.0)
    ref = torch_reference(mu_t, sigma_t, Ft, S2t, dev(edges), dev(groups, torch.int64), dev(weights), G)
    mu, sigma = host(mu_t), host(sigma_t)
    F, S2 = (None, None) if Ft is None else (host(Ft), host(S2t))
    n, k = mu.shape
    g, w = np.asarray(groups), np.asarray(weights, dtype=np.float64)
    cols = [mu] + ([] if F is None else list(F))
    muY = np.asarray(model.muY).reshape(-1)
    E = max(np.max(np.abs(np.asarray(edges)[None, :] - muY[:, None])), 0.0) + max(np.max(np.abs(c - muY)) for c in cols)
    s_min = np.sqrt(min(sigma.min(), S2.min() if S2 is not None else sigma.min()))
    W = np.array([w[g == gi].sum() for gi in range(G)])
    ng = np.array([(g == gi).sum() for gi in range(G)])
    tol_h = EPS * W * (ng + 64.0 * (1.0 + E / s_min))
    tol_m = np.empty((len(cols), G, k, 2))
    for c, m_ in enumerate(cols):
        for gi in range(G):
            r = g == gi
            tol_m[c, gi, :, 0] = ng[gi] * EPS * (w[r] @ np.abs(m_[r]))
            tol_m[c, gi, :, 1] = ng[gi] * EPS * (w[r] @ (m_[r] * m_[r]))
    return ref, tol_h, tol_m, ng * EPS * W, mu


def same_stack(a, b, what):
    for f, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), (what, f)


@pytest.mark.parametrize("method", COV)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_stack_parity(method, hetero, k):
    """1500 rows on 1024-row tiles, dimension 1 missing on 20 % and dimension 4 on 10 % of the rows independently (four patterns), three
    groups with rows left out and random weights, 1, 37 and 300 bins, no draws and 5 seeded draws; a selection; column 0 against the
    call without draws bit for bit."""
    d, ns, G, m = 5, 1500, 3, 24
    model = model_with_priors(method, m, d, k, hetero, seed=4300 + 100 * COV.index(method) + 10 * k + hetero)
    X = knock_out(catalogue(model, ns, seed=k + 40), seed=k + 41)
    Xd = dev(X)
    groups, weights = setting(ns, G, seed=m)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        mu0 = host(p.predict_missing_cov_dev(Xd)[0])
        for B in (1, 37, 300):
            edges = np.linspace(*np.percentile(mu0, [3, 97]), B + 1)
            res = {}
            for nd in (0, 5):
                ref, th, tm, tw, mu = stack_inputs(p, model, Xd, edges, nd, dict(seed=77), groups, weights, G)
                rd = res[nd] = p.stack_missing_cov_dev(Xd, edges, n_draws=nd, seed=77, groups=gd, n_groups=G, weights=wd)
                what = f"{method} hetero={hetero} k={k} B={B} draws={nd}"
                assert rd.hist.shape == (1 + nd, G, k, B)
                assert_close(rd, ref, th, tm, tw, what)
                if nd:
                    assert rd.hist[1:].sum() > 0.0
            same_stack([res[5].hist[:1], res[5].sum_w, res[5].sum_mu[:1], res[5].sum_mu2[:1]], res[0][:4], "column 0 of the call with draws")
        sel = torch.zeros(ns, dtype=torch.bool, device=DEV)
        sel[::2] = True
        same_stack(p.stack_missing_cov_dev(Xd, edges, n_draws=5, seed=77, groups=gd, n_groups=G, weights=wd, selection=sel),
                   p.stack_missing_cov_dev(Xd[::2].contiguous(), edges, n_draws=5, seed=77, groups=gd[::2], n_groups=G, weights=wd[::2]),
                   "selection")
        assert p.route.endswith(route_tail(m, stack=True)), p.route


def test_a_catalogue_is_the_sum_of_its_patterns_and_complete_rows_are_stack_dev():
    n, d, m, k, nd, G = 1400, 5, 24, 2, 5, 3
    model = model_with_priors("VC", m, d, k, True, seed=281)
    X = knock_out(catalogue(model, n, seed=82), seed=83)
    Xd = dev(X)
    groups, weights = setting(n, G, seed=5)
    gd, wd = dev(groups, torch.int64), dev(weights)
    codes = np.isnan(X) @ (1 << np.arange(d))
    kw = dict(n_draws=nd, seed=9, n_groups=G)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        edges = np.linspace(*np.percentile(host(p.predict_missing_cov_dev(Xd)[0]), [3, 97]), 51)
        whole = p.stack_missing_cov_dev(Xd, edges, groups=gd, weights=wd, **kw)
        same_stack(p.stack_missing_cov_dev(Xd, edges, groups=gd, weights=wd, **kw), whole, "the same call twice")
        total = None
        for code in np.unique(codes):                                      # ascending pattern code
            idx = torch.from_numpy(np.flatnonzero(codes == code)).to(DEV)
            one = (p.stack_dev if code == 0 else p.stack_missing_cov_dev)(Xd[idx], edges, groups=gd[idx], weights=wd[idx], **kw)
            total = list(one[:4]) if total is None else [t + a for t, a in zip(total, one[:4])]
        same_stack(total, whole[:4], "the += of the single-pattern calls")
        full = torch.from_numpy(codes == 0).to(DEV)
        same_stack(p.stack_missing_cov_dev(Xd[full], edges, groups=gd[full], weights=wd[full], **kw),
                   p.stack_dev(Xd[full], edges, groups=gd[full], weights=wd[full], **kw), "a catalogue without NaN")


# ---- 6. the state of the slab ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [30, 141])
def test_the_slab_is_filled_by_whichever_kernel_comes_first(m):
    """m = 30 keeps its table in one slab on the handle, m = 141 at d = 3 with one dimension missing passes two slabs per tile.  A fresh
    handle whose first call is return_gamma=True (the gamma kernel fills the slab) followed by predict_missing_cov_dev (which reads
    it), and pattern A, then B, then A again: every call gives the bits of the same call on a fresh handle."""
    assert slabs_rule(30, 2) == 1 and slabs_rule(141, 2) == 2
    d, k, n, nd = 3, 1, 300, 3
    model = model_with_priors("VC", m, d, k, True, seed=600 + m)
    XA, XB = catalogue(model, n, seed=61), catalogue(model, n, seed=62)
    XA[:, 1] = NAN
    XB[:, 0] = NAN
    XA, XB = dev(XA), dev(XB)

    def moments(q, x):
        return q.predict_missing_cov_dev(x)

    def gamma(q, x):
        return q.draws_missing_cov_dev(x, nd, seed=4, return_gamma=True)

    fresh = {}
    for name, call, x in (("moments A", moments, XA), ("gamma A", gamma, XA), ("moments B", moments, XB), ("gamma B", gamma, XB)):
        with gpz_amd.Predictor(model, tile_rows=256) as q:
            fresh[name] = call(q, x)

    def same(got, name):
        assert all(torch.equal(a, b) for a, b in zip(got, fresh[name])), name

    with gpz_amd.Predictor(model, tile_rows=256) as p:                     # gamma first, then the moments
        same(gamma(p, XA), "gamma A")
        same(moments(p, XA), "moments A")
        same(gamma(p, XA), "gamma A")
    with gpz_amd.Predictor(model, tile_rows=256) as p:                     # A, B, A, each with both kernels in either order
        same(moments(p, XA), "moments A")
        same(gamma(p, XB), "gamma B")
        same(moments(p, XB), "moments B")
        same(gamma(p, XA), "gamma A")
        same(moments(p, XA), "moments A")
        same(moments(p, XB), "moments B")
        same(gamma(p, XB), "gamma B")


# ---- 7. sharing a handle ------------------------------------------------------------------------------------------------------------------
def test_noisy_and_missing_stacks_share_a_handle_in_either_order():
    """stack_noisy_cov_dev and stack_missing_cov_dev on one handle: gpart, the widths' neighbours and the two chunk counts are shared
    state.  m = 100 has 2 chunks of the noisy kind and 16 of the missing one.  In either order each call gives the bits of a fresh
    handle."""
    m, d, k, n, nd, G = 100, 3, 2, 300, 4, 2
    model = model_with_priors("VC", m, d, k, True, seed=4243)
    X = catalogue(model, n, seed=3)
    Xd, Xm = dev(X), dev(knock_out(X, seed=4, cols=((0, 0.3), (2, 0.2))))
    Psi = dev(noise(n, d, seed=5))
    e = np.linspace(-2.0, 2.0, 41) + float(np.mean(model.muY))
    calls = {"noisy": lambda p: p.stack_noisy_cov_dev(Xd, Psi, e, n_draws=nd, seed=6, n_groups=G),
             "missing": lambda p: p.stack_missing_cov_dev(Xm, e, n_draws=nd, seed=6, n_groups=G),
             "missing gamma": lambda p: p.draws_missing_cov_dev(Xm, nd + 3, seed=7, return_gamma=True),
             "noisy gamma": lambda p: p.draws_noisy_cov_dev(Xd, Psi, nd + 1, seed=8, return_gamma=True)}
    alone = {}
    for name, call in calls.items():
        with gpz_amd.Predictor(model, tile_rows=256) as p:
            alone[name] = call(p)

    def same(got, name, order):
        for u, v in zip(got, alone[name]):
            assert (torch.equal(u, v) if isinstance(u, torch.Tensor) else np.array_equal(u, v)), (order, name)

    for order in (("noisy", "missing", "noisy gamma", "missing gamma", "noisy", "missing"),
                  ("missing", "noisy", "missing gamma", "noisy gamma", "missing", "noisy")):
        with gpz_amd.Predictor(model, tile_rows=256) as p:
            for name in order:
                same(calls[name](p), name, order)
            assert "k_predict_noisy_cov_gamma" in p.route and "k_predict_missing_cov_gamma" in p.route, p.route


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
ERR_ARG, ERR_UNSUPPORTED = -1, -5                                        # include/gpz_hip.h


def raw_calls(p, x, obs, nd, G, B, lab=None, wt=None):
    """Both C entries on one group with every output preset to -7: (rc of the stack, rc of the draws), their messages, the outputs."""
    k, n = p._k, x.shape[0]
    muX, sdX, muY = p._norm_vectors()
    stream = torch.cuda.current_stream(x.device).cuda_stream
    es = np.ascontiguousarray(np.linspace(-3, 3, B + 1)[None, :] - muY[:, None])
    out = [np.full(s, -7.0) for s in ((1 + nd, G, k, B), (G,), (1 + nd, G, k), (1 + nd, G, k))]
    h = p._handle()
    rc1 = p._lib.gpz_predictor_stack_missing_cov_dev(h, *p._x_args(x), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(p._priors), obs, nd, 5,
                                                     None, _lib.dptr(es), B, None if lab is None else lab.data_ptr(), G,
                                                     None if wt is None else wt.data_ptr(), *(_lib.dptr(a) for a in out), _lib.dptr(muY),
                                                     stream)
    msg1 = p._lib.gpz_last_error().decode() if rc1 else ""
    Fd = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    Gm = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    rc2 = p._lib.gpz_predictor_draws_gamma_missing_cov_dev(h, *p._x_args(x), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                           _lib.dptr(p._priors), obs, nd, 5, None, Fd.data_ptr(), Gm.data_ptr(), stream)
    msg2 = p._lib.gpz_last_error().decode() if rc2 else ""
    torch.cuda.synchronize()
    return (rc1, rc2), (msg1, msg2), out, [Fd, Gm]


def untouched(out, FG):
    return all(np.all(a == -7.0) for a in out) and all(bool((t == -7.0).all()) for t in FG)


@pytest.mark.parametrize("kw", [{"method": "VD"}, {"m": 257}, {"d": 11}, {"k": 9}])
def test_models_outside_the_scope_are_refused_by_the_c_entries(kw):
    a = {"method": "VC", "m": 20, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    X = catalogue(model, 40, seed=6)
    X[:, 1] = NAN
    diag = a["method"] == "VD"
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match="stack_missing_dev" if diag else "predict_missing_cov_fits"):
            p.stack_missing_cov_dev(dev(X), np.linspace(-3, 3, 11), n_draws=2)
        with pytest.raises(ValueError, match="draws_dev" if diag else "predict_missing_cov_fits"):
            p.draws_missing_cov_dev(dev(X), 4, return_gamma=True)
        held = p.info[1]
        rcs, msgs, out, FG = raw_calls(p, dev(X), (1 << a["d"]) - 3, 3, 2, 10)
        assert rcs == (ERR_UNSUPPORTED, ERR_UNSUPPORTED), (rcs, msgs)
        assert all(("gpz_predictor_run_missing_dev" if diag else "predict_missing_cov_fits") in t for t in msgs), msgs
        assert untouched(out, FG)
        assert p.info[1] == held and "missing" not in p.route            # the handle gained no byte


def test_bad_groups_labels_and_weights_are_refused_with_the_outputs_untouched():
    n, d, k, nd, G, B = 3000, 5, 2, 3, 2, 10
    model = model_with_priors("VC", 20, d, k, True, seed=88)
    Xh = catalogue(model, n, seed=89)
    Xh[:, 3] = NAN
    X = dev(Xh)
    mask = 0b10111
    e = np.linspace(-3, 3, B + 1)
    with gpz_amd.Predictor(model, tile_rows=1 << 10) as p:
        good_s = p.stack_missing_cov_dev(X, e, n_draws=nd, seed=5, n_groups=G)
        good_g = p.draws_missing_cov_dev(X, nd, seed=5, return_gamma=True)
        rcs, _, out, FG = raw_calls(p, X, mask, nd, G, B)
        assert rcs == (0, 0) and all(np.all(a != -7.0) for a in out[1:]) and all(bool((t != -7.0).all()) for t in FG)
        assert torch.equal(FG[1].permute(0, 2, 1), good_g[1]) and torch.equal(FG[0].permute(0, 2, 1), good_g[0])
        held = p.info[1]
        two = X.clone()
        two[2000:, 0] = NAN                                                # two patterns in one group
        nan_obs = X.clone()
        nan_obs[2999, 4] = NAN                                             # a NaN in an observed dimension
        num_miss = X.clone()
        num_miss[1234, 3] = 0.5                                            # a number in a missing one
        bad_lab = torch.zeros(n, dtype=torch.int32, device=DEV)
        bad_lab[2998] = G
        bad_wt = torch.ones(n, dtype=torch.float64, device=DEV)
        bad_wt[7] = -1.0
        nan_wt = torch.ones(n, dtype=torch.float64, device=DEV)
        nan_wt[2999] = NAN
        for what, x, obs, lab, wt, text in (("two patterns", two, mask, None, None, "share one NaN pattern"),
                                            ("NaN in o", nan_obs, mask, None, None, "share one NaN pattern"),
                                            ("number in u", num_miss, mask, None, None, "share one NaN pattern"),
                                            ("full mask", X, 0b11111, None, None, "no dimension is missing"),
                                            ("mask past d", X, 0b110111, None, None, "above d"),
                                            ("bad label", X, mask, bad_lab, None, "label"),
                                            ("negative weight", X, mask, None, bad_wt, "weight"),
                                            ("NaN weight", X, mask, None, nan_wt, "weight")):
            rcs, msgs, out, FG = raw_calls(p, x, obs, nd, G, B, lab, wt)
            assert rcs[0] == ERR_ARG and text in msgs[0], (what, rcs, msgs)
            assert all(np.all(a == -7.0) for a in out), what               # refused before any tile kernel has run
            if lab is None and wt is None:
                assert rcs[1] == ERR_ARG and text in msgs[1] and untouched(out, FG), (what, rcs, msgs)
            else:
                assert rcs[1] == 0, (what, rcs, msgs)                      # (the draws take no labels or weights)
            assert p.info[1] == held, what
            same_stack(p.stack_missing_cov_dev(X, e, n_draws=nd, seed=5, n_groups=G), good_s, what)   # the handle works on the next call
            assert all(torch.equal(u, v) for u, v in zip(p.draws_missing_cov_dev(X, nd, seed=5, return_gamma=True), good_g)), what
        with pytest.raises(_lib.GpzError, match="label"):
            p.stack_missing_cov_dev(X, e, groups=torch.full((n,), 7, device=DEV), n_groups=2)
        with pytest.raises(_lib.GpzError, match="weight"):
            p.stack_missing_cov_dev(X, e, weights=bad_wt)


# ---- 9. memory and route ----------------------------------------------------------------------------------------------------------------
def test_memory_and_route():
    d, nd, m, k, G, B, T = 5, 4, 30, 1, 4, 50, 1024
    model = model_with_priors("VC", m, d, k, True, seed=195)
    n = 20_000
    gen = torch.Generator(device=DEV).manual_seed(98)
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=gen) * torch.from_numpy(model.sdX).to(DEV) + \
        torch.from_numpy(model.muX).to(DEV)
    two = X.clone()
    two[torch.rand(n, device=DEV, generator=gen) < 0.2, 1] = NAN
    eight = X.clone()
    for c in (0, 2, 4):
        eight[torch.rand(n, device=DEV, generator=gen) < 0.3, c] = NAN
    pairs_tail = f"; missing: k_predict_missing_cov_pairs ({chunks_rule(m)} pair chunks)"
    with gpz_amd.Predictor(model, tile_rows=T) as p, gpz_amd.Predictor(model, tile_rows=T) as q:
        # a handle that never calls the new entries holds the bytes it held: q stays on the entries of the parent
        for h in (p, q):
            h.predict_dev(X[:300]); h.draws_dev(X[:300], nd); h.predict_missing_cov_dev(two[:2000]); h.draws_missing_cov_dev(two[:2000], nd)
        held = p.info[1]
        assert held == q.info[1]
        assert p.route.endswith(pairs_tail), p.route                     # the clause it ends in today
        edges = np.linspace(*np.percentile(host(p.predict_missing_cov_dev(two[:2000])[0]), [3, 97]), B + 1)
        # the first gamma call adds its bytes once: the chunk slab alone
        p.draws_missing_cov_dev(two[:2000], nd, return_gamma=True)
        first = p.info[1]
        assert first == held + chunks_rule(m) * nd * k * T * 8, (first - held)
        assert p.route.endswith(pairs_tail + route_tail(m)), p.route
        p.draws_missing_cov_dev(two, nd, return_gamma=True)
        assert p.info[1] == first                                        # 2000 rows or 20 000: the same bytes
        # the first stack call adds its bytes once
        p.stack_missing_cov_dev(two[:2000], edges, n_draws=nd, seed=3, n_groups=G)
        stacked = p.info[1]
        assert stacked > first
        assert p.route.endswith(pairs_tail + route_tail(m, stack=True)), p.route
        p.stack_missing_cov_dev(two, edges, n_draws=nd, seed=3, n_groups=G)
        p.draws_missing_cov_dev(two, nd, return_gamma=True)
        assert p.info[1] == stacked                                      # ten times the rows
        assert len(p._nan_groups_dev(eight)) == 8
        p.stack_missing_cov_dev(eight, edges, n_draws=nd, seed=3, n_groups=G)
        p.draws_missing_cov_dev(eight, nd, return_gamma=True)
        assert p.info[1] == stacked                                      # eight patterns
        q.predict_missing_cov_dev(eight); q.draws_missing_cov_dev(eight, nd)
        assert q.info[1] == held and q.route.endswith(pairs_tail)
    # no draws: no factors, no W, no draws buffer and no chunk slab
    with gpz_amd.Predictor(model, tile_rows=T) as r, gpz_amd.Predictor(model, tile_rows=T) as s:
        r.predict_missing_cov_dev(two[:2000])
        s.predict_missing_cov_dev(two[:2000])
        base = r.info[1]
        assert base == s.info[1]
        res = r.stack_missing_cov_dev(two[:2000], edges, n_groups=G)
        assert res.hist.shape == (1, G, k, B) and res.hist.sum() > 0.0
        assert "factors" not in r.route and "draws:" not in r.route, r.route
        assert r.route.endswith(route_tail(m, stack=True)), r.route
        s.stack_missing_cov_dev(two[:2000], edges, n_draws=nd, n_groups=G)
        assert base < r.info[1] < s.info[1]
        # what the call without draws added: the widths of one column and the stack's own buffers (edges, accumulators, row slabs)
        rec = G * B + 3 * G
        want = k * T * 8 + (k * (B + 1) + k) * 8 + k * rec * 8 * (1 + stack_slabs(k, rec, T))
        assert r.info[1] - base == want, (r.info[1] - base, want)
