"""The stacked n(z) and gamma under every weight draw for rows with input noise and missing inputs on a covariance kind
(Predictor.stack_noisy_missing_cov_dev / draws_noisy_missing_cov_dev(..., return_gamma=True); k_predict_noisy_missing_cov_gamma.hip)
against the existing entries of the handle, ``gpz_amd.predict`` and the oracle: gamma_s against predict_noisy_missing_cov_dev's gamma of
the model whose weights are the draw's at every pair-count, chunk, slab and column edge and every number of observed dimensions, the
same bits over tiles, orders, company, splits and layouts, the stack against a torch reduction of the device's own per-row numbers, Psi in
the missing dimensions, the state of the slab, the refusals of the C entries and constant memory.

Gates.  gamma_s is measured against parent code, never against itself.  In tests 1 to 3 each case computes the spread of the parent's two
routes on the w_s model, predict_noisy_missing_cov_dev against gpz_amd.predict(X, ms, Psi=Psi); the gate of the case is 10 x that spread
(a third summation order and, in test 2, host-formed weights), never tighter than 1e-12 (the gamma gate between those two routes in
tests/test_predictor_noisy_missing_cov.py) and never looser than the project's 1e-9; rel <= 1e-8 against the oracle.  The largest values
seen on an MI355X: GATE_SEEN.  The stack: the derived tolerances of tests/test_predictor_stack_missing.py, unchanged, with s_min taken
over the new widths."""
import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import nrel, synth_model
from test_predictor_draws_cpu import philox_normals
from test_predictor_missing import model_with_priors
from test_predictor_missing_cov_cpu import chunks_rule
from test_predictor_noisy_missing_cov_cpu import slabs_rule
from test_predictor_stack import EPS, assert_close, setting
from test_predictor_stack_missing_cov import (catalogue, exact_model, exact_weights, knock_out, noise, same_stack, torch_reference,
                                              untouched, with_weights)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COV = ("GC", "VC")
NAN = float("nan")
# the largest nrel of gamma_s against predict_noisy_missing_cov_dev of the w_s model seen on an MI355X, and the largest spread of the
# parent's two routes beside it: over the cases of test 1, of test 2 and of test 3; the largest rel against the oracle (m <= 7, 60 rows)
GATE_SEEN = {"exact weights": (9.09e-15, 2.13e-14), "seeded draws": (6.97e-15, 1.99e-14), "column edges": (4.84e-14, 3.0e-14),
             "oracle": 1.3e-14}


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def gate_of(spread):
    """10 x the spread of the parent's two routes, never tighter than 1e-12, never looser than 1e-9."""
    return min(max(10.0 * spread, 1e-12), 1e-9)


def parent_gamma(ms, X, Psi, rows, tile_rows=256):
    """gamma of the model ms by the parent's two routes: predict_noisy_missing_cov_dev on a handle of its own over all rows, and
    gpz_amd.predict(X, ms, Psi=Psi) over ``rows`` (which leaves out rows with nothing observed: the one-shot route refuses them)."""
    with gpz_amd.Predictor(ms, tile_rows=tile_rows) as q:
        a = host(q.predict_noisy_missing_cov_dev(dev(X), dev(Psi))[4])
    b = np.array(gpz_amd.predict(X[rows], ms, Psi=Psi[rows])[4])
    return a, nrel(a[rows], b)


def route_tail(m, stack=False):
    return (f"; noisy missing per draw: k_predict_noisy_missing_cov_gamma ({chunks_rule(m)} pair chunks)" +
            (" + k_stack_tile_w" if stack else ""))


def pairs_tail(m):
    return f"; noisy missing: k_predict_noisy_missing_cov_pairs ({chunks_rule(m)} pair chunks)"


def gam(p, x, psi, nd, **kw):
    return p.draws_noisy_missing_cov_dev(x, psi, nd, return_gamma=True, **kw)[1]


# ---- 1. gamma_s with exact weights --------------------------------------------------------------------------------------------------------
# (m, d, k, n_draws, missing dimension): the pair-count and chunk edges in m at d = 3 with dimension 1 missing (NO = 2); m = 108 | 109 one
# slab | two; m = 250; d = 5 with dimension 1 missing ([o u] = [0 2 3 4 1] is not its own inverse); d = 10, NO = 9 at m = 240, the
# largest LDS; then d = 2 .. 10 with the last dimension missing, NO = 1 .. 9, at m = 20.  64 draws only where m <= 33; k = 8 with 17
# draws is 136 columns, a second pass of one block.
M_CASES = [(1, 3, 1, 17, 1), (2, 3, 3, 5, 1), (7, 3, 8, 5, 1), (10, 3, 1, 64, 1), (11, 3, 1, 5, 1), (15, 3, 3, 1, 1), (16, 3, 1, 17, 1),
           (22, 3, 8, 17, 1), (23, 3, 1, 5, 1), (31, 3, 1, 64, 1), (32, 3, 3, 5, 1), (33, 3, 1, 17, 1), (108, 3, 1, 1, 1),
           (109, 3, 1, 3, 1), (250, 3, 1, 3, 1), (7, 5, 1, 64, 1), (240, 10, 1, 1, 9)]
NO_CASES = [(20, d, (1, 3, 8)[d % 3], (5, 1, 17)[d % 3], d - 1) for d in range(2, 11)]
CASES = M_CASES + NO_CASES


@pytest.mark.parametrize("m,d,k,nd,gone", CASES)
def test_gamma_per_draw_with_exact_weights(m, d, k, nd, gone):
    """The reference is predict_noisy_missing_cov_dev's gamma of the model with w := w_s on a handle of its own (the same quantity by
    definition, parent code), per draw.  300 rows of one pattern on 256-row tiles: a full tile and a partial one, and a last workgroup
    of 44 rows; behind them ten rows with nothing observed, which go to k_predict_missing_cov_gamma.  Row 3 has psi = 0 in its first
    observed dimension and row 4 in all of them.  m = 1, 2, 7 are 1, 3 and 28 pairs: a partial K step; 10 | 11, 15 | 16, 22 | 23,
    31 | 32 are the chunk counts 1 | 2, 2 | 4, 4 | 8, 8 | 16; m = 33 has components past eight 4-record stages; m = 108 | 109 is
    one slab | two.  Where m <= 7, the first 60 rows against the oracle's gamma of the w_s model at rel <= 1e-8, on the first, the
    middle and the last draw."""
    assert slabs_rule(108, 3, 2) == 1 and slabs_rule(109, 3, 2) == 2 and slabs_rule(250, 3, 2) == 16
    ns = 310
    model = exact_model(COV[(m + d) % 2], m, d, k, bool((m + k) % 2), seed=13000 + 100 * d + 10 * k + m)
    X = catalogue(model, ns, seed=m + d)
    X[:300, gone] = NAN
    X[300:, :] = NAN
    Psi = noise(ns, d, seed=m + d + 1)
    first = 1 if gone == 0 else 0
    Psi[3, first] = 0.0
    Psi[4, :] = 0.0
    rows = np.arange(ns) < 300
    Z = np.random.default_rng(nd + m).standard_normal((m, nd, k))
    W = exact_weights(model, Z)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F, Gam = p.draws_noisy_missing_cov_dev(dev(X), dev(Psi), nd, Z=Z, return_gamma=True)
        assert p.route.endswith(route_tail(m)), p.route
        assert "k_stack_tile" not in p.route                             # no stack call on this handle
        assert torch.equal(F, p.draws_noisy_missing_cov_dev(dev(X), dev(Psi), nd, Z=Z))
    assert Gam.shape == (nd, ns, k) and Gam.dtype == torch.float64
    Gam = host(Gam)
    worst, spread, worst_orc = 0.0, 0.0, 0.0
    for s in range(nd):
        ms = with_weights(model, W[:, s, :])
        ref, sp = parent_gamma(ms, X, Psi, rows)
        worst, spread = max(worst, nrel(Gam[s], ref)), max(spread, sp)
        if m <= 7 and s in {0, nd // 2, nd - 1}:
            worst_orc = max(worst_orc, rel(Gam[s, :60], O.predict_any(X[:60], ms, Psi=Psi[:60])[4]))
    print(f"m={m} d={d} k={k} nd={nd}: worst nrel of gamma_s against predict_noisy_missing_cov_dev of the w_s model {worst:.3g}; "
          f"spread of the parent's two routes {spread:.3g}; worst rel against the oracle {worst_orc:.3g}")
    assert worst <= gate_of(spread), (worst, spread)
    assert worst_orc <= 1e-8, worst_orc


# ---- 2. gamma_s with a general iSigma_w ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
def test_gamma_per_draw_with_seeded_draws(method):
    """Seeded draws of a general iSigma_w; w_s formed on the host as w + chol(sym(iSigma_w)) z_s with the Philox normals of the seed.
    Four patterns and complete rows (whose gamma_s is draws_noisy_cov_dev's)."""
    m, d, k, nd, ns, seed = 60, 5, 2, 4, 600, 31
    model = model_with_priors(method, m, d, k, True, seed=77)
    X = knock_out(catalogue(model, ns, seed=78), seed=79)
    Psi = noise(ns, d, seed=80)
    rows = np.ones(ns, dtype=bool)
    z = philox_normals(seed, m, nd, k)
    iS = model.sets["best"]["iSigma_w"]
    L = [np.linalg.cholesky(0.5 * (iS[:, :, o] + iS[:, :, o].T)) for o in range(k)]
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        Gam = host(gam(p, dev(X), dev(Psi), nd, seed=seed))
    figures = []
    for s in range(nd):
        ws = np.stack([model.sets["best"]["w"][:, o] + L[o] @ z[:, s, o] for o in range(k)], axis=1)
        ref, spread = parent_gamma(with_weights(model, ws), X, Psi, rows)
        figures.append((nrel(Gam[s], ref), spread))
        print(f"{method} draw {s}: nrel(gamma_s, predict_noisy_missing_cov_dev of w_s) {figures[-1][0]:.3g}; spread of the parent's two "
              f"routes {spread:.3g}")
    for s, (got, spread) in enumerate(figures):
        assert got <= gate_of(spread), (s, got, spread)


# ---- 3. column edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncol,k,d", [(1, 1, 3), (15, 3, 3), (16, 1, 3), (17, 1, 3), (127, 1, 3), (128, 8, 3), (129, 1, 3), (256, 8, 3),
                                      (257, 1, 3), (64, 8, 8), (65, 1, 8)])
def test_column_edges(ncol, k, d):
    """m = 17, VC, the last dimension missing: n_draws k at a partial block, a full block, the pass edge on gridDim.z (8 blocks, 128
    columns; with seven observed dimensions, d = 8, 4 blocks, 64 columns) and one column past two full passes; rows at the edges of a
    wave's 16 rows and a workgroup's 64.  Each case against test 1's reference on the first, the middle and the last draw."""
    m, nmax, nd = 17, 300, ncol // k
    model = exact_model("VC", m, d, k, True, seed=1300 + ncol)
    X = catalogue(model, nmax, seed=ncol)
    X[:, d - 1] = NAN
    Psi = noise(nmax, d, seed=ncol + 1)
    rows = np.ones(nmax, dtype=bool)
    Z = np.random.default_rng(ncol).standard_normal((m, nd, k))
    W = exact_weights(model, Z)
    draws = sorted({0, nd // 2, nd - 1})
    ref, spread = {}, 0.0
    for s in draws:
        ref[s], sp = parent_gamma(with_weights(model, W[:, s, :]), X, Psi, rows)
        spread = max(spread, sp)
    Xd, Pd = dev(X), dev(Psi)
    worst = 0.0
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        for n in (1, 15, 16, 17, 63, 64, 65, 300):
            Gam = gam(p, Xd[:n], Pd[:n], nd, Z=Z)
            assert Gam.shape == (nd, n, k) and bool(torch.isfinite(Gam).all())
            for s in draws:
                worst = max(worst, nrel(host(Gam[s]), ref[s][:n]))
    print(f"ncol={ncol} k={k} d={d}: worst nrel {worst:.3g}; spread of the parent's two routes {spread:.3g}")
    assert worst <= gate_of(spread), (worst, spread)


# ---- 4. the same bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,m,k", [("VC", 40, 2), ("GC", 23, 1)])
def test_same_bits_over_tiles_orders_company_splits_layouts_and_draws(method, m, k):
    n, d, nd = 1400, 5, 5
    model = model_with_priors(method, m, d, k, True, seed=181 + m)
    X32 = knock_out(catalogue(model, n, seed=82), seed=83).astype(np.float32)
    P32 = noise(n, d, seed=84).astype(np.float32)
    X, Psi = X32.astype(np.float64), P32.astype(np.float64)
    Xd, Pd = dev(X), dev(Psi)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    Z17 = np.random.default_rng(2).standard_normal((m, 17, k))
    codes = np.isnan(X) @ (1 << np.arange(d))
    full = torch.from_numpy(codes == 0).to(DEV)

    def both(q, x, psi, ndr=nd, **kw):
        return q.draws_noisy_missing_cov_dev(x, psi, ndr, Z=Z17[:, :ndr], return_gamma=True, **kw)

    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F5, G5 = both(p, Xd, Pd)
        assert torch.equal(p.draws_noisy_missing_cov_dev(Xd, Pd, nd, Z=Z17[:, :nd]), F5), "F against the call without return_gamma"
        assert bool((G5 != 0.0).all())
        Ff, Gf = p.draws_noisy_cov_dev(Xd[full], Pd[full], nd, Z=Z17[:, :nd], return_gamma=True)
        assert torch.equal(F5[:, full], Ff) and torch.equal(G5[:, full], Gf), "complete rows: draws_noisy_cov_dev's"
        F17, G17 = both(p, Xd, Pd, 17)
        assert torch.equal(G17[:nd], G5) and torch.equal(F17[:nd], F5), "the first 5 of 17 draws"
        Fp, Gp = both(p, Xd[perm], Pd[perm])
        assert torch.equal(Gp, G5[:, perm]) and torch.equal(Fp, F5[:, perm]), "a row permutation"
        halves = [both(p, Xd[:333], Pd[:333]), both(p, Xd[333:], Pd[333:])]
        assert torch.equal(torch.cat([h[1] for h in halves], dim=1), G5), "a split into two calls"
        for code in np.unique(codes):                                      # a row alone, a row among its group only
            rows = np.flatnonzero(codes == code)
            r = int(rows[len(rows) // 2])
            assert torch.equal(both(p, Xd[r:r + 1], Pd[r:r + 1])[1], G5[:, r:r + 1]), ("alone", code)
            idx = torch.from_numpy(rows).to(DEV)
            assert torch.equal(both(p, Xd[idx], Pd[idx])[1], G5[:, rows]), ("its group", code)
        X2, P2 = dev(np.repeat(X, 2, axis=0)), dev(np.repeat(Psi, 2, axis=0))
        wide = torch.full((n, 2 * d), 3.0, dtype=torch.float64, device=DEV)
        wide[:, ::2] = Xd
        widep = torch.full((n, 2 * d), 3.0, dtype=torch.float64, device=DEV)
        widep[:, ::2] = Pd
        for x, psi, what in ((dev(X32, torch.float32), dev(P32, torch.float32), "float32"),
                             (Xd.T.contiguous().T, Pd.T.contiguous().T, "transposed"), (X2[::2], P2[::2], "row-sliced"),
                             (dev(X32, torch.float32).T.contiguous().T, Pd, "float32 transposed X, float64 Psi"),
                             (Xd, dev(P32, torch.float32).T.contiguous().T, "float32 transposed Psi"),
                             (wide[:, ::2], widep[:, ::2], "column-strided")):
            Fx, Gx = both(p, x, psi)
            assert torch.equal(Gx, G5) and torch.equal(Fx, F5), what
        sel = torch.zeros(n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        assert torch.equal(both(p, Xd, Pd, selection=sel)[1], G5[:, ::2]), "selection"
    for T in (64, 1024, None):
        with gpz_amd.Predictor(model, tile_rows=T) as q:
            Fq, Gq = both(q, Xd, Pd)
            assert torch.equal(Gq, G5) and torch.equal(Fq, F5), T


# ---- 5. stack parity --------------------------------------------------------------------------------------------------------------------
def stack_inputs(p, model, Xd, Pd, edges, n_draws, draw_kw, groups, weights, G):
    """torch_reference fed with the device's own per-row numbers (predict_noisy_missing_cov_dev and
    draws_noisy_missing_cov_dev(return_gamma=True)), and the tolerances of test_predictor_stack_missing.py's stack_inputs with s_min
    over the new widths."""
    mu_t, sigma_t, _, beta_t = p.predict_noisy_missing_cov_dev(Xd, Pd)[:4]
    Ft = S2t = None
    if n_draws:
        Ft, Gt = p.draws_noisy_missing_cov_dev(Xd, Pd, n_draws, return_gamma=True, **draw_kw)
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


@pytest.mark.parametrize("method", COV)
@pytest.mark.parametrize("hetero,k", [(False, 1), (True, 3)])
def test_stack_parity(method, hetero, k):
    """1500 rows on 1024-row tiles, Psi on every row, dimension 1 missing on 20 % and dimension 4 on 10 % of the rows independently (four
    patterns) and one row with nothing observed, three groups with rows left out and random weights, 1, 37 and 300 bins, no draws and 5
    seeded draws; a selection; column 0 against the call without draws bit for bit."""
    d, ns, G, m = 5, 1500, 3, 24
    model = model_with_priors(method, m, d, k, hetero, seed=4400 + 100 * COV.index(method) + 10 * k + hetero)
    X = knock_out(catalogue(model, ns, seed=k + 40), seed=k + 41)
    X[9, :] = NAN
    Xd, Pd = dev(X), dev(noise(ns, d, seed=k + 42))
    groups, weights = setting(ns, G, seed=m)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        mu0 = host(p.predict_noisy_missing_cov_dev(Xd, Pd)[0])
        for B in (1, 37, 300):
            edges = np.linspace(*np.percentile(mu0, [3, 97]), B + 1)
            res = {}
            for nd in (0, 5):
                ref, th, tm, tw, mu = stack_inputs(p, model, Xd, Pd, edges, nd, dict(seed=77), groups, weights, G)
                rd = res[nd] = p.stack_noisy_missing_cov_dev(Xd, Pd, edges, n_draws=nd, seed=77, groups=gd, n_groups=G, weights=wd)
                what = f"{method} hetero={hetero} k={k} B={B} draws={nd}"
                assert rd.hist.shape == (1 + nd, G, k, B)
                assert_close(rd, ref, th, tm, tw, what)
                if nd:
                    assert rd.hist[1:].sum() > 0.0
            same_stack([res[5].hist[:1], res[5].sum_w, res[5].sum_mu[:1], res[5].sum_mu2[:1]], res[0][:4], "column 0 of the call with draws")
        sel = torch.zeros(ns, dtype=torch.bool, device=DEV)
        sel[::2] = True
        same_stack(p.stack_noisy_missing_cov_dev(Xd, Pd, edges, n_draws=5, seed=77, groups=gd, n_groups=G, weights=wd, selection=sel),
                   p.stack_noisy_missing_cov_dev(Xd[::2].contiguous(), Pd[::2].contiguous(), edges, n_draws=5, seed=77, groups=gd[::2],
                                                 n_groups=G, weights=wd[::2]), "selection")
        assert p.route.endswith(route_tail(m, stack=True)), p.route
        assert p.stack_noisy_missing_cov_dev(Xd[:64], Pd[:64], edges, n_groups=G).hist.shape == (65, G, k, 300)   # 64 draws by default


def test_a_catalogue_is_the_sum_of_its_patterns_and_the_other_kinds_keep_their_bits():
    n, d, m, k, nd, G = 1400, 5, 24, 2, 5, 3
    model = model_with_priors("VC", m, d, k, True, seed=281)
    X = knock_out(catalogue(model, n, seed=82), seed=83)
    X[1390:, :] = NAN                                                     # ten rows with nothing observed
    Xd, Pd = dev(X), dev(noise(n, d, seed=84))
    groups, weights = setting(n, G, seed=5)
    gd, wd = dev(groups, torch.int64), dev(weights)
    codes = np.isnan(X) @ (1 << np.arange(d))
    kw = dict(n_draws=nd, seed=9, n_groups=G)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        edges = np.linspace(*np.percentile(host(p.predict_noisy_missing_cov_dev(Xd, Pd)[0]), [3, 97]), 51)
        whole = p.stack_noisy_missing_cov_dev(Xd, Pd, edges, groups=gd, weights=wd, **kw)
        same_stack(p.stack_noisy_missing_cov_dev(Xd, Pd, edges, groups=gd, weights=wd, **kw), whole, "the same call twice")
        total = None
        for code in np.unique(codes):                                      # ascending pattern code
            idx = torch.from_numpy(np.flatnonzero(codes == code)).to(DEV)
            one = (p.stack_noisy_cov_dev if code == 0 else p.stack_noisy_missing_cov_dev)(Xd[idx], Pd[idx], edges, groups=gd[idx],
                                                                                        weights=wd[idx], **kw)
            total = list(one[:4]) if total is None else [t + a for t, a in zip(total, one[:4])]
        same_stack(total, whole[:4], "the += of the single-pattern calls")
        parts = [p.stack_noisy_missing_cov_dev(Xd[a:b], Pd[a:b], edges, groups=gd[a:b], weights=wd[a:b], **kw)
                 for a, b in ((0, 500), (500, 1400))]
        # additive over chunks of the catalogue: the fields are sums over at most 1400 rows taken in another order, n eps = 3.1e-13
        for f, (u, v, w) in enumerate(zip(parts[0][:4], parts[1][:4], whole[:4])):
            assert np.allclose(u + v, w, rtol=1e-12, atol=1e-12 * np.abs(w).max()), f
        full = torch.from_numpy(codes == 0).to(DEV)
        same_stack(p.stack_noisy_missing_cov_dev(Xd[full], Pd[full], edges, groups=gd[full], weights=wd[full], **kw),
                   p.stack_noisy_cov_dev(Xd[full], Pd[full], edges, groups=gd[full], weights=wd[full], **kw), "a catalogue without NaN")
        none = torch.from_numpy(codes == (1 << d) - 1).to(DEV)
        same_stack(p.stack_noisy_missing_cov_dev(Xd[none], Pd[none], edges, groups=gd[none], weights=wd[none], **kw),
                   p.stack_missing_cov_dev(Xd[none], edges, groups=gd[none], weights=wd[none], **kw), "rows with nothing observed")
        Fn, Gn = p.draws_noisy_missing_cov_dev(Xd[none], Pd[none], nd, seed=9, return_gamma=True)
        Fm, Gm = p.draws_missing_cov_dev(Xd[none], nd, seed=9, return_gamma=True)
        assert torch.equal(Fn, Fm) and torch.equal(Gn, Gm), "rows with nothing observed: draws_missing_cov_dev's gamma"


# ---- 6. Psi in a missing dimension ----------------------------------------------------------------------------------------------------------
def test_psi_in_a_missing_dimension_is_not_read():
    n, d, m, k, nd = 700, 5, 24, 2, 3
    model = model_with_priors("GC", m, d, k, True, seed=611)
    X = knock_out(catalogue(model, n, seed=62), seed=63)
    Psi = noise(n, d, seed=64)
    e = np.linspace(-2.0, 2.0, 41) + float(np.mean(model.muY))
    miss = np.isnan(X)
    assert miss.any()
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        G0 = gam(p, dev(X), dev(Psi), nd, seed=3)
        S0 = p.stack_noisy_missing_cov_dev(dev(X), dev(Psi), e, n_draws=nd, seed=3)
        for junk in (NAN, -1.0, float("inf")):
            P2 = Psi.copy()
            P2[miss] = junk
            assert torch.equal(gam(p, dev(X), dev(P2), nd, seed=3), G0), junk
            same_stack(p.stack_noisy_missing_cov_dev(dev(X), dev(P2), e, n_draws=nd, seed=3), S0, junk)


# ---- 7. the state of the slab ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [30, 109])
def test_the_slab_is_filled_by_whichever_kernel_comes_first(m):
    """m = 30 keeps its table in one slab on the handle, m = 109 at d = 3 with one dimension missing passes two slabs per tile.  A fresh
    handle whose first call is return_gamma=True (the gamma kernel fills the slab) followed by predict_noisy_missing_cov_dev (which
    reads it), and pattern A, then B, then A again: every call gives the bits of the same call on a fresh handle."""
    assert slabs_rule(30, 3, 2) == 1 and slabs_rule(109, 3, 2) == 2
    d, k, n, nd = 3, 1, 300, 3
    model = model_with_priors("VC", m, d, k, True, seed=600 + m)
    XA, XB = catalogue(model, n, seed=61), catalogue(model, n, seed=62)
    XA[:, 1] = NAN
    XB[:, 0] = NAN
    XA, XB, Pd = dev(XA), dev(XB), dev(noise(n, d, seed=63))

    def moments(q, x):
        return q.predict_noisy_missing_cov_dev(x, Pd)

    def gamma(q, x):
        return q.draws_noisy_missing_cov_dev(x, Pd, nd, seed=4, return_gamma=True)

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


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
ERR_ARG, ERR_UNSUPPORTED = -1, -5                                        # include/gpz_hip.h


def raw_calls(p, x, psi, obs, nd, G, B, lab=None, wt=None):
    """Both C entries on one group with every output preset to -7: (rc of the stack, rc of the draws), their messages, the outputs."""
    k, n = p._k, x.shape[0]
    muX, sdX, muY = p._norm_vectors()
    sd2 = np.ascontiguousarray(sdX ** 2)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    es = np.ascontiguousarray(np.linspace(-3, 3, B + 1)[None, :] - muY[:, None])
    out = [np.full(s, -7.0) for s in ((1 + nd, G, k, B), (G,), (1 + nd, G, k), (1 + nd, G, k))]
    lead = [p._handle(), *p._x_args(x), *p._psi_args(psi, n), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(sd2)]
    rc1 = p._lib.gpz_predictor_stack_noisy_missing_cov_dev(*lead, _lib.dptr(p._priors), obs, nd, 5, None, _lib.dptr(es), B,
                                                           None if lab is None else lab.data_ptr(), G,
                                                           None if wt is None else wt.data_ptr(), *(_lib.dptr(a) for a in out),
                                                           _lib.dptr(muY), stream)
    msg1 = p._lib.gpz_last_error().decode() if rc1 else ""
    Fd = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    Gm = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    rc2 = p._lib.gpz_predictor_draws_gamma_noisy_missing_cov_dev(*lead, _lib.dptr(muY), _lib.dptr(p._priors), obs, nd, 5, None,
                                                                 Fd.data_ptr(), Gm.data_ptr(), stream)
    msg2 = p._lib.gpz_last_error().decode() if rc2 else ""
    torch.cuda.synchronize()
    return (rc1, rc2), (msg1, msg2), out, [Fd, Gm]


@pytest.mark.parametrize("kw", [{"method": "VD"}, {"m": 257}, {"d": 11}, {"k": 9}])
def test_models_outside_the_scope_are_refused_by_the_c_entries(kw):
    a = {"method": "VC", "m": 20, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    X = catalogue(model, 40, seed=6)
    X[:, 1] = NAN
    Psi = dev(noise(40, a["d"], seed=7))
    diag = a["method"] == "VD"
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match="stack_noisy_missing_dev" if diag else "predict_missing_cov_fits"):
            p.stack_noisy_missing_cov_dev(dev(X), Psi, np.linspace(-3, 3, 11), n_draws=2)
        with pytest.raises(ValueError, match="draws_noisy_missing_dev" if diag else "predict_missing_cov_fits"):
            p.draws_noisy_missing_cov_dev(dev(X), Psi, 4, return_gamma=True)
        held = p.info[1]
        rcs, msgs, out, FG = raw_calls(p, dev(X), Psi, (1 << a["d"]) - 3, 3, 2, 10)
        assert rcs == (ERR_UNSUPPORTED, ERR_UNSUPPORTED), (rcs, msgs)
        assert all(("gpz_predictor_run_noisy_missing_dev" if diag else "predict_missing_cov_fits") in t for t in msgs), msgs
        assert untouched(out, FG)
        assert p.info[1] == held and "missing" not in p.route            # the handle gained no byte


def test_bad_groups_labels_weights_and_psi_are_refused_with_the_outputs_untouched():
    n, d, k, nd, G, B = 3000, 5, 2, 3, 2, 10
    model = model_with_priors("VC", 20, d, k, True, seed=88)
    Xh = catalogue(model, n, seed=89)
    Xh[:, 3] = NAN
    X, Psi = dev(Xh), dev(noise(n, d, seed=90))
    mask = 0b10111
    e = np.linspace(-3, 3, B + 1)
    with gpz_amd.Predictor(model, tile_rows=1 << 10) as p:
        good_s = p.stack_noisy_missing_cov_dev(X, Psi, e, n_draws=nd, seed=5, n_groups=G)
        good_g = p.draws_noisy_missing_cov_dev(X, Psi, nd, seed=5, return_gamma=True)
        rcs, _, out, FG = raw_calls(p, X, Psi, mask, nd, G, B)
        assert rcs == (0, 0) and all(np.all(a != -7.0) for a in out[1:]) and all(bool((t != -7.0).all()) for t in FG)
        assert torch.equal(FG[1].permute(0, 2, 1), good_g[1]) and torch.equal(FG[0].permute(0, 2, 1), good_g[0])
        held = p.info[1]
        two = X.clone()
        two[2000:, 0] = NAN                                                # two patterns in one group
        num_miss = X.clone()
        num_miss[1234, 3] = 0.5                                            # a number in a missing dimension
        neg_psi = Psi.clone()
        neg_psi[2999, 4] = -1.0                                            # a bad variance in an observed dimension
        nan_psi = Psi.clone()
        nan_psi[0, 0] = NAN
        bad_lab = torch.zeros(n, dtype=torch.int32, device=DEV)
        bad_lab[2998] = G
        bad_wt = torch.ones(n, dtype=torch.float64, device=DEV)
        bad_wt[7] = -1.0
        for what, x, psi, obs, lab, wt, text in (("two patterns", two, Psi, mask, None, None, "share one NaN pattern"),
                                                 ("number in u", num_miss, Psi, mask, None, None, "share one NaN pattern"),
                                                 ("full mask", X, Psi, 0b11111, None, None, "no dimension is missing"),
                                                 ("mask past d", X, Psi, 0b110111, None, None, "above d"),
                                                 ("negative Psi", X, neg_psi, mask, None, None, "Psi has an element"),
                                                 ("NaN Psi", X, nan_psi, mask, None, None, "Psi has an element"),
                                                 ("bad label", X, Psi, mask, bad_lab, None, "label"),
                                                 ("negative weight", X, Psi, mask, None, bad_wt, "weight")):
            rcs, msgs, out, FG = raw_calls(p, x, psi, obs, nd, G, B, lab, wt)
            assert rcs[0] == ERR_ARG and text in msgs[0], (what, rcs, msgs)
            assert all(np.all(a == -7.0) for a in out), what               # refused before any tile kernel has run
            if lab is None and wt is None:
                assert rcs[1] == ERR_ARG and text in msgs[1] and untouched(out, FG), (what, rcs, msgs)
            else:
                assert rcs[1] == 0, (what, rcs, msgs)                      # (the draws take no labels or weights)
            assert p.info[1] == held, what
            same_stack(p.stack_noisy_missing_cov_dev(X, Psi, e, n_draws=nd, seed=5, n_groups=G), good_s, what)   # the next call works
            assert all(torch.equal(u, v) for u, v in zip(p.draws_noisy_missing_cov_dev(X, Psi, nd, seed=5, return_gamma=True), good_g)), what
        with pytest.raises(_lib.GpzError, match="label"):
            p.stack_noisy_missing_cov_dev(X, Psi, e, groups=torch.full((n,), 7, device=DEV), n_groups=2)
        with pytest.raises(_lib.GpzError, match="weight"):
            p.stack_noisy_missing_cov_dev(X, Psi, e, weights=bad_wt)


# ---- 9. memory and route ----------------------------------------------------------------------------------------------------------------
def test_memory_and_route():
    d, nd, m, k, G, B, T = 5, 4, 30, 1, 4, 50, 1024
    model = model_with_priors("VC", m, d, k, True, seed=195)
    n = 20_000
    gen = torch.Generator(device=DEV).manual_seed(98)
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=gen) * torch.from_numpy(model.sdX).to(DEV) + \
        torch.from_numpy(model.muX).to(DEV)
    Psi = 0.05 * torch.rand((n, d), dtype=torch.float64, device=DEV, generator=gen)
    two = X.clone()
    two[torch.rand(n, device=DEV, generator=gen) < 0.2, 1] = NAN
    eight = X.clone()
    for c in (0, 2, 4):
        eight[torch.rand(n, device=DEV, generator=gen) < 0.3, c] = NAN
    with gpz_amd.Predictor(model, tile_rows=T) as p, gpz_amd.Predictor(model, tile_rows=T) as q:
        # a handle that never calls the new entries holds the bytes it held: q stays on the entries of the parent
        for h in (p, q):
            h.predict_noisy_cov_dev(X[:300], Psi[:300]); h.draws_noisy_cov_dev(X[:300], Psi[:300], nd)
            h.predict_noisy_missing_cov_dev(two[:2000], Psi[:2000]); h.draws_noisy_missing_cov_dev(two[:2000], Psi[:2000], nd)
        held, route = p.info[1], p.route
        assert held == q.info[1] and route == q.route
        assert route.endswith(pairs_tail(m)), route                       # the clause it ends in today
        edges = np.linspace(*np.percentile(host(p.predict_noisy_missing_cov_dev(two[:2000], Psi[:2000])[0]), [3, 97]), B + 1)
        # the first gamma call adds its bytes once (the complete rows' gamma per draw among them)
        p.draws_noisy_missing_cov_dev(two[:2000], Psi[:2000], nd, return_gamma=True)
        first = p.info[1]
        assert first > held
        assert p.route.endswith(pairs_tail(m) + route_tail(m)), p.route
        p.draws_noisy_missing_cov_dev(two, Psi, nd, return_gamma=True)
        assert p.info[1] == first                                        # 2000 rows or 20 000: the same bytes
        # the first stack call adds its bytes once
        p.stack_noisy_missing_cov_dev(two[:2000], Psi[:2000], edges, n_draws=nd, seed=3, n_groups=G)
        stacked = p.info[1]
        assert stacked > first
        assert p.route.endswith(pairs_tail(m) + route_tail(m, stack=True)), p.route
        p.stack_noisy_missing_cov_dev(two, Psi, edges, n_draws=nd, seed=3, n_groups=G)
        p.draws_noisy_missing_cov_dev(two, Psi, nd, return_gamma=True)
        assert p.info[1] == stacked                                      # ten times the rows
        assert len(p._nan_groups_dev(eight)) == 8
        p.stack_noisy_missing_cov_dev(eight, Psi, edges, n_draws=nd, seed=3, n_groups=G)
        p.draws_noisy_missing_cov_dev(eight, Psi, nd, return_gamma=True)
        assert p.info[1] == stacked                                      # eight patterns
        q.predict_noisy_missing_cov_dev(eight, Psi); q.draws_noisy_missing_cov_dev(eight, Psi, nd)
        assert q.info[1] == held and q.route == route
