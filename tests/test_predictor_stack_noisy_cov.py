"""The stacked n(z) and gamma under every weight draw for rows with input noise on a covariance kind (Predictor.stack_noisy_cov_dev /
draws_noisy_cov_dev(..., return_gamma=True); k_predict_noisy_cov_gamma.hip) against the existing entries of the handle, ``gpz_amd.predict``
and the oracle: gamma_s against predict_noisy_cov_dev's gamma of the model whose weights are the draw's, every column, row, stage and
chunk edge, the same bits over tiles, orders, splits and layouts, the Psi = 0 limit, the stack against ``stack_reference_w`` fed with the
device's own per-row numbers, the refusals and constant memory.

Gates: gamma_s with exact weights at the project's gamma gate for these kinds (GATE["gamma"] of test_predictor_noisy_cov.py, nrel <=
1e-10); with a general iSigma_w max(1e-11, 10 x the spread of the parent's two routes); the stack at the derived tolerance of
tests/test_predictor_stack_noisy.py, unchanged, with s_min taken over the new widths."""
import copy

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, nrel, synth_model
from test_predictor_draws_cpu import philox_normals
from test_predictor_noisy import dev, host, noise
from test_predictor_noisy_cov import GATE
from test_predictor_noisy_cov_cpu import cov_chunks_rule
from test_predictor_stack import EPS, assert_close, setting
from test_predictor_stack_noisy_cpu import gamma_chunks_rule, stack_reference_w

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COV = ("GC", "VC")


def with_weights(model, w):
    """The model with w := w (m x k) in its set."""
    other = copy.deepcopy(model)
    other.sets["best"]["w"] = np.array(w, dtype=np.float64)
    return other


def gamma_of(model, X, Psi, tile_rows=256):
    """predict_noisy_cov_dev's gamma on a handle of its own: existing code."""
    with gpz_amd.Predictor(model, tile_rows=tile_rows) as q:
        return host(q.predict_noisy_cov_dev(dev(X), dev(Psi))[4])


def exact_model(method, m, d, k, hetero, seed):
    """iSigma_w = 2^-10 I: its Cholesky factor is exactly 2^-5 I, so w_s = w + 2^-5 z_s is the same double on host and device."""
    model = synth_model(method, m, d, k, hetero, seed=seed)
    model.sets["best"]["iSigma_w"] = np.stack([2.0 ** -10 * np.eye(m)] * k, axis=2)
    return model


def exact_weights(model, Z):
    return model.sets["best"]["w"][:, None, :] + 2.0 ** -5 * Z             # (m, nd, k)


def route_tail(m, stack=False):
    return f"; noise per draw: k_predict_noisy_cov_gamma ({gamma_chunks_rule(m)} pair chunks)" + (" + k_stack_tile_w" if stack else "")


# ---- 1. gamma_s with exact weights --------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 17), (2, 3, 5), (5, 1, 64), (5, 8, 5), (8, 1, 5), (10, 1, 5), (10, 8, 17), (5, 3, 1)]
MS = [1, 2, 7, 33, 90, 91, 128, 157, 250]
CASES = [(m, d, k, nd) for m in MS for (d, k, nd) in SHAPES if nd < 64 or m <= 33]


@pytest.mark.parametrize("method", COV)
@pytest.mark.parametrize("m,d,k,nd", CASES)
def test_gamma_per_draw_with_exact_weights(method, m, d, k, nd):
    """The reference is predict_noisy_cov_dev's gamma of the model with w := w_s (the same quantity by definition, existing code), at the
    project's gamma gate for these kinds, nrel <= 1e-10 per draw.  300 rows on 256-row tiles (a full tile and a partial one, and a last
    workgroup of 44 rows).  m = 1, 2, 7 are 1, 3 and 28 pairs: a partial K step and partial stages; m = 33 is 561 pairs, 17 stages and a
    tail of 17; m = 90 | 91, 128, 157 are the edges of the chunk counts 1 | 2, 3, 4.  Where m <= 33, 60 rows against the oracle's
    predict_noisy of the w_s model at rel <= 1e-8, on the first, the middle and the last draw (at m = 33, where an oracle call takes
    about 2 s, on the last one alone): every draw is already held to the handle's own gamma of its w_s model, so the oracle only guards
    against an error that both routes of the handle share, and such an error sits in the pair densities and the records, which no
    draw's weights enter."""
    ns = 300
    model = exact_model(method, m, d, k, bool((m + k) % 2), seed=11000 + 100 * d + 10 * k + m)
    X, Psi = catalogue(model, ns, seed=m + d), noise(ns, d, seed=m + k)
    Z = np.random.default_rng(nd + m).standard_normal((m, nd, k))
    W = exact_weights(model, Z)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F, Gam = p.draws_noisy_cov_dev(dev(X), dev(Psi), nd, Z=Z, return_gamma=True)
        assert p.route.endswith(route_tail(m)), p.route
        assert "k_stack_tile" not in p.route                             # no stack call on this handle
        assert torch.equal(F, p.draws_noisy_cov_dev(dev(X), dev(Psi), nd, Z=Z))
    assert Gam.shape == (nd, ns, k) and Gam.dtype == torch.float64
    Gam = host(Gam)
    worst, worst_orc = 0.0, 0.0
    for s in range(nd):
        ms = with_weights(model, W[:, s, :])
        worst = max(worst, nrel(Gam[s], gamma_of(ms, X, Psi)))
        if m <= 33 and s in ({nd - 1} if m == 33 else {0, nd // 2, nd - 1}):
            worst_orc = max(worst_orc, rel(Gam[s, :60], O.predict_noisy(X[:60], Psi[:60], ms)[4]))
    print(f"{method} m={m} d={d} k={k} nd={nd}: worst nrel of gamma_s against predict_noisy_cov_dev of the w_s model {worst:.3g}; "
          f"worst rel against the oracle {worst_orc:.3g}")
    assert worst <= GATE["gamma"], worst
    assert worst_orc <= 1e-8, worst_orc


# ---- 2. gamma_s with a general iSigma_w ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
def test_gamma_per_draw_with_seeded_draws(method):
    """Seeded draws of a general iSigma_w; w_s formed on the host as w + chol(sym(iSigma_w)) z_s with the Philox normals of the seed.
    Yardstick: the disagreement of two routes of the parent, gamma of the w := w_s model from the handle's predict_noisy_cov_dev against
    gpz_amd.predict.  Gate: max(1e-11, 10 x that spread) - the factor 10 for a third summation order and the host-formed w_s."""
    m, d, k, nd, ns, seed = 60, 5, 2, 6, 600, 31
    model = synth_model(method, m, d, k, True, seed=77)
    X, Psi = catalogue(model, ns, seed=78), noise(ns, d, seed=79)
    z = philox_normals(seed, m, nd, k)
    iS = model.sets["best"]["iSigma_w"]
    L = [np.linalg.cholesky(0.5 * (iS[:, :, o] + iS[:, :, o].T)) for o in range(k)]
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F, Gam = p.draws_noisy_cov_dev(dev(X), dev(Psi), nd, seed=seed, return_gamma=True)
    Gam = host(Gam)
    figures = []
    for s in range(nd):
        ws = np.stack([model.sets["best"]["w"][:, o] + L[o] @ z[:, s, o] for o in range(k)], axis=1)
        ms = with_weights(model, ws)
        a = gamma_of(ms, X, Psi)
        b = gpz_amd.predict(X, ms, Psi=Psi)[4]
        figures.append((nrel(Gam[s], a), nrel(a, b)))
        print(f"{method} draw {s}: nrel(gamma_s, predict_noisy_cov_dev of w_s) {figures[-1][0]:.3g}; spread of the parent's two routes "
              f"{figures[-1][1]:.3g}")
    for s, (got, spread) in enumerate(figures):
        assert got <= max(1e-11, 10 * spread), (s, got, spread)


# ---- 3. column and row edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncol", [1, 15, 16, 17, 64, 65, 128, 129])
def test_column_and_row_edges(ncol):
    """m = 17, d = 3, VC, k = 1: n_draws at a partial block, a full block and the pass edge on gridDim.z for 4 or 8 blocks per pass; rows
    at the edges of a wave's 16 rows and a workgroup's 64, on 64-row and 256-row tiles.  Each case against test 1's reference on the
    first, the middle and the last draw."""
    m, d, k, nmax = 17, 3, 1, 257
    model = exact_model("VC", m, d, k, True, seed=1200 + ncol)
    X, Psi = catalogue(model, nmax, seed=ncol), noise(nmax, d, seed=ncol + 1)
    Z = np.random.default_rng(ncol).standard_normal((m, ncol, k))
    W = exact_weights(model, Z)
    draws = sorted({0, ncol // 2, ncol - 1})
    ref = {s: gamma_of(with_weights(model, W[:, s, :]), X, Psi) for s in draws}
    Xd, Pd = dev(X), dev(Psi)
    worst = 0.0
    for tile in (64, 256):
        with gpz_amd.Predictor(model, tile_rows=tile) as p:
            for n in (1, 15, 16, 17, 63, 64, 65, 257):
                F, Gam = p.draws_noisy_cov_dev(Xd[:n], Pd[:n], ncol, Z=Z, return_gamma=True)
                assert Gam.shape == (ncol, n, k) and bool(torch.isfinite(Gam).all())
                for s in draws:
                    worst = max(worst, nrel(host(Gam[s]), ref[s][:n]))
                    assert nrel(host(Gam[s]), ref[s][:n]) <= GATE["gamma"], (tile, n, s, nrel(host(Gam[s]), ref[s][:n]))
    print(f"ncol={ncol}: worst nrel {worst:.3g}")


# ---- 4. the same bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
def test_same_bits_over_tiles_orders_splits_and_layouts(method):
    n, d, m, k, nd = 1500, 5, 40, 2, 5
    model = synth_model(method, m, d, k, True, seed=81)
    X32 = catalogue(model, n, seed=82).astype(np.float32)
    P32 = noise(n, d, seed=83).astype(np.float32)
    X, Psi = X32.astype(np.float64), P32.astype(np.float64)
    Xd, Pd = dev(X), dev(Psi)
    groups, weights = setting(n, 3, seed=5)
    gd, wd = dev(groups, torch.int64), dev(weights)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    kw = dict(n_draws=nd, seed=9, n_groups=3)

    def gam(p, x, psi, draws=nd, **more):
        return p.draws_noisy_cov_dev(x, psi, draws, seed=9, return_gamma=True, **more)[1]

    with gpz_amd.Predictor(model, tile_rows=256) as p:
        edges = np.linspace(*np.percentile(host(p.predict_noisy_cov_dev(Xd, Pd)[0]), [3, 97]), 51)
        G5 = gam(p, Xd, Pd)
        b = p.stack_noisy_cov_dev(Xd, Pd, edges, groups=gd, weights=wd, **kw)
        c = p.stack_noisy_cov_dev(Xd, Pd, edges, groups=gd, weights=wd, **kw)
        for u, v in zip(b, c):
            assert np.array_equal(u, v)                                  # the same call twice

        def same(got, what):
            assert torch.equal(got, G5), (what, float((got - G5).abs().max()))

        def same_stack(got, what):
            for u, v in zip(got, b):
                assert np.array_equal(u, v), what

        same(gam(p, Xd, Pd, 17)[:nd], "the first 5 of 17 draws")
        same(torch.cat([gam(p, Xd[:333], Pd[:333]), gam(p, Xd[333:], Pd[333:])], dim=1), "a split into two calls")
        assert torch.equal(gam(p, Xd[perm], Pd[perm]), G5[:, perm]), "a row permutation"
        same(gam(p, dev(X32, torch.float32), dev(P32, torch.float32)), "float32")
        same(gam(p, Xd.T.contiguous().T, Pd.T.contiguous().T), "transposed views")
        X2, P2 = dev(np.repeat(X, 2, axis=0)), dev(np.repeat(Psi, 2, axis=0))
        same(gam(p, X2[::2], P2[::2]), "row-sliced views")
        same_stack(p.stack_noisy_cov_dev(dev(X32, torch.float32), dev(P32, torch.float32), edges, groups=gd, weights=wd, **kw), "float32")
        same_stack(p.stack_noisy_cov_dev(X2[::2], P2.T.contiguous().T[::2], edges, groups=gd, weights=wd, **kw), "strided")
        col = Pd[:, 2].contiguous()
        full = col[:, None].expand(n, d).contiguous()
        bc = gam(p, Xd, full)
        assert torch.equal(gam(p, Xd, col[:, None]), bc), "Psi (n, 1)"
        assert torch.equal(gam(p, Xd, col), bc), "Psi (n,)"
        sb = p.stack_noisy_cov_dev(Xd, full, edges, groups=gd, weights=wd, **kw)
        for u, v in zip(p.stack_noisy_cov_dev(Xd, col[:, None], edges, groups=gd, weights=wd, **kw), sb):
            assert np.array_equal(u, v), "Psi (n, 1) in the stack"
        # a split on the last tile edge adds to the bits of the whole call (the accumulators take the tiles in their order, and the second
        # part is then one tile: whole = (sum of the tiles before) + last, as the += forms it); anywhere else within the stack's tolerance
        for cut in (1280, 700):
            parts = [p.stack_noisy_cov_dev(Xd[i:j], Pd[i:j], edges, groups=gd[i:j], weights=wd[i:j], **kw) for i, j in ((0, cut), (cut, n))]
            total = [parts[0][f] + parts[1][f] for f in range(4)]
            if cut % 256 == 0:
                for u, v in zip(total, b):
                    assert np.array_equal(u, v), "a split on the last tile edge"
            else:
                ref, th, tm, tw, _ = reference_w(p, model, Xd, Pd, edges, nd, 9, groups, weights, 3)
                assert_close(gpz_amd.api.StackResult(*total, edges), ref, th, tm, tw, "a split inside a tile")
        # the selection applies to rows, Psi, labels and weights alike
        sel = torch.zeros(n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        half = p.stack_noisy_cov_dev(Xd[sel], Pd[sel], edges, groups=gd[sel], weights=wd[sel], **kw)
        for u, v in zip(p.stack_noisy_cov_dev(Xd, Pd, edges, groups=gd, weights=wd, selection=sel, **kw), half):
            assert np.array_equal(u, v)
        assert torch.equal(gam(p, Xd, Pd, selection=sel), G5[:, ::2])
    # other tile sizes: gamma_s bit for bit.  The stack's row slabs and the order in which the accumulators take the tiles follow the tile
    # size (k_stack_tile_w and k_stack_accum, unchanged), so its sums run in another order and its bits differ from those of 256-row
    # tiles (seen at both sizes): it is held to the stack tolerance, as the diagonal kinds' stack is
    for T in (64, 1024):
        with gpz_amd.Predictor(model, tile_rows=T) as q:
            assert torch.equal(gam(q, Xd, Pd), G5), T
            res = q.stack_noisy_cov_dev(Xd, Pd, edges, groups=gd, weights=wd, **kw)
            ref, th, tm, tw, _ = reference_w(q, model, Xd, Pd, edges, nd, 9, groups, weights, 3)
            assert_close(res, ref, th, tm, tw, f"{T}-row tiles")


# ---- 5. Psi = 0 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
def test_zero_noise_gives_zero_gamma_and_finite_widths(method):
    """|gamma_s| <= 1e-11 |mu_s^2| per draw; gamma_s is then rounding noise of either sign, and the stack runs with finite widths because
    the draw columns clamp it at 0."""
    n, d, m, k, nd = 500, 5, 60, 2, 4
    model = synth_model(method, m, d, k, True, seed=61)
    X = catalogue(model, n, seed=62)
    Xd, P0 = dev(X), torch.zeros((n, d), dtype=torch.float64, device=DEV)
    with gpz_amd.Predictor(model) as p:
        F, Gam = p.draws_noisy_cov_dev(Xd, P0, nd, seed=3, return_gamma=True)
        mu2 = (host(F) - model.muY) ** 2
        for s in range(nd):
            ratio = np.linalg.norm(host(Gam[s])) / np.linalg.norm(mu2[s])
            print(f"{method} draw {s}: |gamma_s| / |mu_s^2| {ratio:.3g}")
            assert ratio <= 1e-11, (s, ratio)
        edges = np.linspace(*np.percentile(host(F), [3, 97]), 41)
        res = p.stack_noisy_cov_dev(Xd, P0, edges, n_draws=nd, seed=3)
        assert all(np.all(np.isfinite(a)) for a in res)
        assert np.all(res.hist >= 0.0) and res.hist[1:].sum() > 0.0


# ---- 6. stack parity --------------------------------------------------------------------------------------------------------------------
def reference_w(p, model, Xd, Pd, edges, n_draws, seed, groups, weights, G):
    """stack_reference_w fed with the device's own per-row numbers (predict_noisy_cov_dev and draws_noisy_cov_dev(return_gamma=True)), and
    the tolerances of test_predictor_stack_noisy.py's reference_w with s_min over the new widths."""
    mu, sigma, _, beta = (host(t) for t in p.predict_noisy_cov_dev(Xd, Pd)[:4])
    F = S2 = None
    if n_draws:
        Ft, Gt = p.draws_noisy_cov_dev(Xd, Pd, n_draws, seed=seed, return_gamma=True)
        F, S2 = host(Ft), beta[None] + np.maximum(host(Gt), 0.0)
    ref = stack_reference_w(mu, sigma, F, S2, edges, groups, weights, n_groups=G)
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
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_stack_parity(method, hetero, k):
    """2500 rows on 1024-row tiles (the last one partial), three groups with rows left out and random weights, 1, 37 and 300 bins, no
    draws and 5 seeded draws; column 0's sum_mu / sum_w against predict_noisy_cov_dev's weighted mean."""
    d, ns, G, m = 5, 2500, 3, 40
    model = synth_model(method, m, d, k, hetero, seed=4000 + 100 * COV.index(method) + 10 * k + hetero)
    X, Psi = catalogue(model, ns, seed=k + 40), noise(ns, d, seed=k + 41)
    Xd, Pd = dev(X), dev(Psi)
    groups, weights = setting(ns, G, seed=m)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        mu0 = host(p.predict_noisy_cov_dev(Xd, Pd)[0])
        for B in (1, 37, 300):
            edges = np.linspace(*np.percentile(mu0, [3, 97]), B + 1)
            for nd in (0, 5):
                ref, th, tm, tw, mu = reference_w(p, model, Xd, Pd, edges, nd, 77, groups, weights, G)
                rd = p.stack_noisy_cov_dev(Xd, Pd, edges, n_draws=nd, seed=77, groups=gd, n_groups=G, weights=wd)
                what = f"{method} hetero={hetero} k={k} B={B} draws={nd}"
                assert rd.hist.shape == (1 + nd, G, k, B)
                assert_close(rd, ref, th, tm, tw, what)
                if nd:
                    assert rd.hist[1:].sum() > 0.0
                for gi in range(G):
                    r = groups == gi
                    mean = (weights[r] @ mu[r]) / weights[r].sum()
                    tol = (tm[0, gi, :, 0] + 8 * EPS * np.abs(weights[r] @ mu[r])) / weights[r].sum() + 4 * EPS * np.abs(mean)
                    assert np.all(np.abs(rd.sum_mu[0, gi] / rd.sum_w[gi] - mean) <= tol), (what, gi)
        assert p.route.endswith(route_tail(m, stack=True)), p.route


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
ERR_ARG, ERR_UNSUPPORTED = -1, -5                                       # include/gpz_hip.h


def raw_entries(p, model, x, psi, lab, wt, G, B, nd):
    """Both C entries on outputs prefilled with -7: the return codes, the messages and the outputs."""
    d, k, n = model.d, model.k, x.shape[0]
    muX, sdX, muY = p._norm_vectors()
    sd2 = np.ascontiguousarray(sdX ** 2)
    edges = np.ascontiguousarray(np.linspace(-3, 3, B + 1)[None, :] - muY[:, None])
    stream = torch.cuda.current_stream(x.device).cuda_stream
    lib, h = p._lib, p._handle()
    lead = (h, *p._x_args(x), *p._psi_args(psi, n), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(sd2))
    out = [np.full(s, -7.0) for s in ((1 + nd, G, k, B), (G,), (1 + nd, G, k), (1 + nd, G, k))]
    rc1 = lib.gpz_predictor_stack_noisy_cov_dev(*lead, nd, 1, None, _lib.dptr(edges), B, None if lab is None else lab.data_ptr(), G,
                                                None if wt is None else wt.data_ptr(), *(_lib.dptr(a) for a in out), _lib.dptr(muY), stream)
    msg1 = lib.gpz_last_error().decode() if rc1 else ""
    F = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    Gm = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    rc2 = lib.gpz_predictor_draws_gamma_noisy_cov_dev(*lead, _lib.dptr(muY), nd, 1, None, F.data_ptr(), Gm.data_ptr(), stream)
    msg2 = lib.gpz_last_error().decode() if rc2 else ""
    torch.cuda.synchronize()
    return (rc1, rc2), (msg1, msg2), out, (F, Gm)


@pytest.mark.parametrize("kw", [{"method": "VD"}, {"d": 12}, {"m": 300}, {"k": 9}])
def test_models_outside_the_scope_are_refused(kw):
    a = {"method": "VC", "m": 20, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    X, Psi = dev(catalogue(model, 40, seed=6)), dev(noise(40, a["d"], seed=7))
    e = np.linspace(-3, 3, 11)
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match="stack_noisy_dev" if a["method"] == "VD" else "predict_noisy_cov_fits"):
            p.stack_noisy_cov_dev(X, Psi, e, n_draws=2)
        with pytest.raises(ValueError, match="draws_dev" if a["method"] == "VD" else "predict_noisy_cov_fits"):
            p.draws_noisy_cov_dev(X, Psi, 4, return_gamma=True)
        held = p.info[1]
        rcs, msgs, out, FG = raw_entries(p, model, X, Psi, None, None, 2, 10, 3)     # the C entries refuse it themselves
        assert rcs == (ERR_UNSUPPORTED, ERR_UNSUPPORTED), (rcs, msgs)
        assert all("predict_noisy_cov_fits" in t for t in msgs), msgs
        assert all(np.all(a_ == -7.0) for a_ in out) and all(bool((t == -7.0).all()) for t in FG)
        assert p.info[1] == held and "noise" not in p.route              # the handle gained no byte


def test_bad_rows_noise_labels_and_weights_are_refused_with_the_outputs_untouched():
    n, d, m, k, G, B, nd = 300, 3, 12, 2, 2, 10, 3
    model = synth_model("VC", m, d, k, False, seed=13)
    X, Psi = catalogue(model, n, seed=14), noise(n, d, seed=15)

    def bad(a, at, v):
        b = np.array(a, dtype=np.float64)
        b[at] = v
        return b

    cases = [("nan in X", bad(X, (7, 1), np.nan), Psi, None, None, ERR_UNSUPPORTED),
             ("negative Psi", X, bad(Psi, (9, 0), -1e-3), None, None, ERR_ARG),
             ("nan Psi", X, bad(Psi, (9, 2), np.nan), None, None, ERR_ARG),
             ("inf Psi", X, bad(Psi, (299, 1), np.inf), None, None, ERR_ARG),
             ("bad label", X, Psi, bad(np.zeros(n), 5, G).astype(np.int32), None, ERR_ARG),
             ("bad weight", X, Psi, None, bad(np.ones(n), 11, -1.0), ERR_ARG)]
    e = np.linspace(-3, 3, B + 1)
    with gpz_amd.Predictor(model, tile_rows=128) as p:
        Xd, Pd = dev(X), dev(Psi)
        good_s = p.stack_noisy_cov_dev(Xd, Pd, e, n_draws=nd, seed=1, n_groups=G)
        good_g = p.draws_noisy_cov_dev(Xd, Pd, nd, seed=1, return_gamma=True)
        assert np.all(np.isfinite(good_s.hist)) and good_s.hist[1:].sum() > 0.0
        rcs, _, out, FG = raw_entries(p, model, Xd, Pd, None, None, G, B, nd)
        assert rcs == (0, 0) and all(np.all(a != -7.0) for a in out[1:]) and all(bool((t != -7.0).all()) for t in FG)
        held = p.info[1]
        for what, x, psi, lab, wt, want in cases:
            lt = None if lab is None else torch.from_numpy(lab).to(DEV)
            wtt = None if wt is None else dev(wt)
            rcs, msgs, out, FG = raw_entries(p, model, dev(x), dev(psi), lt, wtt, G, B, nd)
            assert rcs[0] == want, (what, rcs, msgs)
            assert rcs[1] == (0 if lab is not None or wt is not None else want), (what, rcs, msgs)   # (the draws take no labels)
            assert all(np.all(a == -7.0) for a in out), what              # refused before any tile kernel has run
            if rcs[1]:
                assert all(bool((t == -7.0).all()) for t in FG), what
            assert p.info[1] == held, what
            again = p.stack_noisy_cov_dev(Xd, Pd, e, n_draws=nd, seed=1, n_groups=G)   # the next good call: the bits it gave before
            for u, v in zip(again, good_s):
                assert np.array_equal(u, v), what
            for u, v in zip(p.draws_noisy_cov_dev(Xd, Pd, nd, seed=1, return_gamma=True), good_g):
                assert torch.equal(u, v), what
        with pytest.raises(_lib.GpzError, match="Psi has an element"):
            p.stack_noisy_cov_dev(Xd, dev(bad(Psi, (0, 0), -1.0)), e)
        with pytest.raises(_lib.GpzError, match="missing values"):
            p.draws_noisy_cov_dev(dev(bad(X, (3, 0), np.nan)), Pd, nd, return_gamma=True)
        with pytest.raises(_lib.GpzError, match="label"):
            p.stack_noisy_cov_dev(Xd, Pd, e, groups=torch.full((n,), 7, device=DEV), n_groups=2)


def test_a_scan_refusal_on_a_fresh_handle_writes_nothing_and_adds_its_bytes_once():
    """The scans of X and Psi run behind rows_prepare, as for the diagonal kinds: a first call that a scan refuses leaves the outputs
    untouched, and leaves on the handle what the kind's tables and slots take - no more than a good call of the same shape takes, and
    nothing on the second refusal.  A model outside the scope is refused before anything is taken (the test above)."""
    n, d, m, k, G, B, nd = 300, 3, 12, 2, 2, 10, 3
    model = synth_model("VC", m, d, k, False, seed=13)
    X, Psi = catalogue(model, n, seed=14), noise(n, d, seed=15)
    bad_x = np.array(X)
    bad_x[7, 1] = np.nan
    with gpz_amd.Predictor(model, tile_rows=128) as p, gpz_amd.Predictor(model, tile_rows=128) as q:
        p.predict_dev(dev(X)); q.predict_dev(dev(X))
        fresh = p.info[1]
        assert fresh == q.info[1]
        rcs, msgs, out, FG = raw_entries(p, model, dev(bad_x), dev(Psi), None, None, G, B, nd)
        assert rcs == (ERR_UNSUPPORTED, ERR_UNSUPPORTED), (rcs, msgs)
        assert all(np.all(a == -7.0) for a in out) and all(bool((t == -7.0).all()) for t in FG)
        refused = p.info[1]
        rcs, _, out, FG = raw_entries(p, model, dev(bad_x), dev(Psi), None, None, G, B, nd)
        assert rcs == (ERR_UNSUPPORTED, ERR_UNSUPPORTED) and p.info[1] == refused            # the second refusal adds nothing
        rcs, _, _, _ = raw_entries(q, model, dev(X), dev(Psi), None, None, G, B, nd)
        assert rcs == (0, 0)
        print(f"bytes: fresh {fresh}, after a refused first call {refused}, after a good first call {q.info[1]}")
        assert fresh <= refused <= q.info[1]
        rcs, _, out_p, FG_p = raw_entries(p, model, dev(X), dev(Psi), None, None, G, B, nd)  # the refused handle then works
        rcs2, _, out_q, FG_q = raw_entries(q, model, dev(X), dev(Psi), None, None, G, B, nd)
        assert rcs == (0, 0) and rcs2 == (0, 0) and p.info[1] == q.info[1]
        assert all(np.array_equal(u, v) for u, v in zip(out_p, out_q)) and all(torch.equal(u, v) for u, v in zip(FG_p, FG_q))


# ---- 7b. the tile route of the handle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
def test_the_tile_route_of_the_handle(method):
    """force_tiles=True: the PHI tile of the draws is the tile route's own, and W has mp rows.  gamma_s against predict_noisy_cov_dev of
    the w_s model at the gamma gate, the draws against the fused-route handle's at 1e-12 (test 8 of test_predictor_noisy_cov.py's gate
    for two orders of the same product), the stack against stack_reference_w fed with this handle's own per-row numbers."""
    n, d, m, k, nd, G = 1500, 5, 40, 2, 5, 3
    model = exact_model(method, m, d, k, True, seed=321)
    X, Psi = catalogue(model, n, seed=322), noise(n, d, seed=323)
    Xd, Pd = dev(X), dev(Psi)
    Z = np.random.default_rng(324).standard_normal((m, nd, k))
    W = exact_weights(model, Z)
    groups, weights = setting(n, G, seed=5)
    with gpz_amd.Predictor(model, tile_rows=1024, force_tiles=True) as p, gpz_amd.Predictor(model, tile_rows=1024) as q:
        assert p.route.startswith("tiles:") and q.route.startswith("fused:")
        F, Gam = p.draws_noisy_cov_dev(Xd, Pd, nd, Z=Z, return_gamma=True)
        assert p.route.endswith(route_tail(m)), p.route
        Fq = q.draws_noisy_cov_dev(Xd, Pd, nd, Z=Z)
        assert nrel(host(F), host(Fq)) <= 1e-12, nrel(host(F), host(Fq))
        for s in range(nd):
            ref = gamma_of(with_weights(model, W[:, s, :]), X, Psi)
            print(f"{method} tile route, draw {s}: nrel {nrel(host(Gam[s]), ref):.3g}")
            assert nrel(host(Gam[s]), ref) <= GATE["gamma"], (s, nrel(host(Gam[s]), ref))
        edges = np.linspace(*np.percentile(host(p.predict_noisy_cov_dev(Xd, Pd)[0]), [3, 97]), 38)
        res = p.stack_noisy_cov_dev(Xd, Pd, edges, n_draws=nd, seed=77, groups=dev(groups, torch.int64), n_groups=G, weights=dev(weights))
        ref, th, tm, tw, _ = reference_w(p, model, Xd, Pd, edges, nd, 77, groups, weights, G)
        assert_close(res, ref, th, tm, tw, f"{method} tile route")
        assert p.route.endswith(route_tail(m, stack=True)), p.route


# ---- 8. memory and route ----------------------------------------------------------------------------------------------------------------
def test_memory_and_route():
    d, nd, m, k, G, B, T = 5, 4, 60, 1, 4, 50, 1024
    model = synth_model("VC", m, d, k, True, seed=195)
    X, Psi = dev(catalogue(model, 5000, seed=196)), dev(noise(5000, d, seed=197))
    noise_tail = f"; noise: k_predict_noisy_cov_small ({cov_chunks_rule(m, d, k)} pair chunks)"
    with gpz_amd.Predictor(model, tile_rows=T) as p, gpz_amd.Predictor(model, tile_rows=T) as q:
        # a handle that never calls the new entries holds the bytes it held: q stays on the entries of the parent
        for h in (p, q):
            h.predict_dev(X[:300]); h.draws_dev(X[:300], nd); h.predict_noisy_cov_dev(X[:300], Psi[:300])
            h.draws_noisy_cov_dev(X[:300], Psi[:300], nd)
        held = p.info[1]
        assert held == q.info[1]
        assert p.route.endswith(noise_tail), p.route                     # the clause it ends in today
        edges = np.linspace(*np.percentile(host(p.predict_noisy_cov_dev(X, Psi)[0]), [3, 97]), B + 1)
        # the first gamma call adds its bytes once
        p.draws_noisy_cov_dev(X[:300], Psi[:300], nd, return_gamma=True)
        first = p.info[1]
        assert first == held + gamma_chunks_rule(m) * nd * k * T * 8, (first - held)   # the chunk slab alone
        assert p.route.endswith(route_tail(m)), p.route
        p.draws_noisy_cov_dev(X, Psi, nd, return_gamma=True)
        assert p.info[1] == first                                        # 300 rows or 5000: the same bytes
        # the first stack call adds its bytes once
        p.stack_noisy_cov_dev(X[:300], Psi[:300], edges, n_draws=nd, seed=3, n_groups=G)
        stacked = p.info[1]
        assert stacked > first
        assert p.route.endswith(route_tail(m, stack=True)), p.route
        for ns in (5000, 17, 1024, 1025):
            p.stack_noisy_cov_dev(X[:ns], Psi[:ns], edges, n_draws=nd, seed=3, n_groups=G)
            p.draws_noisy_cov_dev(X[:ns], Psi[:ns], nd, return_gamma=True)
        assert p.info[1] == stacked
        assert q.info[1] == held and q.route.endswith(noise_tail)
    # 5000 rows first: the same bytes as 300 rows first; draws alone leave no "noise" in the route
    with gpz_amd.Predictor(model, tile_rows=T) as r:
        r.draws_noisy_cov_dev(X[:300], Psi[:300], nd)
        assert "noise" not in r.route, r.route
        r.predict_dev(X[:300]); r.draws_dev(X[:300], nd); r.predict_noisy_cov_dev(X[:300], Psi[:300])
        r.draws_noisy_cov_dev(X, Psi, nd, return_gamma=True)
        r.stack_noisy_cov_dev(X, Psi, edges, n_draws=nd, seed=3, n_groups=G)
        assert r.info[1] == stacked
    # a fresh handle whose first call with Psi is one of the new ones
    with gpz_amd.Predictor(model, tile_rows=T) as r:
        F, Gam = r.draws_noisy_cov_dev(X[:300], Psi[:300], nd, seed=3, return_gamma=True)
        assert r.route.endswith(route_tail(m)) and noise_tail in r.route, r.route
        with gpz_amd.Predictor(model, tile_rows=T) as s:
            assert torch.equal(s.draws_noisy_cov_dev(X[:300], Psi[:300], nd, seed=3), F)
    # no draws: no factors, no W, no draws buffer and no chunk slab
    with gpz_amd.Predictor(model, tile_rows=T) as r, gpz_amd.Predictor(model, tile_rows=T) as s:
        r.predict_noisy_cov_dev(X[:300], Psi[:300])
        s.predict_noisy_cov_dev(X[:300], Psi[:300])
        base = r.info[1]
        res = r.stack_noisy_cov_dev(X, Psi, edges, n_groups=G)
        assert res.hist.shape == (1, G, k, B) and res.hist.sum() > 0.0
        assert "factors" not in r.route and "draws:" not in r.route, r.route
        assert r.route.endswith(route_tail(m, stack=True)), r.route
        s.stack_noisy_cov_dev(X, Psi, edges, n_draws=nd, n_groups=G)
        assert base < r.info[1] < s.info[1]
        # what the call without draws added holds no slab, no W and no draws slot: the widths of one column and the stack's own buffers
        rec = G * B + 3 * G
        from test_predictor_stack import stack_slabs
        want = k * T * 8 + (k * (B + 1) + k) * 8 + k * rec * 8 * (1 + stack_slabs(k, rec, T))
        assert r.info[1] - base == want, (r.info[1] - base, want)
