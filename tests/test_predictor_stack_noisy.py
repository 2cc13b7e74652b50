"""Stacks of rows with input noise and gamma under every weight draw (Predictor.stack_noisy / stack_noisy_dev / draws_dev(..., Psi=,
return_gamma=True); k_predict_noisy_gamma.hip, k_predict_stack_w.hip) against the existing entries of the handle, ``gpz_amd.predict``
and the oracle: gamma_s against predict_dev(X, Psi) of the model whose weights are the draw's, the Psi = 0 limit, the stack against
``stack_reference_w`` fed with the device's own per-row numbers, the same bits over tiles, orders, splits and layouts, additivity, the
refusals and constant memory.

Stack tolerance: the derived one of tests/test_predictor_stack.py, unchanged, with s_min taken over the new widths."""
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
from test_predictor_stack import EPS, assert_close, setting, stack_slabs
from test_predictor_stack_noisy_cpu import gamma_chunks_rule, stack_reference_w

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIAG = ("GL", "VL", "GD", "VD")


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def noise(n, d, seed):
    return np.random.default_rng(seed).gamma(1.0, 0.05, (n, d))


def with_weights(model, w):
    """The model with w := w (m x k) in its set."""
    other = copy.deepcopy(model)
    other.sets["best"]["w"] = np.array(w, dtype=np.float64)
    return other


def gamma_of(model, X, Psi, tile_rows=256):
    """predict_dev(X, Psi)'s gamma on a handle of its own: existing code."""
    with gpz_amd.Predictor(model, tile_rows=tile_rows) as q:
        return host(q.predict_dev(dev(X), Psi=dev(Psi))[4])


# ---- 1. gamma_s with exact weights --------------------------------------------------------------------------------------------------------
# every value of d, k and n_draws of the issue at every m; all draws of a case are checked
SHAPES = [(1, 1, 17), (1, 3, 64), (5, 1, 64), (5, 8, 5), (20, 1, 5), (20, 8, 17), (5, 3, 1)]


@pytest.mark.parametrize("m", [7, 17, 50, 100, 140, 250])
@pytest.mark.parametrize("d,k,nd", SHAPES)
def test_gamma_per_draw_with_exact_weights(m, d, k, nd):
    """iSigma_w = 2^-10 I: the Cholesky factor is exactly 2^-5 I, so w_s = w + 2^-5 z_s is the same double on host and device.  The
    reference is predict_dev(X, Psi)'s gamma of the model with w := w_s (the same quantity by definition), at the project's own gate
    nrel <= 1e-11 per draw.  ns = 600 over 256-row tiles; m = 7, 17, 50, 250 are 28, 153, 1275 and 31 375 pairs: partial 4-pair K
    steps and partial 32-record stages; m = 7, 17, 50 run in 1 pair chunk, m = 100 in 2, m = 140 in 3, m = 250 in 4: every chunk count.
    Where m <= 50, 100 rows against the oracle at rel <= 1e-8: every draw, except at m = 50 with 64 draws, where it is every 8th
    draw and the last (an oracle call takes 0.1 s there).  Nine are enough in that case: every one of the 64 draws is already held
    to predict_dev of its own w_s model at 1e-11, so the oracle only guards against an error that both routes of the handle share,
    and such an error sits in the pair densities and the table, which no draw's weights enter."""
    ns = 600
    model = synth_model("VD" if (m + d) % 2 else "GL", m, d, k, bool(k % 2), seed=9000 + 100 * d + 10 * k + m)
    model.sets["best"]["iSigma_w"] = np.stack([2.0 ** -10 * np.eye(m)] * k, axis=2)
    X, Psi = catalogue(model, ns, seed=m + d), noise(ns, d, seed=m + k)
    Z = np.random.default_rng(nd + m).standard_normal((m, nd, k))
    W = model.sets["best"]["w"][:, None, :] + 2.0 ** -5 * Z             # (m, nd, k)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F, Gam = p.draws_dev(dev(X), nd, Z=Z, Psi=dev(Psi), return_gamma=True)
        assert p.route.endswith(f"; noise per draw: k_predict_noisy_gamma ({gamma_chunks_rule(m)} pair chunks)"), p.route
        assert "k_stack_tile" not in p.route                             # no stack call on this handle
        assert torch.equal(F, p.draws_dev(dev(X), nd, Z=Z, Psi=dev(Psi)))
    assert Gam.shape == (nd, ns, k) and Gam.dtype == torch.float64
    Gam = host(Gam)
    worst = 0.0
    for s in range(nd):
        ms = with_weights(model, W[:, s, :])
        ref = gamma_of(ms, X, Psi)
        worst = max(worst, nrel(Gam[s], ref))
        assert nrel(Gam[s], ref) <= 1e-11, (s, nrel(Gam[s], ref))
        if m <= 50 and (m < 50 or nd < 64 or s % 8 == 0 or s == nd - 1):
            orc = O.predict_noisy(X[:100], Psi[:100], ms)[4]
            assert rel(Gam[s, :100], orc) <= 1e-8, (s, rel(Gam[s, :100], orc))
    print(f"m={m} d={d} k={k} nd={nd}: worst nrel of gamma_s against predict_dev of the w_s model {worst:.3g}")


# ---- 2. gamma_s with a general iSigma_w ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["VD", "GL"])
def test_gamma_per_draw_with_seeded_draws(method):
    """Seeded draws of a general iSigma_w; w_s formed on the host as w + chol(sym(iSigma_w)) z_s with the Philox normals of the seed.
    Yardstick: the disagreement of two routes of the parent, gamma of the w := w_s model from the handle's predict_dev against
    gpz_amd.predict.  Gate: max(1e-11, 10 x that spread) - the factor 10 for a third summation order and the host-formed w_s.
    Measured on one MI355X: nrel 1.0e-14 .. 1.5e-14 (VD) and 4.3e-15 .. 5.7e-15 (GL) against spreads of
    4.9e-14 .. 6.4e-14 and 1.9e-14 .. 2.2e-14, so the gate in force is 1e-11."""
    m, d, k, nd, ns, seed = 60, 5, 2, 6, 600, 31
    model = synth_model(method, m, d, k, True, seed=77)
    X, Psi = catalogue(model, ns, seed=78), noise(ns, d, seed=79)
    z = philox_normals(seed, m, nd, k)
    iS = model.sets["best"]["iSigma_w"]
    L = [np.linalg.cholesky(0.5 * (iS[:, :, o] + iS[:, :, o].T)) for o in range(k)]
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F, Gam = p.draws_dev(dev(X), nd, seed=seed, Psi=dev(Psi), return_gamma=True)
    Gam = host(Gam)
    for s in range(nd):
        ws = np.stack([model.sets["best"]["w"][:, o] + L[o] @ z[:, s, o] for o in range(k)], axis=1)
        ms = with_weights(model, ws)
        a = gamma_of(ms, X, Psi)
        b = gpz_amd.predict(X, ms, Psi=Psi)[4]
        spread = nrel(a, b)
        got = nrel(Gam[s], a)
        print(f"{method} draw {s}: nrel(gamma_s, predict_dev of w_s) {got:.3g}; spread of the parent's two routes {spread:.3g}")
        assert got <= max(1e-11, 10 * spread), (s, got, spread)


# ---- 3. Psi = 0 -------------------------------------------------------------------------------------------------------------------------
def test_zero_noise_gives_zero_gamma_and_finite_widths():
    """|gamma_s| <= 1e-11 |mu_s^2| (the gate and the reasoning of test_zero_noise_is_the_noise_free_prediction); gamma_s is then rounding
    noise of either sign, and the stack runs with finite widths because the draw columns clamp it at 0."""
    n, d, m, k, nd = 500, 5, 60, 2, 4
    model = synth_model("VD", m, d, k, True, seed=61)
    X = catalogue(model, n, seed=62)
    Xd, P0 = dev(X), torch.zeros((n, d), dtype=torch.float64, device=DEV)
    with gpz_amd.Predictor(model) as p:
        F, Gam = p.draws_dev(Xd, nd, seed=3, Psi=P0, return_gamma=True)
        mu2 = (host(F) - model.muY) ** 2
        for s in range(nd):
            assert np.linalg.norm(host(Gam[s])) <= 1e-11 * np.linalg.norm(mu2[s]), s
        edges = np.linspace(*np.percentile(host(F), [3, 97]), 41)
        res = p.stack_noisy_dev(Xd, P0, edges, n_draws=nd, seed=3)
        assert all(np.all(np.isfinite(a)) for a in res)
        assert np.all(res.hist >= 0.0) and res.hist[1:].sum() > 0.0


# ---- 4. stack parity --------------------------------------------------------------------------------------------------------------------
def reference_w(p, model, Xd, Pd, edges, n_draws, seed, groups, weights, G):
    """stack_reference_w fed with the device's own per-row numbers, and test_predictor_stack.py's tolerances with s_min over the new widths."""
    mu, sigma, _, beta = (host(t) for t in p.predict_dev(Xd, Psi=Pd)[:4])
    F = S2 = None
    if n_draws:
        Ft, Gt = p.draws_dev(Xd, n_draws, seed=seed, Psi=Pd, return_gamma=True)
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


@pytest.mark.parametrize("method", DIAG)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_stack_parity(method, hetero, k):
    """2500 rows on 1024-row tiles (the last one partial), three groups with rows left out and random weights, 1, 37 and 300 bins, no
    draws and 5 seeded draws, host and device entries; column 0's sum_mu / sum_w against predict_dev's weighted mean."""
    d, ns, G, m = 5, 2500, 3, 40
    model = synth_model(method, m, d, k, hetero, seed=4000 + 100 * DIAG.index(method) + 10 * k + hetero)
    X, Psi = catalogue(model, ns, seed=k + 40), noise(ns, d, seed=k + 41)
    Xd, Pd = dev(X), dev(Psi)
    groups, weights = setting(ns, G, seed=m)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        mu0 = host(p.predict_dev(Xd, Psi=Pd)[0])
        for B in (1, 37, 300):
            edges = np.linspace(*np.percentile(mu0, [3, 97]), B + 1)
            for nd in (0, 5):
                ref, th, tm, tw, mu = reference_w(p, model, Xd, Pd, edges, nd, 77, groups, weights, G)
                rd = p.stack_noisy_dev(Xd, Pd, edges, n_draws=nd, seed=77, groups=gd, n_groups=G, weights=wd)
                rh = p.stack_noisy(X, Psi, edges, n_draws=nd, seed=77, groups=groups, n_groups=G, weights=weights)
                what = f"{method} hetero={hetero} k={k} B={B} draws={nd}"
                assert_close(rd, ref, th, tm, tw, what + " dev")
                assert_close(rh, ref, th, tm, tw, what + " host")
                for gi in range(G):
                    r = groups == gi
                    mean = (weights[r] @ mu[r]) / weights[r].sum()
                    tol = (tm[0, gi, :, 0] + 8 * EPS * np.abs(weights[r] @ mu[r])) / weights[r].sum() + 4 * EPS * np.abs(mean)
                    assert np.all(np.abs(rd.sum_mu[0, gi] / rd.sum_w[gi] - mean) <= tol), (what, gi)


# ---- 5. bits ----------------------------------------------------------------------------------------------------------------------------
def test_same_bits_over_entries_tiles_orders_splits_and_layouts():
    n, d, m, k = 700, 5, 40, 2
    model = synth_model("VD", m, d, k, True, seed=81)
    X32 = catalogue(model, n, seed=82).astype(np.float32)
    P32 = noise(n, d, seed=83).astype(np.float32)
    X, Psi = X32.astype(np.float64), P32.astype(np.float64)
    Xd, Pd = dev(X), dev(Psi)
    groups, weights = setting(n, 3, seed=5)
    gd, wd = dev(groups, torch.int64), dev(weights)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        edges = np.linspace(*np.percentile(host(p.predict_dev(Xd, Psi=Pd)[0]), [3, 97]), 51)
        kw = dict(n_draws=5, seed=9, n_groups=3)
        a = p.stack_noisy(X, Psi, edges, groups=groups, weights=weights, **kw)
        b = p.stack_noisy_dev(Xd, Pd, edges, groups=gd, weights=wd, **kw)
        c = p.stack_noisy_dev(Xd, Pd, edges, groups=gd, weights=wd, **kw)
        a2 = p.stack_noisy(X, Psi, edges, groups=groups, weights=weights, **kw)
        for u, v, w, x in zip(a, b, c, a2):
            assert np.array_equal(u, v) and np.array_equal(v, w) and np.array_equal(u, x)   # host = device; the same call twice
        F, G5 = p.draws_dev(Xd, 5, seed=9, Psi=Pd, return_gamma=True)

        def same(got, what):
            assert torch.equal(got, G5), (what, float((got - G5).abs().max()))

        same(p.draws_dev(Xd, 17, seed=9, Psi=Pd, return_gamma=True)[1][:5], "the first 5 of 17 draws")
        same(torch.cat([p.draws_dev(Xd[:333], 5, seed=9, Psi=Pd[:333], return_gamma=True)[1],
                        p.draws_dev(Xd[333:], 5, seed=9, Psi=Pd[333:], return_gamma=True)[1]], dim=1), "a split into two calls")
        gp = p.draws_dev(Xd[perm], 5, seed=9, Psi=Pd[perm], return_gamma=True)[1]
        assert torch.equal(gp, G5[:, perm]), "a row permutation"
        same(p.draws_dev(dev(X32, torch.float32), 5, seed=9, Psi=dev(P32, torch.float32), return_gamma=True)[1], "float32")
        same(p.draws_dev(Xd.T.contiguous().T, 5, seed=9, Psi=Pd.T.contiguous().T, return_gamma=True)[1], "transposed views")
        X2, P2 = dev(np.repeat(X, 2, axis=0)), dev(np.repeat(Psi, 2, axis=0))
        same(p.draws_dev(X2[::2], 5, seed=9, Psi=P2[::2], return_gamma=True)[1], "row-sliced views")
        col = Pd[:, 2].contiguous()
        bc = p.draws_dev(Xd, 5, seed=9, Psi=col[:, None].expand(n, d).contiguous(), return_gamma=True)[1]
        assert torch.equal(p.draws_dev(Xd, 5, seed=9, Psi=col[:, None], return_gamma=True)[1], bc), "Psi (n, 1)"
        assert torch.equal(p.draws_dev(Xd, 5, seed=9, Psi=col, return_gamma=True)[1], bc), "Psi (n,)"
        # selection applies to rows, Psi, labels and weights alike
        sel = np.zeros(n, dtype=bool)
        sel[::2] = True
        half = p.stack_noisy(X[sel], Psi[sel], edges, groups=groups[sel], weights=weights[sel], **kw)
        for got in (p.stack_noisy(X, Psi, edges, groups=groups, weights=weights, selection=sel, **kw),
                    p.stack_noisy_dev(Xd, Pd, edges, groups=gd, weights=wd, selection=dev(sel, torch.bool), **kw)):
            for u, v in zip(got, half):
                assert np.array_equal(u, v)
    for T in (64, 4096):
        with gpz_amd.Predictor(model, tile_rows=T) as q:
            assert torch.equal(q.draws_dev(Xd, 5, seed=9, Psi=Pd, return_gamma=True)[1], G5), T


# ---- 6. additivity ----------------------------------------------------------------------------------------------------------------------
def test_two_chunks_add_to_one_call():
    n, d, m, k, G, B = 3000, 5, 50, 2, 3, 80
    model = synth_model("GD", m, d, k, True, seed=3)
    X, Psi = catalogue(model, n, seed=4), noise(n, d, seed=6)
    Xd, Pd = dev(X), dev(Psi)
    groups, weights = setting(n, G, seed=5)
    gd, wd = dev(groups, torch.int64), dev(weights)
    kw = dict(n_draws=4, seed=11, n_groups=G)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        edges = np.linspace(*np.percentile(host(p.predict_dev(Xd, Psi=Pd)[0]), [3, 97]), B + 1)
        whole = p.stack_noisy_dev(Xd, Pd, edges, groups=gd, weights=wd, **kw)
        parts = [p.stack_noisy_dev(Xd[i:j], Pd[i:j], edges, groups=gd[i:j], weights=wd[i:j], **kw) for i, j in ((0, 1234), (1234, n))]
        ref, th, tm, tw, _ = reference_w(p, model, Xd, Pd, edges, 4, 11, groups, weights, G)
    total = gpz_amd.api.StackResult(*(parts[0][f] + parts[1][f] for f in range(4)), edges)
    assert_close(total, ref, th, tm, tw, "two chunks")
    assert_close(whole, ref, th, tm, tw, "one call")


# ---- 7. refusals on the device -------------------------------------------------------------------------------------------------------------
def test_device_refusals_leave_the_results_untouched():
    n, d, m, k, G, B, nd = 300, 3, 12, 2, 2, 10, 3
    model = synth_model("VD", m, d, k, False, seed=13)
    X, Psi = catalogue(model, n, seed=14), noise(n, d, seed=15)
    muX, sdX, muY = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1), (s,)))
                     for v, s in ((model.muX, d), (model.sdX, d), (model.muY, k)))
    sd2 = np.ascontiguousarray(sdX ** 2)
    edges = np.ascontiguousarray(np.linspace(-3, 3, B + 1)[None, :] - muY[:, None])
    lib = _lib.load()

    def bad(a, at, v):
        b = np.array(a, dtype=np.float64)
        b[at] = v
        return b

    ERR_ARG, ERR_UNSUPPORTED = -1, -5                                   # include/gpz_hip.h
    cases = [("nan in X", bad(X, (7, 1), np.nan), Psi, None, None, ERR_UNSUPPORTED),
             ("negative Psi", X, bad(Psi, (9, 0), -1e-3), None, None, ERR_ARG),
             ("nan Psi", X, bad(Psi, (9, 2), np.nan), None, None, ERR_ARG),
             ("inf Psi", X, bad(Psi, (299, 1), np.inf), None, None, ERR_ARG),
             ("bad label", X, Psi, bad(np.zeros(n), 5, G).astype(np.int32), None, ERR_ARG),
             ("bad weight", X, Psi, None, bad(np.ones(n), 11, -1.0), ERR_ARG)]
    with gpz_amd.Predictor(model, tile_rows=128) as p:
        h = p._handle()
        ok = p.stack_noisy_dev(dev(X), dev(Psi), np.linspace(-3, 3, B + 1), n_draws=nd, seed=1)    # the entry itself works
        assert np.all(np.isfinite(ok.hist))
        for what, x, psi, lab, wt, want in cases:
            xt, pt = dev(x), dev(psi)
            lt = None if lab is None else torch.from_numpy(lab).to(DEV)
            wtt = None if wt is None else dev(wt)
            out = [np.full(s, -7.0) for s in ((1 + nd, G, k, B), (G,), (1 + nd, G, k), (1 + nd, G, k))]
            rc = lib.gpz_predictor_stack_noisy_dev(h, xt.data_ptr(), 0, n, xt.stride(0), xt.stride(1), pt.data_ptr(), 0, pt.stride(0),
                                                   pt.stride(1), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(sd2), nd, 1, None,
                                                   _lib.dptr(edges), B, None if lt is None else lt.data_ptr(), G,
                                                   None if wtt is None else wtt.data_ptr(), *(_lib.dptr(a) for a in out), _lib.dptr(muY),
                                                   torch.cuda.current_stream().cuda_stream)
            msg = lib.gpz_last_error().decode()
            assert rc == want, (what, rc, msg)
            assert all(np.all(a == -7.0) for a in out), what              # nothing was written
            if what != "nan in X" and lab is None and wt is None:
                F = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
                Gm = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
                rc = lib.gpz_predictor_draws_gamma_noisy_dev(h, xt.data_ptr(), 0, n, xt.stride(0), xt.stride(1), pt.data_ptr(), 0,
                                                             pt.stride(0), pt.stride(1), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(sd2),
                                                             _lib.dptr(muY), nd, 1, None, F.data_ptr(), Gm.data_ptr(),
                                                             torch.cuda.current_stream().cuda_stream)
                assert rc == ERR_ARG, (what, rc)
                assert bool((F == -7.0).all()) and bool((Gm == -7.0).all()), what
        with pytest.raises(_lib.GpzError, match="Psi has an element"):
            p.stack_noisy_dev(dev(X), dev(bad(Psi, (0, 0), -1.0)), np.linspace(-3, 3, B + 1))
        with pytest.raises(_lib.GpzError, match="Psi has an element"):    # the host entry's own scan
            lib_rc = p._lib.gpz_predictor_stack_noisy
            Xn = np.asfortranarray((X - model.muX) / model.sdX)
            out = [np.full(s, -7.0) for s in ((1, G, k, B), (G,), (1, G, k), (1, G, k))]
            rc = lib_rc(h, _lib.dptr(Xn), n, _lib.dptr(np.asfortranarray(bad(Psi, (250, 1), np.nan))), 0, 0, None, _lib.dptr(edges), B,
                        None, G, None, *(_lib.dptr(a) for a in out), _lib.dptr(muY))
            assert rc == ERR_ARG and all(np.all(a == -7.0) for a in out)
            _lib.check(rc)


# ---- 8. memory and route ----------------------------------------------------------------------------------------------------------------
def test_memory_and_route():
    model = synth_model("VD", 100, 5, 2, True, seed=8)
    k, G, B, T, nd = 2, 4, 50, 4096, 6
    X, Psi = catalogue(model, 10_000, seed=1), noise(10_000, 5, seed=2)
    Xd, Pd = dev(X), dev(Psi)
    groups, weights = setting(10_000, G, seed=2)
    with gpz_amd.Predictor(model, tile_rows=T) as p, gpz_amd.Predictor(model, tile_rows=T) as q:
        edges = np.linspace(*np.percentile(p.predict(X)[0], [3, 97]), B + 1)
        fresh = q.route
        assert "noise" not in fresh and fresh == f"fused: k_predict_small, {T}-row tiles"
        q.predict(X)
        b0 = p.info[1]
        assert q.info[1] == b0
        # a handle that makes only noise-free calls holds what the parent's rule says (tests/test_predictor_stack.py)
        p.stack(X, edges, groups=groups, n_groups=G, weights=weights)
        rec = G * B + 3 * G
        want = 2 * (T * 4 + T * 8) + (k * (B + 1) + k) * 8 + k * rec * 8 * (1 + stack_slabs(k, rec, T))
        assert p.info[1] - b0 == want, (p.info[1] - b0, want)
        assert "noise" not in p.route and p.route.endswith(f"{stack_slabs(k, rec, T)} row slabs"), p.route
        # the new entry: the same bytes after 1 and after 5 calls, whatever ns
        q.stack_noisy_dev(Xd[:3000], Pd[:3000], edges, n_draws=nd, seed=3, n_groups=G)
        first = q.info[1]
        assert first > b0
        for ns in (10_000, 17, 5000, 4096, 4097):
            q.stack_noisy_dev(Xd[:ns], Pd[:ns], edges, n_draws=nd, seed=3, n_groups=G)
        assert q.info[1] == first
        assert f"; noise per draw: k_predict_noisy_gamma ({gamma_chunks_rule(100)} pair chunks) + k_stack_tile_w" in q.route, q.route
        with gpz_amd.Predictor(model, tile_rows=T) as r:
            r.predict(X)
            r.stack_noisy_dev(Xd, Pd, edges, n_draws=nd, seed=3, n_groups=G)
            assert r.info[1] == first                                    # 10 000 rows first: the same bytes as 3000 rows first
        # no draws: no factor, W, draws or gamma buffer
        with gpz_amd.Predictor(model, tile_rows=T) as r:
            r.predict(X)
            r.stack_noisy_dev(Xd, Pd, edges, n_groups=G)
            assert "factors" not in r.route and "draws:" not in r.route, r.route
            assert r.info[1] < first
