"""Stacked predictive densities on the device (gpz_amd.Predictor.stack over gpz_predictor_stack) against ``stack_reference`` fed with
``predict`` and ``draws`` of the same handle: parity on every method and route, device memory, bit reproducibility, the mean over many
draws, and the edge cases.

Tolerance (derived, not measured): |hist - ref| <= eps W_g (n_g + 64 (1 + E / s_min)) per entry, W_g the group's sum of weights, n_g its
rows, E = max|edge - muY| + max|mu|, s_min the smallest width of the call: n_g eps W_g bounds any summation order of non-negative terms,
64 (1 + E / s_min) covers two CDF evaluations at a few ulp each and the argument rounding of shifting the edges instead of mu.  The sums:
n_g eps sum(omega |mu|^p) plus 8 eps relative."""
import numpy as np
import pytest

import gpz_amd
from gpz_amd import _lib
from test_predictor import synth_model, catalogue
from test_predictor_stack_cpu import stack_reference

pytestmark = pytest.mark.gpu

METHODS = ("GL", "VL", "GD", "VD", "GC", "VC")
EPS = np.finfo(np.float64).eps


def reference_of(p, model, X, edges, n_draws, seed, Z, groups, weights, G):
    """(hist, sum_w, sum_mu, sum_mu2) of stack_reference and the per-entry tolerances of the module docstring."""
    mu, sigma, _, beta = p.predict(X)[:4]
    F = p.draws(X, n_draws, seed=seed, Z=Z) if n_draws else None
    ref = stack_reference(mu, sigma, F, beta, edges, groups, weights, n_groups=G)
    n, k = mu.shape
    g = np.zeros(n, dtype=int) if groups is None else np.asarray(groups)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    cols = [mu] + ([] if F is None else list(F))
    muY = np.asarray(model.muY).reshape(-1)
    E = max(np.max(np.abs(np.asarray(edges)[None, :] - muY[:, None])), 0.0) + max(np.max(np.abs(c - muY)) for c in cols)
    s_min = np.sqrt(min(sigma.min(), beta.min()))
    W = np.array([w[g == gi].sum() for gi in range(G)])
    ng = np.array([(g == gi).sum() for gi in range(G)])
    tol_h = EPS * W * (ng + 64.0 * (1.0 + E / s_min))                    # per group
    tol_m = np.empty((len(cols), G, k, 2))
    for c, m in enumerate(cols):
        for gi in range(G):
            r = g == gi
            tol_m[c, gi, :, 0] = ng[gi] * EPS * (w[r] @ np.abs(m[r]))
            tol_m[c, gi, :, 1] = ng[gi] * EPS * (w[r] @ (m[r] * m[r]))
    return ref, tol_h, tol_m, ng * EPS * W


def assert_close(res, ref, tol_h, tol_m, tol_w, what=""):
    hist, sum_w, sum_mu, sum_mu2 = ref
    assert res.hist.shape == hist.shape and res.sum_mu.shape == sum_mu.shape
    dh = np.abs(res.hist - hist) / np.maximum(tol_h[None, :, None, None], 1e-300)
    dw = np.abs(res.sum_w - sum_w) / np.maximum(tol_w + 8 * EPS * np.abs(sum_w), 1e-300)
    d1 = np.abs(res.sum_mu - sum_mu) / np.maximum(tol_m[..., 0] + 8 * EPS * np.abs(sum_mu), 1e-300)
    d2 = np.abs(res.sum_mu2 - sum_mu2) / np.maximum(tol_m[..., 1] + 8 * EPS * np.abs(sum_mu2), 1e-300)
    print(f"{what} worst error / tolerance: hist {dh.max():.3g}, sum_w {dw.max():.3g}, sum_mu {d1.max():.3g}, sum_mu2 {d2.max():.3g}; "
          f"hist tolerance / largest entry {tol_h.max() / max(hist.max(), 1e-300):.3g}")
    assert np.all(np.isfinite(res.hist))
    assert dh.max() <= 1.0, (what, dh.max())
    assert dw.max() <= 1.0 and d1.max() <= 1.0 and d2.max() <= 1.0, (what, dw.max(), d1.max(), d2.max())


def setting(n, G=3, seed=0):
    """Labels in [-1, G) and random weights for n rows."""
    rng = np.random.default_rng(seed)
    groups = rng.integers(-1, G, n)
    weights = rng.uniform(0.0, 2.0, n)
    return groups, weights


def edges_for(mu, B):
    lo, hi = np.percentile(mu, [3, 97])
    return np.linspace(lo, hi, B + 1)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("force_tiles", [False, True])
def test_parity(method, hetero, k, force_tiles):
    """2500 rows over 512-row tiles (the last one partial), m on both sides of the fused kernels' limit, three groups with some rows left
    out, random weights, 64 bins; no draws, seeded draws and draws from Z."""
    d, ns, G, B = 5, 2500, 3, 64
    for m in (40, 264):
        model = synth_model(method, m, d, k, hetero, seed=100 * METHODS.index(method) + 10 * k + m + hetero)
        X = catalogue(model, ns, seed=m + k)
        groups, weights = setting(ns, G, seed=m)
        Z = np.random.default_rng(m + 1).standard_normal((m, 5, k))
        with gpz_amd.Predictor(model, tile_rows=512, force_tiles=force_tiles) as p:
            edges = edges_for(p.predict(X)[0], B)
            for n_draws, seed, z in ((0, 0, None), (5, 77, None), (5, 0, Z)):
                res = p.stack(X, edges, n_draws=n_draws, seed=seed, Z=z, groups=groups, n_groups=G, weights=weights)
                ref, th, tm, tw = reference_of(p, model, X, edges, n_draws, seed, z, groups, weights, G)
                assert_close(res, ref, th, tm, tw, f"{method} hetero={hetero} k={k} m={m} tiles={force_tiles} draws={n_draws}")
                assert np.array_equal(res.edges, edges)
            assert "stack: k_stack_tile" in p.route, p.route


def stack_slabs(Q, rec, T):
    """predict_stack_slabs of k_predict_stack.hip, stated a second time on purpose: the byte counts below follow from the rule."""
    R = min((8192 + Q - 1) // Q, 64, (T + 255) // 256)
    while R > 1 and Q * R * rec > 2 ** 24:
        R //= 2
    return max(R, 1)


def test_device_memory_and_route():
    model = synth_model("VD", 100, 5, 2, True, seed=8)
    k, G, B, T = 2, 4, 50, 4096
    X = catalogue(model, 10_000, seed=1)
    groups, weights = setting(10_000, G, seed=2)
    with gpz_amd.Predictor(model, tile_rows=T) as p, gpz_amd.Predictor(model, tile_rows=T) as q:
        edges = edges_for(p.predict(X)[0], B)
        q.predict(X)
        b0 = p.info[1]
        assert q.info[1] == b0                                           # before its first stack call: a predict-only handle's bytes
        r0 = p.stack(X, edges, groups=groups, n_groups=G, weights=weights)
        assert "factors" not in p.route and "draws" not in p.route and "stack:" in p.route, p.route
        rec = G * B + 3 * G
        want = 2 * (T * 4 + T * 8) + (k * (B + 1) + k) * 8 + k * rec * 8 * (1 + stack_slabs(k, rec, T))
        assert p.info[1] - b0 == want, (p.info[1] - b0, want)            # labels, weights, edges, accumulators, slabs: no draws buffers
        b1 = p.info[1]
        p.stack(X[:5000], edges, groups=groups[:5000], n_groups=G, weights=weights[:5000])
        assert p.info[1] == b1                                           # the same shape again: nothing new
        # with draws: the same bytes as a handle that made the same draws call, plus the (larger) stack buffers
        p.draws(X[:100], 6, seed=3)
        q.draws(X[:100], 6, seed=3)
        b2 = p.info[1]
        assert b2 - b1 == q.info[1] - b0
        r1 = p.stack(X, edges, n_draws=6, seed=3, groups=groups, n_groups=G, weights=weights)
        Q = 7 * k
        assert p.info[1] - b2 == Q * rec * 8 * (1 + stack_slabs(Q, rec, p.info[0]))   # new accumulators and slabs only
        assert np.array_equal(r1.hist[0], r0.hist[0]) and "factors:" in p.route
        assert p.info[3] == 1 and q.info[3] == 1                         # runs: predict calls only


@pytest.mark.parametrize("method,force_tiles", [("VD", False), ("GC", True)])
def test_reproducibility(method, force_tiles):
    model = synth_model(method, 50, 5, 2, True, seed=3)
    ns, G, B = 6000, 3, 80
    X = catalogue(model, ns, seed=4)
    groups, weights = setting(ns, G, seed=5)
    kw = dict(n_draws=4, seed=11, n_groups=G)
    with gpz_amd.Predictor(model, tile_rows=1024, force_tiles=force_tiles) as p:
        edges = edges_for(p.predict(X)[0], B)
        a = p.stack(X, edges, groups=groups, weights=weights, **kw)
        b = p.stack(X, edges, groups=groups, weights=weights, **kw)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)                                  # the same call: the same bits
        ref, th, tm, tw = reference_of(p, model, X, edges, 4, 11, None, groups, weights, G)
        assert_close(a, ref, th, tm, tw, "tile 1024")
        parts = [p.stack(X[i:j], edges, groups=groups[i:j], weights=weights[i:j], **kw) for i, j in ((0, 1234), (1234, 4000), (4000, ns))]
        summed = type(a)(*[sum(f) for f in zip(*[r[:4] for r in parts])], edges)
        assert_close(summed, ref, th, tm, tw, "three calls")
        perm = np.random.default_rng(6).permutation(ns)
        assert_close(p.stack(X[perm], edges, groups=groups[perm], weights=weights[perm], **kw), ref, th, tm, tw, "permuted")
    with gpz_amd.Predictor(model, tile_rows=2560, force_tiles=force_tiles) as p:
        assert_close(p.stack(X, edges, groups=groups, weights=weights, **kw), ref, th, tm, tw, "tile 2560")


def test_mean_over_many_draws_is_the_predictive_stack():
    S, B = 2000, 40
    model = synth_model("VC", 30, 3, 1, True, seed=9)
    X = catalogue(model, 64, seed=10)
    with gpz_amd.Predictor(model) as p:
        edges = edges_for(p.predict(X)[0], B)
        r = p.stack(X, edges, n_draws=S, seed=77)
    h0, hs = r.hist[0, 0, 0], r.hist[1:, 0, 0]
    se = hs.std(axis=0, ddof=1) / np.sqrt(S)
    big = h0 > 0.01 * h0.sum()
    assert big.sum() >= B // 2
    assert np.all(np.abs(hs.mean(axis=0) - h0)[big] <= 5 * se[big]), np.max(np.abs(hs.mean(axis=0) - h0)[big] / se[big])


def raw_stack(p, model, Xn, ndraws, edges_n, B, group, G, weight):
    lib = _lib.load()
    k = model.k
    out = [np.full(((1 + max(ndraws, 0)) * G * k * B,), np.nan), np.full(G, np.nan), np.full((1 + max(ndraws, 0)) * G * k, np.nan),
           np.full((1 + max(ndraws, 0)) * G * k, np.nan)]
    rc = lib.gpz_predictor_stack(p._handle(), _lib.dptr(Xn), Xn.shape[0], ndraws, 1, None, _lib.dptr(edges_n), B,
                                 None if group is None else group.ctypes.data_as(_lib.c_int32_p), G, _lib.dptr(weight),
                                 *(_lib.dptr(a) for a in out), None)
    return rc, out


def test_edge_cases():
    model = synth_model("VC", 20, 3, 2, True, seed=31)
    ns, k = 300, 2
    X = catalogue(model, ns, seed=32)
    with gpz_amd.Predictor(model) as p:
        mu = p.predict(X)[0]
        edges = edges_for(mu, 16)
        full = p.stack(X, edges, n_draws=3, seed=1)
        # no rows; every row left out
        r = p.stack(X[:0], edges, n_draws=3, seed=1)
        assert r.hist.shape == (4, 1, k, 16) and not r.hist.any() and not r.sum_w.any()
        r = p.stack(X, edges, n_draws=3, seed=1, groups=np.full(ns, -1), n_groups=2)
        assert r.hist.shape == (4, 2, k, 16) and not r.hist.any() and not r.sum_w.any() and not r.sum_mu.any()
        # a weight of 0 is a row left out
        w = np.ones(ns)
        w[::3] = 0.0
        g = np.where(w > 0, 0, -1)
        a, b = p.stack(X, edges, n_draws=3, seed=1, weights=w), p.stack(X, edges, n_draws=3, seed=1, groups=g)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
        # selection = the selected rows
        sel = w > 0
        c = p.stack(X, edges, n_draws=3, seed=1, selection=sel, weights=w, groups=np.zeros(ns, dtype=int))
        d = p.stack(X[sel], edges, n_draws=3, seed=1)
        for u, v in zip(c, d):
            assert np.array_equal(u, v)
        # edges far from every mu: zeros, no NaN
        far = p.stack(X, np.linspace(1e6, 2e6, 9), n_draws=3, seed=1)
        assert not far.hist.any() and np.all(np.isfinite(far.sum_mu)) and np.array_equal(far.sum_w, [float(ns)])
        # a single bin over everything holds every weight; the sums do not depend on the edges
        one = p.stack(X, [-1e6, 1e6], n_draws=3, seed=1, weights=w)
        assert np.allclose(one.hist, w.sum(), rtol=ns * EPS, atol=0) and np.array_equal(one.sum_mu, a.sum_mu)
        assert np.allclose(full.sum_mu[0, 0] / full.sum_w[0], mu.mean(axis=0), rtol=0, atol=1e-13 * np.abs(mu).max())
        # the size limit: G B = 4096 works
        G, B = 64, 64
        groups = np.random.default_rng(1).integers(-1, G, ns)
        e64 = edges_for(mu, B)
        res = p.stack(X, e64, n_draws=2, seed=5, groups=groups, n_groups=G)
        ref, th, tm, tw = reference_of(p, model, X, e64, 2, 5, None, groups, None, G)
        assert_close(res, ref, th, tm, tw, "G B = 4096")
        G, B = 4096, 1
        groups = np.arange(ns) % G
        res = p.stack(X, [edges[0], edges[-1]], groups=groups, n_groups=G)
        ref, th, tm, tw = reference_of(p, model, X, [edges[0], edges[-1]], 0, 0, None, groups, None, G)
        assert_close(res, ref, th, tm, tw, "G = 4096")
        # the raw entry: refusals
        Xn = np.asfortranarray((X[:10] - model.muX) / model.sdX)
        en = np.ascontiguousarray(edges[None, :] - np.asarray(model.muY).reshape(k, 1))
        rc, out = raw_stack(p, model, Xn, 0, en, 16, None, 1, None)
        assert rc == 0 and np.all(np.isfinite(out[0]))
        big = np.ascontiguousarray(np.tile(np.linspace(0.0, 1.0, 4098), (k, 1)))
        assert raw_stack(p, model, Xn, 0, big, 4097, None, 1, None)[0] == -1          # G B over GPZ_STACK_MAX_GROUP_BINS
        assert "GPZ_STACK_MAX_GROUP_BINS" in _lib.load().gpz_last_error().decode()
        assert raw_stack(p, model, Xn, 0, en, 16, None, 257, None)[0] == -1           # 257 x 16 bins
        assert raw_stack(p, model, Xn, -1, en, 16, None, 1, None)[0] == -1
        assert raw_stack(p, model, Xn, 8192, en, 16, None, 1, None)[0] == -1          # (1 + ndraws) k over GPZ_DRAWS_MAX_COLUMNS
        assert raw_stack(p, model, Xn, 0, en, 0, None, 1, None)[0] == -1
        bad = en.copy()
        bad[1, 5] = bad[1, 4]
        assert raw_stack(p, model, Xn, 0, bad, 16, None, 1, None)[0] == -1
        bad[1, 5] = np.nan
        assert raw_stack(p, model, Xn, 0, bad, 16, None, 1, None)[0] == -1
        lab = np.zeros(10, dtype=np.int32)
        lab[3] = 2
        assert raw_stack(p, model, Xn, 0, en, 16, lab, 2, None)[0] == -1
        lab[3] = -2
        assert raw_stack(p, model, Xn, 0, en, 16, lab, 2, None)[0] == -1
        for v in (-1.0, np.nan, np.inf):
            wt = np.ones(10)
            wt[7] = v
            assert raw_stack(p, model, Xn, 0, en, 16, None, 1, wt)[0] == -1
        # rows with NaN
        Xb = X.copy()
        Xb[7, 1] = np.nan
        with pytest.raises(ValueError, match="1 rows"):
            p.stack(Xb, edges)
        Xbn = np.asfortranarray((Xb[:10] - model.muX) / model.sdX)
        assert raw_stack(p, model, Xbn, 0, en, 16, None, 1, None)[0] == -5
        assert raw_stack(p, model, Xbn, 2, en, 16, None, 1, None)[0] == -5
        again = p.stack(X, edges, n_draws=3, seed=1)                     # the handle is fine after the refusals
        for u, v in zip(full, again):
            assert np.array_equal(u, v)
    with pytest.raises(RuntimeError):
        p.stack(X, edges)
