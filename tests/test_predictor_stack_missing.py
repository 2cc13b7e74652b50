"""Stacks of rows with missing inputs and gamma under every weight draw (Predictor.stack_missing_dev, draws_dev(..., missing=True,
return_gamma=True); k_predict_missing_gamma.hip) against the existing entries of the handle, ``gpz_amd.predict`` and the oracle: gamma_s
against predict_dev(X, missing=True) of the model whose weights are the draw's, the stack against ``stack_reference_w`` fed with the
device's own per-row numbers, the same bits over tiles, orders, company, layouts and numbers of draws, additivity, the refusals and
constant memory.

Stack tolerance: the derived one of tests/test_predictor_stack.py, unchanged, with s_min taken over the new widths.

Bits: gamma_s is held to the same bits over everything the issue lists.  The stack's fields are sums over rows in the order of
DESIGN.md section 14, which is not redefined here: as for ``stack_dev``, another tile size or row order may change their last bits, so
the stack is held to the same bits where its order of summation is the same (the same call twice, every layout of X, the columns of a
call with fewer draws, a catalogue against the sum of its patterns) and to ``assert_close`` over tile sizes and a permutation."""
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
from test_predictor_missing_cpu import chunks_rule
from test_predictor_stack import EPS, assert_close, setting
from test_predictor_stack_noisy import with_weights
from test_predictor_stack_noisy_cpu import stack_reference_w

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIAG = ("GL", "VL", "GD", "VD")
NAN = float("nan")


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def gamma_of(model, X, tile_rows=256):
    """predict_dev(X, missing=True)'s gamma on a handle of its own: existing code."""
    with gpz_amd.Predictor(model, tile_rows=tile_rows) as q:
        return host(q.predict_dev(dev(X), missing=True)[4])


def four_patterns(X):
    """Of every ten rows: five with one dimension missing (the last one), one with only dimension 0 observed, one with nothing observed,
    three complete.  At d = 1 the first and the third are one pattern and the second is complete."""
    X = X.copy()
    r = np.arange(X.shape[0]) % 10
    X[r < 5, X.shape[1] - 1] = NAN
    X[r == 5, 1:] = NAN
    X[r == 6, :] = NAN
    return X


# ---- 1. gamma_s with exact weights --------------------------------------------------------------------------------------------------------
# every m of the issue with two of its shapes (d, k, n_draws); every shape at four or five values of m
A, B_, C, D, E, F_ = (1, 1, 17), (5, 1, 64), (5, 3, 1), (5, 8, 5), (20, 1, 5), (20, 8, 17)
CASES = [(1, A), (1, D), (2, B_), (2, C), (11, E), (11, F_), (17, A), (17, B_), (62, C), (62, D), (63, E), (63, F_), (80, A), (80, C),
         (100, B_), (100, D), (105, E), (105, A), (115, F_), (115, C), (120, B_), (120, E), (128, D), (128, F_), (256, B_), (256, F_)]


@pytest.mark.parametrize("m,shape", CASES)
def test_gamma_per_draw_with_exact_weights(m, shape):
    """iSigma_w = 2^-10 I: the Cholesky factor is exactly 2^-5 I, so w_s = w + 2^-5 z_s is the same double on host and device.  The
    reference is predict_dev(X, missing=True)'s gamma of the model with w := w_s (the same quantity by definition), at the project's own
    gate nrel <= 1e-11 per draw over the rows with missing values; complete rows are exactly 0.0.  600 rows on 256-row tiles (the
    largest group has 300).  m = 1 .. 256 walks the chunk counts 1, 2, 3, 4, 5, 6, 7, 8 (62 | 63, 80, 100, 105, 115, 120, 128) and the
    edges of the 16-wide K blocks and 64-pair groups; the columns are 17, 64, 3, 40, 5 and 136: partial 16-column blocks, and 136 is a
    second launch of one block behind eight.  Where m <= 50, the first 100 rows (all four patterns) against the oracle at rel <= 1e-8:
    every draw, except with 64 draws, where it is every 8th draw and the last.  Nine are enough there: every one of the 64 draws is
    already held to predict_dev of its own w_s model at 1e-11, so the oracle only guards against an error that both routes of the
    handle share, and such an error sits in the pair expectations and the tables, which no draw's weights enter."""
    d, k, nd = shape
    ns = 600
    model = model_with_priors("VD" if (m + d) % 2 else "GL", m, d, k, bool(k % 2), seed=9100 + 100 * d + 10 * k + m)
    model.sets["best"]["iSigma_w"] = np.stack([2.0 ** -10 * np.eye(m)] * k, axis=2)
    X = four_patterns(catalogue(model, ns, seed=m + d))
    miss = np.isnan(X).any(axis=1)
    Z = np.random.default_rng(nd + m).standard_normal((m, nd, k))
    W = model.sets["best"]["w"][:, None, :] + 2.0 ** -5 * Z             # (m, nd, k)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        Fd, Gam = p.draws_dev(dev(X), nd, Z=Z, missing=True, return_gamma=True)
        assert p.route.endswith(f"; missing per draw: k_predict_missing_gamma ({chunks_rule(m)} pair chunks)"), p.route
        assert "k_stack_tile" not in p.route                             # no stack call on this handle
        assert torch.equal(Fd, p.draws_dev(dev(X), nd, Z=Z, missing=True))
    assert Gam.shape == (nd, ns, k) and Gam.dtype == torch.float64
    Gam = host(Gam)
    assert np.all(Gam[:, ~miss] == 0.0)
    worst = 0.0
    for s in range(nd):
        ms = with_weights(model, W[:, s, :])
        ref = gamma_of(ms, X)
        got = nrel(Gam[s][miss], ref[miss])
        worst = max(worst, got)
        assert got <= 1e-11, (s, got)
        if m <= 50 and (nd < 64 or s % 8 == 0 or s == nd - 1):
            orc = O.predict_any(X[:100], ms)[4]
            assert rel(Gam[s, :100], orc) <= 1e-8, (s, rel(Gam[s, :100], orc))
    print(f"m={m} d={d} k={k} nd={nd}: worst nrel of gamma_s against predict_dev of the w_s model {worst:.3g}")


# ---- 2. gamma_s with a general iSigma_w ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["VD", "GL"])
def test_gamma_per_draw_with_seeded_draws(method):
    """Seeded draws of a general iSigma_w; w_s formed on the host as w + chol(sym(iSigma_w)) z_s with the Philox normals of the seed.
    Yardstick: the disagreement of two routes of the parent, gamma of the w := w_s model from the handle's predict_dev(missing=True)
    against gpz_amd.predict.  Gate: max(1e-11, 10 x that spread) - the factor 10 for a third summation order and the host-formed w_s,
    as in test_predictor_stack_noisy.py.  The measured figures are in DESIGN.md section 19."""
    m, d, k, nd, ns, seed = 60, 5, 2, 6, 600, 31
    model = model_with_priors(method, m, d, k, True, seed=77)
    X = knock_out(catalogue(model, ns, seed=78), seed=79)
    miss = np.isnan(X).any(axis=1)
    z = philox_normals(seed, m, nd, k)
    iS = model.sets["best"]["iSigma_w"]
    L = [np.linalg.cholesky(0.5 * (iS[:, :, o] + iS[:, :, o].T)) for o in range(k)]
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        _, Gam = p.draws_dev(dev(X), nd, seed=seed, missing=True, return_gamma=True)
    Gam = host(Gam)
    for s in range(nd):
        ws = np.stack([model.sets["best"]["w"][:, o] + L[o] @ z[:, s, o] for o in range(k)], axis=1)
        ms = with_weights(model, ws)
        a = gamma_of(ms, X)
        b = gpz_amd.predict(X, ms)[4]
        spread = nrel(a[miss], b[miss])
        got = nrel(Gam[s][miss], a[miss])
        print(f"{method} draw {s}: nrel(gamma_s, predict_dev of w_s) {got:.3g}; spread of the parent's two routes {spread:.3g}")
        assert got <= max(1e-11, 10 * spread), (s, got, spread)
        assert np.all(Gam[s][~miss] == 0.0)


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------------------
def same_stack(a, b, what):
    for f, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), (what, f)


def test_same_bits_over_tiles_orders_company_layouts_and_draws():
    n, d, m, k, nd = 1400, 5, 40, 2, 5
    model = model_with_priors("VD", m, d, k, True, seed=81)
    X32 = knock_out(catalogue(model, n, seed=82), seed=83).astype(np.float32)
    X = X32.astype(np.float64)
    Xd = dev(X)
    groups, weights = setting(n, 3, seed=5)
    gd, wd = dev(groups, torch.int64), dev(weights)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    Z17 = np.random.default_rng(2).standard_normal((m, 17, k))
    kw = dict(n_groups=3, groups=gd, weights=wd)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        edges = np.linspace(*np.percentile(host(p.predict_dev(Xd, missing=True)[0]), [3, 97]), 51)
        G5 = p.draws_dev(Xd, nd, Z=Z17[:, :nd], missing=True, return_gamma=True)[1]
        S5 = p.stack_missing_dev(Xd, edges, n_draws=nd, Z=Z17[:, :nd], **kw)

        def gam(x, ndr=nd, q=p):
            return q.draws_dev(x, ndr, Z=Z17[:, :ndr], missing=True, return_gamma=True)[1]

        def stack(x, ndr=nd, q=p, **over):
            return q.stack_missing_dev(x, edges, n_draws=ndr, Z=Z17[:, :ndr], **{**kw, **over})

        same_stack(stack(Xd), S5, "the same call twice")
        assert torch.equal(gam(Xd), G5)
        # n_draws = s + 1 against a larger n_draws, with Z given: draw s is the same weight draw, in another column of W
        assert torch.equal(gam(Xd, 17)[:nd], G5), "the first 5 of 17 draws"
        S17 = stack(Xd, 17)
        same_stack([S17.hist[:1 + nd], S17.sum_w, S17.sum_mu[:1 + nd], S17.sum_mu2[:1 + nd]], S5[:4], "the first 5 of 17 draws")
        # a permutation of the rows
        assert torch.equal(gam(Xd[perm]), G5[:, perm]), "a row permutation"
        # a row alone, a row among its group, a row among other groups and complete rows
        codes = np.isnan(X) @ (1 << np.arange(d))
        for code in np.unique(codes):
            rows = np.flatnonzero(codes == code)
            r = int(rows[len(rows) // 2])
            assert torch.equal(gam(Xd[r:r + 1]), G5[:, r:r + 1]), ("alone", code)
            assert torch.equal(gam(Xd[torch.from_numpy(rows).to(DEV)]), G5[:, rows]), ("its group", code)
        # float32 / transposed / strided X
        X2 = dev(np.repeat(X, 2, axis=0))
        for x, what in ((dev(X32, torch.float32), "float32"), (Xd.T.contiguous().T, "transposed"), (X2[::2], "row-sliced"),
                        (dev(X32, torch.float32).T.contiguous().T, "float32 transposed")):
            assert torch.equal(gam(x), G5), what
            same_stack(stack(x), S5, what)
        # the catalogue is the sum of its patterns in ascending code order; complete rows alone are stack_dev
        total = None
        for code in np.unique(codes):
            idx = torch.from_numpy(np.flatnonzero(codes == code)).to(DEV)
            one = (p.stack_dev if code == 0 else p.stack_missing_dev)(Xd[idx], edges, n_draws=nd, Z=Z17[:, :nd], n_groups=3,
                                                                      groups=gd[idx], weights=wd[idx])
            total = list(one[:4]) if total is None else [t + a for t, a in zip(total, one[:4])]
        same_stack(total, S5[:4], "the sum of the patterns")
        full = torch.from_numpy(codes == 0).to(DEV)
        same_stack(stack(Xd[full], groups=gd[full], weights=wd[full]),
                   p.stack_dev(Xd[full], edges, n_draws=nd, Z=Z17[:, :nd], n_groups=3, groups=gd[full], weights=wd[full]), "complete rows")
        sel = torch.zeros(n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        same_stack(stack(Xd, selection=sel), stack(Xd[::2].contiguous(), groups=gd[::2], weights=wd[::2]), "selection")
        ref = stack_inputs(p, model, Xd, edges, nd, dict(Z=Z17[:, :nd]), groups, weights, 3)
    # tile sizes: gamma_s to the bit, the stack within its tolerances (its sums run in the order of the tiles)
    for T in (1024, None):
        with gpz_amd.Predictor(model, tile_rows=T) as q:
            assert torch.equal(gam(Xd, q=q), G5), T
            assert_close(stack(Xd, q=q), *ref[:4], f"tile_rows={T}")
            assert_close(stack(Xd[perm], q=q, groups=gd[perm], weights=wd[perm]), *ref[:4], f"tile_rows={T}, permuted")


@pytest.mark.parametrize("k", [1, 2])
def test_every_row_count_of_a_group(k):
    """A single-pattern group of n rows at the edges of the 32-row blocks, the 256-row tiles and 1024 rows: gamma_s of every shorter call
    and its draws are the first rows of the longest call bit for bit, and the stack of every count holds all its rows."""
    d, m, nd = 5, 17, 3
    model = model_with_priors("VD", m, d, k, True, seed=950 + k)
    X = catalogue(model, 1025, seed=93)
    X[:, 2] = NAN
    Xd = dev(X)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        Ff, Gf = p.draws_dev(Xd, nd, seed=3, missing=True, return_gamma=True)
        edges = np.linspace(*np.percentile(host(Ff), [3, 97]), 31)
        for n in (1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025):
            Fn, Gn = p.draws_dev(Xd[:n], nd, seed=3, missing=True, return_gamma=True)
            assert Gn.shape == (nd, n, k) and torch.equal(Gn, Gf[:, :n]) and torch.equal(Fn, Ff[:, :n]), n
            res = p.stack_missing_dev(Xd[:n], edges, n_draws=nd, seed=3)
            assert res.sum_w[0] == n and np.all(np.isfinite(res.hist)), n


# ---- 4. stack parity --------------------------------------------------------------------------------------------------------------------
def stack_inputs(p, model, Xd, edges, n_draws, draw_kw, groups, weights, G):
    """stack_reference_w fed with the device's own per-row numbers, and test_predictor_stack.py's tolerances with s_min over the new widths."""
    mu, sigma, _, beta = (host(t) for t in p.predict_dev(Xd, missing=True)[:4])
    F = S2 = None
    if n_draws:
        Ft, Gt = p.draws_dev(Xd, n_draws, missing=True, return_gamma=True, **draw_kw)
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
    """2500 rows on 1024-row tiles, dimension 1 missing on 20 % and dimension 4 on 10 % of the rows independently (four patterns), three
    groups with rows left out and random weights, 1, 37 and 300 bins, no draws and 5 seeded draws; column 0's sum_mu / sum_w against
    predict_dev's weighted mean."""
    d, ns, G, m = 5, 2500, 3, 40
    model = model_with_priors(method, m, d, k, hetero, seed=4100 + 100 * DIAG.index(method) + 10 * k + hetero)
    X = knock_out(catalogue(model, ns, seed=k + 40), seed=k + 41)
    Xd = dev(X)
    groups, weights = setting(ns, G, seed=m)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        mu0 = host(p.predict_dev(Xd, missing=True)[0])
        for B in (1, 37, 300):
            edges = np.linspace(*np.percentile(mu0, [3, 97]), B + 1)
            for nd in (0, 5):
                ref, th, tm, tw, mu = stack_inputs(p, model, Xd, edges, nd, dict(seed=77), groups, weights, G)
                rd = p.stack_missing_dev(Xd, edges, n_draws=nd, seed=77, groups=gd, n_groups=G, weights=wd)
                what = f"{method} hetero={hetero} k={k} B={B} draws={nd}"
                assert_close(rd, ref, th, tm, tw, what)
                for gi in range(G):
                    r = groups == gi
                    mean = (weights[r] @ mu[r]) / weights[r].sum()
                    tol = (tm[0, gi, :, 0] + 8 * EPS * np.abs(weights[r] @ mu[r])) / weights[r].sum() + 4 * EPS * np.abs(mean)
                    assert np.all(np.abs(rd.sum_mu[0, gi] / rd.sum_w[gi] - mean) <= tol), (what, gi)


# ---- 5. additivity ----------------------------------------------------------------------------------------------------------------------
def test_two_chunks_add_to_one_call():
    n, d, m, k, G, B = 3000, 5, 50, 2, 3, 80
    model = model_with_priors("GD", m, d, k, True, seed=3)
    X = knock_out(catalogue(model, n, seed=4), seed=6)
    Xd = dev(X)
    groups, weights = setting(n, G, seed=5)
    gd, wd = dev(groups, torch.int64), dev(weights)
    kw = dict(n_draws=4, seed=11, n_groups=G)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        edges = np.linspace(*np.percentile(host(p.predict_dev(Xd, missing=True)[0]), [3, 97]), B + 1)
        whole = p.stack_missing_dev(Xd, edges, groups=gd, weights=wd, **kw)
        parts = [p.stack_missing_dev(Xd[i:j], edges, groups=gd[i:j], weights=wd[i:j], **kw) for i, j in ((0, 1234), (1234, n))]
        ref, th, tm, tw, _ = stack_inputs(p, model, Xd, edges, 4, dict(seed=11), groups, weights, G)
    total = gpz_amd.api.StackResult(*(parts[0][f] + parts[1][f] for f in range(4)), edges)
    assert_close(total, ref, th, tm, tw, "two chunks")
    assert_close(whole, ref, th, tm, tw, "one call")


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
ERR_ARG, ERR_UNSUPPORTED = -1, -5                                        # include/gpz_hip.h


def raw_calls(p, x, obs, nd, G, B, edges, lab=None, wt=None, draws=True):
    """Both C entries on one group with every output preset to -7: (rc of the stack, its message, rc of the draws, its message, outputs)."""
    k, n = p._k, x.shape[0]
    muX, sdX, muY = p._norm_vectors()
    stream = torch.cuda.current_stream(x.device).cuda_stream
    es = np.ascontiguousarray(edges[None, :] - muY[:, None])
    out = [np.full(s, -7.0) for s in ((1 + nd, G, k, B), (G,), (1 + nd, G, k), (1 + nd, G, k))]
    h = p._handle()
    rc1 = p._lib.gpz_predictor_stack_missing_dev(h, *p._x_args(x), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(p._priors), obs, nd, 5, None,
                                                 _lib.dptr(es), B, None if lab is None else lab.data_ptr(), G,
                                                 None if wt is None else wt.data_ptr(), *(_lib.dptr(a) for a in out), _lib.dptr(muY), stream)
    msg1 = p._lib.gpz_last_error().decode() if rc1 else ""
    if not draws:
        return rc1, msg1, 0, "", out, []
    Fd = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    Gm = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    rc2 = p._lib.gpz_predictor_draws_gamma_missing_dev(h, *p._x_args(x), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                       _lib.dptr(p._priors), obs, nd, 5, None, Fd.data_ptr(), Gm.data_ptr(), stream)
    msg2 = p._lib.gpz_last_error().decode() if rc2 else ""
    torch.cuda.synchronize()
    return rc1, msg1, rc2, msg2, out, [Fd, Gm]


def test_bad_groups_labels_and_weights_are_refused_with_the_outputs_untouched():
    n, d, k, nd, G, B = 3000, 5, 2, 3, 2, 10
    model = model_with_priors("VD", 20, d, k, True, seed=88)
    Xh = catalogue(model, n, seed=89)
    Xh[:, 3] = NAN
    X = dev(Xh)
    mask = 0b10111
    edges = np.linspace(-3.0, 3.0, B + 1)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        good = p.stack_missing_dev(X, edges, n_draws=nd, seed=5, n_groups=G)
        rc1, _, rc2, _, out, dr = raw_calls(p, X, mask, nd, G, B, edges)
        assert rc1 == 0 and rc2 == 0 and all(np.all(a != -7.0) for a in out) and all(bool((t != -7.0).all()) for t in dr)
        same_stack(out, good[:4], "the C entry is the method")
        two = X.clone()
        two[2000:, 0] = NAN                                               # two patterns in one group
        nan_obs = X.clone()
        nan_obs[2999, 4] = NAN                                            # a NaN in an observed dimension
        num_miss = X.clone()
        num_miss[1234, 3] = 0.5                                           # a number in a missing one
        for what, x, obs, text in (("two patterns", two, mask, "share one NaN pattern"), ("NaN in o", nan_obs, mask, "share one NaN pattern"),
                                   ("number in u", num_miss, mask, "share one NaN pattern"),
                                   ("full mask", X, 0b11111, "no dimension is missing"), ("mask past d", X, 0b110111, "above d")):
            rc1, msg1, rc2, msg2, out, dr = raw_calls(p, x, obs, nd, G, B, edges)
            assert rc1 == ERR_ARG and rc2 == ERR_ARG, (what, rc1, rc2)
            assert text in msg1 and text in msg2, (what, msg1, msg2)
            assert all(np.all(a == -7.0) for a in out) and all(bool((t == -7.0).all()) for t in dr), what
        # labels and weights (the stack entry alone takes them)
        lab = torch.zeros(n, dtype=torch.int32, device=DEV)
        lab[5] = G
        wt = torch.ones(n, dtype=torch.float64, device=DEV)
        wt[11] = -1.0
        winf = torch.ones(n, dtype=torch.float64, device=DEV)
        winf[n - 1] = float("inf")
        for what, l, w, text in (("bad label", lab, None, "label"), ("negative weight", None, wt, "weight"), ("infinite weight", None, winf, "weight")):
            rc1, msg1, _, _, out, _ = raw_calls(p, X, mask, nd, G, B, edges, lab=l, wt=w, draws=False)
            assert rc1 == ERR_ARG and text in msg1, (what, rc1, msg1)
            assert all(np.all(a == -7.0) for a in out), what
        with pytest.raises(_lib.GpzError, match="label"):
            p.stack_missing_dev(X, edges, groups=lab.long(), n_groups=G)
        with pytest.raises(_lib.GpzError, match="weight"):
            p.stack_missing_dev(X, edges, weights=wt)
        # columns over GPZ_DRAWS_MAX_COLUMNS: (1 + ndraws) k for the stack, ndraws k for the draws
        over = gpz_amd.api.GPZ_DRAWS_MAX_COLUMNS // k
        rc1, msg1, _, _, out, _ = raw_calls(p, X[:8], mask, over, 1, 1, np.array([-1.0, 1.0]), draws=False)
        assert rc1 == ERR_ARG and str(gpz_amd.api.GPZ_DRAWS_MAX_COLUMNS) in msg1, msg1
        assert all(np.all(a == -7.0) for a in out)
        muX, sdX, muY = p._norm_vectors()
        Gm = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
        rc2 = p._lib.gpz_predictor_draws_gamma_missing_dev(p._handle(), *p._x_args(X[:8]), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                           _lib.dptr(p._priors), mask, over + 1, 5, None, Gm.data_ptr(), Gm.data_ptr(),
                                                           torch.cuda.current_stream().cuda_stream)
        assert rc2 == ERR_ARG and float(Gm[0]) == -7.0
        with pytest.raises(ValueError, match="over the limit"):
            p.stack_missing_dev(X, edges, n_draws=over)
        with pytest.raises(ValueError, match="over the limit"):
            p.draws_dev(X, over + 1, missing=True, return_gamma=True)
        same_stack(p.stack_missing_dev(X, edges, n_draws=nd, seed=5, n_groups=G), good, "the handle works on the next call")
        assert p.predict(Xh[:50])[4].min() > 0.0                          # predict() keeps accepting these rows


@pytest.mark.parametrize("kw", [{"m": 300}, {"d": 24}, {"k": 9}, {"method": "VC"}])
def test_shapes_outside_the_route_are_refused(kw):
    a = {"method": "VD", "m": 20, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    Xh = catalogue(model, 40, seed=6)
    Xh[:, 1] = NAN
    X = dev(Xh)
    edges = np.linspace(-3.0, 3.0, 11)
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match="predict_missing_fits"):
            p.stack_missing_dev(X, edges)
        with pytest.raises(ValueError, match="predict_missing_fits"):
            p.draws_dev(X, 2, missing=True, return_gamma=True)
        rc1, msg1, rc2, msg2, out, dr = raw_calls(p, X, (1 << a["d"]) - 3, 2, 1, 10, edges)
        assert rc1 == ERR_UNSUPPORTED and rc2 == ERR_UNSUPPORTED, (rc1, rc2)
        assert "predict_missing_fits" in msg1 and "predict_missing_fits" in msg2
        assert all(np.all(t == -7.0) for t in out) and all(bool((t == -7.0).all()) for t in dr)
        assert "missing" not in p.route
        assert np.all(np.isfinite(p.predict(Xh)[0]))                      # predict() keeps accepting these rows


# ---- 7. memory and route ----------------------------------------------------------------------------------------------------------------
def test_memory_and_route():
    d, nd, G, B, T = 5, 6, 4, 50, 4096
    model = model_with_priors("VD", 100, d, 2, True, seed=8)
    n = 30_000
    gen = torch.Generator(device=DEV).manual_seed(98)
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=gen) * torch.from_numpy(model.sdX).to(DEV) + \
        torch.from_numpy(model.muX).to(DEV)
    two = X.clone()
    two[torch.rand(n, device=DEV, generator=gen) < 0.2, 1] = NAN
    eight = X.clone()
    for c in (0, 2, 4):
        eight[torch.rand(n, device=DEV, generator=gen) < 0.3, c] = NAN
    edges = np.linspace(-2.0, 2.0, B + 1) + float(np.asarray(model.muY).reshape(-1)[0])

    def old_entries(h):
        h.predict_dev(two[:1000], missing=True)
        h.draws_dev(two[:1000], nd, seed=3, missing=True)
        h.stack_dev(X[:1000], edges, n_draws=nd, seed=3, n_groups=G)

    with gpz_amd.Predictor(model, tile_rows=T) as p, gpz_amd.Predictor(model, tile_rows=T) as q:
        old_entries(p)
        old_entries(q)
        held, text = q.info[1], q.route
        assert p.info[1] == held and p.route == text
        assert "per draw" not in text and text.endswith(f"; missing: k_predict_missing_pairs ({chunks_rule(100)} pair chunks), {T}-row tiles")
        p.stack_missing_dev(two[:3000], edges, n_draws=nd, seed=3, n_groups=G)
        p.draws_dev(two[:3000], nd, seed=3, missing=True, return_gamma=True)
        first = p.info[1]
        assert first > held                                               # the first new call adds once
        assert p.route.startswith(text) and p.route[len(text):] == \
            f"; missing per draw: k_predict_missing_gamma ({chunks_rule(100)} pair chunks) + k_stack_tile_w", p.route
        p.stack_missing_dev(two, edges, n_draws=nd, seed=3, n_groups=G)   # ten times the rows
        p.draws_dev(two, nd, seed=3, missing=True, return_gamma=True)
        assert p.info[1] == first
        assert len(p._nan_groups_dev(eight)) == 8
        p.stack_missing_dev(eight, edges, n_draws=nd, seed=3, n_groups=G)  # more patterns
        p.draws_dev(eight[:5000], nd, seed=3, missing=True, return_gamma=True)
        assert p.info[1] == first
        old_entries(q)
        q.predict_dev(eight, missing=True)
        assert q.info[1] == held and q.route == text                      # a handle that calls only the old entries holds what it held
