"""Stacks of rows with input noise and missing inputs and gamma under every weight draw (Predictor.stack_noisy_missing_dev,
draws_noisy_missing_dev(..., return_gamma=True); k_predict_noisy_missing_gamma.hip) against the existing entries of the handle,
``gpz_amd.predict`` and the oracle: gamma_s against predict_noisy_missing_dev of the model whose weights are the draw's, the stack against
``stack_reference_w`` fed with the device's own per-row numbers, the same bits over tiles, orders, company, layouts and numbers of draws,
Psi in the missing dimensions, Psi = 0, additivity, the refusals and constant memory.

Stack tolerance: the derived one of tests/test_predictor_stack.py, unchanged, with s_min taken over the new widths.

Bits: gamma_s is held to the same bits over everything listed.  The stack's fields are sums over rows in the order of DESIGN.md section
14: as for ``stack_dev``, another tile size or row order may change their last bits, so the stack is held to the same bits where its
order of summation is the same (the same call twice, every layout, the columns of a call with fewer draws, a catalogue against the sum of
its patterns, a catalogue without NaN against ``stack_noisy_dev``) and to ``assert_close`` over tile sizes and a permutation."""
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
from test_predictor_stack_missing import four_patterns
from test_predictor_stack_noisy import noise, with_weights
from test_predictor_stack_noisy_cpu import stack_reference_w

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIAG = ("GL", "VL", "GD", "VD")
NAN = float("nan")
ERR_ARG, ERR_UNSUPPORTED = -1, -5                                        # include/gpz_hip.h


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def gamma_of(model, X, Psi, tile_rows=256):
    """predict_noisy_missing_dev(X, Psi)'s gamma on a handle of its own: existing code."""
    with gpz_amd.Predictor(model, tile_rows=tile_rows) as q:
        return host(q.predict_noisy_missing_dev(dev(X), dev(Psi))[4])


def suffix(m, stack=False):
    return f"; noisy missing per draw: k_predict_noisy_missing_gamma ({chunks_rule(m)} pair chunks)" + (" + k_stack_tile_w" if stack else "")


# ---- 1. gamma_s with exact weights --------------------------------------------------------------------------------------------------------
# every m with two of the shapes (d, k, n_draws); every shape at four or five values of m
A, B_, C, D, E, F_ = (1, 1, 17), (5, 1, 64), (5, 3, 1), (5, 8, 5), (20, 1, 5), (20, 8, 17)
CASES = [(1, A), (1, D), (2, C), (2, E), (11, E), (11, F_), (17, A), (17, C), (62, B_), (62, D), (63, E), (63, F_), (80, A), (80, B_),
         (100, B_), (100, D), (105, E), (105, A), (115, F_), (115, C), (120, B_), (120, E), (128, D), (128, F_), (256, B_), (256, F_)]


@pytest.mark.parametrize("m,shape", CASES)
def test_gamma_per_draw_with_exact_weights(m, shape):
    """iSigma_w = 2^-10 I: the Cholesky factor is exactly 2^-5 I, so w_s = w + 2^-5 z_s is the same double on host and device.  The
    reference is predict_noisy_missing_dev(X, Psi)'s gamma of the model with w := w_s (the same quantity by definition, the parent's
    code), at the project's own gate nrel <= 1e-11 per draw over ALL rows: the complete rows go through k_predict_noisy_gamma and are
    not zero.  600 rows on 256-row tiles.  m = 1 .. 256 walks the chunk counts 1 .. 8 and the edges of the 16-wide K blocks and 64-pair
    groups; the columns are 17, 64, 3, 40, 5 and 136: partial 16-column blocks, and 136 is a second launch of one block behind eight.
    Where m <= 50, the first 100 rows (all four patterns) of every draw against the oracle at rel <= 1e-8."""
    d, k, nd = shape
    ns = 600
    model = model_with_priors("VD" if (m + d) % 2 else "GL", m, d, k, bool(k % 2), seed=9300 + 100 * d + 10 * k + m)
    model.sets["best"]["iSigma_w"] = np.stack([2.0 ** -10 * np.eye(m)] * k, axis=2)
    X = four_patterns(catalogue(model, ns, seed=m + d))
    Psi = noise(ns, d, seed=m + d + 1)
    full = ~np.isnan(X).any(axis=1)
    Z = np.random.default_rng(nd + m).standard_normal((m, nd, k))
    W = model.sets["best"]["w"][:, None, :] + 2.0 ** -5 * Z             # (m, nd, k)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        Fd, Gam = p.draws_noisy_missing_dev(dev(X), dev(Psi), nd, Z=Z, return_gamma=True)
        assert p.route.endswith(suffix(m)), p.route
        assert "k_stack_tile" not in p.route                             # no stack call on this handle
        assert torch.equal(Fd, p.draws_noisy_missing_dev(dev(X), dev(Psi), nd, Z=Z))
    assert Gam.shape == (nd, ns, k) and Gam.dtype == torch.float64
    Gam = host(Gam)
    assert full.any() and np.all(Gam[:, full] != 0.0)
    worst = 0.0
    for s in range(nd):
        ms = with_weights(model, W[:, s, :])
        got = nrel(Gam[s], gamma_of(ms, X, Psi))
        worst = max(worst, got)
        assert got <= 1e-11, (s, got)
        if m <= 50:
            orc = O.predict_any(X[:100], ms, Psi=Psi[:100])[4]
            assert rel(Gam[s, :100], orc) <= 1e-8, (s, rel(Gam[s, :100], orc))
    print(f"m={m} d={d} k={k} nd={nd}: worst nrel of gamma_s against predict_noisy_missing_dev of the w_s model {worst:.3g}")


# ---- 2. gamma_s with a general iSigma_w ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["VD", "GL"])
def test_gamma_per_draw_with_seeded_draws(method):
    """Seeded draws of a general iSigma_w; w_s formed on the host as w + chol(sym(iSigma_w)) z_s with the Philox normals of the seed.
    Yardstick: the disagreement of two routes of the parent, gamma of the w := w_s model from the handle's predict_noisy_missing_dev
    against gpz_amd.predict(X, ms, Psi=Psi).  Gate: max(1e-11, 10 x that spread) - the factor 10 for a third summation order and the
    host-formed w_s, as in test_predictor_stack_missing.py.  The measured figures are in DESIGN.md section 23."""
    m, d, k, nd, ns, seed = 60, 5, 2, 6, 600, 31
    model = model_with_priors(method, m, d, k, True, seed=177)
    X = knock_out(catalogue(model, ns, seed=78), seed=79)
    Psi = noise(ns, d, seed=80)
    z = philox_normals(seed, m, nd, k)
    iS = model.sets["best"]["iSigma_w"]
    L = [np.linalg.cholesky(0.5 * (iS[:, :, o] + iS[:, :, o].T)) for o in range(k)]
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        _, Gam = p.draws_noisy_missing_dev(dev(X), dev(Psi), nd, seed=seed, return_gamma=True)
    Gam = host(Gam)
    for s in range(nd):
        ws = np.stack([model.sets["best"]["w"][:, o] + L[o] @ z[:, s, o] for o in range(k)], axis=1)
        ms = with_weights(model, ws)
        a = gamma_of(ms, X, Psi)
        b = gpz_amd.predict(X, ms, Psi=Psi)[4]
        spread = nrel(a, b)
        got = nrel(Gam[s], a)
        print(f"{method} draw {s}: nrel(gamma_s, predict_noisy_missing_dev of w_s) {got:.3g}; spread of the parent's two routes {spread:.3g}")
        assert got <= max(1e-11, 10 * spread), (s, got, spread)


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------------------
def same_stack(a, b, what):
    for f, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), (what, f)


def stack_inputs(p, model, Xd, Pd, edges, n_draws, draw_kw, groups, weights, G):
    """stack_reference_w fed with the device's own per-row numbers, and test_predictor_stack.py's tolerances with s_min over the new widths."""
    mu, sigma, _, beta = (host(t) for t in p.predict_noisy_missing_dev(Xd, Pd)[:4])
    F = S2 = None
    if n_draws:
        Ft, Gt = p.draws_noisy_missing_dev(Xd, Pd, n_draws, return_gamma=True, **draw_kw)
        F, S2 = host(Ft), beta[None] + np.maximum(host(Gt), 0.0)
    ref = stack_reference_w(mu, sigma, F, S2, edges, groups, weights, n_groups=G)
    n, k = mu.shape
    g, w = np.asarray(groups), np.asarray(weights, dtype=np.float64)
    cols = [mu] + ([] if F is None else list(F))
    muY = np.asarray(model.muY).reshape(-1)
    E_ = max(np.max(np.abs(np.asarray(edges)[None, :] - muY[:, None])), 0.0) + max(np.max(np.abs(c - muY)) for c in cols)
    s_min = np.sqrt(min(sigma.min(), S2.min() if S2 is not None else sigma.min()))
    W = np.array([w[g == gi].sum() for gi in range(G)])
    ng = np.array([(g == gi).sum() for gi in range(G)])
    tol_h = EPS * W * (ng + 64.0 * (1.0 + E_ / s_min))
    tol_m = np.empty((len(cols), G, k, 2))
    for c, m_ in enumerate(cols):
        for gi in range(G):
            r = g == gi
            tol_m[c, gi, :, 0] = ng[gi] * EPS * (w[r] @ np.abs(m_[r]))
            tol_m[c, gi, :, 1] = ng[gi] * EPS * (w[r] @ (m_[r] * m_[r]))
    return ref, tol_h, tol_m, ng * EPS * W, mu


def test_same_bits_over_tiles_orders_company_layouts_and_draws():
    n, d, m, k, nd = 1400, 5, 40, 2, 5
    model = model_with_priors("VD", m, d, k, True, seed=281)
    X32 = knock_out(catalogue(model, n, seed=82), seed=83).astype(np.float32)
    P32 = noise(n, d, seed=84).astype(np.float32)
    X, Psi = X32.astype(np.float64), P32.astype(np.float64)
    Xd, Pd = dev(X), dev(Psi)
    groups, weights = setting(n, 3, seed=5)
    gd, wd = dev(groups, torch.int64), dev(weights)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    Z17 = np.random.default_rng(2).standard_normal((m, 17, k))
    kw = dict(n_groups=3, groups=gd, weights=wd)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        edges = np.linspace(*np.percentile(host(p.predict_noisy_missing_dev(Xd, Pd)[0]), [3, 97]), 51)

        def gam(x, psi, ndr=nd, q=p):
            return q.draws_noisy_missing_dev(x, psi, ndr, Z=Z17[:, :ndr], return_gamma=True)[1]

        def stack(x, psi, ndr=nd, q=p, **over):
            return q.stack_noisy_missing_dev(x, psi, edges, n_draws=ndr, Z=Z17[:, :ndr], **{**kw, **over})

        G5, S5 = gam(Xd, Pd), stack(Xd, Pd)
        same_stack(stack(Xd, Pd), S5, "the same call twice")
        assert torch.equal(gam(Xd, Pd), G5)
        # n_draws = 5 against 17, with Z given: draw s is the same weight draw, in another column of W
        assert torch.equal(gam(Xd, Pd, 17)[:nd], G5), "the first 5 of 17 draws"
        S17 = stack(Xd, Pd, 17)
        same_stack([S17.hist[:1 + nd], S17.sum_w, S17.sum_mu[:1 + nd], S17.sum_mu2[:1 + nd]], S5[:4], "the first 5 of 17 draws")
        # a permutation of the rows
        assert torch.equal(gam(Xd[perm], Pd[perm]), G5[:, perm]), "a row permutation"
        # a row alone, a row among its group, a row among other groups and complete rows
        codes = np.isnan(X) @ (1 << np.arange(d))
        for code in np.unique(codes):
            rows = np.flatnonzero(codes == code)
            r = int(rows[len(rows) // 2])
            assert torch.equal(gam(Xd[r:r + 1], Pd[r:r + 1]), G5[:, r:r + 1]), ("alone", code)
            idx = torch.from_numpy(rows).to(DEV)
            assert torch.equal(gam(Xd[idx], Pd[idx]), G5[:, rows]), ("its group", code)
        # float32 / transposed / strided X and Psi
        X2, P2 = dev(np.repeat(X, 2, axis=0)), dev(np.repeat(Psi, 2, axis=0))
        for x, psi, what in ((dev(X32, torch.float32), dev(P32, torch.float32), "float32"), (Xd, dev(P32, torch.float32), "float32 Psi"),
                             (Xd.T.contiguous().T, Pd.T.contiguous().T, "transposed"), (Xd.T.contiguous().T, Pd, "mixed layouts"),
                             (X2[::2], P2[::2], "row-sliced")):
            assert torch.equal(gam(x, psi), G5), what
            same_stack(stack(x, psi), S5, what)
        # Psi as (n, d), (n, 1) and (n,) where equal
        col = Pd[:, 2].contiguous()
        Gc, Sc = gam(Xd, col[:, None].expand(n, d).contiguous()), stack(Xd, col[:, None].expand(n, d).contiguous())
        for psi, what in ((col[:, None], "Psi (n, 1)"), (col, "Psi (n,)"), (Pd[:, 2], "Psi (n,) strided")):
            assert torch.equal(gam(Xd, psi), Gc), what
            same_stack(stack(Xd, psi), Sc, what)
        # the catalogue is the sum of its patterns in ascending code order; complete rows alone are stack_noisy_dev
        total = None
        for code in np.unique(codes):
            idx = torch.from_numpy(np.flatnonzero(codes == code)).to(DEV)
            one = (p.stack_noisy_dev if code == 0 else p.stack_noisy_missing_dev)(Xd[idx], Pd[idx], edges, n_draws=nd, Z=Z17[:, :nd],
                                                                                  n_groups=3, groups=gd[idx], weights=wd[idx])
            total = list(one[:4]) if total is None else [t + a for t, a in zip(total, one[:4])]
        same_stack(total, S5[:4], "the sum of the patterns")
        full = torch.from_numpy(codes == 0).to(DEV)
        same_stack(stack(Xd[full], Pd[full], groups=gd[full], weights=wd[full]),
                   p.stack_noisy_dev(Xd[full], Pd[full], edges, n_draws=nd, Z=Z17[:, :nd], n_groups=3, groups=gd[full], weights=wd[full]),
                   "a catalogue without NaN")
        assert torch.equal(gam(Xd[full], Pd[full]),
                           p.draws_dev(Xd[full], nd, Z=Z17[:, :nd], Psi=Pd[full], return_gamma=True)[1]), "complete rows"
        sel = torch.zeros(n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        same_stack(stack(Xd, Pd, selection=sel), stack(Xd[::2].contiguous(), Pd[::2].contiguous(), groups=gd[::2], weights=wd[::2]),
                   "selection")
        ref = stack_inputs(p, model, Xd, Pd, edges, nd, dict(Z=Z17[:, :nd]), groups, weights, 3)
    # tile sizes: gamma_s to the bit, the stack within its tolerances (its sums run in the order of the tiles)
    for T in (128, 1024):
        with gpz_amd.Predictor(model, tile_rows=T) as q:
            assert torch.equal(gam(Xd, Pd, q=q), G5), T
            assert_close(stack(Xd, Pd, q=q), *ref[:4], f"tile_rows={T}")
            assert_close(stack(Xd[perm], Pd[perm], q=q, groups=gd[perm], weights=wd[perm]), *ref[:4], f"tile_rows={T}, permuted")


# ---- 4. every row count of one group -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_every_row_count_of_a_group(k):
    """Every n = 1 .. 70 rows of a single-pattern group (the edges of the 32-row blocks on both sides): gamma_s, the draws and nothing
    else of the call are the same rows cut out of a 600-row call, bit for bit."""
    d, m, nd = 3, 20, 3
    model = model_with_priors("VD", m, d, k, True, seed=2950 + k)
    X = catalogue(model, 600, seed=93)
    X[:, 1] = NAN
    Xd, Pd = dev(X), dev(noise(600, d, seed=94))
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        Ff, Gf = p.draws_noisy_missing_dev(Xd, Pd, nd, seed=3, return_gamma=True)
        for n in range(1, 71):
            at = 7 * n % 500                                             # any place in the long call
            Fn, Gn = p.draws_noisy_missing_dev(Xd[at:at + n], Pd[at:at + n], nd, seed=3, return_gamma=True)
            assert Gn.shape == (nd, n, k) and torch.equal(Gn, Gf[:, at:at + n]) and torch.equal(Fn, Ff[:, at:at + n]), n


# ---- 5. Psi in the missing dimensions ------------------------------------------------------------------------------------------------------
def raw_calls(p, x, psi, obs, nd, G, B, edges, lab=None, wt=None, draws=True):
    """Both C entries on one group with every output preset to -7: (rc of the stack, its message, rc of the draws, its message, the
    stack's outputs, [F, Gam])."""
    k, n = p._k, x.shape[0]
    muX, sdX, muY = p._norm_vectors()
    sd2 = np.ascontiguousarray(sdX ** 2)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    es = np.ascontiguousarray(edges[None, :] - muY[:, None])
    out = [np.full(s, -7.0) for s in ((1 + nd, G, k, B), (G,), (1 + nd, G, k), (1 + nd, G, k))]
    lead = [p._handle(), *p._x_args(x), *p._psi_args(psi, n), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(sd2)]
    rc1 = p._lib.gpz_predictor_stack_noisy_missing_dev(*lead, _lib.dptr(p._priors), obs, nd, 5, None, _lib.dptr(es), B,
                                                       None if lab is None else lab.data_ptr(), G, None if wt is None else wt.data_ptr(),
                                                       *(_lib.dptr(a) for a in out), _lib.dptr(muY), stream)
    msg1 = p._lib.gpz_last_error().decode() if rc1 else ""
    if not draws:
        return rc1, msg1, 0, "", out, []
    Fd = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    Gm = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    rc2 = p._lib.gpz_predictor_draws_gamma_noisy_missing_dev(*lead, _lib.dptr(muY), _lib.dptr(p._priors), obs, nd, 5, None, Fd.data_ptr(),
                                                             Gm.data_ptr(), stream)
    msg2 = p._lib.gpz_last_error().decode() if rc2 else ""
    torch.cuda.synchronize()
    return rc1, msg1, rc2, msg2, out, [Fd, Gm]


def untouched(out, dr):
    return all(np.all(a == -7.0) for a in out) and all(bool((t == -7.0).all()) for t in dr)


def test_psi_in_missing_dimensions_is_not_read():
    """NaN, inf and -1 in Psi where X is NaN change no bit of gamma_s or of the stack; the same values in an observed dimension are
    refused by both C entries with the outputs untouched."""
    n, d, k, nd, m, G, B = 600, 5, 2, 3, 30, 2, 20
    model = model_with_priors("VD", m, d, k, True, seed=388)
    X = knock_out(catalogue(model, n, seed=89), seed=90)
    X[7, :] = NAN
    Psi = noise(n, d, seed=91)
    nan = np.isnan(X)
    Xd, Pd = dev(X), dev(Psi)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        edges = np.linspace(*np.percentile(host(p.predict_noisy_missing_dev(Xd, Pd)[0]), [3, 97]), B + 1)

        def both(psi):
            return p.draws_noisy_missing_dev(Xd, psi, nd, seed=5, return_gamma=True), p.stack_noisy_missing_dev(Xd, psi, edges, n_draws=nd, seed=5)

        P32 = dev(Psi.astype(np.float32), torch.float32)
        ref = {torch.float64: both(Pd), torch.float32: both(P32)}
        for v in (NAN, float("inf"), -1.0):
            bad = Psi.copy()
            bad[nan] = v
            for psi in (dev(bad), dev(bad.astype(np.float32), torch.float32)):
                (F, Gm), S = both(psi)
                (Fr, Gr), Sr = ref[psi.dtype]
                assert torch.equal(F, Fr) and torch.equal(Gm, Gr), v
                same_stack(S[:4], Sr[:4], v)
        # one group through the C entries: dimension 4 missing
        g = np.flatnonzero(~nan[:, 1] & nan[:, 4])
        Xg, Pg, ng = dev(X[g]), Psi[g].copy(), g.size
        (Fg, Gg), Sg = (p.draws_noisy_missing_dev(Xg, dev(Pg), nd, seed=5, return_gamma=True),
                        p.stack_noisy_missing_dev(Xg, dev(Pg), edges, n_draws=nd, seed=5, n_groups=G))
        rc1, _, rc2, _, out, dr = raw_calls(p, Xg, dev(Pg), 0b01111, nd, G, B, edges)
        assert rc1 == 0 and rc2 == 0
        same_stack(out, Sg[:4], "the C entry is the method")
        assert torch.equal(dr[0].permute(0, 2, 1), Fg) and torch.equal(dr[1].permute(0, 2, 1), Gg)
        held = p.info[1]
        for v, at, c in ((NAN, ng - 1, 3), (float("inf"), 0, 0), (-1.0, ng // 2, 2)):
            bad = Pg.copy()
            bad[at, c] = v
            rc1, msg1, rc2, msg2, out, dr = raw_calls(p, Xg, dev(bad), 0b01111, nd, G, B, edges)
            assert rc1 == ERR_ARG and rc2 == ERR_ARG, (v, rc1, rc2)
            assert "Psi has an element that is NaN, infinite or negative" in msg1 and "Psi has an element" in msg2, (msg1, msg2)
            assert untouched(out, dr), v                                   # refused before any tile kernel has run
            miss = Pg.copy()
            miss[at, 4] = v                                                # the same value where the group's X is NaN: taken
            rc1, _, rc2, _, out, dr = raw_calls(p, Xg, dev(miss), 0b01111, nd, G, B, edges)
            assert rc1 == 0 and rc2 == 0, v
            same_stack(out, Sg[:4], v)
            assert torch.equal(dr[1].permute(0, 2, 1), Gg), v
        assert p.info[1] == held
        with pytest.raises(_lib.GpzError, match="Psi"):                    # and through the methods: in the row's observed dimensions
            p.stack_noisy_missing_dev(Xd, dev(np.where(nan, Psi, -1.0)), edges)
        with pytest.raises(_lib.GpzError, match="Psi"):
            p.draws_noisy_missing_dev(Xd, dev(np.where(nan, Psi, -1.0)), nd, return_gamma=True)


# ---- 6. Psi = 0 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,k", [("VD", 1), ("GD", 3)])
def test_zero_noise_is_gamma_per_draw_for_missing_inputs(method, k):
    """Psi = 0 on the rows with missing values: gamma_s agrees with draws_dev(X, ..., missing=True, return_gamma=True) at nrel <= 1e-11
    per draw (another record table and rsqrt in place of a stored 1 / C: not the same bits)."""
    n, d, m, nd = 600, 5, 60, 5
    model = model_with_priors(method, m, d, k, True, seed=360 + k)
    X = knock_out(catalogue(model, n, seed=61), seed=62, cols=((1, 0.4), (4, 0.3)))
    X[3, :] = NAN
    miss = np.isnan(X).any(axis=1)
    Xd = dev(X)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        Fz, Gz = p.draws_noisy_missing_dev(Xd, torch.zeros((n, d), dtype=torch.float64, device=DEV), nd, seed=8, return_gamma=True)
        Fm, Gm = p.draws_dev(Xd, nd, seed=8, missing=True, return_gamma=True)
    assert miss.sum() > 100
    for s in range(nd):
        got = nrel(host(Gz[s])[miss], host(Gm[s])[miss])
        print(f"{method} k={k} draw {s}: nrel of gamma_s at Psi = 0 against the noise-free gamma_s {got:.3g}")
        assert got <= 1e-11, (s, got)
        assert nrel(host(Fz[s])[miss], host(Fm[s])[miss]) <= 1e-12


# ---- 7. stack parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", DIAG)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_stack_parity(method, hetero, k):
    """600 rows on 256-row tiles, dimension 1 missing on 20 % and dimension 4 on 10 % of the rows independently (four patterns), Psi
    everywhere, three groups with rows left out and random weights, 1, 37 and 300 bins, no draws and 5 seeded draws; column 0's
    sum_mu / sum_w against predict_noisy_missing_dev's weighted mean."""
    d, ns, G, m = 5, 600, 3, 40
    model = model_with_priors(method, m, d, k, hetero, seed=5100 + 100 * DIAG.index(method) + 10 * k + hetero)
    X = knock_out(catalogue(model, ns, seed=k + 40), seed=k + 41)
    Xd, Pd = dev(X), dev(noise(ns, d, seed=k + 42))
    groups, weights = setting(ns, G, seed=m)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        mu0 = host(p.predict_noisy_missing_dev(Xd, Pd)[0])
        for B in (1, 37, 300):
            edges = np.linspace(*np.percentile(mu0, [3, 97]), B + 1)
            for nd in (0, 5):
                ref, th, tm, tw, mu = stack_inputs(p, model, Xd, Pd, edges, nd, dict(seed=77), groups, weights, G)
                rd = p.stack_noisy_missing_dev(Xd, Pd, edges, n_draws=nd, seed=77, groups=gd, n_groups=G, weights=wd)
                what = f"{method} hetero={hetero} k={k} B={B} draws={nd}"
                assert_close(rd, ref, th, tm, tw, what)
                for gi in range(G):
                    r = groups == gi
                    mean = (weights[r] @ mu[r]) / weights[r].sum()
                    tol = (tm[0, gi, :, 0] + 8 * EPS * np.abs(weights[r] @ mu[r])) / weights[r].sum() + 4 * EPS * np.abs(mean)
                    assert np.all(np.abs(rd.sum_mu[0, gi] / rd.sum_w[gi] - mean) <= tol), (what, gi)
        assert p.route.endswith(suffix(m, stack=True)), p.route


def test_two_chunks_add_to_one_call():
    n, d, m, k, G, B = 600, 5, 50, 2, 3, 80
    model = model_with_priors("GD", m, d, k, True, seed=13)
    X = knock_out(catalogue(model, n, seed=4), seed=6)
    Xd, Pd = dev(X), dev(noise(n, d, seed=7))
    groups, weights = setting(n, G, seed=5)
    gd, wd = dev(groups, torch.int64), dev(weights)
    kw = dict(n_draws=4, seed=11, n_groups=G)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        edges = np.linspace(*np.percentile(host(p.predict_noisy_missing_dev(Xd, Pd)[0]), [3, 97]), B + 1)
        whole = p.stack_noisy_missing_dev(Xd, Pd, edges, groups=gd, weights=wd, **kw)
        parts = [p.stack_noisy_missing_dev(Xd[i:j], Pd[i:j], edges, groups=gd[i:j], weights=wd[i:j], **kw) for i, j in ((0, 234), (234, n))]
        ref, th, tm, tw, _ = stack_inputs(p, model, Xd, Pd, edges, 4, dict(seed=11), groups, weights, G)
    total = gpz_amd.api.StackResult(*(parts[0][f] + parts[1][f] for f in range(4)), edges)
    assert_close(total, ref, th, tm, tw, "two chunks")
    assert_close(whole, ref, th, tm, tw, "one call")


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def test_bad_groups_labels_and_weights_are_refused_with_the_outputs_untouched():
    n, d, k, nd, G, B = 600, 5, 2, 3, 2, 10
    model = model_with_priors("VD", 20, d, k, True, seed=488)
    Xh = catalogue(model, n, seed=89)
    Xh[:, 3] = NAN
    X, Psi = dev(Xh), dev(noise(n, d, seed=92))
    mask = 0b10111
    edges = np.linspace(-3.0, 3.0, B + 1)
    with gpz_amd.Predictor(model, tile_rows=256) as p, gpz_amd.Predictor(model, tile_rows=256) as q:
        good = p.stack_noisy_missing_dev(X, Psi, edges, n_draws=nd, seed=5, n_groups=G)
        rc1, _, rc2, _, out, dr = raw_calls(p, X, Psi, mask, nd, G, B, edges)
        assert rc1 == 0 and rc2 == 0 and all(np.all(a != -7.0) for a in out) and all(bool((t != -7.0).all()) for t in dr)
        same_stack(out, good[:4], "the C entry is the method")
        two = X.clone()
        two[400:, 0] = NAN                                                # two patterns in one group
        nan_obs = X.clone()
        nan_obs[n - 1, 4] = NAN                                           # a NaN in an observed dimension
        num_miss = X.clone()
        num_miss[234, 3] = 0.5                                            # a number in a missing one
        q.predict_noisy_missing_dev(X[:50], Psi[:50])                     # the parent's call: the device entries' own buffers exist
        before, route = q.info[1], q.route
        for what, x, obs, text in (("a row off the pattern", two, mask, "share one NaN pattern"),
                                   ("NaN in o", nan_obs, mask, "share one NaN pattern"), ("number in u", num_miss, mask, "share one NaN pattern"),
                                   ("full mask", X, 0b11111, "no dimension is missing"), ("mask past d", X, 0b110111, "above d")):
            for h in (p, q):                                              # q: a handle that has made no stack or gamma call gains no byte
                rc1, msg1, rc2, msg2, out, dr = raw_calls(h, x, Psi, obs, nd, G, B, edges)
                assert rc1 == ERR_ARG and rc2 == ERR_ARG, (what, rc1, rc2)
                assert text in msg1 and text in msg2, (what, msg1, msg2)
                assert untouched(out, dr), what
        # labels and weights (the stack entry alone takes them)
        lab = torch.zeros(n, dtype=torch.int32, device=DEV)
        lab[5] = G
        wt = torch.ones(n, dtype=torch.float64, device=DEV)
        wt[11] = -1.0
        winf = torch.ones(n, dtype=torch.float64, device=DEV)
        winf[n - 1] = float("inf")
        for what, l, w, text in (("bad label", lab, None, "label"), ("negative weight", None, wt, "weight"), ("infinite weight", None, winf, "weight")):
            for h in (p, q):
                rc1, msg1, _, _, out, _ = raw_calls(h, X, Psi, mask, nd, G, B, edges, lab=l, wt=w, draws=False)
                assert rc1 == ERR_ARG and text in msg1, (what, rc1, msg1)
                assert all(np.all(a == -7.0) for a in out), what
        assert q.info[1] == before and q.route == route and "per draw" not in route
        with pytest.raises(_lib.GpzError, match="label"):
            p.stack_noisy_missing_dev(X, Psi, edges, groups=lab.long(), n_groups=G)
        with pytest.raises(_lib.GpzError, match="weight"):
            p.stack_noisy_missing_dev(X, Psi, edges, weights=wt)
        same_stack(p.stack_noisy_missing_dev(X, Psi, edges, n_draws=nd, seed=5, n_groups=G), good, "the handle works on the next call")


@pytest.mark.parametrize("kw", [{"m": 300}, {"d": 24}, {"k": 9}, {"method": "VC"}])
def test_shapes_outside_the_route_are_refused(kw):
    a = {"method": "VD", "m": 20, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    Xh = catalogue(model, 40, seed=6)
    Xh[:, 1] = NAN
    X, Psi = dev(Xh), dev(noise(40, a["d"], seed=7))
    edges = np.linspace(-3.0, 3.0, 11)
    text = {"m": "m <= 256, not m = 300", "d": "d <= 20, not d = 24", "k": "k <= 8, not k = 9", "method": "a diagonal kind .* not VC"}[list(kw)[0]]
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match="stack_noisy_missing_dev needs a model inside predict_missing_fits.*" + text):
            p.stack_noisy_missing_dev(X, Psi, edges)
        with pytest.raises(ValueError, match="draws_noisy_missing_dev needs a model inside predict_missing_fits.*" + text):
            p.draws_noisy_missing_dev(X, Psi, 2, return_gamma=True)
        rc1, msg1, rc2, msg2, out, dr = raw_calls(p, X, Psi, (1 << a["d"]) - 3, 2, 1, 10, edges)
        assert rc1 == ERR_UNSUPPORTED and rc2 == ERR_UNSUPPORTED, (rc1, rc2)
        assert "predict_missing_fits" in msg1 and "predict_missing_fits" in msg2
        cond = {"m": "m 300", "d": "d 24", "k": "k 9", "method": "method VC"}[list(kw)[0]]
        assert cond in msg1 and cond in msg2, (msg1, msg2)               # the condition is named
        assert untouched(out, dr)
        assert "missing" not in p.route


# ---- 9. memory and route ----------------------------------------------------------------------------------------------------------------
def test_memory_and_route():
    d, nd, G, B, T = 5, 6, 4, 50, 1024
    model = model_with_priors("VD", 40, d, 2, True, seed=18)
    n = 12_000
    gen = torch.Generator(device=DEV).manual_seed(98)
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=gen) * torch.from_numpy(model.sdX).to(DEV) + \
        torch.from_numpy(model.muX).to(DEV)
    Psi = 0.05 * torch.rand((n, d), dtype=torch.float64, device=DEV, generator=gen)
    two = X.clone()
    two[torch.rand(n, device=DEV, generator=gen) < 0.2, 1] = NAN
    eight = X.clone()
    for c in (0, 2, 4):
        eight[torch.rand(n, device=DEV, generator=gen) < 0.3, c] = NAN
    edges = np.linspace(-2.0, 2.0, B + 1) + float(np.asarray(model.muY).reshape(-1)[0])

    def old_entries(h):                                                   # the parent's calls for such rows: none of it is new
        h.predict_noisy_missing_dev(two[:1200], Psi[:1200])
        h.draws_noisy_missing_dev(two[:1200], Psi[:1200], nd, seed=3)
        h.draws_dev(X[:1200], nd, seed=3, Psi=Psi[:1200], return_gamma=True)   # (the complete rows' gamma and stack, whose route
        h.stack_noisy_dev(X[:1200], Psi[:1200], edges, n_draws=nd, seed=3, n_groups=G)   # text stands in front of this kind's)

    with gpz_amd.Predictor(model, tile_rows=T) as p, gpz_amd.Predictor(model, tile_rows=T) as q:
        old_entries(p)
        old_entries(q)
        held, text = q.info[1], q.route
        assert p.info[1] == held and p.route == text
        assert "noisy missing per draw" not in text and text.endswith(f"; noisy missing: k_predict_noisy_missing_pairs ({chunks_rule(40)} pair chunks)")
        p.draws_noisy_missing_dev(two[:1200], Psi[:1200], nd, seed=3, return_gamma=True)
        assert p.route.startswith(text) and "; noisy missing per draw: k_predict_noisy_missing_gamma" in p.route
        assert not p.route.endswith("k_stack_tile_w")                     # a gamma call alone: no widths
        p.stack_noisy_missing_dev(two[:1200], Psi[:1200], edges, n_draws=nd, seed=3, n_groups=G)
        first = p.info[1]
        assert first > held                                               # the first new calls add once
        assert p.route.endswith(suffix(40, stack=True)), p.route
        p.stack_noisy_missing_dev(two, Psi, edges, n_draws=nd, seed=3, n_groups=G)   # ten times the rows
        p.draws_noisy_missing_dev(two, Psi, nd, seed=3, return_gamma=True)
        assert p.info[1] == first
        assert len(p._nan_groups_dev(eight)) == 8
        p.stack_noisy_missing_dev(eight, Psi, edges, n_draws=nd, seed=3, n_groups=G)  # eight patterns
        p.draws_noisy_missing_dev(eight[:5000], Psi[:5000], nd, seed=3, return_gamma=True)
        assert p.info[1] == first
        old_entries(q)
        q.predict_noisy_missing_dev(eight, Psi)
        assert q.info[1] == held and q.route == text                      # a handle that only calls the parent's entries holds what it held
