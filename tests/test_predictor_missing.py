"""Rows with missing inputs on the predictor handle (Predictor.predict_dev / draws_dev with missing=True, k_predict_missing.hip) against
the one-shot predictMissing route and the oracle: parity over the diagonal kinds, every width, block edge and row count of a group, the
same bits over tile sizes, row orders and the company a row keeps, every layout of X, the draws as an exact square root, the refusals
of the C entries and constant memory.

Gates: nrel <= 1e-11 against gpz_amd.predict on all five outputs (the gate of test_mixed_catalogue_row_for_row and of
test_predictor_noisy.py) and rel <= 1e-8 against oracle.gpz_oracle.predict_any (the project's oracle gate)."""

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, nrel, synth_model
from test_predictor_draws_cpu import philox_normals
from test_predictor_missing_cpu import chunks_rule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIAG = ("GL", "VL", "GD", "VD")
NAMES = ("mu", "sigma", "nu", "beta_i", "gamma")
NAN = float("nan")


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def model_with_priors(method, m, d, k, hetero, seed):
    model = synth_model(method, m, d, k, hetero, seed)
    model.sets["best"]["priors"] = np.random.default_rng(seed + 1).dirichlet(np.full(m, 2.0))
    return model


def knock_out(X, seed, cols=((1, 0.2), (4, 0.1))):
    """Column c missing on a fraction f of the rows, independently per column."""
    rng = np.random.default_rng(seed)
    X = X.copy()
    for c, f in cols:
        X[rng.random(X.shape[0]) < f, c] = NAN
    return X


def reference(X, model):
    """(predict() on all rows it accepts, None), or, where it does not accept the rows with nothing observed, (predict() on the others
    with the oracle's values in those rows, their mask)."""
    try:
        return [np.array(a) for a in gpz_amd.predict(X, model)[:5]], None
    except _lib.GpzError:
        none = np.isnan(X).all(axis=1)
        assert none.any() and not none.all()
        part = gpz_amd.predict(X[~none], model)[:5]
        orc = O.predict_any(X[none], model)[:5]
        out = [np.empty((X.shape[0], model.k)) for _ in range(5)]
        for o, a, b in zip(out, part, orc):
            o[~none] = a
            o[none] = b
        return out, none


def check_parity(out, ref):
    """nrel <= 1e-11 on all five outputs over the rows predict() gave; rel <= 1e-8 on the rows that are the oracle's."""
    ref, orc_rows = ref
    for name, a, b in zip(NAMES, out, ref):
        a = host(a) if isinstance(a, torch.Tensor) else a
        assert a.shape == b.shape, (name, a.shape, b.shape)
        keep = slice(None) if orc_rows is None else ~orc_rows
        print(f"nrel {name}: {nrel(a[keep], b[keep]):.3e}")
        assert nrel(a[keep], b[keep]) <= 1e-11, (name, nrel(a[keep], b[keep]))
        if orc_rows is not None:
            assert rel(a[orc_rows], b[orc_rows]) <= 1e-8, (name, rel(a[orc_rows], b[orc_rows]))


def check_gamma_sign(out, X):
    miss = np.isnan(X).any(axis=1)
    g = host(out[4])
    assert np.all(g[miss] > 0.0) and np.all(g[~miss] == 0.0)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", DIAG)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_parity_with_predict_and_the_oracle(method, hetero, k):
    """2500 rows over 1024-row tiles: dimension 1 missing on 20 % and dimension 4 on 10 % of the rows independently, one row with only
    dimension 0 observed and one with nothing observed."""
    d, ns = 5, 2500
    for m in (7, 50, 250):
        model = model_with_priors(method, m, d, k, hetero, seed=3000 * DIAG.index(method) + 100 * hetero + 10 * k + m)
        X = knock_out(catalogue(model, ns, seed=m), seed=m + 1)
        X[5, 1:] = NAN
        X[9, :] = NAN
        full = ~np.isnan(X).any(axis=1)
        ref = reference(X, model)
        with gpz_amd.Predictor(model, tile_rows=1024) as p:
            out = p.predict_dev(dev(X), missing=True)
            assert f"; missing: k_predict_missing_pairs ({chunks_rule(m)} pair chunks)" in p.route, p.route
            check_parity(out, ref)
            check_gamma_sign(out, X)
            alone = p.predict_dev(dev(X[full]))
            fd = torch.from_numpy(full).to(DEV)
            assert all(torch.equal(a[fd], b) for a, b in zip(out, alone))
            if m <= 50:
                orc = O.predict_any(X[:150], model)
                for name, a, b in zip(NAMES, out, orc):
                    assert rel(host(a)[:150], b) <= 1e-8, (name, rel(host(a)[:150], b))


# ---- 2. every width ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 21)))
def test_every_width(d):
    """Bit 0 alone missing, bit d - 1 alone missing, a single observed dimension (each of the two ends), nothing observed."""
    n, m, k = 300, 20, 1 if d % 2 else 3
    model = model_with_priors("VD" if d % 2 else "GD", m, d, k, True, seed=400 + d)
    X = catalogue(model, n, seed=d)
    X[0:60, 0] = NAN
    if d > 1:
        X[60:120, d - 1] = NAN
        X[120:125, 1:] = NAN                                               # only dimension 0 observed
        X[125:130, :d - 1] = NAN                                           # only dimension d - 1 observed
        X[130, :] = NAN
    ref = reference(X, model)
    with gpz_amd.Predictor(model) as p:
        out = p.predict_dev(dev(X), missing=True)
        check_parity(out, ref)
        check_gamma_sign(out, X)
        F = p.draws_dev(dev(X), 2, Z=np.zeros((m, 2, k)), missing=True)
        assert nrel(host(F[1]), host(out[0])) <= 1e-12


# ---- 3. every block edge -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 11, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256])
def test_every_block_edge(m):
    """m at the edges of the 16-column K blocks and the 64-pair groups (m = 11: 66 pairs, one group and two pairs)."""
    d, n = 3, 200
    for k in (1, 8):
        model = model_with_priors("VL" if m % 2 else "VD", m, d, k, bool(m % 3), seed=800 + 10 * m + k)
        X = knock_out(catalogue(model, n, seed=m), seed=m + 7, cols=((1, 0.3),))
        X[np.random.default_rng(m).random(n) < 0.1] *= np.array([NAN, 1.0, NAN])
        ref = reference(X, model)
        with gpz_amd.Predictor(model) as p:
            out = p.predict_dev(dev(X), missing=True)
            check_parity(out, ref)
            check_gamma_sign(out, X)
            assert f"({chunks_rule(m)} pair chunks)" in p.route
            F = p.draws_dev(dev(X), 2, Z=np.zeros((m, 2, k)), missing=True)
            assert nrel(host(F[0]), host(out[0])) <= 1e-12


# ---- 4. every row count of a group ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_every_row_count_of_a_group(k):
    """A group of n rows at the edges of the 32-row blocks, the 128-row tiles of the product and the 1024-row tile of the handle: parity
    on the longest call, and every shorter one is its first rows bit for bit."""
    d, m, nd = 5, 17, 3
    model = model_with_priors("VD", m, d, k, True, seed=950 + k)
    X = catalogue(model, 1025, seed=93)
    X[:, 2] = NAN
    ref = reference(X, model)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        Xd = dev(X)
        full = p.predict_dev(Xd, missing=True)
        Ff = p.draws_dev(Xd, nd, seed=3, missing=True)
        check_parity(full, ref)
        for n in (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024):
            out = p.predict_dev(Xd[:n], missing=True)
            assert all(o.shape == (n, k) and torch.equal(o, f[:n]) for o, f in zip(out, full)), n
            assert torch.equal(p.draws_dev(Xd[:n], nd, seed=3, missing=True), Ff[:, :n]), n


# ---- 5. the same bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,m,k", [("VD", 100, 1), ("GL", 130, 3)])
def test_same_bits_over_tiles_row_orders_and_company(method, m, k):
    n, d, nd = 3000, 5, 5
    model = model_with_priors(method, m, d, k, True, seed=45 + m)
    X = knock_out(catalogue(model, n, seed=46), seed=47)
    perm = np.random.default_rng(48).permutation(n)
    Xd, pd = dev(X), torch.from_numpy(perm).to(DEV)

    def both(p, x):
        return tuple(p.predict_dev(x, missing=True)) + (p.draws_dev(x, nd, seed=9, missing=True),)

    outs = []
    for tile in (64, 1000, None):
        with gpz_amd.Predictor(model, tile_rows=tile) as p:
            outs.append(both(p, Xd))
            if tile == 1000:
                shuf = both(p, Xd[pd])
                rows = [int(np.flatnonzero(np.isnan(X[:, 1]) & ~np.isnan(X[:, 4]))[3]), int(np.flatnonzero(np.isnan(X[:, 4]))[0]),
                        int(np.flatnonzero(~np.isnan(X).any(axis=1))[2])]
                single = [both(p, Xd[r:r + 1]) for r in rows]
                only = torch.from_numpy(np.isnan(X[:, 1]) & ~np.isnan(X[:, 4])).to(DEV)   # one group, the others removed
                group = both(p, Xd[only])
    base = outs[0]
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, base))
    assert all(torch.equal(a, b[pd]) for a, b in zip(shuf[:5], base[:5]))
    assert torch.equal(shuf[5], base[5][:, pd])
    for r, s in zip(rows, single):
        assert all(torch.equal(a, b[r:r + 1]) for a, b in zip(s[:5], base[:5])), r
        assert torch.equal(s[5], base[5][:, r:r + 1]), r
    assert all(torch.equal(a, b[only]) for a, b in zip(group[:5], base[:5]))
    assert torch.equal(group[5], base[5][:, only])


# ---- 6. layouts ----------------------------------------------------------------------------------------------------------------------------
def test_layouts_of_x_give_the_same_bits():
    """float32, a transposed view and a row-sliced view: each is the call on a contiguous float64 copy of the same values."""
    n, d, nd = 700, 5, 4
    model = model_with_priors("VD", 40, d, 2, True, seed=84)
    X32 = knock_out(catalogue(model, 2 * n, seed=85), seed=86).astype(np.float32)
    Xd = dev(X32.astype(np.float64))
    one = X32.copy()
    one[:, 3] = NAN                                                        # one group: the tensor is read as it lies
    one[:, 1] = 0.25
    one[:, 4] = 0.5
    Od = dev(one.astype(np.float64))
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        def both(x):
            return tuple(p.predict_dev(x, missing=True)) + (p.draws_dev(x, nd, seed=4, missing=True),)

        def same(a, b, what):
            for i, (s, t) in enumerate(zip(a, b)):
                assert torch.equal(s, t), (what, i)

        for x32, xd, what in ((X32, Xd, "mixed"), (one, Od, "one group")):
            ref = both(xd.contiguous())
            same(both(dev(x32, torch.float32)), ref, what + " float32")
            same(both(xd.T.contiguous().T), ref, what + " column-major")
            same(both(dev(x32, torch.float32).T.contiguous().T), ref, what + " float32 column-major")
            half = both(xd[::2].contiguous())
            same(both(xd[::2]), half, what + " row-sliced view")
            same([t[::2] if t.dim() == 2 else t[:, ::2] for t in ref], half, what + " rows of the whole call")
            sel = torch.zeros(2 * n, dtype=torch.bool, device=DEV)
            sel[::2] = True
            same(tuple(p.predict_dev(xd, selection=sel, missing=True)) + (p.draws_dev(xd, nd, seed=4, selection=sel, missing=True),),
                 half, what + " selection")


# ---- 7. draws ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_draws_are_an_exact_square_root_with_missing_inputs(k):
    n, d, m = 200, 4, 30
    model = model_with_priors("VD", m, d, k, True, seed=75 + k)
    X = knock_out(catalogue(model, n, seed=76), seed=77, cols=((0, 0.3), (2, 0.3)))
    Xd = dev(X)
    full = ~np.isnan(X).any(axis=1)
    iS = model.sets["best"]["iSigma_w"]
    with gpz_amd.Predictor(model) as p:
        PHI = p.predict(X, return_phi=True)[5]
        mu = host(p.predict_dev(Xd, missing=True)[0])
        eye = np.stack([np.eye(m)] * k, axis=2)
        F = host(p.draws_dev(Xd, m, Z=eye, missing=True))                  # (m, n, k)
        for o in range(k):
            D = F[:, :, o] - mu[:, o]
            S = 0.5 * (iS[:, :, o] + iS[:, :, o].T)
            assert nrel(D.T @ D, PHI @ S @ PHI.T) <= 1e-10, nrel(D.T @ D, PHI @ S @ PHI.T)
        F0 = host(p.draws_dev(Xd, 3, Z=np.zeros((m, 3, k)), missing=True))
        assert all(nrel(F0[s], mu) <= 1e-12 for s in range(3))
        seeded = p.draws_dev(Xd, 7, seed=12345, missing=True)
        given = host(p.draws_dev(Xd, 7, Z=philox_normals(12345, m, 7, k), missing=True))
        assert nrel(host(seeded), given) <= 1e-12
        # draw s is one weight draw for the rows of every group: the complete rows are the draws of a call without the others
        fd = torch.from_numpy(full).to(DEV)
        assert torch.equal(seeded[:, fd], p.draws_dev(Xd[fd], 7, seed=12345))
        with pytest.raises(_lib.GpzError, match="missing values"):         # and without the keyword the rows are refused as before
            p.draws_dev(Xd, 7, seed=12345)
        with pytest.raises(_lib.GpzError, match="missing values"):
            p.predict_dev(Xd)


# ---- 8. refusals at the C entries -------------------------------------------------------------------------------------------------------------
def test_bad_groups_are_refused_with_the_outputs_untouched():
    n, d, k, nd = 20_000, 5, 2, 3
    model = model_with_priors("VD", 20, d, k, True, seed=88)
    Xh = catalogue(model, n, seed=89)
    Xh[:, 3] = NAN
    X = dev(Xh)
    mask = 0b10111
    with gpz_amd.Predictor(model, tile_rows=1 << 12) as p:
        good = p.predict_dev(X[:500], missing=True)
        muX, sdX, muY = p._norm_vectors()
        pri = p._priors
        stream = torch.cuda.current_stream(X.device).cuda_stream

        def raw(x, obs):
            out = [torch.full((k, n), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
            F = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
            rc1 = p._lib.gpz_predictor_run_missing_dev(p._handle(), *p._x_args(x), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                       _lib.dptr(pri), obs, *(t.data_ptr() for t in out), stream)
            msg = p._lib.gpz_last_error().decode() if rc1 else ""
            rc2 = p._lib.gpz_predictor_draws_missing_dev(p._handle(), *p._x_args(x), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                         _lib.dptr(pri), obs, nd, 5, None, F.data_ptr(), stream)
            torch.cuda.synchronize()
            return rc1, rc2, out + [F], msg

        rc1, rc2, outs, _ = raw(X, mask)
        assert rc1 == 0 and rc2 == 0 and all(bool((t != -7.0).all()) for t in outs)
        assert all(torch.equal(a[:500], b) for a, b in zip(outs[:5], good))
        two = X.clone()
        two[15_000:, 0] = NAN                                              # two patterns in one group
        nan_obs = X.clone()
        nan_obs[19_999, 4] = NAN                                           # a NaN in an observed dimension
        num_miss = X.clone()
        num_miss[12_345, 3] = 0.5                                          # a number in a missing one
        for what, x, obs, text in (("two patterns", two, mask, "share one NaN pattern"), ("NaN in o", nan_obs, mask, "share one NaN pattern"),
                                   ("number in u", num_miss, mask, "share one NaN pattern"),
                                   ("full mask", X, 0b11111, "no dimension is missing"), ("mask past d", X, 0b110111, "above d")):
            rc1, rc2, outs, msg = raw(x, obs)
            assert rc1 == -1 and rc2 == -1, (what, rc1, rc2)               # GPZ_ERR_ARG
            assert text in msg, (what, msg)
            assert all(bool((t == -7.0).all()) for t in outs), what         # refused before any tile kernel has run
            again = p.predict_dev(X[:500], missing=True)                    # the handle works on the next call
            assert all(torch.equal(a, b) for a, b in zip(again, good))


@pytest.mark.parametrize("kw", [{"m": 300}, {"d": 24}, {"k": 9}, {"method": "VC"}])
def test_shapes_outside_the_route_are_refused_by_the_c_entry(kw):
    a = {"method": "VD", "m": 20, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    X = catalogue(model, 40, seed=6)
    X[:, 1] = NAN
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match="predict_missing_fits"):
            p.predict_dev(dev(X), missing=True)
        muX, sdX, muY = p._norm_vectors()
        out = [torch.empty((a["k"], 40), dtype=torch.float64, device=DEV).T for _ in range(5)]
        h = p._handle()
        with pytest.raises(_lib.GpzError, match="predict_missing_fits") as ei:
            _lib.check(p._lib.gpz_predictor_run_missing_dev(h, *p._x_args(dev(X)), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                            None, (1 << a["d"]) - 3, *(t.data_ptr() for t in out), None))
        assert ei.value.code == -5                                         # GPZ_ERR_UNSUPPORTED
        assert "missing" not in p.route


# ---- 9. memory -----------------------------------------------------------------------------------------------------------------------------
def test_memory_is_added_once_and_never_grows_with_rows_or_patterns():
    d, nd = 5, 4
    model = model_with_priors("VD", 30, d, 1, True, seed=97)
    n = 200_000
    gen = torch.Generator(device=DEV).manual_seed(98)
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=gen) * torch.from_numpy(model.sdX).to(DEV) + \
        torch.from_numpy(model.muX).to(DEV)
    two = X.clone()
    two[torch.rand(n, device=DEV, generator=gen) < 0.2, 1] = NAN
    eight = X.clone()
    for c in (0, 2, 4):
        eight[torch.rand(n, device=DEV, generator=gen) < 0.3, c] = NAN
    with gpz_amd.Predictor(model, tile_rows=1 << 16) as p, gpz_amd.Predictor(model, tile_rows=1 << 16) as q:
        q.predict_dev(X[:1000]); q.draws_dev(X[:1000], nd)                   # a handle that never sees the keyword ...
        p.predict_dev(X[:1000]); p.draws_dev(X[:1000], nd)
        held = p.info[1]
        assert held == q.info[1]
        small = p.predict_dev(two[:1000], missing=True)
        p.draws_dev(two[:1000], nd, missing=True)
        first = p.info[1]
        assert first > held
        out = p.predict_dev(two, missing=True)
        p.draws_dev(two[:50_000], nd, missing=True)
        assert p.info[1] == first                                            # 200 000 rows: the same bytes
        assert all(torch.equal(a, b[:1000]) for a, b in zip(small, out))
        assert len(p._nan_groups_dev(eight)) == 8
        p.predict_dev(eight[:20_000], missing=True)
        p.draws_dev(eight[:20_000], nd, missing=True)
        assert p.info[1] == first                                            # eight patterns: the same bytes
        q.predict_dev(X); q.draws_dev(X[:50_000], nd)
        assert q.info[1] == held                                             # ... holds what it held
