"""Rows with both input noise and missing inputs on the predictor handle (Predictor.predict_noisy_missing_dev / draws_noisy_missing_dev,
k_predict_noisy_missing.hip) against the one-shot predictNoisyMissing route and the oracle: parity over the diagonal kinds, every width,
block edge and row count of a group, the same bits over tile sizes, row orders and the company a row keeps, every layout of X and Psi,
Psi unread in the missing dimensions, the Psi = 0 limit, the draws as an exact square root, the refusals of the C entries and constant
memory.

Gates: nrel <= 1e-11 against gpz_amd.predict(X, model, Psi=Psi) on all five outputs (the gate of test_predictor_noisy.py and
test_predictor_missing.py for the same kind of comparison) and rel <= 1e-8 against oracle.gpz_oracle.predict_any (the project's oracle
gate)."""

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
from test_predictor_noisy import noise

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIAG = ("GL", "VL", "GD", "VD")
NAMES = ("mu", "sigma", "nu", "beta_i", "gamma")
NAN = float("nan")


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def reference(X, Psi, model):
    """(predict() on all rows it accepts, None), or, where it does not accept the rows with nothing observed, (predict() on the others
    with the oracle's values in those rows, their mask)."""
    try:
        return [np.array(a) for a in gpz_amd.predict(X, model, Psi=Psi)[:5]], None
    except _lib.GpzError:
        none = np.isnan(X).all(axis=1)
        assert none.any() and not none.all()
        part = gpz_amd.predict(X[~none], model, Psi=Psi[~none])[:5]
        orc = O.predict_any(X[none], model, Psi=Psi[none])[:5]
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
    assert np.all(host(out[4])[miss] > 0.0)


def suffix(m):
    return f"; noisy missing: k_predict_noisy_missing_pairs ({chunks_rule(m)} pair chunks)"


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", DIAG)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_parity_with_predict_and_the_oracle(method, hetero, k):
    """2500 rows over 1024-row tiles, Psi on every row: dimension 1 missing on 20 % and dimension 4 on 10 % of the rows independently,
    one row with only dimension 0 observed and one with nothing observed."""
    d, ns = 5, 2500
    for m in (7, 50, 250):
        model = model_with_priors(method, m, d, k, hetero, seed=5000 * DIAG.index(method) + 100 * hetero + 10 * k + m)
        X = knock_out(catalogue(model, ns, seed=m), seed=m + 1)
        X[5, 1:] = NAN
        X[9, :] = NAN
        Psi = noise(ns, d, seed=m + 2)
        full = ~np.isnan(X).any(axis=1)
        ref = reference(X, Psi, model)
        with gpz_amd.Predictor(model, tile_rows=1024) as p:
            out = p.predict_noisy_missing_dev(dev(X), dev(Psi))
            assert p.route.endswith(suffix(m)), p.route
            check_parity(out, ref)
            check_gamma_sign(out, X)
            alone = p.predict_dev(dev(X[full]), Psi=dev(Psi[full]))
            fd = torch.from_numpy(full).to(DEV)
            assert all(torch.equal(a[fd], b) for a, b in zip(out, alone))
            if m <= 50:
                orc = O.predict_any(X[:150], model, Psi=Psi[:150])
                for name, a, b in zip(NAMES, out, orc):
                    assert rel(host(a)[:150], b) <= 1e-8, (name, rel(host(a)[:150], b))


# ---- 2. every width ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 21)))
def test_every_width(d):
    """Bit 0 alone missing, bit d - 1 alone missing, a single observed dimension (each of the two ends), nothing observed."""
    n, m, k = 300, 20, 1 if d % 2 else 3
    model = model_with_priors("VD" if d % 2 else "GD", m, d, k, True, seed=1400 + d)
    X = catalogue(model, n, seed=d)
    X[0:60, 0] = NAN
    if d > 1:
        X[60:120, d - 1] = NAN
        X[120:125, 1:] = NAN                                               # only dimension 0 observed
        X[125:130, :d - 1] = NAN                                           # only dimension d - 1 observed
        X[130, :] = NAN
    Psi = noise(n, d, seed=d + 50)
    ref = reference(X, Psi, model)
    with gpz_amd.Predictor(model) as p:
        out = p.predict_noisy_missing_dev(dev(X), dev(Psi))
        check_parity(out, ref)
        check_gamma_sign(out, X)
        F = p.draws_noisy_missing_dev(dev(X), dev(Psi), 2, Z=np.zeros((m, 2, k)))
        assert nrel(host(F[1]), host(out[0])) <= 1e-12


# ---- 3. every block edge -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 11, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256])
def test_every_block_edge(m):
    """m at the edges of the 16-column K blocks and the 64-pair groups (m = 11: 66 pairs, one group and two pairs)."""
    d, n = 3, 200
    for k in (1, 8):
        model = model_with_priors("VL" if m % 2 else "VD", m, d, k, bool(m % 3), seed=1800 + 10 * m + k)
        X = knock_out(catalogue(model, n, seed=m), seed=m + 7, cols=((1, 0.3),))
        X[np.random.default_rng(m).random(n) < 0.1] *= np.array([NAN, 1.0, NAN])
        Psi = noise(n, d, seed=m + 9)
        ref = reference(X, Psi, model)
        with gpz_amd.Predictor(model) as p:
            out = p.predict_noisy_missing_dev(dev(X), dev(Psi))
            check_parity(out, ref)
            check_gamma_sign(out, X)
            assert p.route.endswith(suffix(m)), p.route
            F = p.draws_noisy_missing_dev(dev(X), dev(Psi), 2, Z=np.zeros((m, 2, k)))
            assert nrel(host(F[0]), host(out[0])) <= 1e-12


# ---- 4. every row count of a group ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_every_row_count_of_a_group(k):
    """A group of n rows at the edges of the 32-row blocks, the 128-row tiles of the product and the 1024-row tile of the handle: parity
    on the longest call, and every shorter one is its first rows bit for bit, draws included."""
    d, m, nd = 5, 17, 3
    model = model_with_priors("VD", m, d, k, True, seed=1950 + k)
    X = catalogue(model, 1025, seed=93)
    X[:, 2] = NAN
    Psi = noise(1025, d, seed=94)
    ref = reference(X, Psi, model)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        Xd, Pd = dev(X), dev(Psi)
        full = p.predict_noisy_missing_dev(Xd, Pd)
        Ff = p.draws_noisy_missing_dev(Xd, Pd, nd, seed=3)
        check_parity(full, ref)
        for n in (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024):
            out = p.predict_noisy_missing_dev(Xd[:n], Pd[:n])
            assert all(o.shape == (n, k) and torch.equal(o, f[:n]) for o, f in zip(out, full)), n
            assert torch.equal(p.draws_noisy_missing_dev(Xd[:n], Pd[:n], nd, seed=3), Ff[:, :n]), n


# ---- 5. the same bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,m,k", [("VD", 100, 1), ("GL", 130, 3)])
def test_same_bits_over_tiles_row_orders_and_company(method, m, k):
    n, d, nd = 3000, 5, 5
    model = model_with_priors(method, m, d, k, True, seed=145 + m)
    X = knock_out(catalogue(model, n, seed=46), seed=47)
    Psi = noise(n, d, seed=49)
    perm = np.random.default_rng(48).permutation(n)
    Xd, Pd, pd = dev(X), dev(Psi), torch.from_numpy(perm).to(DEV)

    def both(p, x, psi):
        return tuple(p.predict_noisy_missing_dev(x, psi)) + (p.draws_noisy_missing_dev(x, psi, nd, seed=9),)

    outs = []
    for tile in (64, 1000, None):
        with gpz_amd.Predictor(model, tile_rows=tile) as p:
            outs.append(both(p, Xd, Pd))
            if tile == 1000:
                shuf = both(p, Xd[pd], Pd[pd])
                rows = [int(np.flatnonzero(np.isnan(X[:, 1]) & ~np.isnan(X[:, 4]))[3]), int(np.flatnonzero(np.isnan(X[:, 4]))[0]),
                        int(np.flatnonzero(~np.isnan(X).any(axis=1))[2])]
                single = [both(p, Xd[r:r + 1], Pd[r:r + 1]) for r in rows]
                only = torch.from_numpy(np.isnan(X[:, 1]) & ~np.isnan(X[:, 4])).to(DEV)   # one group, the others removed
                group = both(p, Xd[only], Pd[only])
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
def test_layouts_of_x_and_psi_give_the_same_bits():
    """float32, transposed storage, row-sliced views, Psi as (n, 1) and (n,): each is the call on a contiguous float64 copy of the same
    values, bit for bit."""
    n, d, nd = 700, 5, 4
    model = model_with_priors("VD", 40, d, 2, True, seed=184)
    X32 = knock_out(catalogue(model, 2 * n, seed=85), seed=86).astype(np.float32)
    P32 = noise(2 * n, d, seed=87).astype(np.float32)
    Xd, Pd = dev(X32.astype(np.float64)), dev(P32.astype(np.float64))     # the same values as float64
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        def both(x, psi, **kw):
            return tuple(p.predict_noisy_missing_dev(x, psi, **kw)) + (p.draws_noisy_missing_dev(x, psi, nd, seed=4, **kw),)

        def same(a, b, what):
            for i, (s, t) in enumerate(zip(a, b)):
                assert torch.equal(s, t), (what, i)

        ref = both(Xd.contiguous(), Pd.contiguous())
        same(both(dev(X32, torch.float32), dev(P32, torch.float32)), ref, "float32")
        same(both(Xd, dev(P32, torch.float32)), ref, "float32 Psi")
        same(both(dev(X32, torch.float32), Pd), ref, "float32 X")
        same(both(Xd.T.contiguous().T, Pd.T.contiguous().T), ref, "transposed storage")
        same(both(Xd.T.contiguous().T, Pd), ref, "mixed layouts")
        half = both(Xd[::2].contiguous(), Pd[::2].contiguous())
        same(both(Xd[::2], Pd[::2]), half, "row-sliced views")
        same([t[::2] if t.dim() == 2 else t[:, ::2] for t in ref], half, "rows of the whole call")
        col = Pd[:, 2].contiguous()
        bc = both(Xd, col[:, None].expand(2 * n, d).contiguous())
        same(both(Xd, col[:, None]), bc, "Psi (n, 1)")
        same(both(Xd, col), bc, "Psi (n,)")
        same(both(Xd, Pd[:, 2]), bc, "Psi (n,) strided")
        sel = torch.zeros(2 * n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        same(both(Xd, Pd, selection=sel), half, "selection")


# ---- 7. Psi in the missing dimensions ------------------------------------------------------------------------------------------------------
def test_psi_in_missing_dimensions_is_not_read():
    """NaN, inf and -1 in Psi where X is NaN change no bit; the same values in an observed dimension are refused by the C entries with the
    outputs untouched."""
    n, d, k, nd, m = 3000, 5, 2, 3, 30
    model = model_with_priors("VD", m, d, k, True, seed=188)
    X = knock_out(catalogue(model, n, seed=89), seed=90)
    X[7, :] = NAN
    Psi = noise(n, d, seed=91)
    nan = np.isnan(X)
    Xd, Pd = dev(X), dev(Psi)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        ref = tuple(p.predict_noisy_missing_dev(Xd, Pd)) + (p.draws_noisy_missing_dev(Xd, Pd, nd, seed=2),)
        for v in (NAN, float("inf"), -1.0):
            bad = Psi.copy()
            bad[nan] = v
            for psi in (dev(bad), dev(bad.astype(np.float32), torch.float32)):
                want = ref
                if psi.dtype == torch.float32:
                    P32 = dev(Psi.astype(np.float32), torch.float32)
                    want = tuple(p.predict_noisy_missing_dev(Xd, P32)) + (p.draws_noisy_missing_dev(Xd, P32, nd, seed=2),)
                got = tuple(p.predict_noisy_missing_dev(Xd, psi)) + (p.draws_noisy_missing_dev(Xd, psi, nd, seed=2),)
                assert all(torch.equal(a, b) for a, b in zip(got, want)), v
        # one group through the C entries: dimension 4 missing
        g = np.flatnonzero(~nan[:, 1] & nan[:, 4])
        Xg, Pg, ng = dev(X[g]), Psi[g].copy(), g.size
        muX, sdX, muY = p._norm_vectors()
        sd2 = np.ascontiguousarray(sdX ** 2)
        stream = torch.cuda.current_stream(Xd.device).cuda_stream
        good = p.predict_noisy_missing_dev(Xg, dev(Pg))

        def raw(psi, obs=0b01111):
            out = [torch.full((k, ng), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
            F = torch.full((nd, k, ng), -7.0, dtype=torch.float64, device=DEV)
            lead = [p._handle(), *p._x_args(Xg), *p._psi_args(psi, ng), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(sd2), _lib.dptr(muY),
                    _lib.dptr(p._priors), obs]
            rc1 = p._lib.gpz_predictor_run_noisy_missing_dev(*lead, *(t.data_ptr() for t in out), stream)
            msg = p._lib.gpz_last_error().decode() if rc1 else ""
            rc2 = p._lib.gpz_predictor_draws_noisy_missing_dev(*lead, nd, 5, None, F.data_ptr(), stream)
            torch.cuda.synchronize()
            return rc1, rc2, out + [F], msg

        rc1, rc2, outs, _ = raw(dev(Pg))
        assert rc1 == 0 and rc2 == 0 and all(bool((t != -7.0).all()) for t in outs)
        assert all(torch.equal(a, b) for a, b in zip(outs[:5], good))
        for v, at, c in ((NAN, ng - 1, 3), (float("inf"), 0, 0), (-1e-300, ng // 2, 2)):
            bad = Pg.copy()
            bad[at, c] = v
            rc1, rc2, outs, msg = raw(dev(bad))
            assert rc1 == -1 and rc2 == -1, (v, rc1, rc2)                   # GPZ_ERR_ARG
            assert "Psi has an element that is NaN, infinite or negative" in msg, msg
            assert all(bool((t == -7.0).all()) for t in outs), v            # refused before any tile kernel has run
            miss = Pg.copy()
            miss[at, 4] = v                                                 # the same value where the group's X is NaN: taken
            rc1, rc2, outs, _ = raw(dev(miss))
            assert rc1 == 0 and rc2 == 0 and all(torch.equal(a, b) for a, b in zip(outs[:5], good)), v
        one = dev(Pg[:, :1])                                                # the broadcast column is scanned too
        one[ng // 3, 0] = -1.0
        rc1, rc2, outs, msg = raw(one)
        assert rc1 == -1 and rc2 == -1 and "Psi" in msg and all(bool((t == -7.0).all()) for t in outs)
        with pytest.raises(_lib.GpzError, match="Psi"):                     # and through the method: in the row's observed dimensions
            p.predict_noisy_missing_dev(Xd, dev(np.where(nan, Psi, -1.0)))


# ---- 8. Psi = 0 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,k", [("VD", 1), ("GD", 3)])
def test_zero_noise_is_the_prediction_for_missing_inputs(method, k):
    """On the rows with missing values only (predictNoisy's nu of complete rows differs from predictFull's for the unsymmetrised
    iSigma_w of the test models; test_predictor_noisy.py covers that): mu and beta_i at nrel <= 1e-12, nu at 1e-11,
    |gamma - gamma_missing| <= 1e-11 |mu^2| with mu before muY - the gates of test_zero_noise_is_the_noise_free_prediction."""
    n, d, m = 600, 5, 60
    model = model_with_priors(method, m, d, k, True, seed=160 + k)
    X = knock_out(catalogue(model, n, seed=61), seed=62, cols=((1, 0.4), (4, 0.3)))
    X[3, :] = NAN
    miss = np.isnan(X).any(axis=1)
    Xd = dev(X)
    with gpz_amd.Predictor(model) as p:
        z = [host(t)[miss] for t in p.predict_noisy_missing_dev(Xd, torch.zeros((n, d), dtype=torch.float64, device=DEV))]
        f = [host(t)[miss] for t in p.predict_dev(Xd, missing=True)]
    assert miss.sum() > 100
    print("mu", nrel(z[0], f[0]), "beta", nrel(z[3], f[3]), "nu", nrel(z[2], f[2]))
    assert nrel(z[0], f[0]) <= 1e-12 and nrel(z[3], f[3]) <= 1e-12
    assert nrel(z[2], f[2]) <= 1e-11, nrel(z[2], f[2])
    mu0 = z[0] - model.muY
    print("gamma", np.linalg.norm(z[4] - f[4]) / np.linalg.norm(mu0 ** 2))
    assert np.linalg.norm(z[4] - f[4]) <= 1e-11 * np.linalg.norm(mu0 ** 2)


# ---- 9. draws ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_draws_are_an_exact_square_root(k):
    n, d, m = 200, 4, 30
    model = model_with_priors("VD", m, d, k, True, seed=175 + k)
    X = knock_out(catalogue(model, n, seed=76), seed=77, cols=((0, 0.3), (2, 0.3)))
    Psi = noise(n, d, seed=78)
    Xd, Pd = dev(X), dev(Psi)
    full = ~np.isnan(X).any(axis=1)
    iS = model.sets["best"]["iSigma_w"]
    with gpz_amd.Predictor(model) as p:
        PHI = gpz_amd.predict(X, model, Psi=Psi)[5]
        mu = host(p.predict_noisy_missing_dev(Xd, Pd)[0])
        eye = np.stack([np.eye(m)] * k, axis=2)
        F = host(p.draws_noisy_missing_dev(Xd, Pd, m, Z=eye))              # (m, n, k)
        for o in range(k):
            D = F[:, :, o] - mu[:, o]
            S = 0.5 * (iS[:, :, o] + iS[:, :, o].T)
            assert nrel(D.T @ D, PHI @ S @ PHI.T) <= 1e-10, nrel(D.T @ D, PHI @ S @ PHI.T)
        F0 = host(p.draws_noisy_missing_dev(Xd, Pd, 3, Z=np.zeros((m, 3, k))))
        assert all(nrel(F0[s], mu) <= 1e-12 for s in range(3))
        seeded = p.draws_noisy_missing_dev(Xd, Pd, 7, seed=12345)
        given = host(p.draws_noisy_missing_dev(Xd, Pd, 7, Z=philox_normals(12345, m, 7, k)))
        assert nrel(host(seeded), given) <= 1e-12
        # draw s is one weight draw for the rows of every group (the cross-group blocks of D'D above hold for that reason alone): the
        # complete rows are the draws of a call without the others, and so is a group with missing values
        fd = torch.from_numpy(full).to(DEV)
        assert torch.equal(seeded[:, fd], p.draws_dev(Xd[fd], 7, seed=12345, Psi=Pd[fd]))
        gd = torch.from_numpy(np.isnan(X[:, 0]) & ~np.isnan(X[:, 2])).to(DEV)
        assert int(gd.sum()) > 10 and torch.equal(seeded[:, gd], p.draws_noisy_missing_dev(Xd[gd], Pd[gd], 7, seed=12345))
        assert not torch.equal(seeded, p.draws_dev(Xd, 7, seed=12345, missing=True))   # (and they are not the noise-free draws)


# ---- 10. refusals at the C entries -----------------------------------------------------------------------------------------------------------
def test_bad_groups_are_refused_with_the_outputs_untouched():
    n, d, k, nd = 5000, 5, 2, 3
    model = model_with_priors("VD", 20, d, k, True, seed=288)
    Xh = catalogue(model, n, seed=89)
    Xh[:, 3] = NAN
    X, Psi = dev(Xh), dev(noise(n, d, seed=92))
    mask = 0b10111
    with gpz_amd.Predictor(model, tile_rows=1 << 12) as p:
        good = p.predict_noisy_missing_dev(X[:500], Psi[:500])
        muX, sdX, muY = p._norm_vectors()
        sd2 = np.ascontiguousarray(sdX ** 2)
        stream = torch.cuda.current_stream(X.device).cuda_stream

        def raw(x, obs):
            out = [torch.full((k, n), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
            F = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
            lead = [p._handle(), *p._x_args(x), *p._psi_args(Psi, n), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(sd2), _lib.dptr(muY),
                    _lib.dptr(p._priors), obs]
            rc1 = p._lib.gpz_predictor_run_noisy_missing_dev(*lead, *(t.data_ptr() for t in out), stream)
            msg = p._lib.gpz_last_error().decode() if rc1 else ""
            rc2 = p._lib.gpz_predictor_draws_noisy_missing_dev(*lead, nd, 5, None, F.data_ptr(), stream)
            torch.cuda.synchronize()
            return rc1, rc2, out + [F], msg

        rc1, rc2, outs, _ = raw(X, mask)
        assert rc1 == 0 and rc2 == 0 and all(bool((t != -7.0).all()) for t in outs)
        assert all(torch.equal(a[:500], b) for a, b in zip(outs[:5], good))
        two = X.clone()
        two[4000:, 0] = NAN                                                # two patterns in one group
        nan_obs = X.clone()
        nan_obs[n - 1, 4] = NAN                                            # a NaN in an observed dimension
        num_miss = X.clone()
        num_miss[2345, 3] = 0.5                                            # a number in a missing one
        for what, x, obs, text in (("two patterns", two, mask, "share one NaN pattern"), ("NaN in o", nan_obs, mask, "share one NaN pattern"),
                                   ("number in u", num_miss, mask, "share one NaN pattern"),
                                   ("full mask", X, 0b11111, "no dimension is missing"), ("mask past d", X, 0b110111, "above d")):
            rc1, rc2, outs, msg = raw(x, obs)
            assert rc1 == -1 and rc2 == -1, (what, rc1, rc2)               # GPZ_ERR_ARG
            assert text in msg, (what, msg)
            assert all(bool((t == -7.0).all()) for t in outs), what         # refused before any tile kernel has run
            again = p.predict_noisy_missing_dev(X[:500], Psi[:500])         # the handle works on the next call
            assert all(torch.equal(a, b) for a, b in zip(again, good))


@pytest.mark.parametrize("kw", [{"m": 300}, {"d": 24}, {"k": 9}, {"method": "VC"}])
def test_shapes_outside_the_route_are_refused_by_the_c_entries(kw):
    a = {"method": "VD", "m": 20, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    X = catalogue(model, 40, seed=6)
    X[:, 1] = NAN
    Psi = noise(40, a["d"], seed=7)
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match="predict_missing_fits"):
            p.predict_noisy_missing_dev(dev(X), dev(Psi))
        with pytest.raises(ValueError, match="predict_missing_fits"):
            p.draws_noisy_missing_dev(dev(X), dev(Psi), 4)
        muX, sdX, muY = p._norm_vectors()
        out = [torch.empty((a["k"], 40), dtype=torch.float64, device=DEV).T for _ in range(5)]
        F = torch.empty((4, a["k"], 40), dtype=torch.float64, device=DEV)
        lead = [p._handle(), *p._x_args(dev(X)), *p._psi_args(dev(Psi), 40), _lib.dptr(muX), _lib.dptr(sdX),
                _lib.dptr(np.ascontiguousarray(sdX ** 2)), _lib.dptr(muY), None, (1 << a["d"]) - 3]
        for call in (lambda: p._lib.gpz_predictor_run_noisy_missing_dev(*lead, *(t.data_ptr() for t in out), None),
                     lambda: p._lib.gpz_predictor_draws_noisy_missing_dev(*lead, 4, 0, None, F.data_ptr(), None)):
            with pytest.raises(_lib.GpzError, match="predict_missing_fits") as ei:
                _lib.check(call())
            assert ei.value.code == -5                                     # GPZ_ERR_UNSUPPORTED
        assert "missing" not in p.route


# ---- 11. memory ----------------------------------------------------------------------------------------------------------------------------
def test_memory_is_added_once_and_never_grows_with_rows_or_patterns():
    d, nd = 5, 4
    model = model_with_priors("VD", 30, d, 1, True, seed=197)
    n = 60_000
    gen = torch.Generator(device=DEV).manual_seed(98)
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=gen) * torch.from_numpy(model.sdX).to(DEV) + \
        torch.from_numpy(model.muX).to(DEV)
    Psi = 0.05 * torch.rand((n, d), dtype=torch.float64, device=DEV, generator=gen)
    two = X.clone()
    two[torch.rand(n, device=DEV, generator=gen) < 0.2, 1] = NAN
    eight = X.clone()
    for c in (0, 2, 4):
        eight[torch.rand(n, device=DEV, generator=gen) < 0.3, c] = NAN
    with gpz_amd.Predictor(model, tile_rows=1 << 14) as p, gpz_amd.Predictor(model, tile_rows=1 << 14) as q:
        def usual(h):                                                        # every row kind a handle had before: none of it is new
            h.predict_dev(X[:1000]); h.draws_dev(X[:1000], nd)
            h.predict_dev(X[:1000], Psi=Psi[:1000]); h.draws_dev(X[:1000], nd, Psi=Psi[:1000])
            h.predict_dev(two[:1000], missing=True); h.draws_dev(two[:1000], nd, missing=True)
        usual(q)                                                             # a handle that never makes such a call ...
        usual(p)
        held, route = p.info[1], p.route
        assert held == q.info[1] and route == q.route and "noisy missing" not in route
        small = p.predict_noisy_missing_dev(two[:1000], Psi[:1000])
        p.draws_noisy_missing_dev(two[:1000], Psi[:1000], nd)
        first = p.info[1]
        assert first > held and p.route.startswith(route) and p.route[len(route):].startswith("; noisy missing: ")
        out = p.predict_noisy_missing_dev(two, Psi)
        p.draws_noisy_missing_dev(two[:20_000], Psi[:20_000], nd)
        assert p.info[1] == first                                            # 60 000 rows: the same bytes
        assert all(torch.equal(a, b[:1000]) for a, b in zip(small, out))
        assert len(p._nan_groups_dev(eight)) == 8
        p.predict_noisy_missing_dev(eight[:20_000], Psi[:20_000])
        p.draws_noisy_missing_dev(eight[:20_000], Psi[:20_000], nd)
        assert p.info[1] == first                                            # eight patterns: the same bytes
        usual(q); q.predict_dev(two, missing=True)
        assert q.info[1] == held and q.route == route                        # ... holds what it held and says what it said
    with gpz_amd.Predictor(model, tile_rows=1 << 14) as r:                   # a fresh handle: the first such call brings all it needs
        r.predict_dev(X[:1000])
        base = r.info[1]
        r.predict_noisy_missing_dev(two[:1000], Psi[:1000])
        grown = r.info[1]
        assert grown > base
        r.predict_noisy_missing_dev(eight, Psi)
        assert r.info[1] == grown
