"""Input noise on the predictor handle (Predictor.predict_dev / draws_dev / draws with Psi=, k_predict_noisy.hip) against the one-shot
predictNoisy route and the oracle: parity over the diagonal kinds, every layout of X and Psi, every instantiated width and block edge,
the same bits over tile sizes and row orders, the Psi = 0 limit, the draws as an exact square root, the refusals and constant memory."""

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, nrel, synth_model
from test_predictor_draws_cpu import philox_normals
from test_predictor_noisy_cpu import chunks_rule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIAG = ("GL", "VL", "GD", "VD")
NAMES = ("mu", "sigma", "nu", "beta_i", "gamma")


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def noise(n, d, seed):
    return np.random.default_rng(seed).gamma(1.0, 0.05, (n, d))


def check_parity(out, ref, gate=1e-11):
    """The norm ratio on all five outputs (gamma element by element differs by up to 1e-9 where gamma ~ 1e-7 mu^2)."""
    for name, a, b in zip(NAMES, out, ref):
        a = host(a) if isinstance(a, torch.Tensor) else a
        assert a.shape == b.shape, (name, a.shape, b.shape)
        assert nrel(a, b) <= gate, (name, nrel(a, b))


# ---- 1. parity against the existing routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", DIAG)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_parity_with_predict_and_the_oracle(method, hetero, k):
    """ns = 2500 over 1024-row tiles (the last one partial) against predict(X, model, Psi=Psi) at nrel <= 1e-11 on all five outputs;
    150 rows against the oracle's predict_noisy at rel <= 1e-8 where m <= 50."""
    d, ns = 5, 2500
    for m in (7, 50, 250):
        model = synth_model(method, m, d, k, hetero, seed=2000 * DIAG.index(method) + 100 * hetero + 10 * k + m)
        X = catalogue(model, ns, seed=m)
        Psi = noise(ns, d, seed=m + 1)
        ref = gpz_amd.predict(X, model, Psi=Psi)
        with gpz_amd.Predictor(model, tile_rows=1024) as p:
            out = p.predict_dev(dev(X), Psi=dev(Psi))
            assert p.route.endswith(f"; noise: k_predict_noisy_small ({chunks_rule(m, d, k)} pair chunks)"), p.route
            check_parity(out, ref)
            assert np.any(host(out[4]) != 0.0)
            if m <= 50:
                orc = O.predict_noisy(X[:150], Psi[:150], model)
                sub = p.predict_dev(dev(X[:150]), Psi=dev(Psi[:150]))
                for name, a, b in zip(NAMES, sub, orc):
                    assert rel(host(a), b) <= 1e-8, (name, rel(host(a), b))
                assert all(torch.equal(a, b[:150]) for a, b in zip(sub, out))


# ---- 2. layouts --------------------------------------------------------------------------------------------------------------------------
def test_layouts_of_x_and_psi_give_the_same_bits():
    """float32, a transposed view, a row-sliced view, Psi as (n, 1) and (n,): each is the call on a contiguous float64 copy of the same
    values, bit for bit."""
    n, d, nd = 700, 5, 6
    model = synth_model("VD", 40, d, 2, True, seed=81)
    X32 = catalogue(model, 2 * n, seed=82).astype(np.float32)
    P32 = noise(2 * n, d, seed=83).astype(np.float32)
    Xd, Pd = dev(X32.astype(np.float64)), dev(P32.astype(np.float64))                  # the same values as float64
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        def both(x, psi):
            return tuple(p.predict_dev(x, Psi=psi)) + (p.draws_dev(x, nd, seed=4, Psi=psi),)

        def same(a, b, what):
            for i, (s, t) in enumerate(zip(a, b)):
                assert torch.equal(s, t), (what, i, float((s - t).abs().max()))

        ref = both(Xd.contiguous(), Pd.contiguous())
        same(both(dev(X32, torch.float32), dev(P32, torch.float32)), ref, "float32")
        same(both(Xd, dev(P32, torch.float32)), ref, "float32 Psi")
        same(both(Xd.T.contiguous().T, Pd.T.contiguous().T), ref, "transposed views")
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
        same(tuple(p.predict_dev(Xd, selection=sel, Psi=Pd)) + (p.draws_dev(Xd, nd, seed=4, selection=sel, Psi=Pd),), half, "selection")


# ---- 3. edges -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 20])
def test_every_width_and_padding(d):
    n = 257
    for k in (1, 8):
        model = synth_model("VD" if d % 2 else "GD", 17, d, k, True, seed=300 + 10 * d + k)
        X, Psi = catalogue(model, n, seed=d), noise(n, d, seed=d + 50)
        ref = gpz_amd.predict(X, model, Psi=Psi)
        with gpz_amd.Predictor(model) as p:
            check_parity(p.predict_dev(dev(X), Psi=dev(Psi)), ref)
            F = p.draws_dev(dev(X), 3, Z=np.zeros((17, 3, k)), Psi=dev(Psi))
            assert nrel(host(F[1]), ref[0]) <= 1e-12


CHUNK_EDGES = [m for m in range(2, 257) if chunks_rule(m, 3, 1) != chunks_rule(m - 1, 3, 1)]


@pytest.mark.parametrize("m", sorted({1, 2, 15, 16, 17, 255, 256} | {m + s for m in CHUNK_EDGES for s in (-1, 0)}))
def test_every_block_count_and_chunk_change(m):
    """m at the edges of the 16-column blocks of the draws and on both sides of every change of predict_noisy_chunks."""
    d, n = 3, 65
    for k in (1, 8):
        model = synth_model("VL" if m % 2 else "VD", m, d, k, bool(m % 3), seed=700 + 10 * m + k)
        X, Psi = catalogue(model, n, seed=m), noise(n, d, seed=m + 50)
        ref = gpz_amd.predict(X, model, Psi=Psi)
        with gpz_amd.Predictor(model) as p:
            check_parity(p.predict_dev(dev(X), Psi=dev(Psi)), ref)
            assert f"({chunks_rule(m, d, k)} pair chunks)" in p.route
            F = p.draws_dev(dev(X), 2, Z=np.zeros((m, 2, k)), Psi=dev(Psi))
            assert nrel(host(F[0]), ref[0]) <= 1e-12


@pytest.mark.parametrize("k", [1, 8])
def test_every_row_count(k):
    """n at the edges of the 32-row blocks of the draws and the 64-lane waves and 256-row workgroups of the pair kernel: parity on the
    longest call, and every shorter one is its first rows bit for bit."""
    d, m, nd = 5, 17, 3
    model = synth_model("VD", m, d, k, True, seed=900 + k)
    X, Psi = catalogue(model, 257, seed=91), noise(257, d, seed=92)
    ref = gpz_amd.predict(X, model, Psi=Psi)
    with gpz_amd.Predictor(model) as p:
        Xd, Pd = dev(X), dev(Psi)
        full = p.predict_dev(Xd, Psi=Pd)
        Ff = p.draws_dev(Xd, nd, seed=3, Psi=Pd)
        check_parity(full, ref)
        for n in (1, 31, 32, 33, 63, 64, 65, 255, 256):
            out = p.predict_dev(Xd[:n], Psi=Pd[:n])
            assert all(o.shape == (n, k) and torch.equal(o, f[:n]) for o, f in zip(out, full)), n
            assert torch.equal(p.draws_dev(Xd[:n], nd, seed=3, Psi=Pd[:n]), Ff[:, :n]), n


@pytest.mark.parametrize("kw", [{"m": 300}, {"d": 24}, {"k": 9}, {"method": "VC"}])
def test_shapes_outside_the_route_raise(kw):
    a = {"method": "VD", "m": 20, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    X, Psi = catalogue(model, 40, seed=6), noise(40, a["d"], seed=7)
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.predict_dev(dev(X), Psi=dev(Psi))
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.draws_dev(dev(X), 4, Psi=dev(Psi))
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.draws(X, 4, Psi=Psi)
        # the C entries refuse it themselves and name the condition
        muX, sdX, muY = p._norm_vectors()
        Xd, Pd = dev(X), dev(Psi)
        out = [torch.empty((a["k"], 40), dtype=torch.float64, device=DEV).T for _ in range(5)]
        h = p._handle()
        with pytest.raises(_lib.GpzError, match="predict_noisy_fits") as ei:
            _lib.check(p._lib.gpz_predictor_run_noisy_dev(h, *p._x_args(Xd), *p._psi_args(Pd, 40), _lib.dptr(muX), _lib.dptr(sdX),
                                                          _lib.dptr(np.ascontiguousarray(sdX ** 2)), _lib.dptr(muY),
                                                          *(t.data_ptr() for t in out), None))
        assert ei.value.code == -5                                       # GPZ_ERR_UNSUPPORTED
        assert len(p.predict_dev(Xd)) == 5 and "noise" not in p.route    # and stays on its current route


# ---- 4. the same bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,m,k", [("VD", 100, 1), ("GL", 130, 3)])
def test_same_bits_over_tiles_and_row_orders(method, m, k):
    n, d, nd = 3000, 5, 5
    model = synth_model(method, m, d, k, True, seed=40 + m)
    X, Psi = catalogue(model, n, seed=41), noise(n, d, seed=42)
    perm = np.random.default_rng(43).permutation(n)
    Xd, Pd, pd = dev(X), dev(Psi), torch.from_numpy(perm).to(DEV)
    outs = []
    for tile in (64, 1000, None):
        with gpz_amd.Predictor(model, tile_rows=tile) as p:
            outs.append(tuple(p.predict_dev(Xd, Psi=Pd)) + (p.draws_dev(Xd, nd, seed=9, Psi=Pd),))
            if tile == 1000:
                shuf = tuple(p.predict_dev(Xd[pd], Psi=Pd[pd])) + (p.draws_dev(Xd[pd], nd, seed=9, Psi=Pd[pd]),)
                Fh = p.draws(X, nd, seed=9, Psi=Psi)
                Fh1 = p.draws(X, nd, seed=9, Psi=Psi[:, :1])
                Fd1 = p.draws_dev(Xd, nd, seed=9, Psi=Pd[:, :1])
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    assert all(torch.equal(a, b[pd]) for a, b in zip(shuf[:5], outs[0][:5]))
    assert torch.equal(shuf[5], outs[0][5][:, pd])
    assert np.array_equal(Fh, host(outs[0][5]))                          # the host draws: the same bits
    assert np.array_equal(Fh1, host(Fd1))


# ---- 5. Psi = 0 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,k", [("VD", 1), ("GD", 3)])
def test_zero_noise_is_the_noise_free_prediction(method, k):
    """mu and beta_i at nrel <= 1e-12, |gamma| <= 1e-11 |mu^2|.  nu sums the lower triangle of iSigma_w doubled, as the reference does, so
    it is the noise-free nu of the model with iSigma_w = tril(iS) + tril(iS, -1)' (the test models' iSigma_w is not symmetric); the gate
    is the parity test's 1e-11: with Psi = 0 a pair term exp(lnZ_ab - q / 2) prod r equals phi_a phi_b up to the rounding of exponents
    of size <= 1e2, a few 1e-14, and both sides add m^2 / 2 such terms."""
    n, d, m = 500, 5, 60
    model = synth_model(method, m, d, k, True, seed=60 + k)
    X = catalogue(model, n, seed=61)
    iS = model.sets["best"]["iSigma_w"]
    sym = synth_model(method, m, d, k, True, seed=60 + k)
    sym.sets["best"]["iSigma_w"] = np.stack([np.tril(iS[:, :, o]) + np.tril(iS[:, :, o], -1).T for o in range(k)], axis=2)
    Xd = dev(X)
    with gpz_amd.Predictor(model) as p, gpz_amd.Predictor(sym) as ps:
        z = p.predict_dev(Xd, Psi=torch.zeros((n, d), dtype=torch.float64, device=DEV))
        f = p.predict_dev(Xd)
        fs = ps.predict_dev(Xd)
    assert nrel(host(z[0]), host(f[0])) <= 1e-12 and nrel(host(z[3]), host(f[3])) <= 1e-12
    mu0 = host(z[0]) - model.muY
    assert np.linalg.norm(host(z[4])) <= 1e-11 * np.linalg.norm(mu0 ** 2), np.linalg.norm(host(z[4])) / np.linalg.norm(mu0 ** 2)
    assert nrel(host(z[2]), host(fs[2])) <= 1e-11, nrel(host(z[2]), host(fs[2]))
    assert nrel(host(z[2]), host(f[2])) > 1e-6                            # (the unsymmetrised model's nu is another number)


# ---- 6. draws with Psi ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_draws_are_an_exact_square_root_under_noise(k):
    n, d, m = 200, 4, 30
    model = synth_model("VD", m, d, k, True, seed=70 + k)
    X, Psi = catalogue(model, n, seed=71), noise(n, d, seed=72)
    Xd, Pd = dev(X), dev(Psi)
    iS = model.sets["best"]["iSigma_w"]
    with gpz_amd.Predictor(model) as p:
        PHI = p.predict(X, Psi=Psi, return_phi=True)[5]
        mu = host(p.predict_dev(Xd, Psi=Pd)[0])
        eye = np.stack([np.eye(m)] * k, axis=2)
        F = host(p.draws_dev(Xd, m, Z=eye, Psi=Pd))                      # (m, n, k)
        for o in range(k):
            D = F[:, :, o] - mu[:, o]
            S = 0.5 * (iS[:, :, o] + iS[:, :, o].T)
            assert nrel(D.T @ D, PHI @ S @ PHI.T) <= 1e-10, nrel(D.T @ D, PHI @ S @ PHI.T)
        F0 = host(p.draws_dev(Xd, 3, Z=np.zeros((m, 3, k)), Psi=Pd))
        assert all(nrel(F0[s], mu) <= 1e-12 for s in range(3))
        seeded = host(p.draws_dev(Xd, 7, seed=12345, Psi=Pd))
        given = host(p.draws_dev(Xd, 7, Z=philox_normals(12345, m, 7, k), Psi=Pd))
        assert nrel(seeded, given) <= 1e-12
        assert nrel(p.draws(X, 7, seed=12345, Psi=Psi), given) <= 1e-12
        assert not np.array_equal(seeded, host(p.draws_dev(Xd, 7, seed=12345)))   # (and they are not the noise-free draws)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_bad_rows_and_bad_noise_are_refused_with_the_outputs_untouched():
    n, d, k, nd = 70_000, 5, 2, 3
    model = synth_model("VD", 20, d, k, True, seed=85)
    X, Psi = dev(catalogue(model, n, seed=86)), dev(noise(n, d, seed=87))
    with gpz_amd.Predictor(model, tile_rows=1 << 14) as p:
        good = p.predict_dev(X[:500], Psi=Psi[:500])
        muX, sdX, muY = p._norm_vectors()
        sd2 = np.ascontiguousarray(sdX ** 2)
        stream = torch.cuda.current_stream(X.device).cuda_stream

        def raw(x, psi):
            out = [torch.full((k, n), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
            F = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
            rc1 = p._lib.gpz_predictor_run_noisy_dev(p._handle(), *p._x_args(x), *p._psi_args(psi, n), _lib.dptr(muX), _lib.dptr(sdX),
                                                     _lib.dptr(sd2), _lib.dptr(muY), *(t.data_ptr() for t in out), stream)
            rc2 = p._lib.gpz_predictor_draws_noisy_dev(p._handle(), *p._x_args(x), *p._psi_args(psi, n), _lib.dptr(muX), _lib.dptr(sdX),
                                                       _lib.dptr(sd2), _lib.dptr(muY), nd, 5, None, F.data_ptr(), stream)
            torch.cuda.synchronize()
            return rc1, rc2, out + [F]

        rc1, rc2, outs = raw(X, Psi)
        assert rc1 == 0 and rc2 == 0 and all(bool((t != -7.0).all()) for t in outs)
        bad_x = X.clone()
        bad_x[60_001, 3] = float("nan")
        for what, x, psi, code in [("NaN in X", bad_x, Psi, -5)] + [
                (f"Psi {v}", X, Psi.clone().index_put_((torch.tensor([at], device=DEV), torch.tensor([c], device=DEV)),
                                                     torch.tensor([v], dtype=torch.float64, device=DEV)), -1)
                for v, at, c in ((float("nan"), 69_999, 4), (float("inf"), 0, 0), (-1e-300, 33_333, 2))]:
            rc1, rc2, outs = raw(x, psi)
            assert rc1 == code and rc2 == code, (what, rc1, rc2)
            assert all(bool((t == -7.0).all()) for t in outs), what         # refused before any tile kernel has run
            with pytest.raises(_lib.GpzError):
                p.predict_dev(x, Psi=psi)
            with pytest.raises(_lib.GpzError):
                p.draws_dev(x, nd, Psi=psi)
            again = p.predict_dev(X[:500], Psi=Psi[:500])                    # the handle works on the next call
            assert all(torch.equal(a, b) for a, b in zip(again, good))
        one = Psi[:, :1].clone()                                             # the broadcast column is scanned too
        one[12_345, 0] = -1.0
        with pytest.raises(_lib.GpzError, match="Psi"):
            p.predict_dev(X, Psi=one)


# ---- 8. memory --------------------------------------------------------------------------------------------------------------------------------
def test_memory_is_added_once_and_never_grows_with_the_rows():
    d, nd = 5, 4
    model = synth_model("VD", 100, d, 1, True, seed=95)
    n = 300_000
    gen = torch.Generator(device=DEV).manual_seed(96)
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=gen) * torch.from_numpy(model.sdX).to(DEV) + \
        torch.from_numpy(model.muX).to(DEV)
    Psi = 0.05 * torch.rand((n, d), dtype=torch.float64, device=DEV, generator=gen)
    with gpz_amd.Predictor(model, tile_rows=1 << 16) as p, gpz_amd.Predictor(model, tile_rows=1 << 16) as q:
        q.predict_dev(X[:1000]); q.draws_dev(X[:1000], nd)                   # a handle that never sees Psi ...
        p.predict_dev(X[:1000]); p.draws_dev(X[:1000], nd)
        held = p.info[1]
        assert held == q.info[1]
        p.predict_dev(X[:2000]); p.draws_dev(X[:2000], nd)
        assert p.info[1] == held                                             # ... holds what it held: no-Psi calls add nothing
        small = p.predict_dev(X[:1000], Psi=Psi[:1000])
        first = p.info[1]
        assert first > held
        out = p.predict_dev(X, Psi=Psi)
        assert p.info[1] == first                                            # 300 000 rows in 65 536-row tiles: the same bytes
        assert all(torch.equal(a, b[:1000]) for a, b in zip(small, out))
        p.draws_dev(X[:1000], nd, Psi=Psi[:1000])
        drawn = p.info[1]
        p.draws_dev(X, nd, Psi=Psi)
        assert p.info[1] == drawn == first                                   # the draws with Psi use the slots that are there
        assert q.info[1] == held
        q.draws_dev(X[:1000], nd, Psi=Psi[:1000])                            # draws alone take the Psi slots, not the pair table
        assert "noise" not in q.route and held < q.info[1] < first
