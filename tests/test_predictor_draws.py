"""Posterior draws of the predictive mean (gpz_amd.Predictor.draws over gpz_predictor_draws): the exact covariance of the draws against
predict()'s nu and PHI on both routes, the seeded normals against a NumPy Philox, bit reproducibility over tiles, row orders, calls and
draw counts, the eigen-factor of a semidefinite iSigma_w, a trained model, constant device memory over a stream, and the edge cases."""

import numpy as np
import pytest

import gpz_amd
from gpz_amd import _lib
from test_predictor import synth_model, catalogue, nrel
from test_predictor_draws_cpu import philox_normals

pytestmark = pytest.mark.gpu

METHODS = ("GL", "VL", "GD", "VD", "GC", "VC")


def eye_z(m, k):
    return np.repeat(np.eye(m)[:, :, None], k, axis=2)


def check_exact_covariance(p, model, X, tol):
    """Z = I_m: D_o = F_o - mu_o is PHI R_o, so sum_s D^2 = nu row for row and D_o' D_o = PHI S_o PHI'; Z = 0 gives mu."""
    m, k = model.m, model.k
    mu, _, nu, _, _, PHI = p.predict(X, return_phi=True)
    F = p.draws(X, m, Z=eye_z(m, k))
    assert F.shape == (m, X.shape[0], k)
    D = F - mu[None]
    assert nrel(np.sum(D * D, axis=0), nu) <= tol, nrel(np.sum(D * D, axis=0), nu)
    iS = np.asarray(model.sets["best"]["iSigma_w"]).reshape(m, m, k)
    for o in range(k):
        S = 0.5 * (iS[:, :, o] + iS[:, :, o].T)
        C = D[:, :, o].T @ D[:, :, o]
        assert nrel(C, PHI @ S @ PHI.T) <= tol, (o, nrel(C, PHI @ S @ PHI.T))
    F0 = p.draws(X, 3, Z=np.zeros((m, 3, k)))
    for s in range(3):
        assert nrel(F0[s], mu) <= 1e-12


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("force_tiles", [False, True])
def test_exact_covariance(method, hetero, k, force_tiles):
    """m on both sides of the fused kernel's limit (ceil16(m) <= 256); iSigma_w not symmetric, so only its symmetric part may show."""
    d, ns = 5, 700
    for m in (40, 264):
        model = synth_model(method, m, d, k, hetero, seed=100 * METHODS.index(method) + 10 * k + m + hetero)
        X = catalogue(model, ns, seed=m + k)
        with gpz_amd.Predictor(model, tile_rows=512, force_tiles=force_tiles) as p:
            check_exact_covariance(p, model, X, 1e-10)
            fused = m <= 256 and not force_tiles
            r = p.route
            assert ("draws: fused k_predict_draws" if fused else "draws: tiles k_phi + k_tgemm") in r, r
            assert r.endswith("factors:" + " cholesky" * k), r
            assert p.info[3] == 1                                        # runs: predict calls only


def test_exact_covariance_wide_inputs():
    model = synth_model("VD", 60, 24, 2, True, seed=5)                   # d > 20: the tile route
    X = catalogue(model, 500, seed=6)
    with gpz_amd.Predictor(model) as p:
        check_exact_covariance(p, model, X, 1e-10)
        assert "draws: tiles" in p.route


@pytest.mark.parametrize("m,force_tiles", [(50, False), (50, True), (300, False)])
def test_seeded_draws_are_the_numpy_philox(m, force_tiles):
    k = 2
    model = synth_model("GD", m, 4, k, True, seed=m)
    X = catalogue(model, 300, seed=1)
    with gpz_amd.Predictor(model, force_tiles=force_tiles) as p:
        for q in (0, 12345, 2 ** 64 - 1):
            a = p.draws(X, 7, seed=q)
            b = p.draws(X, 7, Z=philox_normals(q, m, 7, k))
            assert nrel(a, b) <= 1e-12, (q, nrel(a, b))


def test_sample_moments_of_many_draws():
    S = 4000
    model = synth_model("VC", 30, 3, 1, True, seed=9)
    X = catalogue(model, 64, seed=10)
    with gpz_amd.Predictor(model) as p:
        mu, _, nu = p.predict(X)[:3]
        F = p.draws(X, S, seed=77)[:, :, 0]
    sd = np.sqrt(nu[:, 0])
    assert np.all(np.abs(F.mean(0) - mu[:, 0]) <= 5 * sd / np.sqrt(S))
    assert np.all(np.abs(F.var(0) / nu[:, 0] - 1) <= 5 * np.sqrt(2 / S))


@pytest.mark.parametrize("method,force_tiles", [("VD", False), ("GC", False), ("VD", True)])
def test_same_bits_for_every_tile_row_order_and_split(method, force_tiles):
    model = synth_model(method, 50, 5, 2, True, seed=3)
    X = catalogue(model, 5000, seed=4)
    perm = np.random.default_rng(5).permutation(5000)
    runs = []
    for tile in (1000, 4096, None):
        with gpz_amd.Predictor(model, tile_rows=tile, force_tiles=force_tiles) as p:
            runs.append(p.draws(X, 16, seed=11))
            if tile is None:
                assert np.array_equal(p.draws(X[perm], 16, seed=11), runs[0][:, perm])
                split = np.concatenate([p.draws(X[:1234], 16, seed=11), p.draws(X[1234:], 16, seed=11)], axis=1)
                assert np.array_equal(split, runs[0])
                assert np.array_equal(p.draws(X, 8, seed=11), runs[0][:8])
                other = p.draws(X, 16, seed=12)
                assert np.mean(other == runs[0]) < 0.01
    for r in runs[1:]:
        assert np.array_equal(r, runs[0])


@pytest.mark.parametrize("m", [40, 264])
def test_semidefinite_isigma_takes_the_eigen_factor(m):
    k = 2
    model = synth_model("VD", m, 5, k, True, seed=m + 1)
    rng = np.random.default_rng(m)
    iS = np.empty((m, m, k))
    for o in range(k):
        A = rng.standard_normal((m, m // 2)) / np.sqrt(m)
        iS[:, :, o] = 0.05 * (A @ A.T)
    model.sets["best"]["iSigma_w"] = iS
    X = catalogue(model, 400, seed=2)
    with gpz_amd.Predictor(model) as p:
        check_exact_covariance(p, model, X, 1e-9)
        assert p.route.endswith("factors: eigen eigen"), p.route


def test_trained_model_draws_average_to_the_mean():
    import test_reference_run as RR
    z = RR.load("ref_train_demo_2D")
    model = RR.demo_model(z, gpz_amd.Model)
    S = 2000
    with gpz_amd.Predictor(model) as p:
        mu, _, nu = p.predict(z["Xs"])[:3]
        F = p.draws(z["Xs"], S, seed=2024)
    assert F.shape == (S,) + mu.shape
    assert np.all(np.abs(F.mean(0) - mu) <= 5 * np.sqrt(nu / S) + 1e-12)


def test_stream_of_draws_in_constant_device_memory():
    model = synth_model("VD", 100, 5, 1, True, seed=8)
    rng = np.random.default_rng(9)
    with gpz_amd.Predictor(model) as p:
        p.predict(catalogue(model, 1000, seed=1))
        b0 = p.info[1]
        with gpz_amd.Predictor(model) as q:                              # a predict-only handle holds the same bytes
            q.predict(catalogue(model, 10, seed=2))
            assert q.info[1] == b0
        X = catalogue(model, 500_000, seed=3)
        F = p.draws(X[:1000], 32, seed=1)
        b1 = p.info[1]
        assert b1 > b0
        for c in range(4):
            X = model.muX + model.sdX * rng.standard_normal((500_000, model.d))
            F = p.draws(X, 32, seed=1)
            assert F.shape == (32, 500_000, 1) and np.all(np.isfinite(F))
            assert p.info[1] == b1
        assert p.info[3] == 1


def test_edge_cases():
    model = synth_model("VC", 20, 3, 2, True, seed=31)
    X = catalogue(model, 100, seed=32)
    with gpz_amd.Predictor(model) as p:
        assert p.draws(X[:0], 5, seed=1).shape == (5, 0, 2)
        one = p.draws(X[:1], 5, seed=1)
        assert one.shape == (5, 1, 2)
        assert np.array_equal(one, p.draws(X, 5, seed=1)[:, :1])
        sel = np.zeros(100, dtype=bool)
        sel[[3, 50]] = True
        assert np.array_equal(p.draws(X, 5, seed=1, selection=sel), p.draws(X[sel], 5, seed=1))
        Xn = X.copy()
        Xn[7, 1] = np.nan
        with pytest.raises(ValueError, match="1 rows"):
            p.draws(Xn, 5)
        lib = _lib.load()
        Xc = np.asfortranarray((Xn[:10] - model.muX) / model.sdX)
        F = np.empty((10, 2, 5), order="F")
        assert lib.gpz_predictor_draws(p._handle(), _lib.dptr(Xc), 10, 5, 1, None, _lib.dptr(F)) == -5
        assert lib.gpz_predictor_draws(p._handle(), _lib.dptr(Xc), 10, 0, 1, None, _lib.dptr(F)) == -1
        assert lib.gpz_predictor_draws(p._handle(), _lib.dptr(Xc), 10, 8193, 1, None, _lib.dptr(F)) == -1
        assert p.info[3] == 0
    with pytest.raises(RuntimeError):
        p.draws(X, 5)
