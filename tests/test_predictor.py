"""The streaming predictor (gpz_amd.Predictor over gpz_predictor_*) against predict(): parity on both routes over every method, the route
each shape takes, bit-for-bit reproducibility over tile sizes and row orders, a multi-tile stream with constant device memory, every
branch on the frozen fixtures, and the edge cases."""

import numpy as np
import pytest

import gpz_amd
from gpz_amd import _lib
from helpers import golden_names, load_predict_golden, rel

pytestmark = pytest.mark.gpu

METHODS = ("GL", "VL", "GD", "VD", "GC", "VC")


def nrel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def synth_model(method, m, d, k, hetero, seed):
    """A model with a well-conditioned random parameter set (no training needed for a comparison of two prediction paths).
    inv(Sigma_w) is deliberately not symmetric, so a transposed operand shows."""
    rng = np.random.default_rng(seed)
    model = gpz_amd.Model(m=m, d=d, k=k, method=method, heteroscedastic=hetero)
    P = rng.standard_normal((m, d))
    if method[1] == "C":
        blocks = 1 if method == "GC" else m
        G = np.concatenate([(0.6 * np.eye(d) + 0.08 * rng.standard_normal((d, d))).ravel(order="F") for _ in range(blocks)])
    else:
        G = rng.uniform(0.4, 0.9, model.g_dim)
    parts = [P.ravel(order="F"), G, rng.uniform(-1, 1, m * k), rng.uniform(-3, -1, k)]
    if hetero:
        parts += [0.05 * rng.standard_normal(m * k), rng.uniform(-1, 1, m * k)]
    theta = np.concatenate(parts)
    A = rng.standard_normal((m, m)) / np.sqrt(m)
    iS = np.stack([0.05 * (A @ A.T) + 0.02 * np.eye(m) + 1e-3 * rng.standard_normal((m, m)) for _ in range(k)], axis=2)
    model.muX = rng.standard_normal(d)
    model.sdX = rng.uniform(0.5, 2.0, d)
    model.muY = rng.standard_normal(k)
    model.sets["best"] = {"theta": theta, "w": rng.standard_normal((m, k)), "iSigma_w": iS}
    model.sets["last"] = {"theta": theta.copy(), "w": 0.5 * rng.standard_normal((m, k)), "iSigma_w": iS[:, ::-1, :].copy()}
    return model


def catalogue(model, n, seed):
    rng = np.random.default_rng(seed)
    return model.muX + model.sdX * rng.standard_normal((n, model.d))


def fused_fits(m, k, d=5):
    return ((m + 2 * k + 15) // 16) * 16 <= 256 and d <= 20 and k <= 8


def check_parity(out, ref, phi=None):
    mu, sigma, nu, beta, gamma = out[:5]
    assert nrel(mu, ref[0]) <= 1e-12 and nrel(beta, ref[3]) <= 1e-12, (nrel(mu, ref[0]), nrel(beta, ref[3]))
    assert nrel(nu, ref[2]) <= 1e-11, nrel(nu, ref[2])
    assert nrel(sigma, ref[1]) <= 1e-11
    assert np.all(gamma == 0.0)
    if phi is not None:
        assert nrel(phi, ref[5]) <= 1e-13, nrel(phi, ref[5])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_parity_and_route(method, hetero, k):
    """Complete rows, ns = 2500 over 1024-row tiles (the last one partial), m on both sides of the fused-route boundary."""
    d, ns = 5, 2500
    for m in (7, 50, 200, 256 - 2 * k, 257 - 2 * k, 1000):
        model = synth_model(method, m, d, k, hetero, seed=1000 * METHODS.index(method) + 100 * hetero + 10 * k + m)
        X = catalogue(model, ns, seed=m)
        ref = gpz_amd.predict(X, model)
        with gpz_amd.Predictor(model, tile_rows=1024) as p:
            assert p.info[2] == (0 if fused_fits(m, k) else 1), (m, k, p.route)
            check_parity(p.predict(X), ref)
            out = p.predict(X, return_phi=True)
            check_parity(out, ref, phi=out[5])
        if m in (50, 200):   # the tile route where the fused kernel fits: same answers
            with gpz_amd.Predictor(model, tile_rows=1024, force_tiles=True) as p:
                assert p.info[2] == 1
                check_parity(p.predict(X), ref)


def test_wide_inputs_take_the_tile_route():
    """d = 24 has no instantiated PHI kernel (runtime-d route): tiles, whatever m."""
    model = synth_model("VD", 40, 24, 1, True, seed=3)
    X = catalogue(model, 1500, seed=4)
    ref = gpz_amd.predict(X, model)
    with gpz_amd.Predictor(model, tile_rows=1000) as p:
        assert p.info[2] == 1
        check_parity(p.predict(X), ref)


@pytest.mark.parametrize("method", ["VD", "VC"])
def test_same_bits_for_every_tile_size_and_row_order(method):
    model = synth_model(method, 100, 10, 2, True, seed=7)
    X = catalogue(model, 5000, seed=8)
    outs = []
    for tr in (64, 1000, None):
        with gpz_amd.Predictor(model, tile_rows=tr) as p:
            assert p.info[2] == 0
            outs.append(p.predict(X))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)
    perm = np.random.default_rng(9).permutation(X.shape[0])
    with gpz_amd.Predictor(model) as p:
        op = p.predict(X[perm])
    for a, b in zip(outs[0], op):
        assert np.array_equal(a[perm], b)


def test_stream_of_many_tiles_in_constant_device_memory():
    model = synth_model("VD", 100, 5, 1, True, seed=11)
    X = catalogue(model, 3_000_000, seed=12)
    with gpz_amd.Predictor(model, tile_rows=1 << 16) as p:
        p.predict(X[:1000])
        held = p.info[1]
        out = p.predict(X)
        assert p.info[1] == held and p.info[3] == 2
    sub = np.sort(np.random.default_rng(13).choice(X.shape[0], 20_000, replace=False))
    ref = gpz_amd.predict(X[sub], model)
    check_parity([o[sub] for o in out], ref)


@pytest.mark.parametrize("name", golden_names("p_"))
def test_predict_golden_through_the_predictor(name):
    """The frozen predict() cases (full / noisy / missing / noisy + missing, mixed NaN patterns) at the gate of
    test_predict_golden_through_c_abi."""
    g, model, Psi = load_predict_golden(name)
    with gpz_amd.Predictor(model) as p:
        out = p.predict(g["Xs"], Psi=Psi, return_phi=True)
    for i, key in enumerate(("mu", "sigma", "nu", "beta_i", "gamma", "PHI")):
        assert rel(out[i], g[key]) <= 1e-8, key


def _reference_run():
    import test_reference_run as RR
    return RR


@pytest.mark.parametrize("name", golden_names("ref_predict_"))
def test_executed_reference_predict_through_the_predictor(name):
    """What the reference's predict.m returned, at the gates of test_hip_path_against_the_executed_reference_predict."""
    RR = _reference_run()
    g = RR.load(name)
    model, Xs, Psi = RR.predict_inputs(g)
    with gpz_amd.Predictor(model) as p:
        out = p.predict(Xs, Psi=Psi, return_phi=True)
    tol = max(1e-8, 2000.0 * RR.cov_cond(model, g["theta"]) * 2.2e-16)
    for key, val in zip(("mu", "sigma", "nu", "beta_i", "gamma", "PHIs"), out):
        assert rel(val, g[key]) <= tol, (key, rel(val, g[key]))


def test_executed_demos_through_the_predictor():
    RR = _reference_run()
    z = RR.load("ref_train_demo_sinc")
    model = RR.demo_model(z, gpz_amd.Model)
    with gpz_amd.Predictor(model) as p:
        out = p.predict(z["Xs"], return_phi=True)
        for key, val in zip(("mu", "sigma", "nu", "beta_i", "gamma"), out):
            assert rel(val, z["grid_" + key]) <= 1e-8, key
        te = z["testing"].astype(bool)
        mu, sigma = p.predict(z["X"], Psi=z["Psi"], selection=te)[:2]
        assert rel(mu, z["test_mu"]) <= 1e-8 and rel(sigma, z["test_sigma"]) <= 1e-8
    z = RR.load("ref_train_demo_2D")
    model = RR.demo_model(z, gpz_amd.Model)
    with gpz_amd.Predictor(model) as p:
        RR._demo_2d_predictions(z, lambda X, mdl: p.predict(X, return_phi=True), model, 1e-8)


@pytest.mark.parametrize("method", ["VD", "GC"])
def test_mixed_catalogue_row_for_row(method):
    """Complete rows, rows with missing values (three patterns) and, in the second call, input noise on every row: the complete group
    goes through the handle, the others through gpz_predict_missing - the result equals predict() row for row."""
    d, m = 4, 30
    model = synth_model(method, m, d, 2, True, seed=21)
    rng = np.random.default_rng(22)
    X = catalogue(model, 3000, seed=23)
    X[rng.random(3000) < 0.2, 1] = np.nan
    X[rng.random(3000) < 0.1, 3] = np.nan
    Psi = rng.gamma(1.0, 0.05, (3000, d))
    with gpz_amd.Predictor(model, tile_rows=1000) as p:
        for psi in (None, Psi):
            out = p.predict(X, Psi=psi, return_phi=True)
            ref = gpz_amd.predict(X, model, Psi=psi)
            for a, b in zip(out, ref[:6]):
                assert nrel(a, b) <= 1e-11
            full = ~np.isnan(X).any(axis=1)
            if psi is None:
                assert np.all(out[4][full] == 0.0)


def test_edge_cases():
    model = synth_model("VC", 20, 3, 2, True, seed=31)
    X = catalogue(model, 777, seed=32)
    with gpz_amd.Predictor(model) as p:
        one = p.predict(X[:1], return_phi=True)
        ref = gpz_amd.predict(X[:1], model)
        check_parity(one, ref, phi=one[5])
        empty = p.predict(X[:0], return_phi=True)
        assert [a.shape for a in empty] == [(0, 2)] * 5 + [(0, 20)]
        for n in (5, 777, 31, 32, 33, 1, 400, 64, 2, 500):   # one handle, ten calls of different sizes
            check_parity(p.predict(X[:n]), gpz_amd.predict(X[:n], model))
        assert p.info[3] == 11                                    # (ns = 0 never reaches the handle)
        # a NaN row straight to the C entry is refused
        lib = _lib.load()
        Xn = np.asfortranarray((X[:10] - model.muX) / model.sdX)
        Xn[4, 1] = np.nan
        o = [np.empty((10, 2), order="F") for _ in range(4)]
        rc = lib.gpz_predictor_run(p._handle(), _lib.dptr(Xn), 10, None, 0, *(_lib.dptr(a) for a in o), None)
        assert rc == -5                                                # GPZ_ERR_UNSUPPORTED
    with gpz_amd.Predictor(model, whichSet="last") as p:
        check_parity(p.predict(X), gpz_amd.predict(X, model, whichSet="last"))
    with pytest.raises(RuntimeError):
        p.predict(X)
    with pytest.raises(RuntimeError):
        p.info


def test_one_input_dimension():
    """d = 1: init rewrites the method to ?L (init.m:12-14); the handle runs the d = 1 kernels."""
    rng = np.random.default_rng(41)
    Xt = rng.uniform(-3, 3, (400, 1))
    Yt = np.sinc(Xt) + 0.05 * rng.standard_normal((400, 1))
    model = gpz_amd.init(Xt, Yt, "VC", 12)
    assert model.method == "VL"
    X = rng.uniform(-3, 3, (1000, 1))
    with gpz_amd.Predictor(model, whichSet="last") as p:
        assert p.info[2] == 0
        out = p.predict(X[:, 0], return_phi=True)
    ref = gpz_amd.predict(X, model, whichSet="last")
    check_parity(out, ref, phi=out[5])
