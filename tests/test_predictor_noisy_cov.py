"""Input noise for the covariance kinds on the predictor handle (Predictor.predict_noisy_cov_dev / draws_noisy_cov_dev,
k_predict_noisy_cov.hip) against the one-shot predictNoisy route and the oracle: parity over GC and VC, every width, every block, stage
and chunk edge, every row count, the same bits over tile sizes, row orders and splits, every layout of X and Psi, the edges of Psi, the
draws as an exact square root, the refusals and constant memory.

The gates against ``predict`` were measured on an MI355X at the shapes of this file before they were set (each test prints its figures
first): ten times the largest value seen, rounded up to a power of ten, and never looser than 1e-9."""

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, nrel, synth_model
from test_predictor_draws_cpu import philox_normals
from test_predictor_noisy import NAMES, dev, host, noise
from test_predictor_noisy_cov_cpu import cov_chunks_rule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COV = ("GC", "VC")
# nrel of each output against predict(X, model, Psi=Psi).  Largest value measured over every comparison of this file (tests 1, 2, 3, 4 and
# 7): mu 8.3e-16, sigma 8.5e-14, nu 2.3e-15, beta_i 5.2e-16, gamma 7.3e-12 (gamma = the pair sum - mu^2 cancels most at d = 1 .. 2)
GATE = {"mu": 1e-14, "sigma": 1e-12, "nu": 1e-13, "beta_i": 1e-14, "gamma": 1e-10}
# Psi = 0 against the noise-free prediction: measured mu 3.1e-16, beta_i 2.3e-16, nu 1.6e-15, |gamma| / |mu^2| 1.4e-15
GATE_ZERO = 1e-13


def check_parity(out, ref, what):
    """The norm ratio on all five outputs, each printed before it is held against the gate."""
    for name, a, b in zip(NAMES, out, ref):
        a = host(a) if isinstance(a, torch.Tensor) else a
        assert a.shape == b.shape, (name, a.shape, b.shape)
        print(f"nrel {what} {name} {nrel(a, b):.3e}")
    for name, a, b in zip(NAMES, out, ref):
        a = host(a) if isinstance(a, torch.Tensor) else a
        assert nrel(a, b) <= GATE[name], (what, name, nrel(a, b))


def both(p, x, psi, nd=4, seed=4, **kw):
    return tuple(p.predict_noisy_cov_dev(x, psi, **kw)) + (p.draws_noisy_cov_dev(x, psi, nd, seed=seed, **kw),)


def same(a, b, what):
    for i, (s, t) in enumerate(zip(a, b)):
        assert s.shape == t.shape and torch.equal(s, t), (what, i, float((s - t).abs().max()))


# ---- 1. parity against the existing routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_parity_with_predict_and_the_oracle(method, hetero, k):
    """ns = 2500 over 1024-row tiles (the last one partial) against predict(X, model, Psi=Psi) on all five outputs; at m = 7, 60 rows
    against the oracle's predict_noisy at rel <= 1e-8."""
    d, ns = 5, 2500
    for m in (7, 50, 250):
        model = synth_model(method, m, d, k, hetero, seed=3000 * COV.index(method) + 100 * hetero + 10 * k + m)
        X = catalogue(model, ns, seed=m)
        Psi = noise(ns, d, seed=m + 1)
        ref = gpz_amd.predict(X, model, Psi=Psi)
        with gpz_amd.Predictor(model, tile_rows=1024) as p:
            out = p.predict_noisy_cov_dev(dev(X), dev(Psi))
            assert p.route.endswith(f"; noise: k_predict_noisy_cov_small ({cov_chunks_rule(m, d, k)} pair chunks)"), p.route
            check_parity(out, ref, f"parity {method} h{int(hetero)} k{k} m{m}")
            assert np.any(host(out[4]) != 0.0)
            if m == 7:
                orc = O.predict_noisy(X[:60], Psi[:60], model)
                sub = p.predict_noisy_cov_dev(dev(X[:60]), dev(Psi[:60]))
                for name, a, b in zip(NAMES, sub, orc):
                    print(f"rel oracle {method} h{int(hetero)} k{k} {name} {rel(host(a), b):.3e}")
                    assert rel(host(a), b) <= 1e-8, (name, rel(host(a), b))
                same(sub, [o[:60] for o in out], "the first rows of the whole call")


# ---- 2. every width ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
@pytest.mark.parametrize("d", range(1, 11))
def test_every_width(method, d):
    """m = 33: one full LDS stage and one record of basis functions, 561 pairs = 17 stages and an odd tail of 17."""
    n, m = 300, 33
    for k in (1, 8):
        model = synth_model(method, m, d, k, True, seed=400 + 20 * d + k + COV.index(method))
        X, Psi = catalogue(model, n, seed=d), noise(n, d, seed=d + 50)
        ref = gpz_amd.predict(X, model, Psi=Psi)
        with gpz_amd.Predictor(model) as p:
            check_parity(p.predict_noisy_cov_dev(dev(X), dev(Psi)), ref, f"width {method} d{d} k{k}")
            F = p.draws_noisy_cov_dev(dev(X), dev(Psi), 3, Z=np.zeros((m, 3, k)))
            assert nrel(host(F[1]), ref[0]) <= 1e-12, nrel(host(F[1]), ref[0])


# ---- 3. block, stage and chunk edges ---------------------------------------------------------------------------------------------------------
CHUNK_EDGES = [m for m in range(2, 257) if cov_chunks_rule(m, 3, 1) != cov_chunks_rule(m - 1, 3, 1)]


@pytest.mark.parametrize("m", sorted({1, 2, 15, 16, 17, 31, 32, 33, 255, 256} | {m + s for m in CHUNK_EDGES for s in (-1, 0)}))
def test_every_block_stage_and_chunk_edge(m):
    d, n, k = 3, 300, 1
    model = synth_model("VC", m, d, k, bool(m % 3), seed=800 + 10 * m)
    X, Psi = catalogue(model, n, seed=m), noise(n, d, seed=m + 50)
    ref = gpz_amd.predict(X, model, Psi=Psi)
    with gpz_amd.Predictor(model) as p:
        check_parity(p.predict_noisy_cov_dev(dev(X), dev(Psi)), ref, f"edge m{m}")
        assert f"k_predict_noisy_cov_small ({cov_chunks_rule(m, d, k)} pair chunks)" in p.route
        F = p.draws_noisy_cov_dev(dev(X), dev(Psi), 2, Z=np.zeros((m, 2, k)))
        assert nrel(host(F[0]), ref[0]) <= 1e-12, nrel(host(F[0]), ref[0])


# ---- 4. row counts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8])
def test_every_row_count(k):
    """n at the edges of the 64-lane waves, the 256-row workgroups and the 128-row tiles of the product: every shorter call is the first
    rows of the longest one bit for bit."""
    d, m = 5, 17
    model = synth_model("VC", m, d, k, True, seed=950 + k)
    X, Psi = catalogue(model, 257, seed=91), noise(257, d, seed=92)
    with gpz_amd.Predictor(model) as p:
        Xd, Pd = dev(X), dev(Psi)
        full = both(p, Xd, Pd)
        check_parity(full[:5], gpz_amd.predict(X, model, Psi=Psi), f"rows k{k}")
        for n in (1, 63, 64, 65, 255, 256, 257):
            out = both(p, Xd[:n], Pd[:n])
            assert all(o.shape == (n, k) for o in out[:5]) and out[5].shape == (4, n, k)
            same(out, [f[:n] for f in full[:5]] + [full[5][:, :n]], f"n = {n}")


# ---- 5. the same bits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,m,k", [("VC", 100, 1), ("GC", 130, 3)])
def test_same_bits_over_tiles_row_orders_and_splits(method, m, k):
    n, d = 2500, 5
    model = synth_model(method, m, d, k, True, seed=45 + m)
    X, Psi = catalogue(model, n, seed=46), noise(n, d, seed=47)
    perm = torch.from_numpy(np.random.default_rng(48).permutation(n)).to(DEV)
    Xd, Pd = dev(X), dev(Psi)
    outs = []
    for tile in (256, 1024, None):
        with gpz_amd.Predictor(model, tile_rows=tile) as p:
            outs.append(both(p, Xd, Pd))
            if tile == 1024:
                shuf = both(p, Xd[perm], Pd[perm])
                cut = 1100
                halves = [both(p, Xd[:cut], Pd[:cut]), both(p, Xd[cut:], Pd[cut:])]
    for o in outs[1:]:
        same(o, outs[0], "tile sizes")
    same(shuf[:5], [t[perm] for t in outs[0][:5]], "a permutation of the rows")
    assert torch.equal(shuf[5], outs[0][5][:, perm])
    same([torch.cat([a, b], dim=0) for a, b in zip(halves[0][:5], halves[1][:5])], outs[0][:5], "two calls")
    assert torch.equal(torch.cat([halves[0][5], halves[1][5]], dim=1), outs[0][5])


# ---- 6. layouts --------------------------------------------------------------------------------------------------------------------------------
def test_layouts_of_x_and_psi_give_the_same_bits():
    """float32, a transposed view, a row-sliced view, Psi as (n, 1) and (n,), a selection: each is the call on a contiguous float64 copy of
    the same values, bit for bit."""
    n, d = 700, 5
    model = synth_model("VC", 40, d, 2, True, seed=181)
    X32 = catalogue(model, 2 * n, seed=182).astype(np.float32)
    P32 = noise(2 * n, d, seed=183).astype(np.float32)
    Xd, Pd = dev(X32.astype(np.float64)), dev(P32.astype(np.float64))                  # the rounded values as float64
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        ref = both(p, Xd.contiguous(), Pd.contiguous())
        same(both(p, dev(X32, torch.float32), dev(P32, torch.float32)), ref, "float32")
        same(both(p, Xd, dev(P32, torch.float32)), ref, "float32 Psi")
        same(both(p, Xd.T.contiguous().T, Pd.T.contiguous().T), ref, "transposed views")
        same(both(p, Xd.T.contiguous().T, Pd), ref, "mixed layouts")
        half = both(p, Xd[::2].contiguous(), Pd[::2].contiguous())
        same(both(p, Xd[::2], Pd[::2]), half, "row-sliced views")
        same([t[::2] if t.dim() == 2 else t[:, ::2] for t in ref], half, "rows of the whole call")
        col = Pd[:, 2].contiguous()
        bc = both(p, Xd, col[:, None].expand(2 * n, d).contiguous())
        same(both(p, Xd, col[:, None]), bc, "Psi (n, 1)")
        same(both(p, Xd, col), bc, "Psi (n,)")
        same(both(p, Xd, Pd[:, 2]), bc, "Psi (n,) strided")
        sel = torch.zeros(2 * n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        same(both(p, Xd, Pd, selection=sel), half, "selection")


# ---- 7. the edges of Psi -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,k", [("VC", 1), ("GC", 3)])
def test_zero_noise_is_the_noise_free_prediction(method, k):
    """mu and beta_i against predict_dev(X); nu sums the lower triangle of iSigma_w doubled, as the reference does, so it is the noise-free
    nu of the model with iSigma_w = tril(iS) + tril(iS, -1)' (the test models' iSigma_w is not symmetric); gamma ~ 0 against mu^2."""
    n, d, m = 500, 5, 60
    model = synth_model(method, m, d, k, True, seed=160 + k)
    X = catalogue(model, n, seed=161)
    iS = model.sets["best"]["iSigma_w"]
    sym = synth_model(method, m, d, k, True, seed=160 + k)
    sym.sets["best"]["iSigma_w"] = np.stack([np.tril(iS[:, :, o]) + np.tril(iS[:, :, o], -1).T for o in range(k)], axis=2)
    Xd = dev(X)
    with gpz_amd.Predictor(model) as p, gpz_amd.Predictor(sym) as ps:
        z = p.predict_noisy_cov_dev(Xd, torch.zeros((n, d), dtype=torch.float64, device=DEV))
        f = p.predict_dev(Xd)
        fs = ps.predict_dev(Xd)
    mu0 = host(z[0]) - model.muY
    fig = {"mu": nrel(host(z[0]), host(f[0])), "beta_i": nrel(host(z[3]), host(f[3])), "nu": nrel(host(z[2]), host(fs[2])),
           "gamma": float(np.linalg.norm(host(z[4])) / np.linalg.norm(mu0 ** 2))}
    for name, v in fig.items():
        print(f"zero {method} k{k} {name} {v:.3e}")
    assert all(v <= GATE_ZERO for v in fig.values()), fig
    assert nrel(host(z[2]), host(f[2])) > 1e-6                            # (the unsymmetrised model's nu is another number)


@pytest.mark.parametrize("method", COV)
def test_noise_that_is_zero_in_some_dimensions_and_huge_in_one(method):
    n, d, m, k = 400, 5, 45, 2
    model = synth_model(method, m, d, k, True, seed=170)
    X, Psi = catalogue(model, n, seed=171), noise(n, d, seed=172)
    Psi[:, 1] = 0.0
    Psi[::3, 3] = 0.0
    Psi[:, 4] = 1e6
    ref = gpz_amd.predict(X, model, Psi=Psi)
    with gpz_amd.Predictor(model) as p:
        out = both(p, dev(X), dev(Psi))
    assert all(bool(torch.isfinite(t).all()) for t in out)
    check_parity(out[:5], ref, f"psi edges {method}")


# ---- 8. draws ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_draws_are_an_exact_square_root_under_noise(k):
    n, d, m = 200, 4, 30
    model = synth_model("VC", m, d, k, True, seed=270 + k)
    X, Psi = catalogue(model, n, seed=271), noise(n, d, seed=272)
    Xd, Pd = dev(X), dev(Psi)
    iS = model.sets["best"]["iSigma_w"]
    with gpz_amd.Predictor(model) as p:
        PHI = p.predict(X, Psi=Psi, return_phi=True)[5]
        mu = host(p.predict_noisy_cov_dev(Xd, Pd)[0])
        eye = np.stack([np.eye(m)] * k, axis=2)
        F = host(p.draws_noisy_cov_dev(Xd, Pd, m, Z=eye))                 # (m, n, k)
        for o in range(k):
            D = F[:, :, o] - mu[:, o]
            S = 0.5 * (iS[:, :, o] + iS[:, :, o].T)
            assert nrel(D.T @ D, PHI @ S @ PHI.T) <= 1e-10, nrel(D.T @ D, PHI @ S @ PHI.T)
        F0 = host(p.draws_noisy_cov_dev(Xd, Pd, 3, Z=np.zeros((m, 3, k))))
        assert all(nrel(F0[s], mu) <= 1e-12 for s in range(3))
        seeded = host(p.draws_noisy_cov_dev(Xd, Pd, 7, seed=12345))
        given = host(p.draws_noisy_cov_dev(Xd, Pd, 7, Z=philox_normals(12345, m, 7, k)))
        assert nrel(seeded, given) <= 1e-12, nrel(seeded, given)
        assert not np.array_equal(seeded, host(p.draws_dev(Xd, 7, seed=12345)))   # (and they are not the noise-free draws)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------------
def raw_entries(p, x, psi, k, nd=3):
    """Both C entries on outputs pre-filled with a sentinel: the return codes and the outputs."""
    n = x.shape[0]
    muX, sdX, muY = p._norm_vectors()
    sd2 = np.ascontiguousarray(sdX ** 2)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    out = [torch.full((k, n), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
    F = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    lead = (p._handle(), *p._x_args(x), *p._psi_args(psi, n), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(sd2), _lib.dptr(muY))
    rc1 = p._lib.gpz_predictor_run_noisy_cov_dev(*lead, *(t.data_ptr() for t in out), stream)
    msg1 = p._lib.gpz_last_error().decode() if rc1 else ""
    rc2 = p._lib.gpz_predictor_draws_noisy_cov_dev(*lead, nd, 5, None, F.data_ptr(), stream)
    msg2 = p._lib.gpz_last_error().decode() if rc2 else ""
    torch.cuda.synchronize()
    return (rc1, rc2), (msg1, msg2), out + [F]


@pytest.mark.parametrize("kw", [{"method": "VD"}, {"d": 12}, {"m": 300}, {"k": 9}])
def test_shapes_outside_the_route_raise(kw):
    a = {"method": "VC", "m": 20, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    X, Psi = dev(catalogue(model, 40, seed=6)), dev(noise(40, a["d"], seed=7))
    text = "predict_dev" if a["method"] == "VD" else "predict_noisy_cov_fits"
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match=text):
            p.predict_noisy_cov_dev(X, Psi)
        with pytest.raises(ValueError, match=text.replace("predict_dev", "draws_dev")):
            p.draws_noisy_cov_dev(X, Psi, 4)
        rcs, msgs, outs = raw_entries(p, X, Psi, a["k"])                  # the C entries refuse it themselves and name the condition
        assert rcs == (-5, -5), rcs                                       # GPZ_ERR_UNSUPPORTED
        assert all("predict_noisy_cov_fits" in t for t in msgs), msgs
        assert all(bool((t == -7.0).all()) for t in outs)
        assert len(p.predict_dev(X)) == 5 and "noise" not in p.route      # and the handle stays on its current route


def test_the_old_spellings_still_refuse_a_covariance_kind():
    model = synth_model("VC", 20, 5, 1, True, seed=5)
    X, Psi = catalogue(model, 40, seed=6), noise(40, 5, seed=7)
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.predict_dev(dev(X), Psi=dev(Psi))
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.draws_dev(dev(X), 4, Psi=dev(Psi))
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.draws(X, 4, Psi=Psi)
        assert len(p.predict_noisy_cov_dev(dev(X), dev(Psi))) == 5        # the new one takes the same rows


def test_bad_rows_and_bad_noise_are_refused_with_the_outputs_untouched():
    n, d, k = 5000, 5, 2
    model = synth_model("VC", 20, d, k, True, seed=185)
    X, Psi = dev(catalogue(model, n, seed=186)), dev(noise(n, d, seed=187))
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        good = p.predict_noisy_cov_dev(X[:500], Psi[:500])
        rcs, _, outs = raw_entries(p, X, Psi, k)
        assert rcs == (0, 0) and all(bool((t != -7.0).all()) for t in outs)
        bad_x = X.clone()
        bad_x[4001, 3] = float("nan")
        cases = [("NaN in X", bad_x, Psi, -5)]
        for v, at, c in ((float("nan"), 4999, 4), (float("inf"), 0, 0), (-1e-300, 3333, 2)):
            bad = Psi.clone()
            bad[at, c] = v
            cases.append((f"Psi {v}", X, bad, -1))                        # GPZ_ERR_ARG
        for what, x, psi, code in cases:
            rcs, _, outs = raw_entries(p, x, psi, k)
            assert rcs == (code, code), (what, rcs)
            assert all(bool((t == -7.0).all()) for t in outs), what        # refused before any tile kernel has run
            with pytest.raises(_lib.GpzError):
                p.predict_noisy_cov_dev(x, psi)
            with pytest.raises(_lib.GpzError):
                p.draws_noisy_cov_dev(x, psi, 3)
            same(p.predict_noisy_cov_dev(X[:500], Psi[:500]), good, "the handle works on the next call")
        one = Psi[:, :1].clone()                                           # the broadcast column is scanned too
        one[1234, 0] = -1.0
        with pytest.raises(_lib.GpzError, match="Psi"):
            p.predict_noisy_cov_dev(X, one)


# ---- 10. memory and route --------------------------------------------------------------------------------------------------------------------------
def test_memory_is_added_once_and_never_grows_with_the_rows():
    d, nd, m, k = 5, 4, 60, 1
    model = synth_model("VC", m, d, k, True, seed=195)
    X, Psi = dev(catalogue(model, 5000, seed=196)), dev(noise(5000, d, seed=197))
    with gpz_amd.Predictor(model, tile_rows=1024) as p, gpz_amd.Predictor(model, tile_rows=1024) as q:
        q.predict_dev(X[:300]); q.draws_dev(X[:300], nd)                    # a handle that never sees the new entries ...
        p.predict_dev(X[:300]); p.draws_dev(X[:300], nd)
        held = p.info[1]
        assert held == q.info[1]
        p.predict_dev(X); p.draws_dev(X, nd)
        assert p.info[1] == held and "noise" not in p.route                 # ... holds what it held
        small = p.predict_noisy_cov_dev(X[:300], Psi[:300])
        first = p.info[1]
        assert first > held
        assert p.route.endswith(f"; noise: k_predict_noisy_cov_small ({cov_chunks_rule(m, d, k)} pair chunks)"), p.route
        out = p.predict_noisy_cov_dev(X, Psi)
        assert p.info[1] == first                                           # 300 rows or 5000: the same bytes
        same(small, [t[:300] for t in out], "the first rows")
        p.draws_noisy_cov_dev(X[:300], Psi[:300], nd)
        drawn = p.info[1]
        p.draws_noisy_cov_dev(X, Psi, nd)
        assert p.info[1] == drawn
        p.predict_noisy_cov_dev(X, Psi)
        assert p.info[1] == drawn
        assert q.info[1] == held
        q.draws_noisy_cov_dev(X[:300], Psi[:300], nd)                       # draws alone take no pair records and no chunk slab
        assert "noise" not in q.route and held < q.info[1] < drawn
