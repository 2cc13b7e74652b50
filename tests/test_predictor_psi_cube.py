"""Rows with a full input-noise covariance on the predictor handle (Predictor.predict_psi_cube_dev / draws_psi_cube_dev /
stack_psi_cube_dev; k_predict_psi_cube.hip, k_predict_psi_cube_gamma.hip) against the one-shot route ``gpz_amd.predict(X, model,
Psi=cube)``, the oracle and the per-dimension entries of the handle: parity over GC and VC, a cube of diagonals as the per-dimension
route bit for bit, every width, every edge in m, every row count, the same bits over tiles, orders, splits and layouts, the draws and
gamma under every draw, the stack, the refusals on the device and constant memory.

The gates against ``predict`` were measured on an MI355X at the shapes of this file before they were set (each test prints its figures
first): ten times the largest value seen, rounded up to a power of ten, and never looser than 1e-9 (the rule of DESIGN.md section 26).
Largest values measured over tests 1, 3, 4 and 5: mu 1.4e-15, sigma 3.3e-14, nu 1.9e-15,
beta_i 3.4e-16, gamma 1.7e-13; the draws under Z = 0 against predict's mu 1.4e-15, gamma under such a draw against predict's gamma
1.7e-13; the oracle at m = 7 at most 6.6e-14 (gate 1e-8)."""
import copy

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from predict_edges import psi_cube, twin_psi
from test_predictor import catalogue, nrel, synth_model
from test_predictor_noisy import NAMES, dev, host, noise
from test_predictor_noisy_cov import GATE_ZERO
from test_predictor_noisy_cov_cpu import cov_chunks_rule
from test_predictor_stack import EPS, assert_close, setting
from test_predictor_stack_noisy_cpu import gamma_chunks_rule, stack_reference_w

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COV = ("GC", "VC")
# nrel of each output against predict(X, model, Psi=cube): ten times the largest value measured (the header), rounded up to a power of ten
GATE = {"mu": 1e-13, "sigma": 1e-12, "nu": 1e-13, "beta_i": 1e-14, "gamma": 1e-11}
# a draw under Z = 0 against predict's mu (measured 1.4e-15)
GATE_DRAW = 1e-13
# gamma_s of the model with w := w_s against that model's own gamma: the project's gamma gate for these kinds
GATE_GAMMA_S = 1e-10
ERR_ARG, ERR_UNSUPPORTED = -1, -5                                       # include/gpz_hip.h


def cube_of(n, d, seed):
    """u u' + diag(g) per row: exactly symmetric and positive definite, d x d x n."""
    return psi_cube(noise(n, d, seed), 0.3 * np.random.default_rng(seed + 7919).standard_normal((n, d)))


def check_parity(out, ref, what):
    """The norm ratio on all five outputs, each printed before it is held against the gate."""
    for name, a, b in zip(NAMES, out, ref):
        a = host(a) if isinstance(a, torch.Tensor) else a
        assert a.shape == b.shape, (name, a.shape, b.shape)
        print(f"nrel {what} {name} {nrel(a, b):.3e}")
    for name, a, b in zip(NAMES, out, ref):
        a = host(a) if isinstance(a, torch.Tensor) else a
        assert nrel(a, b) <= GATE[name], (what, name, nrel(a, b))


def three(p, x, psi, nd=4, seed=4, **kw):
    """The five moments, the draws and gamma under every draw."""
    return tuple(p.predict_psi_cube_dev(x, psi, **kw)) + tuple(p.draws_psi_cube_dev(x, psi, nd, seed=seed, return_gamma=True, **kw))


def same(a, b, what):
    for i, (s, t) in enumerate(zip(a, b)):
        assert s.shape == t.shape and torch.equal(s, t), (what, i, float((s - t).abs().max()))


def rows_of(out, idx):
    """Rows idx of the seven tensors of three(): (n, k) moments, (nd, n, k) draws and gamma."""
    return [t[idx] if t.dim() == 2 else t[:, idx] for t in out]


# ---- 1. parity against the existing routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_parity_with_predict_and_the_oracle(method, hetero, k):
    """ns = 2500 over 1024-row tiles (the last one partial) against predict(X, model, Psi=cube) on all five outputs; at m = 7, 60 rows
    against the oracle's predict_noisy at rel <= 1e-8."""
    d, ns = 5, 2500
    for m in (7, 50, 250):
        model = synth_model(method, m, d, k, hetero, seed=3100 * (1 + COV.index(method)) + 100 * hetero + 10 * k + m)
        X = catalogue(model, ns, seed=m)
        cube = cube_of(ns, d, seed=m + 1)
        ref = gpz_amd.predict(X, model, Psi=cube)
        with gpz_amd.Predictor(model, tile_rows=1024) as p:
            out = p.predict_psi_cube_dev(dev(X), dev(cube))
            assert p.route.endswith(f"; noise cube: k_predict_psi_cube_small ({cov_chunks_rule(m, d, k)} pair chunks)"), p.route
            assert "k_predict_noisy_cov_small" not in p.route           # the per-dimension kernel has not run on this handle
            check_parity(out, ref, f"parity {method} h{int(hetero)} k{k} m{m}")
            assert np.any(host(out[4]) != 0.0)
            if m == 7:
                orc = O.predict_noisy(X[:60], np.ascontiguousarray(cube[:, :, :60]), model)
                sub = p.predict_psi_cube_dev(dev(X[:60]), dev(cube[:, :, :60]))
                for name, a, b in zip(NAMES, sub, orc):
                    print(f"rel oracle {method} h{int(hetero)} k{k} {name} {rel(host(a), b):.3e}")
                    assert rel(host(a), b) <= 1e-8, (name, rel(host(a), b))
                same(sub, [o[:60] for o in out], "the first rows of the whole call")
                p.draws_psi_cube_dev(dev(X[:60]), dev(cube[:, :, :60]), 2, return_gamma=True)
                assert p.route.endswith(f"; noise cube per draw: k_predict_psi_cube_gamma ({gamma_chunks_rule(m)} pair chunks)"), p.route


# ---- 2. a cube of diagonals is the per-dimension route, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("method,d,m,k", [("VC", 5, 100, 1), ("GC", 10, 130, 3), ("VC", 1, 33, 8)])
def test_a_cube_of_diagonals_is_the_per_dimension_route_bit_for_bit(method, d, m, k):
    """torch.equal on every output of all four questions: S + 0.0 off the diagonal, the same division on it, the same factor and
    density functions and the same order of every sum."""
    n, nd = 700, 5
    model = synth_model(method, m, d, k, True, seed=5200 + m)
    X, Psi = catalogue(model, n, seed=m), noise(n, d, seed=m + 1)
    Xd, Pd, Cd = dev(X), dev(Psi), dev(twin_psi(Psi))
    groups, weights = setting(n, 3, seed=m)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=256) as p, gpz_amd.Predictor(model, tile_rows=256) as q:
        ref = tuple(q.predict_noisy_cov_dev(Xd, Pd)) + tuple(q.draws_noisy_cov_dev(Xd, Pd, nd, seed=4, return_gamma=True))
        same(three(p, Xd, Cd, nd=nd), ref, "moments, draws and gamma per draw")
        edges = np.linspace(*np.percentile(host(ref[0]), [3, 97]), 41)
        kw = dict(n_draws=nd, seed=4, groups=gd, n_groups=3, weights=wd)
        for u, v in zip(p.stack_psi_cube_dev(Xd, Cd, edges, **kw), q.stack_noisy_cov_dev(Xd, Pd, edges, **kw)):
            assert np.array_equal(u, v)
        same(three(q, Xd, Cd, nd=nd), ref, "on the handle that has served the per-dimension route")


# ---- 3. every width ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
@pytest.mark.parametrize("d", range(1, 11))
def test_every_width(method, d):
    """m = 33: one full LDS stage and one record of basis functions, 561 pairs = 17 stages and an odd tail of 17."""
    n, m = 300, 33
    for k in (1, 8):
        model = synth_model(method, m, d, k, True, seed=6400 + 20 * d + k + COV.index(method))
        X, cube = catalogue(model, n, seed=d), cube_of(n, d, seed=d + 50)
        ref = gpz_amd.predict(X, model, Psi=cube)
        with gpz_amd.Predictor(model) as p:
            check_parity(p.predict_psi_cube_dev(dev(X), dev(cube)), ref, f"width {method} d{d} k{k}")
            F = p.draws_psi_cube_dev(dev(X), dev(cube), 3, Z=np.zeros((m, 3, k)))
            print(f"nrel width {method} d{d} k{k} draws {nrel(host(F[1]), ref[0]):.3e}")
            assert nrel(host(F[1]), ref[0]) <= GATE_DRAW, nrel(host(F[1]), ref[0])


# ---- 4. edges in m -------------------------------------------------------------------------------------------------------------------------
CHUNK_EDGES = [m for m in range(2, 257) if cov_chunks_rule(m, 3, 1) != cov_chunks_rule(m - 1, 3, 1)
               or gamma_chunks_rule(m) != gamma_chunks_rule(m - 1)]


@pytest.mark.parametrize("m", sorted({1, 2, 15, 16, 17, 31, 32, 33, 255, 256} | {m + s for m in CHUNK_EDGES for s in (-1, 0)}))
def test_every_block_stage_and_chunk_edge(m):
    d, n, k = 3, 300, 1
    model = synth_model("VC", m, d, k, bool(m % 3), seed=7800 + 10 * m)
    X, cube = catalogue(model, n, seed=m), cube_of(n, d, seed=m + 50)
    ref = gpz_amd.predict(X, model, Psi=cube)
    with gpz_amd.Predictor(model) as p:
        check_parity(p.predict_psi_cube_dev(dev(X), dev(cube)), ref, f"edge m{m}")
        assert f"k_predict_psi_cube_small ({cov_chunks_rule(m, d, k)} pair chunks)" in p.route
        F, Gam = p.draws_psi_cube_dev(dev(X), dev(cube), 2, Z=np.zeros((m, 2, k)), return_gamma=True)
        assert f"k_predict_psi_cube_gamma ({gamma_chunks_rule(m)} pair chunks)" in p.route
        for s in range(2):
            print(f"nrel edge m{m} draw {s}: F {nrel(host(F[s]), ref[0]):.3e} gamma_s {nrel(host(Gam[s]), ref[4]):.3e}")
            assert nrel(host(F[s]), ref[0]) <= GATE_DRAW
            assert nrel(host(Gam[s]), ref[4]) <= GATE["gamma"]


# ---- 5. row counts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8])
def test_every_row_count(k):
    """n at the edges of the 16-row wave slices, the 64-lane waves, the 256-row workgroups and the 128-row tiles of the product: every
    shorter call is the first rows of the longest one bit for bit, for the moments, the draws and Gam."""
    d, m = 5, 17
    model = synth_model("VC", m, d, k, True, seed=8950 + k)
    X, cube = catalogue(model, 257, seed=91), cube_of(257, d, seed=92)
    with gpz_amd.Predictor(model) as p:
        Xd, Cd = dev(X), dev(cube)
        full = three(p, Xd, Cd)
        check_parity(full[:5], gpz_amd.predict(X, model, Psi=cube), f"rows k{k}")
        for n in (1, 63, 64, 65, 255, 256, 257):
            out = three(p, Xd[:n], Cd[:, :, :n])
            assert all(o.shape == (n, k) for o in out[:5]) and out[5].shape == (4, n, k) and out[6].shape == (4, n, k)
            same(out, rows_of(full, slice(0, n)), f"n = {n}")


# ---- 6. the same bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,m,k", [("VC", 100, 1), ("GC", 130, 3)])
def test_same_bits_over_tiles_row_orders_splits_and_draw_counts(method, m, k):
    n, d = 2500, 5
    model = synth_model(method, m, d, k, True, seed=9045 + m)
    X, cube = catalogue(model, n, seed=46), cube_of(n, d, seed=47)
    perm = torch.from_numpy(np.random.default_rng(48).permutation(n)).to(DEV)
    Xd, Cd = dev(X), dev(cube)
    outs = []
    for tile in (256, 1024, None):
        with gpz_amd.Predictor(model, tile_rows=tile) as p:
            outs.append(three(p, Xd, Cd, nd=3))
            if tile == 1024:
                shuf = three(p, Xd[perm], Cd[:, :, perm], nd=3)
                cut = 1100
                halves = [three(p, Xd[:cut], Cd[:, :, :cut], nd=3), three(p, Xd[cut:], Cd[:, :, cut:], nd=3)]
                more = three(p, Xd, Cd, nd=8)
                # one row's matrix passes the scan but is indefinite: no other row's bits move
                odd = Cd.clone()
                odd[1, 0, 1234] = odd[0, 1, 1234] = 50.0
                keep = torch.ones(n, dtype=torch.bool, device=DEV)
                keep[1234] = False
                broken = three(p, Xd, odd, nd=3)
    for o in outs[1:]:
        same(o, outs[0], "tile sizes")
    same(shuf, rows_of(outs[0], perm), "a permutation of the rows")
    same([torch.cat([a, b], dim=0 if a.dim() == 2 else 1) for a, b in zip(*halves)], outs[0], "two calls")
    same(more[:5] + (more[5][:3], more[6][:3]), outs[0], "draw s does not depend on the draws behind it")
    same(rows_of(broken, keep), rows_of(outs[0], keep), "every row but the indefinite one")
    assert not torch.equal(broken[0][1234], outs[0][0][1234])


# ---- 7. layouts ----------------------------------------------------------------------------------------------------------------------------
def test_layouts_of_the_cube_and_of_x_give_the_same_bits():
    """The cube contiguous as (d, d, n), as (n, d, d) under permute, as a strided view into a larger tensor and as float32 holding the
    same values; its strict upper triangle overwritten with NaN; X as float32 and as a transposed view; a selection."""
    n, d = 700, 5
    model = synth_model("VC", 40, d, 2, True, seed=9181)
    X32 = catalogue(model, n, seed=182).astype(np.float32)
    C32 = cube_of(n, d, seed=183).astype(np.float32)                     # still symmetric: the rounding is element by element
    Xd, Cd = dev(X32.astype(np.float64)), dev(C32.astype(np.float64))
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        ref = three(p, Xd.contiguous(), Cd.contiguous())
        assert Cd.stride() == (d * n, n, 1)
        ndd = Cd.permute(2, 0, 1).contiguous()                           # (n, d, d) as a catalogue holds it
        same(three(p, Xd, ndd.permute(1, 2, 0)), ref, "(n, d, d) under permute(1, 2, 0)")
        fortran = dev(np.asfortranarray(C32.astype(np.float64)).T.copy()).permute(2, 1, 0)   # the reference's column-major cube
        assert fortran.stride() == (1, d, d * d)
        same(three(p, Xd, fortran), ref, "column-major d x d x n")
        big = torch.full((d + 1, d + 2, 2 * n + 3), float("nan"), dtype=torch.float64, device=DEV)
        big[1:, 2:, 3::2] = Cd
        same(three(p, Xd, big[1:, 2:, 3::2]), ref, "a strided view into a larger tensor")
        same(three(p, Xd, dev(C32, torch.float32)), ref, "float32")
        upper = Cd.clone()
        iu = torch.triu_indices(d, d, 1, device=DEV)
        upper[iu[0], iu[1], :] = float("nan")
        same(three(p, Xd, upper), ref, "NaN above the diagonal")
        same(three(p, dev(X32, torch.float32), Cd), ref, "float32 X")
        same(three(p, Xd.T.contiguous().T, ndd.permute(1, 2, 0)), ref, "a transposed X")
        sel = torch.zeros(n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        half = three(p, Xd[::2].contiguous(), Cd[:, :, ::2].contiguous())
        same(three(p, Xd, Cd, selection=sel), half, "selection")
        same(rows_of(ref, slice(None, None, 2)), half, "rows of the whole call")


# ---- 8. draws and gamma per draw -----------------------------------------------------------------------------------------------------------
def with_weights(model, w):
    other = copy.deepcopy(model)
    other.sets["best"]["w"] = np.array(w, dtype=np.float64)
    return other


@pytest.mark.parametrize("method", COV)
def test_draws_and_gamma_per_draw_are_the_moments_of_the_w_s_model(method):
    """iSigma_w = 2^-10 I, so w_s = w + 2^-5 z_s is the same double on host and device: F[s] is predict_psi_cube_dev's mu of the handle
    whose weights are w_s and Gam[s] its gamma.  With Z = 0 every Gam[s] is the handle's own gamma."""
    n, d, m, k, nd = 300, 5, 20, 2, 3
    model = synth_model(method, m, d, k, True, seed=9300)
    model.sets["best"]["iSigma_w"] = np.stack([2.0 ** -10 * np.eye(m)] * k, axis=2)
    X, cube = catalogue(model, n, seed=301), cube_of(n, d, seed=302)
    Xd, Cd = dev(X), dev(cube)
    Z = np.random.default_rng(303).standard_normal((m, nd, k))
    W = model.sets["best"]["w"][:, None, :] + 2.0 ** -5 * Z
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F, Gam = p.draws_psi_cube_dev(Xd, Cd, nd, Z=Z, return_gamma=True)
        assert torch.equal(F, p.draws_psi_cube_dev(Xd, Cd, nd, Z=Z))
        own = p.predict_psi_cube_dev(Xd, Cd)
        F0, G0 = p.draws_psi_cube_dev(Xd, Cd, nd, Z=np.zeros((m, nd, k)), return_gamma=True)
    for s in range(nd):
        with gpz_amd.Predictor(with_weights(model, W[:, s, :]), tile_rows=256) as q:
            mom = q.predict_psi_cube_dev(Xd, Cd)
        fm, fg = nrel(host(F[s]), host(mom[0])), nrel(host(Gam[s]), host(mom[4]))
        zm, zg = nrel(host(F0[s]), host(own[0])), nrel(host(G0[s]), host(own[4]))
        print(f"{method} draw {s}: F {fm:.3e} gamma_s {fg:.3e}; Z = 0: F {zm:.3e} gamma_s {zg:.3e}")
        assert fm <= 1e-12 and zm <= 1e-12, (fm, zm)
        assert fg <= GATE_GAMMA_S and zg <= GATE_GAMMA_S, (fg, zg)


# ---- 9. stack ------------------------------------------------------------------------------------------------------------------------------
def reference_w(p, model, Xd, Cd, edges, n_draws, seed, groups, weights, G):
    """stack_reference_w fed with the device's own per-row numbers (predict_psi_cube_dev and draws_psi_cube_dev(return_gamma=True)), and
    the tolerances of test_predictor_stack_noisy_cov.py's reference_w."""
    mu, sigma, _, beta = (host(t) for t in p.predict_psi_cube_dev(Xd, Cd)[:4])
    F = S2 = None
    if n_draws:
        Ft, Gt = p.draws_psi_cube_dev(Xd, Cd, n_draws, seed=seed, return_gamma=True)
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
    return ref, tol_h, tol_m, ng * EPS * W


@pytest.mark.parametrize("method,k", [("VC", 1), ("GC", 3)])
def test_stack(method, k):
    """2500 rows on 1024-row tiles, three groups with rows left out and random weights, 37 bins, no draws and 5 seeded draws: column 0 from
    predict_psi_cube_dev's mu and sigma, column 1 + s with the width beta + max(gamma_s, 0), through the torch-free reference
    reduction; two calls on halves of the rows add to the whole call; the same call twice gives the same bits."""
    d, ns, G, m, B = 5, 2500, 3, 40, 37
    model = synth_model(method, m, d, k, True, seed=9400 + k)
    X, cube = catalogue(model, ns, seed=k + 40), cube_of(ns, d, seed=k + 41)
    Xd, Cd = dev(X), dev(cube)
    groups, weights = setting(ns, G, seed=m)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        mu0 = host(p.predict_psi_cube_dev(Xd, Cd)[0])
        edges = np.linspace(*np.percentile(mu0, [3, 97]), B + 1)
        for nd in (0, 5):
            ref, th, tm, tw = reference_w(p, model, Xd, Cd, edges, nd, 77, groups, weights, G)
            kw = dict(n_draws=nd, seed=77, n_groups=G)
            rd = p.stack_psi_cube_dev(Xd, Cd, edges, groups=gd, weights=wd, **kw)
            assert rd.hist.shape == (1 + nd, G, k, B)
            assert_close(rd, ref, th, tm, tw, f"{method} k={k} draws={nd}")
            for u, v in zip(rd, p.stack_psi_cube_dev(Xd, Cd, edges, groups=gd, weights=wd, **kw)):
                assert np.array_equal(u, v)                              # the same call twice
            one = p.stack_psi_cube_dev(Xd, Cd, edges, **kw)              # no groups, no weights: one group of weight 1
            assert one.sum_w[0] == ns and one.sum_w[1:].sum() == 0.0
            for cut in (1024, 700):                                      # on a tile edge: the bits; inside a tile: the tolerance
                parts = [p.stack_psi_cube_dev(Xd[i:j], Cd[:, :, i:j], edges, groups=gd[i:j], weights=wd[i:j], **kw)
                         for i, j in ((0, cut), (cut, ns))]
                total = [parts[0][f] + parts[1][f] for f in range(4)]
                assert_close(gpz_amd.api.StackResult(*total, edges), ref, th, tm, tw, f"two calls cut at {cut}")
            if nd:
                assert rd.hist[1:].sum() > 0.0
        assert p.route.endswith(f"; noise cube per draw: k_predict_psi_cube_gamma ({gamma_chunks_rule(m)} pair chunks) + k_stack_tile_w"), \
            p.route


# ---- 10. refusals on the device --------------------------------------------------------------------------------------------------------------
def raw_entries(p, x, cube, k, nd=3, B=7):
    """The four C entries on outputs pre-filled with a sentinel: the return codes, the messages and the outputs."""
    n = x.shape[0]
    call = p._dev_begin(x.device)
    out = [torch.full((k, n), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
    F = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    Gm = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    F2 = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    hist, sw, sm, sm2 = (np.full(s, -7.0) for s in ((1 + nd, 1, k, B), (1,), (1 + nd, 1, k), (1 + nd, 1, k)))
    edges = np.ascontiguousarray(np.tile(np.linspace(-3.0, 3.0, B + 1), (k, 1)))
    psi = (cube.data_ptr(), 1 if cube.dtype == torch.float32 else 0, cube.stride(0), cube.stride(1), cube.stride(2))
    lead = (call.h, *p._x_args(x), *psi, _lib.dptr(call.muX), _lib.dptr(call.sdX), _lib.dptr(call.div))
    rcs, msgs = [], []

    def note(rc):
        rcs.append(rc)
        msgs.append(p._lib.gpz_last_error().decode() if rc else "")

    note(p._lib.gpz_predictor_run_psi_cube_dev(*lead, _lib.dptr(call.muY), *(t.data_ptr() for t in out), call.stream))
    note(p._lib.gpz_predictor_draws_psi_cube_dev(*lead, _lib.dptr(call.muY), nd, 5, None, F.data_ptr(), call.stream))
    note(p._lib.gpz_predictor_draws_gamma_psi_cube_dev(*lead, _lib.dptr(call.muY), nd, 5, None, F2.data_ptr(), Gm.data_ptr(), call.stream))
    note(p._lib.gpz_predictor_stack_psi_cube_dev(*lead, nd, 5, None, _lib.dptr(edges), B, None, 1, None, _lib.dptr(hist), _lib.dptr(sw),
                                                 _lib.dptr(sm), _lib.dptr(sm2), None, call.stream))
    torch.cuda.synchronize()
    return tuple(rcs), msgs, out + [F, F2, Gm] + [torch.from_numpy(a) for a in (hist, sw, sm, sm2)]


def test_bad_cubes_and_bad_rows_are_refused_with_the_outputs_untouched():
    n, d, k = 5000, 5, 2
    model = synth_model("VC", 20, d, k, True, seed=9185)
    model.sdX = np.array(model.sdX, dtype=np.float64)
    model.sdX[0] = 1e-155                                                 # sdX[0]^2 is subnormal: a division by it can overflow
    scale = (model.sdX[:, None] * model.sdX[None, :])[:, :, None]
    X, C = dev(catalogue(model, n, seed=186)), dev(cube_of(n, d, seed=187) * scale)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        good = three(p, X[:500], C[:, :, :500])
        assert all(bool(torch.isfinite(t).all()) for t in good)
        rcs, _, outs = raw_entries(p, X, C, k)
        assert rcs == (0, 0, 0, 0) and all(bool((t != -7.0).all()) for t in outs)
        bad_x = X.clone()
        bad_x[4001, 3] = float("nan")
        cases = [("NaN in X", bad_x, C, ERR_UNSUPPORTED)]
        for what, v, r, c, at in (("NaN on the diagonal", float("nan"), 4, 4, 4999), ("+inf on the diagonal", float("inf"), 0, 0, 0),
                                  ("a negative diagonal element", -1e-300, 2, 2, 3333), ("NaN below the diagonal", float("nan"), 3, 1, 77),
                                  ("an overflow after the division", 1e200, 1, 0, 2048)):
            bad = C.clone()
            bad[r, c, at] = v
            cases.append((what, X, bad, ERR_ARG))
        for what, x, cube, code in cases:
            rcs, msgs, outs = raw_entries(p, x, cube, k)
            assert rcs == (code,) * 4, (what, rcs, msgs)
            assert all(bool((t == -7.0).all()) for t in outs), what        # refused before any tile kernel has run
            with pytest.raises(_lib.GpzError):
                p.predict_psi_cube_dev(x, cube)
            with pytest.raises(_lib.GpzError):
                p.draws_psi_cube_dev(x, cube, 3, return_gamma=True)
            with pytest.raises(_lib.GpzError):
                p.stack_psi_cube_dev(x, cube, np.linspace(-3.0, 3.0, 8), n_draws=2)
            same(three(p, X[:500], C[:, :, :500]), good, "the handle works on the next call")
        above = C.clone()
        above[1, 3, 99] = float("nan")                                     # above the diagonal: never read
        assert raw_entries(p, X, above, k)[0] == (0, 0, 0, 0)


@pytest.mark.parametrize("method,k", [("VC", 1), ("GC", 3)])
def test_an_all_zero_cube_is_the_noise_free_prediction(method, k):
    """As the per-dimension file holds Psi = 0: mu and beta_i against predict_dev(X), nu against the model with iSigma_w =
    tril(iS) + tril(iS, -1)', gamma ~ 0 against mu^2, at that file's GATE_ZERO."""
    n, d, m = 500, 5, 60
    model = synth_model(method, m, d, k, True, seed=160 + k)
    X = catalogue(model, n, seed=161)
    iS = model.sets["best"]["iSigma_w"]
    sym = synth_model(method, m, d, k, True, seed=160 + k)
    sym.sets["best"]["iSigma_w"] = np.stack([np.tril(iS[:, :, o]) + np.tril(iS[:, :, o], -1).T for o in range(k)], axis=2)
    Xd = dev(X)
    with gpz_amd.Predictor(model) as p, gpz_amd.Predictor(sym) as ps:
        z = p.predict_psi_cube_dev(Xd, torch.zeros((d, d, n), dtype=torch.float64, device=DEV))
        f = p.predict_dev(Xd)
        fs = ps.predict_dev(Xd)
    mu0 = host(z[0]) - model.muY
    fig = {"mu": nrel(host(z[0]), host(f[0])), "beta_i": nrel(host(z[3]), host(f[3])), "nu": nrel(host(z[2]), host(fs[2])),
           "gamma": float(np.linalg.norm(host(z[4])) / np.linalg.norm(mu0 ** 2))}
    for name, v in fig.items():
        print(f"zero {method} k{k} {name} {v:.3e}")
    assert all(v <= GATE_ZERO for v in fig.values()), fig


# ---- 11. memory ----------------------------------------------------------------------------------------------------------------------------
def test_memory_is_added_once_and_never_grows_with_the_rows():
    """behind predict_noisy_cov_dev the first cube call adds two slots of d (d + 1) / 2 x tile_pad doubles and the
    divisor triangle of d (d + 1) / 2 doubles, tile_pad = tile_rows rounded up to 1024."""
    d, nd, m, k, T = 5, 4, 60, 1, 1024
    NP = d * (d + 1) // 2
    model = synth_model("VC", m, d, k, True, seed=9195)
    X, Psi, C = dev(catalogue(model, 5000, seed=196)), dev(noise(5000, d, seed=197)), dev(cube_of(5000, d, seed=198))
    with gpz_amd.Predictor(model, tile_rows=T) as p, gpz_amd.Predictor(model, tile_rows=T) as q:
        q.predict_dev(X[:300]); q.predict_noisy_cov_dev(X[:300], Psi[:300])     # a handle that never sees a cube ...
        p.predict_dev(X[:300]); p.predict_noisy_cov_dev(X[:300], Psi[:300])
        held = p.info[1]
        assert held == q.info[1]
        small = p.predict_psi_cube_dev(X[:300], C[:, :, :300])
        first = p.info[1]
        assert first - held == 8 * (2 * NP * T + NP), (first - held, 8 * (2 * NP * T + NP))
        out = p.predict_psi_cube_dev(X, C)
        assert p.info[1] == first                                           # 300 rows or 5000: the same bytes
        same(small, [t[:300] for t in out], "the first rows")
        p.draws_psi_cube_dev(X[:300], C[:, :, :300], nd, return_gamma=True)
        drawn = p.info[1]
        p.draws_psi_cube_dev(X, C, nd, return_gamma=True)
        p.predict_psi_cube_dev(X, C)
        assert p.info[1] == drawn
        q.predict_noisy_cov_dev(X, Psi)
        assert q.info[1] == held and "cube" not in q.route                  # ... holds what it held
