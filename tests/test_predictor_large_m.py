"""Predictor(model, large_m=True): complete rows with input noise on the handle past m = 256, up to m = 1024, in the three forms of Psi
(a variance per dimension on a diagonal kind, on GC / VC, and the d x d x n cube), all four questions.  Parity with the one-shot route
of the same handle and the oracle at the first sizes past the old limit, the top of the range, the new PHI kernel at small m against
the fused draws, the flag changing nothing where m <= 256, the same bits over tiles, orders, splits and draw counts, the stack, and
the refusals.  The chunk rules do not change above m = 256 (test_predictor_large_m_cpu.py), so there is no further m to take."""

import copy

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, nrel, synth_model
from test_predictor_large_m_cpu import large_chunks_rule
from test_predictor_noisy import NAMES, check_parity as check_diag, dev, host, noise
from test_predictor_noisy_cov import GATE as GATE_COV, check_parity as check_cov
from test_predictor_psi_cube import GATE_GAMMA_S, check_parity as check_cube, cube_of
from test_predictor_stack import assert_close, setting
from test_predictor_stack_noisy import reference_w as reference_diag
from test_predictor_stack_noisy_cov import reference_w as reference_cov

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ERR_ARG, ERR_UNSUPPORTED = -1, -5                                       # include/gpz_hip.h
GATE_DRAW = 1e-12                                                       # the draws tests' gate (test_predictor_draws.py, test_predictor_noisy.py)


class Form:
    """One of the three forms of Psi: its methods on a Predictor, its noise and the sibling file's parity check."""

    def __init__(self, name):
        self.name = name

    def psi(self, n, d, seed):
        return cube_of(n, d, seed) if self.name == "cube" else noise(n, d, seed)

    def rows(self, Psi, idx):
        return Psi[:, :, idx] if self.name == "cube" else Psi[idx]

    def moments(self, p, X, Psi):
        if self.name == "diag":
            return p.predict_dev(X, Psi=Psi)
        return p.predict_psi_cube_dev(X, Psi) if self.name == "cube" else p.predict_noisy_cov_dev(X, Psi)

    def draws(self, p, X, Psi, nd, **kw):
        if self.name == "diag":
            return p.draws_dev(X, nd, Psi=Psi, **kw)
        return p.draws_psi_cube_dev(X, Psi, nd, **kw) if self.name == "cube" else p.draws_noisy_cov_dev(X, Psi, nd, **kw)

    def stack(self, p, X, Psi, edges, **kw):
        if self.name == "diag":
            return p.stack_noisy_dev(X, Psi, edges, **kw)
        return p.stack_psi_cube_dev(X, Psi, edges, **kw) if self.name == "cube" else p.stack_noisy_cov_dev(X, Psi, edges, **kw)

    def check(self, out, ref, what):
        if self.name == "diag":
            for name, a, b in zip(NAMES, out, ref):
                print(f"nrel {what} {name} {nrel(host(a), b):.3e}")
            return check_diag(out, ref)
        return (check_cube if self.name == "cube" else check_cov)(out, ref, what)


DIAG, COV, CUBE = Form("diag"), Form("cov"), Form("cube")


def all_four(f, p, Xd, Pd, nd=4, seed=4):
    """The five moments, the draws and gamma under every draw."""
    return tuple(f.moments(p, Xd, Pd)) + tuple(f.draws(p, Xd, Pd, nd, seed=seed, return_gamma=True))


def same(a, b, what):
    for i, (s, t) in enumerate(zip(a, b)):
        assert s.shape == t.shape and torch.equal(s, t), (what, i, float((s - t).abs().max()))


def rows_of(out, idx):
    return [t[idx] if t.dim() == 2 else t[:, idx] for t in out]


def with_weights(model, w):
    other = copy.deepcopy(model)
    other.sets["best"]["w"] = np.array(w, dtype=np.float64)
    return other


def exact_draws(model, nd, seed):
    """iSigma_w = 2^-10 I, so that w_s = w + 2^-5 z_s is the same double on the host and the device: Z and the weights of every draw."""
    m, k = model.m, model.k
    model.sets["best"]["iSigma_w"] = np.stack([2.0 ** -10 * np.eye(m)] * k, axis=2)
    Z = np.random.default_rng(seed).standard_normal((m, nd, k))
    return Z, model.sets["best"]["w"][:, None, :] + 2.0 ** -5 * Z


# ---- 1. parity at the first sizes past the old limit -----------------------------------------------------------------------------------
PAST = (257, 272, 273)
CASES_1 = [(DIAG, meth, k, h) for meth in ("VD", "GL") for k in (1, 3) for h in (False, True)] + \
          [(f, meth, k, True) for f in (COV, CUBE) for meth in ("VC", "GC") for k in (1, 3)]


@pytest.mark.parametrize("form,method,k,hetero", CASES_1, ids=lambda v: v.name if isinstance(v, Form) else str(v))
def test_parity_past_the_old_limit(form, method, k, hetero):
    """All five outputs of the *_dev moments against p.predict(X, Psi=Psi) of the same handle, the one-shot route per tile, at the gate
    of the form's sibling file; 33 rows (the draws tile of the tile route is 1024 rows, one partial tile), d = 3."""
    n, d = 33, 3
    for m in PAST:
        model = synth_model(method, m, d, k, hetero, seed=8000 + 10 * m + k + hetero)
        X, Psi = catalogue(model, n, seed=m), form.psi(n, d, seed=m + 1)
        with gpz_amd.Predictor(model, large_m=True) as p:
            ref = p.predict(X, Psi=Psi)
            out = form.moments(p, dev(X), dev(Psi))
            form.check(out, ref, f"{form.name} {method} k{k} h{int(hetero)} m{m}")
            assert np.any(host(out[4]) != 0.0)
            assert f"({large_chunks_rule(m)[0]} pair chunks)" in p.route and f"; noisy large-m: tiles, {large_chunks_rule(m)[0]} chunks" in p.route
            F = form.draws(p, dev(X), dev(Psi), 2, Z=np.zeros((m, 2, k)))
            assert nrel(host(F[1]), ref[0]) <= GATE_DRAW, nrel(host(F[1]), ref[0])


@pytest.mark.parametrize("form,method", [(DIAG, "VD"), (COV, "VC"), (CUBE, "VC")], ids=lambda v: v.name if isinstance(v, Form) else str(v))
def test_the_oracle_at_m_257(form, method):
    m, n, d = 257, 8, 2
    model = synth_model(method, m, d, 1, True, seed=8600)
    X, Psi = catalogue(model, n, seed=1), form.psi(n, d, seed=2)
    orc = O.predict_noisy(X, np.ascontiguousarray(Psi), model)
    with gpz_amd.Predictor(model, large_m=True) as p:
        out = form.moments(p, dev(X), dev(Psi))
    for name, a, b in zip(NAMES, out, orc):
        print(f"rel oracle {form.name} {name} {rel(host(a), b):.3e}")
    for name, a, b in zip(NAMES, out, orc):
        assert rel(host(a), b) <= 1e-8, (name, rel(host(a), b))


# ---- 2. the top of the range -------------------------------------------------------------------------------------------------------------
# nrel of the one-shot route p.predict(X, Psi=Psi) against the oracle's predict_noisy at m = 1024 on the inputs of the test below (VD:
# its 16 rows; VC: its first 4 rows, 37 s of oracle), measured once on one MI355X: both exist without the handle's
# route.  gamma is 86 % of sigma in this model, and it is a sum of 524 800 terms less mu^2, so sigma carries gamma's rounding.
TOP_YARDSTICK = {"diag": {"mu": 2.437e-16, "sigma": 1.996e-12, "nu": 1.533e-15, "beta_i": 1.025e-14, "gamma": 2.317e-12},
                 "cov": {"mu": 3.346e-16, "sigma": 8.608e-12, "nu": 5.980e-16, "beta_i": 2.380e-14, "gamma": 1.019e-11}}


def top_gate(form, name):
    """The gate of the form's sibling file, or four times the yardstick above where that is larger (the longer sums)."""
    return max(1e-11 if form is DIAG else GATE_COV[name], 4.0 * TOP_YARDSTICK[form.name][name])


@pytest.mark.parametrize("form,method", [(DIAG, "VD"), (COV, "VC")], ids=lambda v: v.name if isinstance(v, Form) else str(v))
def test_the_top_of_the_range(form, method):
    """m = 1024: 524 800 pairs.  Moments and the draws against the one-shot route; gamma_s against a second handle whose w is draw
    s's weights, the construction of the siblings' gamma tests.  The moments' gate is top_gate: at the sibling's own gate VC's sigma
    misses (measured 7.5e-12 against 1e-12; gamma 8.7e-12 against 1e-10), while the one-shot route itself stands 8.6e-12 from the
    oracle on the same inputs; every other output is inside the sibling's gate."""
    m, d, k, n, nd = 1024, 2, 1, 16, 4
    model = synth_model(method, m, d, k, True, seed=8700)
    Z, W = exact_draws(model, nd, seed=3)
    X, Psi = catalogue(model, n, seed=4), form.psi(n, d, seed=5)
    Xd, Pd = dev(X), dev(Psi)
    with gpz_amd.Predictor(model, large_m=True) as p:
        ref = p.predict(X, Psi=Psi)
        out = form.moments(p, Xd, Pd)
        for name, u, v in zip(NAMES, out, ref):
            print(f"nrel top {form.name} {name} {nrel(host(u), v):.3e} (gate {top_gate(form, name):.1e})")
        for name, u, v in zip(NAMES, out, ref):
            assert nrel(host(u), v) <= top_gate(form, name), (name, nrel(host(u), v), top_gate(form, name))
        F, Gam = form.draws(p, Xd, Pd, nd, Z=Z, return_gamma=True)
        assert f"; noisy large-m: tiles, 4 chunks" in p.route, p.route
        held = p.info[1]
        for s in range(nd):
            ms = with_weights(model, W[:, s, :])
            with gpz_amd.Predictor(ms, large_m=True) as q:
                one = q.predict(X, Psi=Psi)
                mom = form.moments(q, Xd, Pd)
            print(f"top {form.name} draw {s}: draws {nrel(host(F[s]), one[0]):.3e} gamma_s {nrel(host(Gam[s]), host(mom[4])):.3e}")
            assert nrel(host(F[s]), one[0]) <= GATE_DRAW, (s, nrel(host(F[s]), one[0]))
            assert nrel(host(Gam[s]), host(mom[4])) <= (1e-11 if form is DIAG else GATE_GAMMA_S), (s, nrel(host(Gam[s]), host(mom[4])))
        assert p.info[1] == held


# ---- 3. the new PHI kernel at small m ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 15, 16, 17, 100])
@pytest.mark.parametrize("d", [1, 5, 13, 20])
def test_the_phi_kernel_against_the_fused_draws(m, d):
    """large_m=True with force_tiles=True: E_x[PHI] from k_predict_noisy_phi and the T-GEMM, against k_predict_draws_psi on a default
    handle; with Z = 0 every draw is predict_dev(X, Psi=Psi)'s mu.  n = 1, 63, 64, 65, 1025 as the first rows of one catalogue."""
    k, nd = 2, 3
    model = synth_model("VD" if d % 2 else "GL", m, d, k, True, seed=8800 + 20 * m + d)
    X, Psi = catalogue(model, 1025, seed=m + d), noise(1025, d, seed=m + d + 1)
    Z = np.random.default_rng(m).standard_normal((m, nd, k))
    with gpz_amd.Predictor(model, large_m=True, force_tiles=True) as p, gpz_amd.Predictor(model) as q:
        for n in (1, 63, 64, 65, 1025):
            Xd, Pd = dev(X[:n]), dev(Psi[:n])
            a, b = p.draws_dev(Xd, nd, Psi=Pd, Z=Z), q.draws_dev(Xd, nd, Psi=Pd, Z=Z)
            assert a.shape == b.shape == (nd, n, k)
            assert nrel(host(a), host(b)) <= GATE_DRAW, (n, nrel(host(a), host(b)))
            mu = host(p.predict_dev(Xd, Psi=Pd)[0])
            F0 = host(p.draws_dev(Xd, nd, Psi=Pd, Z=np.zeros((m, nd, k))))
            for s in range(nd):
                assert nrel(F0[s], mu) <= GATE_DRAW, (n, s, nrel(F0[s], mu))
        assert "draws: tiles k_phi + k_tgemm" in p.route and "draws: fused" in q.route
        assert "large-m" not in p.route                                  # (the route text of a model within the old limit does not change)


# ---- 4. the flag changes nothing where it need not ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [100, 256])
@pytest.mark.parametrize("form,method", [(DIAG, "VD"), (COV, "VC"), (CUBE, "GC")], ids=lambda v: v.name if isinstance(v, Form) else str(v))
def test_the_flag_changes_nothing_up_to_256(form, method, m):
    n, d, k = 64, 3, 2
    model = synth_model(method, m, d, k, True, seed=8900 + m)
    X, Psi = catalogue(model, n, seed=m), form.psi(n, d, seed=m + 1)
    Xd, Pd = dev(X), dev(Psi)
    groups, weights = setting(n, 2, seed=m)
    kw = dict(n_draws=8, seed=5, groups=dev(groups, torch.int64), n_groups=2, weights=dev(weights))
    with gpz_amd.Predictor(model, large_m=True) as p, gpz_amd.Predictor(model) as q:
        a, b = all_four(form, p, Xd, Pd, nd=8), all_four(form, q, Xd, Pd, nd=8)
        same(a, b, "moments, draws, gamma per draw")
        edges = np.linspace(*np.percentile(host(a[0]), [3, 97]), 8)
        for u, v in zip(form.stack(p, Xd, Pd, edges, **kw), form.stack(q, Xd, Pd, edges, **kw)):
            assert np.array_equal(u, v)
        assert p.info[1] == q.info[1] and p.route == q.route
        if form is DIAG:
            assert np.array_equal(p.draws(X, 8, seed=5, Psi=Psi), q.draws(X, 8, seed=5, Psi=Psi))
    with gpz_amd.Predictor(model, large_m=True) as p, gpz_amd.Predictor(model) as q:
        assert p.info[1] == q.info[1]                                    # before any Psi: the same bytes


# ---- 5. same bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,method", [(DIAG, "VD"), (COV, "VC")], ids=lambda v: v.name if isinstance(v, Form) else str(v))
def test_same_bits_over_tiles_orders_splits_and_draw_counts(form, method):
    m, n, d, k = 273, 64, 3, 1
    model = synth_model(method, m, d, k, True, seed=9100)
    X, Psi = catalogue(model, n, seed=1), form.psi(n, d, seed=2)
    Xd, Pd = dev(X), dev(Psi)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    with gpz_amd.Predictor(model, large_m=True) as p:
        ref = all_four(form, p, Xd, Pd, nd=8)
        same(rows_of(all_four(form, p, Xd[perm], form.rows(Pd, perm), nd=8), torch.argsort(perm)), ref, "a row permutation")
        parts = [all_four(form, p, Xd[i:j], form.rows(Pd, slice(i, j)), nd=8) for i, j in ((0, 23), (23, n))]
        same([torch.cat([u, v], dim=0 if u.dim() == 2 else 1) for u, v in zip(*parts)], ref, "a split into two calls")
        three = all_four(form, p, Xd, Pd, nd=3)
        same(three[5:], [t[:3] for t in ref[5:]], "3 draws against the first 3 of 8")
        edges = np.linspace(*np.percentile(host(ref[0]), [3, 97]), 8)
        s1, s2 = (form.stack(p, Xd, Pd, edges, n_draws=8, seed=4) for _ in range(2))
        assert np.array_equal(s1.hist, s2.hist)
    with gpz_amd.Predictor(model, large_m=True, tile_rows=64) as q:
        same(all_four(form, q, Xd, Pd, nd=8), ref, "tile_rows = 64")


# ---- 6. the stack ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,method", [(DIAG, "VD"), (COV, "VC")], ids=lambda v: v.name if isinstance(v, Form) else str(v))
def test_the_stack_at_m_273(form, method):
    """Column 0 of the call with draws is the call without draws bit for bit; every column against the siblings' reference reduction
    over the handle's own moments, draws and gamma_s at their tolerances; the host entries of the diagonal form give the bits of
    their _dev twins."""
    m, n, d, k, G, B, nd = 273, 64, 3, 1, 2, 7, 8
    model = synth_model(method, m, d, k, True, seed=9200)
    X, Psi = catalogue(model, n, seed=1), form.psi(n, d, seed=2)
    Xd, Pd = dev(X), dev(Psi)
    groups, weights = setting(n, G, seed=3)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, large_m=True) as p:
        edges = np.linspace(*np.percentile(host(form.moments(p, Xd, Pd)[0]), [3, 97]), B + 1)
        res = form.stack(p, Xd, Pd, edges, n_draws=nd, seed=7, groups=gd, n_groups=G, weights=wd)
        zero = form.stack(p, Xd, Pd, edges, n_draws=0, groups=gd, n_groups=G, weights=wd)
        for u, v in zip((res.hist[:1], res.sum_w, res.sum_mu[:1], res.sum_mu2[:1]), zero[:4]):
            assert np.array_equal(u, v)
        ref, th, tm, tw, _ = (reference_diag if form is DIAG else reference_cov)(p, model, Xd, Pd, edges, nd, 7, groups, weights, G)
        assert_close(res, ref, th, tm, tw, f"stack {form.name}")
        assert res.hist[1:].sum() > 0.0
        if form is DIAG:
            hs = p.stack_noisy(X, Psi, edges, n_draws=nd, seed=7, groups=groups, n_groups=G, weights=weights)
            for u, v in zip(hs, res):
                assert np.array_equal(u, v)
            assert np.array_equal(p.draws(X, nd, seed=7, Psi=Psi), host(p.draws_dev(Xd, nd, seed=7, Psi=Pd)))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_m_1040_is_refused_at_the_c_entry():
    m, n, d, k = 1040, 8, 2, 1
    model = synth_model("VD", m, d, k, False, seed=9300)
    Xd, Pd = dev(catalogue(model, n, seed=1)), dev(noise(n, d, seed=2))
    with gpz_amd.Predictor(model, large_m=True) as p:
        with pytest.raises(ValueError, match="large_m"):
            p.predict_dev(Xd, Psi=Pd)
        held = p.info[1]
        muX, sdX, muY = p._norm_vectors()
        sd2 = np.ascontiguousarray(sdX ** 2)
        stream = torch.cuda.current_stream(Xd.device).cuda_stream
        out = [torch.full((k, n), -7.0, dtype=torch.float64, device=DEV) for _ in range(5)]
        rc = p._lib.gpz_predictor_run_noisy_dev(p._handle(), *p._x_args(Xd), *p._psi_args(Pd, n), _lib.dptr(muX), _lib.dptr(sdX),
                                                _lib.dptr(sd2), _lib.dptr(muY), *(t.data_ptr() for t in out), stream)
        msg = p._lib.gpz_last_error().decode()
        torch.cuda.synchronize()
        assert rc == ERR_UNSUPPORTED and "predict_noisy_fits" in msg and "m 1040" in msg and "1024" in msg, (rc, msg)
        assert all(bool((t == -7.0).all()) for t in out) and p.info[1] == held and "noise" not in p.route


def test_bad_psi_missing_inputs_and_memory_at_m_273():
    m, n, d, k = 273, 40, 3, 1
    model = synth_model("VD", m, d, k, True, seed=9400)
    X, Psi = catalogue(model, 10 * n, seed=1), noise(10 * n, d, seed=2)
    Xd, Pd = dev(X), dev(Psi)
    with gpz_amd.Predictor(model, large_m=True) as p:
        good = all_four(DIAG, p, Xd[:n], Pd[:n])
        held = p.info[1]
        for bad in (np.nan, -1e-3):
            Pb = Pd[:n].clone()
            Pb[7, 1] = bad
            with pytest.raises(_lib.GpzError, match="Psi has an element"):
                p.predict_dev(Xd[:n], Psi=Pb)
            with pytest.raises(_lib.GpzError, match="Psi has an element"):
                p.draws_dev(Xd[:n], 4, Psi=Pb, return_gamma=True)
        same(all_four(DIAG, p, Xd[:n], Pd[:n]), good, "the next good call")
        for call in (lambda: p.predict_dev(Xd[:n], missing=True), lambda: p.predict_noisy_missing_dev(Xd[:n], Pd[:n])):
            with pytest.raises(ValueError, match="m <= 256, not m = 273"):
                call()
        all_four(DIAG, p, Xd, Pd)                                        # ten times the rows
        assert p.info[1] == held
