"""Predictor(model, large_m_missing=True): one NaN-pattern group of a diagonal kind on the handle past m = 256, up to m = 1024, with and
without Psi, all four questions (k_pml_pairs / k_pml_gamma: Pio through LDS in K panels of 128 columns, four groups of 64 pairs per
batch, two where k > 1).  Parity with the one-shot route of the same handle at the first sizes past the old limit and on both sides of
the K-panel edges, the oracle at m = 257, the draws and gamma per draw against handles whose w is the draw's, the stack, the same bits
over tiles, orders, company, splits and draw counts, the flag changing nothing where m <= 256, the top of the range, refusals and memory.
Every case fails without the keyword."""
import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, nrel, synth_model
from test_predictor_large_m import exact_draws, rows_of, same, with_weights
from test_predictor_missing import NAMES, dev, host, model_with_priors
from test_predictor_missing_cpu import chunks_rule
from test_predictor_noisy import noise
from test_predictor_stack import assert_close, setting
from test_predictor_stack_missing import raw_calls as raw_stack, stack_inputs as stack_inputs_clean
from test_predictor_stack_noisy_missing import raw_calls as raw_stack_noisy, stack_inputs as stack_inputs_noisy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
ERR_UNSUPPORTED = -5                                                     # include/gpz_hip.h
GATE, GATE_DRAW, GATE_ORACLE = 1e-11, 1e-12, 1e-8                        # the sibling files' gates (test_predictor_missing.py, _draws.py)
ROUTE = "; missing past 256: k_pml_pairs / k_pml_gamma (K panels of 128, {} groups per batch)"


def npair(m):
    return m * (m + 1) // 2


def five_patterns(X):
    """d = 3.  Groups of 70 rows (dimension 1 missing), 33 (dimensions 0 and 2: two missing), 1 (nothing observed), 31 (dimension 2),
    32 (dimension 0) and 5 complete rows, interleaved: 1, 31, 32, 33 and 70 rows are one row, one row short of a 32-row block, a block,
    a block and a row, and two blocks and a part."""
    assert X.shape == (172, 3)
    X = X.copy()
    order = np.random.default_rng(5).permutation(172)
    for idx, cols in ((order[:70], (1,)), (order[70:103], (0, 2)), (order[103:104], (0, 1, 2)), (order[104:135], (2,)), (order[135:167], (0,))):
        for c in cols:
            X[idx, c] = NAN
    return X


def moments(p, Xd, Pd):
    return p.predict_dev(Xd, missing=True) if Pd is None else p.predict_noisy_missing_dev(Xd, Pd)


def draws(p, Xd, Pd, nd, **kw):
    return p.draws_dev(Xd, nd, missing=True, **kw) if Pd is None else p.draws_noisy_missing_dev(Xd, Pd, nd, **kw)


def stack(p, Xd, Pd, edges, **kw):
    return p.stack_missing_dev(Xd, edges, **kw) if Pd is None else p.stack_noisy_missing_dev(Xd, Pd, edges, **kw)


def all_four(p, Xd, Pd, nd=4, seed=4):
    return tuple(moments(p, Xd, Pd)) + tuple(draws(p, Xd, Pd, nd, seed=seed, return_gamma=True))


def one_shot(p, X, Psi):
    """p.predict(X[, Psi=Psi]) of the same handle: the one-shot gpz_predict_missing per NaN-pattern group, the row with nothing observed
    included."""
    return [np.array(a) for a in p.predict(X, **({} if Psi is None else {"Psi": Psi}))[:5]]


def check(out, ref, gate, what):
    for name, a, b in zip(NAMES, out, ref):
        print(f"nrel {what} {name} {nrel(host(a), b):.3e} (gate {gate:.1e})")
    for name, a, b in zip(NAMES, out, ref):
        a = host(a)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        assert nrel(a, b) <= gate, (what, name, nrel(a, b), gate)


# ---- 1. parity at the edges --------------------------------------------------------------------------------------------------------------
# 257, 272, 273: the first sizes past the old limit and the first step of ceil16(m) (nk = 272, 272, 288: two panels and a part of 16 or
# 32 columns).  Then one m on each side of every edge of the 128-column K panel: 384 | 385, 512 | 513, 640 | 641, 768 | 769, 896 | 897
# (nk = 384 | 400 ... 896 | 912: whole panels on one side, a 16-column panel more on the other; test_the_top_of_the_range is 1024).
# Up to 513 the full cross of kind, k and noise model; above, where a case costs more, one case per m, dealt so that every m pair has
# both kinds, k = 1 (batches of 4) and k = 3 (batches of 2), and rows with and without Psi.
EDGES = (257, 272, 273, 384, 385, 512, 513)
CASES_1 = [(m, meth, k, h) for m in EDGES for meth in ("VD", "GL") for k in (1, 3) for h in (False, True)] + \
          [(640, "VD", 1, False), (641, "GL", 3, True), (768, "GL", 1, True), (769, "VD", 3, False), (896, "VD", 3, True),
           (897, "GL", 1, False)]


@pytest.mark.parametrize("m,method,k,noisy", CASES_1)
def test_parity_at_the_edges(m, method, k, noisy):
    d, n = 3, 172
    model = model_with_priors(method, m, d, k, bool((m + k) % 2), seed=12000 + 10 * m + k)
    X = five_patterns(catalogue(model, n, seed=m))
    Psi = noise(n, d, seed=m + 1) if noisy else None
    full = ~np.isnan(X).any(axis=1)
    with gpz_amd.Predictor(model, large_m_missing=True) as p:
        ref = one_shot(p, X, Psi)
        Xd, Pd = dev(X), None if Psi is None else dev(Psi)
        out = moments(p, Xd, Pd)
        check(out, ref, GATE, f"{method} k{k} m{m} {'psi' if noisy else 'clean'}")
        assert np.all(host(out[4])[~full] > 0.0)
        assert ROUTE.format(4 if k == 1 else 2) in p.route and f"({chunks_rule(m)} pair chunks)" in p.route, p.route
        fd = torch.from_numpy(full).to(DEV)                              # the complete rows beside them: the bits of their own entry
        alone = p.predict_dev(Xd[fd]) if Pd is None else p.predict_dev(Xd[fd], Psi=Pd[fd])
        assert all(torch.equal(a[fd], b) for a, b in zip(out, alone))


@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "psi"])
def test_the_oracle_at_m_257(noisy):
    m, n, d = 257, 4, 2
    model = model_with_priors("VD", m, d, 1, True, seed=12600)
    X = catalogue(model, n, seed=1)
    X[:2, 1] = NAN
    X[2, :] = NAN
    Psi = noise(n, d, seed=2) if noisy else None
    orc = O.predict_any(X, model, **({} if Psi is None else {"Psi": Psi}))[:5]
    with gpz_amd.Predictor(model, large_m_missing=True) as p:
        out = moments(p, dev(X), None if Psi is None else dev(Psi))
    for name, a, b in zip(NAMES, out, orc):
        print(f"rel oracle {name} {rel(host(a), b):.3e}")
    for name, a, b in zip(NAMES, out, orc):
        assert rel(host(a), b) <= GATE_ORACLE, (name, rel(host(a), b))


# ---- 2. the draws and gamma under every draw -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "psi"])
@pytest.mark.parametrize("m", [273, 513])
def test_draws_and_gamma_per_draw(m, noisy):
    """iSigma_w = 2^-10 I: w_s = w + 2^-5 z_s is the same double on the host and the device.  draws[s] against mu, and gamma_s against
    gamma, of the same call on a handle whose w is w_s, at the siblings' gates; 40 rows in two patterns and complete rows."""
    d, k, n, nd = 3, 1, 40, 3
    model = model_with_priors("VD" if m == 273 else "GL", m, d, k, True, seed=12700 + m)
    Z, W = exact_draws(model, nd, seed=3)
    X = catalogue(model, n, seed=4)
    X[:17, 1] = NAN
    X[17:33, 0] = NAN
    X[17:33, 2] = NAN
    miss = np.isnan(X).any(axis=1)
    Psi = noise(n, d, seed=5) if noisy else None
    Xd, Pd = dev(X), None if Psi is None else dev(Psi)
    with gpz_amd.Predictor(model, large_m_missing=True) as p:
        F, Gam = draws(p, Xd, Pd, nd, Z=Z, return_gamma=True)
        assert torch.equal(F, draws(p, Xd, Pd, nd, Z=Z))
        assert ROUTE.format(4) in p.route, p.route
    assert Gam.shape == (nd, n, k)
    for s in range(nd):
        with gpz_amd.Predictor(with_weights(model, W[:, s, :]), large_m_missing=True) as q:
            mom = moments(q, Xd, Pd)
        a, b = nrel(host(F[s]), host(mom[0])), nrel(host(Gam[s])[miss], host(mom[4])[miss])
        print(f"m {m} draw {s}: draws {a:.3e} gamma_s {b:.3e}")
        assert a <= GATE_DRAW, (s, a)
        assert b <= GATE, (s, b)


# ---- 2b. more than 64 columns of draws: several launches of the gamma kernel ----------------------------------------------------------------
# k_pml_gamma carries at most 4 blocks of 16 columns per launch: 70 columns are launches of 4 and 1 blocks, 100 of 4 and 3, and 23
# draws of 3 outputs (69 columns, column o * 23 + s) of 4 and 1; the cases before this one stay inside one launch of 1 or 2 blocks.
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "psi"])
@pytest.mark.parametrize("m,k,nd,some", [(273, 1, 70, (0, 15, 16, 47, 48, 63, 64, 69)), (273, 1, 100, (0, 63, 64, 79, 80, 96, 99)),
                                         (385, 3, 23, (0, 11, 18, 22))])
def test_gamma_per_draw_over_several_launches(m, k, nd, some, noisy):
    """gamma_s and the draws of the draws in `some` (both sides of every launch and block edge) against a handle whose w is w_s; the
    first 3 draws of the call are the bits of a call with 3 draws; the stack with all the draws against the siblings' reduction."""
    d, n = 3, 40
    model = model_with_priors("VD", m, d, k, True, seed=12750 + m + nd)
    Z, W = exact_draws(model, nd, seed=3)
    X = catalogue(model, n, seed=4)
    X[:17, 1] = NAN
    X[17:33, 0] = NAN
    X[17:33, 2] = NAN
    miss = np.isnan(X).any(axis=1)
    Psi = noise(n, d, seed=5) if noisy else None
    Xd, Pd = dev(X), None if Psi is None else dev(Psi)
    with gpz_amd.Predictor(model, large_m_missing=True) as p:
        F, Gam = draws(p, Xd, Pd, nd, Z=Z, return_gamma=True)
        F3, Gam3 = draws(p, Xd, Pd, 3, Z=np.ascontiguousarray(Z[:, :3, :]), return_gamma=True)
        assert torch.equal(F[:3], F3) and torch.equal(Gam[:3], Gam3)
        assert noisy or np.all(host(Gam)[:, ~miss] == 0.0)             # (complete rows: gamma_s is 0 without Psi)
        groups, weights = setting(n, 2, seed=3)
        edges = np.linspace(*np.percentile(host(moments(p, Xd, Pd)[0]), [3, 97]), 8)
        res = stack(p, Xd, Pd, edges, n_draws=nd, Z=Z, groups=dev(groups, torch.int64), n_groups=2, weights=dev(weights))
        if noisy:
            ref, th, tm, tw, _ = stack_inputs_noisy(p, model, Xd, Pd, edges, nd, dict(Z=Z), groups, weights, 2)
        else:
            ref, th, tm, tw, _ = stack_inputs_clean(p, model, Xd, edges, nd, dict(Z=Z), groups, weights, 2)
        assert_close(res, ref, th, tm, tw, f"stack m {m} k {k} {nd} draws")
    for s_ in some:
        with gpz_amd.Predictor(with_weights(model, W[:, s_, :]), large_m_missing=True) as q:
            mom = moments(q, Xd, Pd)
        a, b = nrel(host(F[s_]), host(mom[0])), nrel(host(Gam[s_])[miss], host(mom[4])[miss])
        print(f"m {m} k {k} draw {s_} of {nd}: draws {a:.3e} gamma_s {b:.3e}")
        assert a <= GATE_DRAW, (s_, a)
        assert b <= GATE, (s_, b)


# ---- 3. the stack --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "psi"])
def test_the_stack_at_m_273(noisy):
    """Column 0 of the call with draws is the call without draws bit for bit and follows predict_dev's mu and sigma; column 1 + s follows
    the draws with the width beta + max(gamma_s, 0): the siblings' reference reduction over the handle's own per-row numbers at their
    tolerances."""
    m, n, d, k, G, B, nd = 273, 172, 3, 1, 2, 7, 5
    model = model_with_priors("VD", m, d, k, True, seed=12800)
    X = five_patterns(catalogue(model, n, seed=1))
    Psi = noise(n, d, seed=2) if noisy else None
    Xd, Pd = dev(X), None if Psi is None else dev(Psi)
    groups, weights = setting(n, G, seed=3)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, large_m_missing=True) as p:
        edges = np.linspace(*np.percentile(host(moments(p, Xd, Pd)[0]), [3, 97]), B + 1)
        res = stack(p, Xd, Pd, edges, n_draws=nd, seed=7, groups=gd, n_groups=G, weights=wd)
        zero = stack(p, Xd, Pd, edges, n_draws=0, groups=gd, n_groups=G, weights=wd)
        for u, v in zip((res.hist[:1], res.sum_w, res.sum_mu[:1], res.sum_mu2[:1]), zero[:4]):
            assert np.array_equal(u, v)
        if noisy:
            ref, th, tm, tw, _ = stack_inputs_noisy(p, model, Xd, Pd, edges, nd, dict(seed=7), groups, weights, G)
        else:
            ref, th, tm, tw, _ = stack_inputs_clean(p, model, Xd, edges, nd, dict(seed=7), groups, weights, G)
        assert_close(res, ref, th, tm, tw, f"stack m {m} {'psi' if noisy else 'clean'}")
        assert res.hist[1:].sum() > 0.0


# ---- 4. the same bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "psi"])
@pytest.mark.parametrize("m,k", [(273, 1), (385, 3)])
def test_same_bits_over_tiles_orders_company_splits_and_draw_counts(m, k, noisy):
    d, n = 3, 172
    model = model_with_priors("VD", m, d, k, True, seed=12900 + m)
    X = five_patterns(catalogue(model, n, seed=1))
    Psi = noise(n, d, seed=2) if noisy else None
    Xd, Pd = dev(X), None if Psi is None else dev(Psi)
    rows = lambda t, idx: None if t is None else t[idx]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    with gpz_amd.Predictor(model, large_m_missing=True) as p:
        ref = all_four(p, Xd, Pd, nd=7)
        same(rows_of(all_four(p, Xd[perm], rows(Pd, perm), nd=7), torch.argsort(perm)), ref, "a row permutation")
        parts = [all_four(p, Xd[i:j], rows(Pd, slice(i, j)), nd=7) for i, j in ((0, 61), (61, n))]
        same([torch.cat([u, v], dim=0 if u.dim() == 2 else 1) for u, v in zip(*parts)], ref, "a split into two calls")
        for i in (int(np.flatnonzero(np.isnan(X).any(axis=1))[0]), int(np.flatnonzero(np.isnan(X).all(axis=1))[0])):
            same(all_four(p, Xd[i:i + 1], rows(Pd, slice(i, i + 1)), nd=7), rows_of(ref, slice(i, i + 1)), f"row {i} alone")
        three = all_four(p, Xd, Pd, nd=3)
        same(three[:5], ref[:5], "the moments beside 3 draws")
        same(three[5:], [t[:3] for t in ref[5:]], "3 draws against the first 3 of 7")
        edges = np.linspace(*np.percentile(host(ref[0]), [3, 97]), 8)
        s1, s2 = (stack(p, Xd, Pd, edges, n_draws=7, seed=4) for _ in range(2))
        assert np.array_equal(s1.hist, s2.hist)
    with gpz_amd.Predictor(model, large_m_missing=True, tile_rows=32) as q:
        same(all_four(q, Xd, Pd, nd=7), ref, "tile_rows = 32")


# ---- 5. the flag changes nothing where it need not ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "psi"])
@pytest.mark.parametrize("m", [100, 256])
def test_the_flag_changes_nothing_up_to_256(m, noisy):
    n, d, k = 172, 3, 2
    model = model_with_priors("VD", m, d, k, True, seed=13000 + m)
    X = five_patterns(catalogue(model, n, seed=m))
    Psi = noise(n, d, seed=m + 1) if noisy else None
    Xd, Pd = dev(X), None if Psi is None else dev(Psi)
    groups, weights = setting(n, 2, seed=m)
    kw = dict(n_draws=6, seed=5, groups=dev(groups, torch.int64), n_groups=2, weights=dev(weights))
    with gpz_amd.Predictor(model, large_m_missing=True) as p, gpz_amd.Predictor(model) as q:
        assert p.info[1] == q.info[1]                                    # before any group: the same bytes
        a, b = all_four(p, Xd, Pd, nd=6), all_four(q, Xd, Pd, nd=6)
        same(a, b, "moments, draws, gamma per draw")
        edges = np.linspace(*np.percentile(host(a[0]), [3, 97]), 8)
        for u, v in zip(stack(p, Xd, Pd, edges, **kw), stack(q, Xd, Pd, edges, **kw)):
            assert np.array_equal(u, v)
        assert p.info[1] == q.info[1] and p.route == q.route and "k_pml" not in p.route


# ---- 6. the top of the range ---------------------------------------------------------------------------------------------------------------
# nrel of the one-shot route p.predict(X) against the oracle's predict_any at m = 1024 on the first 2 rows with missing values of the
# test below, measured once on one MI355X with `tools/predict_missing_large_timing.py yardstick`: neither side
# is the handle's route for such rows.  Four times the largest (gamma) is 7.4e-13, so the gate below is the siblings' 1e-11.
TOP_YARDSTICK = {"mu": 7.312e-16, "sigma": 8.958e-14, "nu": 1.199e-14, "beta_i": 2.210e-15, "gamma": 1.857e-13}


def top_gate(name):
    """The siblings' gate, or four times the yardstick above where that is larger (the longer sums; section 36's precedent)."""
    return max(GATE, 4.0 * TOP_YARDSTICK[name])


def top_inputs():
    m, d, k, n = 1024, 2, 1, 16
    model = model_with_priors("VD", m, d, k, True, seed=13100)
    X = catalogue(model, n, seed=4)
    X[:8, 1] = NAN
    return model, X


def test_the_top_of_the_range():
    """m = 1024: 524 800 pairs, U of 4.3 GB, eight K panels.  VD, d = 2, k = 1, 8 rows of one pattern and 8 complete rows against
    p.predict(X) of the same handle."""
    model, X = top_inputs()
    with gpz_amd.Predictor(model, large_m_missing=True) as p:
        ref = [np.array(a) for a in p.predict(X)[:5]]
        held0 = p.info[1]
        out = p.predict_dev(dev(X), missing=True)
        for name, u, v in zip(NAMES, out, ref):
            print(f"nrel top {name} {nrel(host(u), v):.3e} (gate {top_gate(name):.1e})")
        for name, u, v in zip(NAMES, out, ref):
            assert nrel(host(u), v) <= top_gate(name), (name, nrel(host(u), v), top_gate(name))
        assert np.all(host(out[4])[:8] > 0.0) and np.all(host(out[4])[8:] == 0.0)
        assert ROUTE.format(4) in p.route and "(8 pair chunks)" in p.route, p.route
        assert p.info[1] - held0 >= 8 * (npair(1024) * 1024)             # U alone: 4.3 GB, counted


# ---- 7. refusals and memory ------------------------------------------------------------------------------------------------------------------
def test_m_1025_is_refused_at_the_c_entries():
    m, n, d, k, nd, G, B = 1025, 8, 2, 1, 2, 1, 4
    model = model_with_priors("VD", m, d, k, False, seed=13200)
    X = catalogue(model, n, seed=1)
    X[:, 1] = NAN
    Xd, Pd, obs = dev(X), dev(noise(n, d, seed=2)), 0b01
    edges = np.linspace(-1.0, 1.0, B + 1)
    with gpz_amd.Predictor(model, large_m_missing=True) as p:
        for call in (lambda: p.predict_dev(Xd, missing=True), lambda: p.predict_noisy_missing_dev(Xd, Pd),
                     lambda: p.stack_missing_dev(Xd, edges)):
            with pytest.raises(ValueError, match="m <= 1024, not m = 1025"):
                call()
        held = p.info[1]
        muX, sdX, muY = p._norm_vectors()
        sd2 = np.ascontiguousarray(sdX ** 2)
        stream = torch.cuda.current_stream(Xd.device).cuda_stream
        pri = p._priors
        rcs = []

        def said(rc):
            rcs.append((rc, p._lib.gpz_last_error().decode()))

        out = [torch.full((k, n), -7.0, dtype=torch.float64, device=DEV).T for _ in range(10)]
        F = [torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV) for _ in range(2)]
        h = p._handle()
        said(p._lib.gpz_predictor_run_missing_dev(h, *p._x_args(Xd), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY), _lib.dptr(pri), obs,
                                                  *(t.data_ptr() for t in out[:5]), stream))
        said(p._lib.gpz_predictor_draws_missing_dev(h, *p._x_args(Xd), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY), _lib.dptr(pri), obs,
                                                    nd, 5, None, F[0].data_ptr(), stream))
        lead = [h, *p._x_args(Xd), *p._psi_args(Pd, n), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(sd2), _lib.dptr(muY), _lib.dptr(pri), obs]
        said(p._lib.gpz_predictor_run_noisy_missing_dev(*lead, *(t.data_ptr() for t in out[5:]), stream))
        said(p._lib.gpz_predictor_draws_noisy_missing_dev(*lead, nd, 5, None, F[1].data_ptr(), stream))
        torch.cuda.synchronize()
        r1 = raw_stack(p, Xd, obs, nd, G, B, edges)
        r2 = raw_stack_noisy(p, Xd, Pd, obs, nd, G, B, edges)
        rcs += [(r1[0], r1[1]), (r1[2], r1[3]), (r2[0], r2[1]), (r2[2], r2[3])]
        for rc, msg in rcs:                                              # all eight entries: the code, m and the limit
            assert rc == ERR_UNSUPPORTED and "predict_missing_large_fits" in msg and "m 1025" in msg and "1024" in msg, (rc, msg)
        assert all(bool((t == -7.0).all()) for t in out + F + list(r1[5]) + list(r2[5]))
        assert all(np.all(a == -7.0) for a in list(r1[4]) + list(r2[4]))
        assert p.info[1] == held and "missing" not in p.route


def test_without_the_flag_the_c_entry_keeps_its_refusal():
    model = model_with_priors("VD", 273, 2, 1, False, seed=13300)
    X = catalogue(model, 8, seed=1)
    X[:, 1] = NAN
    for flags in ({}, {"large_m": True}):
        with gpz_amd.Predictor(model, **flags) as p:
            muX, sdX, muY = p._norm_vectors()
            out = [torch.full((1, 8), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
            h = p._handle()
            with pytest.raises(_lib.GpzError) as ei:
                _lib.check(p._lib.gpz_predictor_run_missing_dev(h, *p._x_args(dev(X)), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                                None, 0b01, *(t.data_ptr() for t in out), None))
            assert ei.value.code == ERR_UNSUPPORTED
            assert ("missing inputs on the handle need predict_missing_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, k <= 8 and "
                    "ceil16(m) <= 256 (method VD, d 2, m 273, k 1); gpz_predict_missing takes every shape") in str(ei.value)
            assert all(bool((t == -7.0).all()) for t in out)


def test_memory_is_added_once_and_counted():
    """m = 273: the first call for a group adds the tile buffers and the pattern's tables (U: pairs padded to 64 x ceil16(m) doubles),
    counted in info[1]; the same pattern again, ten times the rows and another pattern add nothing."""
    m, d, k, n = 273, 3, 1, 60
    model = model_with_priors("VD", m, d, k, True, seed=13400)
    X = catalogue(model, 10 * n, seed=1)
    X[:, 1] = NAN
    other = X.copy()
    other[:, 1] = X[:, 0]
    other[:, 0] = NAN
    Xd, Od = dev(X), dev(other)
    with gpz_amd.Predictor(model, large_m_missing=True) as p, gpz_amd.Predictor(model, large_m_missing=True) as q:
        q.predict_dev(dev(X[:, [0, 0, 2]]))                              # a handle that never sees a row with NaN ...
        p.predict_dev(dev(X[:, [0, 0, 2]]))
        held = p.info[1]
        assert held == q.info[1]
        first = all_four(p, Xd[:n], None)
        grown = p.info[1]
        u_bytes = 8 * ((npair(m) + 63) // 64 * 64) * 288
        assert grown - held >= u_bytes
        same(all_four(p, Xd[:n], None), first, "the same pattern again")
        assert p.info[1] == grown
        all_four(p, Xd, None)
        all_four(p, Od[:n], None)
        assert p.info[1] == grown
        same(all_four(p, Xd[:n], None), first, "after another pattern")
        assert q.info[1] == held                                         # ... holds what it held
