"""The streaming predictor on the GPU against the extended-precision restatement of predictor_reference.py, element by element, at
every input width, block edge and row count, and the stack kernel at every size of a row's edge window.

A  widths      d = 1 .. 20 x {GL, VD, GC, VC}, m = 33 (both fused kernels) and 254 (fused draws, tiled predict), k = 2: all 22
               instantiations of k_predict_small and of k_predict_draws, every zero-padded covariance width, the device layouts
B  block edges m around every multiple of 16 up to 257, k = 1, 3, 8 (and 9: tiles), d = 5 VD and d = 7 VC
C  row counts  around a 32-row block, a 64-row and a 1024-row tile
D  stack       B = 63 .. 4096 bins on three edge grids: every stack_pass<NE>, the multi-pass loop, the hand-over at lane 63; the
               far tails against 50-digit values

Every case opens its own handle; nothing here retries a GPU step.  test_predictor_reference_cpu.py checks the checker.  The worst
error / gate per quantity is printed when the module finishes (run with -s).

Measured on an MI355X, worst error / gate over the module (478 tests, 70 s):
    PHI 0.35 (GL d=1 m=254), mu 0.39 and draws mu 0.39 (GL d=20 m=33: the rounding of + muY), nu 0.12 (VD d=5 m=1 k=3),
    beta 0.23 and sigma 0.29 (VD d=20 m=33), hist 2.2e-4 (geometric grid, 65 bins), hist tails 0.25 (the bin that straddles +9 widths)
- the same figures, to two digits, as the float64 NumPy evaluation of test_predictor_reference_cpu.py: the kernels are as accurate as a
correctly rounded float64 evaluation of the direct form, on every route."""
import numpy as np
import pytest

import gpz_amd
import predictor_reference as R
from test_predictor import catalogue, nrel, synth_model
from test_predictor_draws import eye_z
from test_predictor_stack import assert_close, edges_for, reference_of, setting

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_WHY)]

WORST = R.Worst()
F64 = np.float64


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\ntest_predictor_sweep: worst error / gate per quantity:", WORST)


def f64(a):
    return np.asarray(a, dtype=F64)


def check_draws(p, model, X, ref, gate, what):
    """Z = 0 gives mu within the mu gate; Z = I_m: the identities of check_exact_covariance (test_predictor_draws.py) at its gate,
    with mu, nu and PHI from the reference."""
    m, k = model.m, model.k
    F0 = p.draws(X, 3, Z=np.zeros((m, 3, k)))
    for s in range(3):
        WORST.add({"draws mu": R.assert_within({"mu": F0[s]}, ref, gate, (what, "Z = 0", s))["mu"]}, what)
    F = p.draws(X, m, Z=eye_z(m, k))
    assert F.shape == (m, X.shape[0], k)
    D = (F.astype(R.LD) - ref["mu"][None]).astype(F64)
    nu, PHI = f64(ref["nu"]), f64(ref["PHI"])
    e_nu = nrel(np.sum(D * D, axis=0), nu)
    assert e_nu <= 1e-10, (what, e_nu)
    iS = ref["_par"]["iS"]
    for o in range(k):
        S = 0.5 * (iS[:, :, o] + iS[:, :, o].T)
        e_c = nrel(D[:, :, o].T @ D[:, :, o], PHI @ S @ PHI.T)
        assert e_c <= 1e-10, (what, o, e_c)


def check_handle(case, model, X, ref, gate, force_tiles, tile_rows):
    """One handle: the route it says it takes, predict with PHI against the reference, the draws.  -> (handle's predict output)"""
    fused_p, fused_d = R.routes(*case)
    what = R.case_id(case) + (" forced tiles" if force_tiles else "")
    with gpz_amd.Predictor(model, tile_rows=tile_rows, force_tiles=force_tiles) as p:
        assert p.info[2] == (0 if fused_p and not force_tiles else 1), (what, p.route)
        out = p.predict(X, return_phi=True)
        assert np.all(out[4] == 0.0)
        WORST.add(R.assert_within(R.named(out), ref, gate, what), what)
        check_draws(p, model, X, ref, gate, what)
        want = "draws: fused k_predict_draws" if fused_d and not force_tiles else "draws: tiles k_phi + k_tgemm"
        assert want in p.route, (what, p.route)
    return out


def case_inputs(case, n=R.WIDTH_N):
    method, d, m, k = case
    model = synth_model(method, m, d, k, True, seed=R.case_seed(*case))
    X = catalogue(model, n, seed=R.case_seed(*case) + 1)
    ref = R.predict_reference(model, X)
    return model, X, ref, R.gates(ref, model)


# ---- A. widths --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.width_cases(), ids=R.case_id)
def test_widths(case):
    """203 rows over 64-row tiles: several tiles, a partial tile and a partial 32-row block."""
    import torch
    from test_predictor_dev import DEV, assert_same, host, layouts
    model, X, ref, gate = case_inputs(case)
    check_handle(case, model, X, ref, gate, False, R.WIDTH_TILE)
    check_handle(case, model, X, ref, gate, True, R.WIDTH_TILE)
    Xd = torch.from_numpy(X).to(DEV)
    with gpz_amd.Predictor(model, tile_rows=R.WIDTH_TILE) as p:
        want = p.predict(X, return_phi=True)
        WORST.add(R.assert_within(R.named(want), ref, gate, R.case_id(case)), R.case_id(case))
        for name, Xl in layouts(Xd).items():
            assert torch.equal(Xl, Xd)
            assert_same(p.predict_dev(Xl, return_phi=True), want, (case, name))
        X32 = Xd.float()
        assert_same(p.predict_dev(X32, return_phi=True), p.predict(host(X32.double()), return_phi=True), (case, "float32"))


# ---- B. block edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.edge_cases(), ids=R.case_id)
def test_block_edges(case):
    model, X, ref, gate = case_inputs(case)
    check_handle(case, model, X, ref, gate, False, R.WIDTH_TILE)
    check_handle(case, model, X, ref, gate, True, R.WIDTH_TILE)


def test_block_edge_routes():
    """What the table is there for: m = 256 is draws-fused and predict-tiled, m = 257 tiles for both, k = 9 predict-tiled."""
    for case, want in ((("VD", 5, 256, 1), (False, True)), (("VD", 5, 257, 1), (False, False)), (("VC", 7, 240, 8), (True, True)),
                       (("VC", 7, 241, 8), (False, True)), (("VD", 5, 40, 9), (False, True))):
        assert case in R.edge_cases() and R.routes(*case) == want, case


# ---- C. row counts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.ROW_TILES)
@pytest.mark.parametrize("spec", R.ROW_MODELS, ids=lambda s: "-".join(str(v) for v in s))
def test_row_counts(spec, T):
    """One handle per model and tile size, calls of every size around a 32-row block and a tile."""
    method, m, d, k = spec
    case = (method, d, m, k)
    model, X, ref, gate = case_inputs(case, n=2 * T + 5)
    with gpz_amd.Predictor(model, tile_rows=T) as p:
        assert p.info[2] == 0 and p.info[0] == T
        for n in R.row_counts(T):
            what = f"{R.case_id(case)} T={T} n={n}"
            rn, gn = R.rows_of(ref, slice(0, n)), {key: val[:n] for key, val in gate.items()}
            out = p.predict(X[:n], return_phi=True)
            assert all(a.shape[0] == n for a in out)
            WORST.add(R.assert_within(R.named(out), rn, gn, what), what)
            check_draws(p, model, X[:n], rn, gn, what)


# ---- D. stack windows -------------------------------------------------------------------------------------------------------------------
def windows(mu, s2, edges):
    """Per row the kernel's window (k_stack_tile): edges within +-9 widths of mu and one more on either side, as (ja, jb); the bins
    ja .. jb - 1 are the row's."""
    B = edges.size - 1
    s = np.sqrt(s2)
    l0 = np.searchsorted(edges, mu - 9.0 * s, side="left")             # edges below lo
    u0 = np.searchsorted(edges, mu + 9.0 * s, side="right")            # edges up to hi
    ja = np.maximum(l0 - 1, 0)
    jb = np.maximum(np.minimum(u0, B), ja)
    return ja, jb


def passes(ja, jb):
    """The stack_pass<NE> instantiations a row's window runs through, in order."""
    out, j0 = [], ja
    while j0 < jb:
        left = jb - j0 + 1
        ne = 4 if left > 128 else (2 if left > 64 else 1)
        out.append(ne)
        j0 += 64 * ne - 1
    return out


def window_census(mu, sigma, edges):
    """(set of NE reached, any row with several passes, fraction of rows of output 0 with more than 255 edges in the window)."""
    reached, multi = set(), False
    for o in range(mu.shape[1]):
        ja, jb = windows(mu[:, o], sigma[:, o], edges)
        for a, b in set(zip(ja.tolist(), jb.tolist())):
            ps = passes(a, b)
            reached |= set(ps)
            multi |= len(ps) > 1
    ja, jb = windows(mu[:, 0], sigma[:, 0], edges)
    return reached, multi, float(np.mean(np.where(jb > ja, jb - ja + 1, 0) > 255))


def grid(name, mu, sigma, B):
    if name == "fine":          # 600 edges within +-9 widths of a typical row, centred on the catalogue
        c, s = np.median(mu[:, 0]), np.sqrt(np.median(sigma[:, 0]))
        h = 18.0 * s / 600.0
        return c + h * (np.arange(B + 1) - B / 2.0)
    if name == "percentile":    # as test_predictor_stack.py
        return edges_for(mu, B)
    lo, hi = np.percentile(mu, [25, 75])                                 # geometric: part of mu below the first edge, part above the last
    return lo + (hi - lo) * (np.geomspace(1.0, 1000.0, B + 1) - 1.0) / 999.0


def stack_model():
    method, d, m, k = R.STACK_MODEL
    model = synth_model(method, m, d, k, True, seed=R.case_seed(*R.STACK_MODEL))
    return model, catalogue(model, R.STACK_N, seed=R.case_seed(*R.STACK_MODEL) + 1)


@pytest.mark.parametrize("name", ["fine", "percentile", "geometric"])
def test_stack_windows(name):
    model, X = stack_model()
    reached, multi = set(), False
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        mu, sigma = p.predict(X)[:2]
        for B in R.STACK_BINS:
            edges = grid(name, mu, sigma, B)
            assert np.all(np.diff(edges) > 0)
            r, mp_, frac = window_census(mu, sigma, edges)
            reached |= r
            multi |= mp_
            if name == "fine" and B >= 300:
                assert frac > 0.5, (B, frac)                             # most rows' windows hold more than 255 edges
            for n_draws in (0, 3):
                what = f"stack {name} B={B} draws={n_draws}"
                res = p.stack(X, edges, n_draws=n_draws, seed=5)
                ref, th, tm, tw = reference_of(p, model, X, edges, n_draws, 5, None, None, None, 1)
                WORST.add({"hist": float(np.max(np.abs(res.hist - ref[0]) / th[None, :, None, None]))}, what)
                assert_close(res, ref, th, tm, tw, what)
        G, B = 4, 1000
        groups, weights = setting(R.STACK_N, G, seed=7)
        edges = grid(name, mu, sigma, B)
        res = p.stack(X, edges, n_draws=3, seed=5, groups=groups, n_groups=G, weights=weights)
        ref, th, tm, tw = reference_of(p, model, X, edges, 3, 5, None, groups, weights, G)
        WORST.add({"hist": float(np.max(np.abs(res.hist - ref[0]) / th[None, :, None, None]))}, f"stack {name} B=1000 G=4")
        assert_close(res, ref, th, tm, tw, f"stack {name} B=1000 G=4")
    # the grid reaches every branch of the histogram loop: it cannot slide back into the path the older tests cover
    assert reached == {1, 2, 4}, (name, reached)
    assert multi, name


def test_passes_rule():
    """The host statement of the kernel's pass loop: 64 NE - 1 bins per pass."""
    assert passes(0, 0) == [] and passes(3, 4) == [1] and passes(0, 63) == [1] and passes(0, 64) == [2] and passes(0, 127) == [2]
    assert passes(0, 128) == [4] and passes(0, 255) == [4] and passes(0, 256) == [4, 1] and passes(10, 10 + 600) == [4, 4, 2]
    assert passes(0, 4096) == [4] * 16 + [1]


def test_stack_tail_accuracy():
    """64 copies of one row, 512 bins out to 9.5 widths on both sides of its mu, against 50-digit values.  Per bin, with t = (e - mu) / s
    at the bin's two edges, Q the normal tail and phi the density, W the sum of the weights and h the bin's exact value:

        W sum_edges [(6 + t^2) eps Q(|t|) + 3 eps |t| phi(t)] + (64 + 2) eps h

    The first term is stack_tail's stated accuracy ((6 + 2 x^2) eps relative with x = t / sqrt 2, test_predictor_stack_cpu.py), the
    second the rounding of t (a square root, a reciprocal, a difference and a product: 4 u < 3 eps, times |dQ / dt| = phi), the third
    the 64 adds into the bin - each rounds by at most u times a partial sum that never exceeds h, so eps h per add with the usual
    factor 2, below the eps W per add that a bound without the sign of the terms would give - and the rounding of the mass and of its
    product with the weight.  Bins wholly beyond the +-9 width cut are left out by the kernel: up to 1.1e-19 W, as it states."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    model = synth_model("VD", 60, 5, 1, True, seed=77)
    model.muY = np.zeros(1)                                              # the kernel's mu and edges are the caller's, bit for bit
    X = np.repeat(catalogue(model, 1, seed=78), 64, axis=0)
    weights = np.random.default_rng(79).uniform(0.5, 2.0, 64)
    B = 512
    with gpz_amd.Predictor(model) as p:
        out = p.predict(X)
        mu0, s2 = float(out[0][0, 0]), float(out[1][0, 0])
        assert np.all(out[0] == mu0) and np.all(out[1] == s2)
        edges = mu0 + np.sqrt(s2) * np.linspace(-9.5, 9.5, B + 1)
        hist = p.stack(X, edges, weights=weights).hist[0, 0, 0]
    W = mp.fsum(mp.mpf(float(w)) for w in weights)
    s = mp.sqrt(mp.mpf(s2))
    t = [(mp.mpf(float(e)) - mp.mpf(mu0)) / s for e in edges]
    cdf = [mp.ncdf(v) for v in t]
    edge_term = [(6 + v * v) * R.EPS * mp.ncdf(-abs(v)) + 3 * R.EPS * abs(v) * mp.npdf(v) for v in t]
    ja, jb = windows(np.array([mu0]), np.array([s2]), edges)
    ja, jb = int(ja[0]), int(jb[0])
    assert 0 < ja < 16 and B - 16 < jb < B                              # the cut falls inside the grid on both sides
    worst, at = 0.0, -1
    for j in range(B):
        h = W * (cdf[j + 1] - cdf[j])
        if ja <= j < jb:
            gate = W * (edge_term[j] + edge_term[j + 1]) + 66 * R.EPS * h
        else:
            assert min(abs(t[j]), abs(t[j + 1])) > 9
            gate = mp.mpf("1.1e-19") * W
        r = float(abs(mp.mpf(float(hist[j])) - h) / gate)
        if r > worst:
            worst, at = r, j
    print(f"stack tails: worst error / gate {worst:.3g} at bin {at} (t = {float(t[at]):.3f}); bins {ja} .. {jb - 1} inside the cut")
    WORST.add({"hist tails": worst}, f"bin {at}")
    assert worst <= 1.0, (worst, at, float(t[at]))
    assert hist[ja] > 0.0 and hist[jb - 1] > 0.0                         # the straddling bins are counted
