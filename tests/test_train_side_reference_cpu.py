"""The checker of test_lbfgs_edges.py and test_prior_edges.py, checked: tests/train_side_reference.py against the oracle's float64
restatements and the executed reference's fixtures, and every fitness condition of its case tables on the reference alone - the
inputs the GPU tests run are the inputs judged here.  No GPU, no built library."""
import os

import numpy as np
import pytest

import train_side_reference as R
from gpz_amd import host
from helpers import GOLDEN, make_problem, rel
from oracle import gpz_oracle as O
from oracle import minfunc_oracle as MF
from test_gpu_parity import phi_tol

pytestmark = pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_WHY)


# ---- the L-BFGS memory ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,corr,steps", [(64, 3, 14), (513, 7, 25), (200, 100, 30)])
def test_two_loop_and_ring_agree_with_the_restated_lbfgs_files(p, corr, steps):
    """Ring / two_loop against oracle/minfunc_oracle.py's lbfgsAdd / lbfgsProd (float64, MATLAB's ring indices) call by call."""
    S = np.zeros((p, corr)); Y = np.zeros((p, corr)); YS = np.zeros(corr)
    start, end, hd = 1, 0, 1.0
    ring = R.Ring(corr)
    for g, g_old, t, d in R.lbfgs_steps(p, steps):
        start, end, hd, skipped = MF.lbfgsAdd(g - g_old, t * d, S, Y, YS, start, end, hd)
        assert ring.add_step(g, g_old, t, d) == (not skipped)
        assert abs(float(ring.hdiag) - hd) <= 1e-13 * abs(hd)
        want = MF.lbfgsProd(g, S, Y, YS, start, end, hd) if end > 0 else -g
        assert R.rel_ld(ring.direction(g), want) <= 1e-13
    assert ring.accepted > corr or steps <= corr


def test_two_loop_agrees_with_the_executed_lbfgs_files():
    """... and against what lbfgsAdd.m / lbfgsProd.m themselves returned (tests/golden/ref_lbfgs_mem.npz)."""
    z = np.load(os.path.join(GOLDEN, "ref_lbfgs_mem.npz"))
    ring = R.Ring(int(z["corrections"]))
    n_added = 0
    for it in range(z["T"].size):
        g, g_old = z["G"][it + 1], z["G"][it]
        assert ring.add_step(g, g_old, float(z["T"][it]), z["D"][it]) == bool(z["added"][it])
        n_added += int(z["added"][it])
        if n_added:
            assert R.rel_ld(ring.direction(g), z["directions"][it]) <= 1e-13, it
    assert n_added > int(z["corrections"])


def test_gram_form_is_the_two_loop():
    """gram_direction_f64 from a list of pairs equals the incrementally grown GramMemory64 and the float64 two-loop to rounding."""
    rng = np.random.default_rng(0)
    pairs = []
    for _ in range(6):
        s = rng.standard_normal(300)
        pairs.append((s, 0.5 * s + 0.1 * rng.standard_normal(300)))
    g = rng.standard_normal(300)
    hd = float(pairs[-1][0] @ pairs[-1][1] / (pairs[-1][1] @ pairs[-1][1]))
    assert R.rel_ld(R.gram_direction_f64(pairs, g, hd), R.two_loop(pairs, g, hd)) <= 1e-13
    assert np.array_equal(R.gram_direction_f64([], g, 1.0), -g)


@pytest.mark.parametrize("p,corr,steps", R.LBFGS_CASES)
def test_lbfgs_cases_are_fit(p, corr, steps):
    """e_ref <= 1e-13 on every row, and the ring really wraps: corrections + 5 accepted pairs wherever steps > corrections."""
    ref = R.lbfgs_case(p, corr, steps, host._LBFGS)
    print("p = %d, corrections = %d: two-loop %.2e, Gram form %.2e, accepted %d of %d" %
          (p, corr, ref["e_two_loop"], ref["e_gram"], ref["accepted"], steps))
    assert ref["e_ref"] <= R.LBFGS_FITNESS
    if steps > corr:
        assert ref["accepted"] >= corr + R.LBFGS_WRAP_MARGIN
    assert not all(ref["added"])                                  # rejected pairs in between


# ---- getPrior and N ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,psi,nanfrac", [("VD", False, 0.0), ("VC", False, 0.0), ("VD", True, 0.3), ("GL", False, 0.0)])
def test_fixed_point_in_float64_is_the_oracles(method, psi, nanfrac):
    model, theta, X, _, Psi, _ = make_problem(400, 3, 7, 1, method, True, seed=77, psi=psi, nanfrac=nanfrac)
    want, count = O.getPrior(X, Psi, theta, model, None, return_iterations=True)
    N = O.getPHI(X, Psi, theta, model, None, want_N=True)[3]
    got, it, ratios = R.prior_fixed_point(N, np.float64)
    assert it == count == len(ratios) and got.dtype == np.float64
    assert rel(got, want) <= 1e-14


@pytest.mark.parametrize("method,d,n,m", [("VD", 2, 300, 65), ("VC", 3, 130, 257), ("GL", 2, 130, 40), ("VL", 4, 50, 9), ("GC", 3, 60, 12)])
def test_norm_densities_agree_with_the_oracle(method, d, n, m):
    model, theta, X = R.n_problem(method, d, n, m)
    N = O.getPHI(X, None, theta, model, None, want_N=True)[3]
    assert rel(R.norm_densities(model, theta, X), N) <= phi_tol(model, theta)


@pytest.mark.parametrize("case", R.PRIOR_CASES, ids=[c["id"] for c in R.PRIOR_CASES])
def test_prior_cases_are_fit(case):
    """The last eight columns carry weight, the long-double prior sums to one, and the float64 fixed point on the same N is within
    the gate's reach of it (1e-8 is the project's gate; the arithmetic is some six orders below)."""
    prior, it, ratios, N = R.prior_reference(case["id"])
    m = case["m"]
    w = R.tail_weight(prior, m)
    p64 = R.prior_fixed_point(np.asarray(N, dtype=np.float64), np.float64)[0]
    print("%s: tail weight %.3f, %d iterations, float64 against long double %.2e" % (case["id"], w, it, R.rel_ld(p64, prior)))
    assert np.all(np.isfinite(np.asarray(prior, dtype=np.float64)))
    assert w >= R.PRIOR_TAIL_FITNESS
    assert abs(float(prior.sum() - 1)) <= 1e-15
    assert R.rel_ld(p64, prior) <= 1e-12


@pytest.mark.parametrize("which", list(R.COUNTED))
def test_counted_cases_are_decidable(which):
    """The three iteration counts fall where they are meant to, and neither the stopping ratio nor the one before it is within 1 %
    of 1e-10; the float64 fixed point counts the same."""
    prior, it, ratios = R.counted_reference(which)
    lo, hi = R.COUNTED[which]
    print("%s: %d iterations, last ratios %s" % (which, it, ", ".join("%.3e" % r for r in ratios[max(0, it - 2):it])))
    assert lo <= it <= hi and len(ratios) == it
    assert R.count_is_decidable(it, ratios)
    model, theta, X = R.counted_problem(which)
    assert O.getPrior(X, None, theta, model, None, return_iterations=True)[1] == it


# ---- Dxy -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DXY_CASES, ids=[c["id"] for c in R.DXY_CASES])
def test_dxy_cases_are_fit(case):
    """The oracle's float64 Dxy meets the gate the kernel is held to, on every case."""
    X, Y = R.dxy_inputs(case)
    D_ld, T = R.dxy_reference(case["id"])
    worst = R.dxy_worst(O.Dxy(X, Y), D_ld, T, case["d"])
    print("%s: oracle error / gate %.3f" % (case["id"], worst))
    assert D_ld.shape == (case["nx"], case["ny"]) and worst <= 1.0
    if case["coincident"]:                                        # the diagonal is zero up to the long-double rounding of the formula
        assert float(np.max(np.diagonal(D_ld) / np.diagonal(T))) <= 2.0 ** -60
