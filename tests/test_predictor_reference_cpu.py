"""The checker of test_predictor_sweep.py is right and has teeth (CPU only): the extended-precision restatement of
predictor_reference.py against the project's own ground truth (oracle.predict on the sweep's models, the frozen complete-row
fixtures), its gates against a plain float64 evaluation of the same direct form (which must pass on every model of the sweep) and
against six mutants of it (each of which must fail), and the sweep table against the routes and instantiations parsed from the
kernel sources.

Worst error / gate of the float64 evaluation over the sweep's models (203 rows each; printed by the tests below):
    PHI 0.35, mu 0.39, nu 0.10, ln beta 0.48, beta 0.23, sigma 0.29
so the gates hold a correctly rounded float64 evaluation with a factor 2 to 10 to spare, and no more."""
import os
import re

import numpy as np
import pytest

import predictor_reference as R
from helpers import golden_names, load_predict_golden, rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, nrel, synth_model

pytestmark = pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_WHY)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def sweep_model(case, hetero=True):
    method, d, m, k = case
    model = synth_model(method, m, d, k, hetero, seed=R.case_seed(*case))
    return model, catalogue(model, R.WIDTH_N, seed=R.case_seed(*case) + 1)


def check_case(case, worst):
    """The reference against oracle.predict at check_parity's gates (test_predictor.py), then the float64 evaluation inside the gates."""
    model, X = sweep_model(case)
    ref = R.predict_reference(model, X)
    mu, sigma, nu, beta, _, PHI = O.predict(X, model)[:6]
    e = {"mu": nrel(mu, f64(ref["mu"])), "beta": nrel(beta, f64(ref["beta"])), "nu": nrel(nu, f64(ref["nu"])),
         "sigma": nrel(sigma, f64(ref["sigma"])), "PHI": nrel(PHI, f64(ref["PHI"]))}
    assert e["mu"] <= 1e-12 and e["beta"] <= 1e-12 and e["nu"] <= 1e-11 and e["sigma"] <= 1e-11 and e["PHI"] <= 1e-13, (case, e)
    gate = R.gates(ref, model)
    out = R.predict_direct(model, X)
    worst.add(R.assert_within({key: out[key] for key in R.QUANTITIES + ("lnbeta",)}, ref, gate, R.case_id(case)), R.case_id(case))


def test_reference_matches_the_oracle_and_float64_passes_the_gates_on_the_width_sweep():
    worst = R.Worst()
    for case in R.width_cases():
        check_case(case, worst)
    print("float64 evaluation, worst error / gate over the width sweep:", worst)


def test_reference_matches_the_oracle_and_float64_passes_the_gates_on_the_block_edge_sweep():
    worst = R.Worst()
    for case in R.edge_cases():
        check_case(case, worst)
    print("float64 evaluation, worst error / gate over the block-edge sweep:", worst)


def test_reference_matches_the_oracle_and_float64_passes_the_gates_on_the_row_and_stack_models():
    worst = R.Worst()
    for method, m, d, k in R.ROW_MODELS:
        check_case((method, d, m, k), worst)
    check_case(R.STACK_MODEL, worst)
    print("float64 evaluation, worst error / gate over the row-count and stack models:", worst)


def test_the_mu_gate_needs_the_muY_term():
    """A row that no basis function covers has mu = muY to the last bit but one, and sum_j |w_j| PHI_ij far below |mu|: the rounding of
    mu + muY is outside the product's bound.  The float64 evaluation misses the gate without the term, by orders of magnitude."""
    case = ("GL", 20, 33, 2)
    model, X = sweep_model(case)
    ref = R.predict_reference(model, X)
    gate = R.gates(ref, model)
    out = R.predict_direct(model, X)
    bare = {"mu": gate["mu"] - R.EPS * np.abs(f64(ref["mu"]))}
    assert R.ratios({"mu": out["mu"]}, ref, bare)["mu"][0] > 100.0
    assert R.ratios({"mu": out["mu"]}, ref, gate)["mu"][0] <= 1.0


def _complete_p():
    """The frozen predict() fixtures without input noise: their complete rows are inside the restatement (a row is computed on its own)."""
    return [name for name in golden_names("p_") if load_predict_golden(name)[2] is None]


def _complete_ref():
    import test_reference_run as RR
    names = []
    for name in golden_names("ref_predict_"):
        _, Xs, Psi = RR.predict_inputs(RR.load(name))
        if Psi is None and not np.isnan(Xs).any():
            names.append(name)
    return names


COMPLETE_P, COMPLETE_REF = _complete_p(), _complete_ref()


def test_some_fixtures_are_inside_the_restatement():
    print(f"no-Psi fixtures: {COMPLETE_P} of p_* (their complete rows), {COMPLETE_REF} of ref_predict_*")
    assert len(COMPLETE_P) >= 4 and len(COMPLETE_REF) >= 6


@pytest.mark.parametrize("name", COMPLETE_P)
def test_reference_on_the_frozen_predict_fixtures(name):
    """The complete rows of the no-Psi fixtures, at the gate of test_predict_golden_through_the_predictor."""
    g, model, _ = load_predict_golden(name)
    full = ~np.isnan(g["Xs"]).any(axis=1)
    assert full.sum() >= 4
    ref = R.predict_reference(model, g["Xs"][full])
    for key, have in (("mu", "mu"), ("sigma", "sigma"), ("nu", "nu"), ("beta_i", "beta"), ("PHI", "PHI")):
        assert rel(f64(ref[have]), g[key][full]) <= 1e-8, (key, rel(f64(ref[have]), g[key][full]))
    assert np.all(g["gamma"][full] == 0.0)


@pytest.mark.parametrize("name", COMPLETE_REF)
def test_reference_on_the_executed_reference_predict(name):
    """What the reference implementation's predict returned, at the gates of test_executed_reference_predict_through_the_predictor."""
    import test_reference_run as RR
    g = RR.load(name)
    model, Xs, _ = RR.predict_inputs(g)
    ref = R.predict_reference(model, Xs)
    tol = max(1e-8, 2000.0 * RR.cov_cond(model, g["theta"]) * 2.2e-16)
    for key, have in (("mu", "mu"), ("sigma", "sigma"), ("nu", "nu"), ("beta_i", "beta"), ("PHIs", "PHI")):
        assert rel(f64(ref[have]), g[key]) <= tol, (key, rel(f64(ref[have]), g[key]))


# ---- the gates are not too loose ------------------------------------------------------------------------------------------------------
MUTANT_MODELS = [("VD", 5, 33, 2), ("VC", 7, 100, 3), ("GC", 13, 254, 2), ("GL", 20, 33, 2), ("VD", 20, 254, 2), ("VC", 1, 33, 2),
                 ("GC", 8, 17, 1)]


def flagged(out, ref, gate):
    """The quantities that assert_within refuses (it must refuse: the caller asserts that the set is not empty)."""
    with pytest.raises(AssertionError):
        R.assert_within(out, ref, gate, "mutant")
    return {key for key, r in R.ratios(out, ref, gate).items() if not r[0] <= 1.0}


@pytest.mark.parametrize("case", MUTANT_MODELS, ids=R.case_id)
def test_mutants_fail_the_checker(case):
    model, X = sweep_model(case)
    m, k, n = model.m, model.k, X.shape[0]
    ref = R.predict_reference(model, X)
    gate = R.gates(ref, model)
    par, Xn = ref["_par"], ref["_Xn"]
    q = R.quadratic_form(model, par, Xn, np.float64)
    PHI = np.exp(-q / 2)

    def result(PHI, **kw):
        out = {"PHI": PHI}
        out.update(R.outputs_from_phi(model, par, PHI, np.float64, **kw))
        return {key: out[key] for key in R.QUANTITIES}

    good = result(PHI)
    R.assert_within(good, ref, gate, "unmutated")
    # one row's mu off by 1e-10 relative
    out = {key: val.copy() for key, val in good.items()}
    out["mu"][n // 2] *= 1.0 + 1e-10
    assert flagged(out, ref, gate) == {"mu"}
    # basis function m - 1 dropped for the rows of the last 32-row block only
    P2 = PHI.copy()
    P2[(n - 1) // 32 * 32:, m - 1] = 0.0
    assert "PHI" in flagged(result(P2), ref, gate)
    # PHI through a float32 exp
    P2 = np.exp((-q / 2).astype(np.float32)).astype(np.float64)
    assert "PHI" in flagged(result(P2), ref, gate)
    # the w and v columns swapped for output k - 1
    w2, v2 = par["w"].copy(), par["v"].copy()
    w2[:, k - 1], v2[:, k - 1] = par["v"][:, k - 1], par["w"][:, k - 1]
    assert {"mu", "beta"} <= flagged(result(PHI, w=w2, v=v2), ref, gate)
    # the padded dimension read as non-zero: q + 1e-12.  (The covariance gate is C (q + sum |s| T) eps with C = 8 de: from de = 12 on that
    # is wider than 1e-12 on every row of these models, which is what a gate that follows |R||x| + |R||p| costs; the narrower widths see it.)
    if model.method[1] != "C" or R.pad_dim(model.d) <= 8:
        assert "PHI" in flagged(result(np.exp(-(q + 1e-12) / 2)), ref, gate)
    # b left out of beta
    assert {"beta", "sigma"} <= flagged(result(PHI, b=np.zeros(k)), ref, gate)


def test_assert_within_reports_the_worst_element():
    case = ("VD", 5, 33, 2)
    model, X = sweep_model(case)
    ref = R.predict_reference(model, X)
    gate = R.gates(ref, model)
    out = {"nu": f64(ref["nu"]).copy()}
    out["nu"][17, 1] *= 1.0 + 1e-9
    with pytest.raises(AssertionError, match=r"nu .* at \(17, 1\)"):
        R.assert_within(out, ref, gate, "one element")
    out["nu"][17, 1] = np.nan
    with pytest.raises(AssertionError, match=r"nu inf at \(17, 1\)"):
        R.assert_within(out, ref, gate, "a NaN")


# ---- the sweep table reaches what it is there to reach ----------------------------------------------------------------------------------
def test_route_mirror_agrees_with_the_sources():
    widths = list(R.PS_WIDTHS)
    assert R.parsed_cases("k_predict_phi.h", "inline bool ps_width_instantiated") == widths
    assert R.parsed_cases("k_predict_small.hip", "static int launch_ps_k") == widths
    assert R.parsed_cases("k_predict_draws.hip", "static int launch_pd_k") == widths
    src = open(os.path.join(R.CSRC, "gpz_ctx.h")).read()
    sup = re.search(r"static const int sup\[\] = \{([^}]*)\}", src).group(1)
    assert [int(v) for v in sup.split(",")] == widths
    assert all(R.pad_dim(d) == min(w for w in widths if w >= d) for d in range(1, 21)) and R.pad_dim(24) == 24
    for name in ("k_predict_small.hip", "k_predict_draws.hip"):
        assert int(re.search(r"#define PS_LDA (\d+)", open(os.path.join(R.CSRC, name)).read()).group(1)) == 262
    small = open(os.path.join(R.CSRC, "k_predict_small.hip")).read()
    draws = open(os.path.join(R.CSRC, "k_predict_draws.hip")).read()
    phi = open(os.path.join(R.CSRC, "k_phi.hip")).read()
    assert "bool phi_is_wide(int de, int k) { return de > 20 || k > 8; }" in phi
    assert "if (phi_is_wide(de, k) || !ps_width_instantiated(de)) return false;" in small
    assert "return ((m + 2 * k + 15) / 16) * 16 <= 256 && predict_small_lds(de) <= 80 * 1024;" in small
    assert "return ((size_t)32 * PS_LDA + 32 * (size_t)de + 4 * 32) * sizeof(double); }" in small
    assert "if (phi_is_wide(de, 1) || !ps_width_instantiated(de)) return false;" in draws
    assert "return ((m + 15) / 16) * 16 <= 256 && predict_draws_lds(de) <= 80 * 1024;" in draws
    assert "return ((size_t)32 * PS_LDA + 32 * (size_t)de) * sizeof(double); }" in draws
    assert "const bool split = nbc < 4;" in draws
    # the boundary the sweep leans on
    assert R.routes("VD", 5, 256 - 2 * 8, 8) == (True, True) and R.routes("VD", 5, 254, 2) == (False, True)
    assert R.routes("VD", 5, 256, 1) == (False, True) and R.routes("VD", 5, 257, 1) == (False, False)
    assert R.routes("VD", 5, 40, 9) == (False, True)      # k = 9: predict on tiles (phi_is_wide), the draws kernel does not look at k


def test_sweep_table_reaches_every_instantiation_block_count_and_split():
    cases = R.width_cases() + R.edge_cases()
    assert len(set(cases)) == len(cases)
    small, draws, nk_small, nk_draws, splits = set(), set(), set(), set(), set()
    for method, d, m, k in cases:
        de, cov = R.pad_dim(d), method[1] == "C"
        fused_p, fused_d = R.routes(method, d, m, k)
        if fused_p:
            small.add((de, cov))
            nk_small.add(R.ceil16(m))
        if fused_d:
            draws.add((de, cov))
            nk_draws.add(R.ceil16(m))
            splits |= R.draws_splits(3 * k) | R.draws_splits(m * k)      # the sweep's two draws calls: 3 draws of Z = 0, m of Z = I
    every = {(de, cov) for de in R.PS_WIDTHS for cov in (False, True)}
    assert len(every) == 22 and small == every and draws == every
    assert nk_small == set(range(16, 257, 16)) and nk_draws == set(range(16, 257, 16))
    assert splits == {False, True}
    # covariance kinds at every zero-padded width, on the fused routes
    padded = {d for method, d, m, k in cases if method[1] == "C" and R.pad_dim(d) != d and R.routes(method, d, m, k)[0]}
    assert padded == {7, 9, 11, 13, 14, 15, 17, 18, 19}
    # k up to the fused limit, and past it
    assert {k for _, _, _, k in cases} >= {1, 2, 3, 8, 9}
    assert any(not R.routes(*c)[0] and R.routes(*c)[1] and c[2] == 256 for c in cases)
    assert any(R.routes(*c) == (False, False) and c[2] == 257 for c in cases)
