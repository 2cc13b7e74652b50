"""gpz_amd.predict (gpz_predict_full / _noisy / _missing) at the chunk and row edges of its host-side rules, on a real MI355X: every
case of predict_edges.CASES against the oracle's six outputs (computed here, or frozen in tests/golden/pe_*.npz where the oracle
needs more than ~2 s), every element against the sum of the absolute terms it is made of (predict_edges.term_scales) and never
under a max norm, and the route the call reports (gpz_predict_last_route) against the restated rule, so that a moved threshold
cannot take a case off its edge unnoticed.

Gates - the project's constants, not fitted to what the GPU returns: 1e-9 for the diagonal kinds, max(1e-8, 10 phi_tol) for GC / VC,
predictor_reference.gates for predictFull.  test_predict_edges_cpu.py holds the oracle itself to a tenth of them on every case.

Worst error / gate per entry and output as test_worst_ratios_report prints them with -s (one MI355X, the run recorded in DESIGN.md):
    N   (predictNoisy)                      PHI 1.4e-05  beta_i 7.8e-07  gamma 4.1e-06  mu 1.9e-06  nu 6.9e-06  sigma 2.9e-06
    MD  (predictMissing, diagonal kinds)    PHI 4.6e-04  beta_i 3.2e-07  gamma 8.3e-05  mu 8.2e-07  nu 6.8e-05  sigma 7.8e-07
    MC  (predictMissing, GC / VC)           PHI 3.6e-06  beta_i 4.0e-08  gamma 1.3e-06  mu 1.0e-06  nu 5.6e-07  sigma 8.7e-07
    F   (predictFull, its own gates)        PHI 0.28  beta 0.027  mu 0.0078  nu 0.0013  sigma 0.014
("One-shot prediction: what holds it", has the table, the fitness numbers and the self-check on a broken launcher.)"""
import numpy as np
import pytest

import gpz_amd
import predict_edges as E
import predictor_reference as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_WHY)]

WORST = {}          # entry -> R.Worst


def note(case, ratios):
    WORST.setdefault(case["entry"], R.Worst()).add(ratios, case["id"])


def check_route(case, route):
    """The entry, the kernel family and the counts the case was chosen for, as the call itself reports them."""
    rule = E.case_rule(case)
    assert case["pred"](rule), (case["id"], case["edge"], rule)
    entry, nums, words = E.parse_route(route)
    assert entry == {"N": "predict_noisy", "MD": "predict_missing", "MC": "predict_missing", "F": "predict_full"}[case["entry"]], route
    assert rule["family"] in words, (rule["family"], route)
    keys = {"N": ("nchunk", "ppc"), "MD": ("cw", "width", "passes", "last", "npg", "splits"),
            "MC": ("nchunk", "ppc", "rows_blk", "blocks"), "F": ("mp",)}[case["entry"]]
    for key in keys:
        assert nums[key] == rule[key], (key, nums[key], rule[key], route)
    if rule["family"].startswith(("pmc_fast", "pmc4")):
        assert nums["phi_chunks"] == rule["phi_chunks"] and nums["noisy"] == (1 if case["psi"] else 0), route
    if rule["family"].startswith("psi<") and not case["twin"]:      # variances arrive as a cube of diagonals and are seen as such
        assert nums["psi_diag"] == (1 if case["psi"] == "var" else 0) and nums["shared"] == (1 if case["method"] == "GC" else 0), route
    assert nums["n_pad"] == rule["n_pad"], (rule["n_pad"], route)


@pytest.mark.parametrize("case", [c for c in E.CASES if c["entry"] != "F"], ids=lambda c: c["id"])
def test_edge_case(case):
    model, Xs, Psi, ref, scales = E.expected(case)
    got = gpz_amd.predict(Xs, model, Psi=Psi)
    route = gpz_amd.predict_last_route()
    out = dict(zip(E.NAMES, got[:6]))
    gate = E.gate_of(model)
    res = E.scaled_errors(out, ref, scales)
    ratios = {name: r[0] / gate for name, r in res.items()}
    note(case, ratios)
    print(case["id"], route, "| error / gate:", ", ".join("%s %.2e" % (name, v) for name, v in sorted(ratios.items())))
    bad = {name: (r[0], r[1]) for name, r in res.items() if not r[0] <= gate}
    assert not bad, (case["id"], case["edge"], "scaled error beyond the gate %.1e at (row, column): %r" % (gate, bad))
    check_route(case, route)


@pytest.mark.parametrize("case", [c for c in E.CASES if c["entry"] == "F"], ids=lambda c: c["id"])
def test_predict_full_edge_case(case):
    model, Xs, _ = E.run_inputs(case)
    ref = R.predict_reference(model, Xs)
    got = gpz_amd.predict(Xs, model)
    route = gpz_amd.predict_last_route()
    assert np.all(got[4] == 0.0)
    out = {"mu": got[0], "sigma": got[1], "nu": got[2], "beta": got[3], "PHI": got[5]}
    ratios = R.assert_within(out, ref, R.gates(ref, model), case["id"])
    note(case, ratios)
    check_route(case, route)


def test_route_text_is_per_call_and_survives_it():
    """The text names the LAST call of this thread, stays readable after it and starts anew with the next one."""
    case = E.CASE_BY_ID["N-VD-d5-k1-m23-synth"]
    model, Xs, Psi = E.run_inputs(case)
    gpz_amd.predict(Xs, model, Psi=Psi)
    first = gpz_amd.predict_last_route()
    assert first == gpz_amd.predict_last_route() and first.startswith("predict_noisy:") and first.count("noisy_diag") == 1
    gpz_amd.predict(Xs, model)
    second = gpz_amd.predict_last_route()
    assert second.startswith("predict_full:") and "noisy" not in second


def test_worst_ratios_report():
    """Last in the file: the worst error / gate per entry and output over the run (the module docstring records a run)."""
    for entry in sorted(WORST):
        print("worst error / gate, %s: %s" % (entry, WORST[entry]))
