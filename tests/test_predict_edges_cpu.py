"""Host-side checks of tests/predict_edges.py, no GPU: the restated rules against the sources they cite, every case against its
predicate, the extended-precision reference against the oracle, the |w| trick against the sums formed term by term, the fixtures
against the table, and the FITNESS of every case - measured on the references alone, before any kernel is judged on it:

    e_ref   the oracle against the extended-precision reference in the per-element scaled measure, at most a tenth of the gate:
            of the case itself for a diagonal kind, of its diagonal-Gamma twin for GC / VC (computed here, or read from the fixture
            where make_golden_predict_edges.py froze it); for the non-diagonal model 200 cond(Gamma_j' Gamma_j) eps is held to a
            tenth of the gate as well (phi_tol's rule, with its 2.2e-16 for eps)
    share   at least 90 % of the PHI of a case are judged relative to their own value

Run with -s for the values per case ("One-shot prediction: what holds it", records a run)."""
import glob
import os
import re

import numpy as np
import pytest

import predict_edges as E
import predictor_reference as R
from oracle import gpz_oracle as O

pytestmark = pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_WHY)


def body_of(filename, start, end="\n}\n"):
    """The text of a source file under gpz_amd/csrc from the first occurrence of ``start`` to the next ``end``, whitespace collapsed."""
    src = open(os.path.join(E.CSRC, filename)).read()
    src = src[src.index(start):]
    return re.sub(r"\s+", " ", src[:src.index(end) + len(end)])


def test_rules_are_the_sources():
    """Every rule of predict_edges is restated from these statements, found inside the function that holds them (the line numbers in
    predict_edges' docstrings are citations only); a change to one of them has to come with a look at the table."""
    quoted = [
        ("gpz_predict.hip", 'extern "C" int gpz_predict_noisy(',
         ["int nchunk = (int)((1024 + (ns + 63) / 64 - 1) / ((ns + 63) / 64));", "if (nchunk > npair) nchunk = (int)npair;",
          "if (nchunk > 256) nchunk = 256;", "const long ppc = (npair + nchunk - 1) / nchunk;", "nchunk = (int)((npair + ppc - 1) / ppc);"]),
        ("gpz_predict.hip", "static int predict_missing_cov(",
         ["long rb = (1L << 26) / ((long)m * d * d);", "if (rb > n) rb = n;", "const bool fast = pmc_fast(d, (int)k);",
          "if (fast && rb > 64) rb = 64;", "if (generic) rb = 1;", "const long want = fast ? 2048 : 64;",
          "int nchunk = (int)(npairs < want ? npairs : want);", "const long ppc = (npairs + nchunk - 1) / nchunk;",
          "nchunk = (int)((npairs + ppc - 1) / ppc);", "const bool generic = d > 64;", "(d > 32 ? launch_pmc_wide : launch_pmc)("]),
        ("gpz_predict.hip", "static int predict_missing_diag(",
         ["int cw = 32;", "while (cw > 1 && (double)np * (double)(cw * mp) * 8.0 > 2e9) cw >>= 1;",
          "const size_t width = (size_t)rup((long)cw * (long)mp, 64);", "const int npg = rup(n, 128);",
          "for (long q0 = 0; q0 < npairs; q0 += (long)width) {", "const int nsp = pm_accum_splits(n);"]),
        ("gpz_predict.hip", 'extern "C" int gpz_predict_missing(', ["if (d > GPZ_PM_MAXD_DIAG) {"]),
        ("k_pmiss_cov.hip", "bool pmc_fast(int d, int k)", ["{ return d >= 2 && (d <= 10 || pmc4_available(d)) && k <= 8; }"], "\n"),
        ("k_pmiss_cov.hip", "void launch_pmc(",
         ["const bool fast = pmc_fast(d, k) && work2 != nullptr && rows_blk <= 64 && !gpz_opts().pmc_scratch;",
          "const int phi_chunks = m < 256 ? m : 256;", "(long)m, phi_chunks, ptab"]),
        ("k_pmiss.hip", "int pm_accum_splits(int n)", ["{ (void)n; return 16; }"], "\n"),
        ("k_pmc4.hip", "bool pmc4_available(int d)", ["{ return d > 10 && d <= 32; }"], "\n"),
        ("k_cpsi4.hip", "bool cpsi4_available(int d)", ["d > 10 && d <= 32;"]),
        ("k_cpsi4w.hip", "bool cpsi4w_available(int d)", ["d > 32 && d <= 48;"]),
        ("k_psi.hip", "int launch_predict_noisy_cov(",
         ["if (cpsi4_available(d) && k <= 8)", "if (cpsi4w_available(d) && k == 1)", "if (n <= 0) return (d >= 2 && d <= 10) ? 0 : -1;"]),
        ("k_psi.hip", "int launch_predict_noisy_diag(",
         ["if (d > 20 || k > 8) return -1;",
          "if (d <= 4) PND(4); else if (d <= 8) PND(8); else if (d <= 12) PND(12); else if (d <= 16) PND(16); else PND(20);"]),
        ("k_gen.hip", "void launch_predict_noisy(",
         ["if (kind != GPZ_KIND_DIAG && k <= 8 &&", "if (kind == GPZ_KIND_DIAG &&",
          'if (d <= GCAP) predict_route_add("gen<%d>", GCAP); else predict_route_add("gen_rt");']),
        ("k_gen.hip", "#define GCAP", ["#define GCAP 20"], "\n"),
        ("gpz_kernels.h", "#define GPZ_PM_MAXD_DIAG", ["#define GPZ_PM_MAXD_DIAG 144"], "\n"),
        ("gpz_ctx.hip", "rs.n_pad =", ["rs.n_pad = rup(rs.n > 0 ? rs.n : 1, 1024) + (c->gen ? 1024 : 0);"], "\n"),
        ("gpz_ctx.hip", "int setup_data(", ["if (c->kind == GPZ_KIND_COV && (Psi || xnan || table)) {", "c->gen = true;"]),
        ("gpz_ctx.hip", "c->mp =", ["c->mp = rup(c->m + c->k, 16);"], "\n"),
    ]
    for fn, start, texts, *end in quoted:
        got = body_of(fn, start, *end)
        for text in texts:
            assert text in got, (fn, start, text)


def test_rules_at_the_values_the_table_was_built_from():
    assert E.noisy_chunks(22, 70) == dict(npair=253, nchunk=253, ppc=1, last=1, row_blocks=2)
    assert E.noisy_chunks(23, 70) == dict(npair=276, nchunk=138, ppc=2, last=2, row_blocks=2)
    assert E.noisy_chunks(34, 70) == dict(npair=595, nchunk=199, ppc=3, last=1, row_blocks=2)
    assert E.noisy_chunks(60, 70) == dict(npair=1830, nchunk=229, ppc=8, last=6, row_blocks=2)
    assert E.noisy_chunks(6, 1025)["ppc"] == 1 and E.noisy_chunks(2000, 64)["nchunk"] <= 256
    r = E.missing_cov_rule(65, 5, 1, 70)
    assert (r["family"], r["rows_blk"], r["blocks"], r["nchunk"], r["ppc"], r["last"]) == ("pmc_fast<5>", 64, 2, 1073, 2, 1)
    assert E.missing_cov_rule(8, 40, 1, 5250)["rows_blk"] == 5242 and E.missing_cov_rule(8, 70, 1, 9)["rows_blk"] == 1
    assert E.missing_cov_rule(13, 4, 9, 20)["family"] == "pmc_scratch" and E.missing_cov_rule(300, 5, 1, 4)["phi_chunks"] == 256
    # the issue placed the second q0 pass at m = 64 (2080 pairs against 2048); mp = rup(m + k, 16) steps to 80 there and the width to 2560
    assert E.missing_diag_rule(64, 1, 40)["passes"] == 1 and E.missing_diag_rule(72, 1, 40)["passes"] == 2
    assert E.missing_diag_rule(1000, 1, 300000)["cw"] < 32
    assert [E.n_pad_rule(*a) for a in ((70, "VD", True, False), (70, "VC", True, False), (1025, "VC", False, False), (40, "GL", False, True),
                                       (1025, "GC", False, True))] == [1024, 2048, 2048, 1024, 3072]
    assert [E.noisy_family(*a) for a in (("VD", 5, 1), ("GL", 20, 3), ("VC", 5, 1), ("GC", 10, 3), ("VC", 12, 2), ("GC", 36, 1), ("VD", 6, 9),
                                         ("VC", 1, 1), ("VL", 24, 1), ("VC", 50, 1), ("GC", 36, 2))] == [
        "noisy_diag<8,1>", "noisy_diag<20,8>", "psi<5,1>", "psi<10,8>", "cpsi4<3,8>", "cpsi4w<9,1>", "gen<20>", "gen<20>", "gen_rt", "gen_rt", "gen_rt"]
    assert E.parse_route("predict_noisy: nchunk=138 ppc=2 n_pad=1024 noisy_diag<8,1>") == (
        "predict_noisy", {"nchunk": 138, "ppc": 2, "n_pad": 1024}, ["noisy_diag<8,1>"])


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c["id"])
def test_case_meets_its_predicate(case):
    rule = E.case_rule(case)
    assert case["edge"] and case["pred"](rule), (case["edge"], rule)


def test_the_table_covers_what_it_is_there_for():
    ids = set(E.CASE_BY_ID)
    fams = {E.case_rule(c)["family"] for c in E.CASES}
    assert {"noisy_diag<8,1>", "noisy_diag<20,8>", "psi<5,1>", "psi<10,8>", "cpsi4<3,8>", "cpsi4w<9,1>", "gen<20>", "gen_rt", "pm_diag",
            "pm_diag_flags", "pmc_fast<5>", "pmc_fast<3>", "pmc4<12>", "pmc_scratch", "pmc_wide", "tgemm"} <= fams
    for m in (22, 23, 34, 60):
        assert {"N-%s-d%d-k%d-m%d-trained" % (meth, d, k, m) for meth, d, k in (("VD", 5, 1), ("GL", 20, 3), ("VC", 5, 1), ("GC", 10, 3),
                                                                                ("VC", 12, 2), ("GC", 36, 1), ("VD", 6, 9), ("VL", 24, 1))} <= ids
    assert sum(c["twin"] for c in E.CASES) == 6 and len([c for c in E.CASES if c["entry"] == "F"]) == 32
    for c in E.CASES:                                  # both families on every diagonal-kind row of the table
        if c["method"][1] != "C" and not c["twin"] and c["entry"] != "F":
            assert c["id"].endswith(("-trained", "-synth")) and c["id"].rsplit("-", 1)[0] + "-synth" in ids and c["id"].rsplit("-", 1)[0] + "-trained" in ids
    for meth in ("VD", "GL"):                          # M-diag: every m in both patterns, with and without Psi
        for m in (63, 64, 65, 71, 72, 73):
            assert {"MD-%s-m%d-p%d-%s-%s" % (meth, m, p, q, f) for p in (0, 1) for q in ("psi", "nopsi") for f in ("trained", "synth")} <= ids


SMALL = [("VD", 4, 9, 2), ("GL", 3, 20, 1), ("VL", 5, 33, 1), ("GD", 2, 6, 1)]       # the shapes of test_gpu_parity's missing-value tests


@pytest.mark.parametrize("family", ["trained", "synth"])
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("method,d,m,k", SMALL)
def test_reference_agrees_with_the_oracle(method, d, m, k, noisy, family):
    """All six outputs, rows of mixed NaN patterns (complete rows among them: predictFull / predictNoisy), with and without Psi."""
    make = E.trained_like_model if family == "trained" else E.synth_model
    model = make(method, d, m, k, seed=61 + d)
    rng = np.random.default_rng(7 + d)
    ns = 83
    Xs = model.muX + model.sdX * rng.standard_normal((ns, d))
    miss = rng.random((ns, d)) < 0.3
    miss[miss.all(axis=1), 0] = False
    Xs[miss] = np.nan
    Psi = rng.gamma(1.0, 0.1, (ns, d)) if noisy else None
    out = E.oracle_outputs(model, Xs, Psi)
    scales = E.term_scales(model, out, E.oracle_outputs(E.abs_model(model), Xs, Psi))
    ref = E.ld_reference(model, Xs, Psi)
    res = E.scaled_errors(out, ref, scales)
    print(method, family, noisy, {name: "%.1e" % r[0] for name, r in res.items()})
    assert E.worst_of(res) <= E.DIAG_GATE / 10, res
    if not noisy:                                       # the complete rows without Psi are O.predict's
        full = ~miss.any(axis=1)
        assert full.any()
        pf = O.predict(Xs[full], model)
        assert np.max(np.abs(pf[5] - ref["PHI"][full].astype(np.float64))) <= 1e-14 and np.all(ref["gamma"][full] == 0)


def test_reference_reads_the_lower_triangle_of_inv_sigma_w():
    """The pair loop takes iSigma_w(i, j), i >= j, twice: with the synthetic (non-symmetric) inv(Sigma_w) the transposed reading
    misses the oracle by far more than the gate, so a kernel that swaps (a, b) shows."""
    model = E.synth_model("VD", 4, 9, 2, seed=3)
    rng = np.random.default_rng(4)
    Xs = model.muX + model.sdX * rng.standard_normal((30, 4))
    Psi = rng.gamma(1.0, 0.1, (30, 4))
    out = E.oracle_outputs(model, Xs, Psi)
    scales = E.term_scales(model, out, E.oracle_outputs(E.abs_model(model), Xs, Psi))
    swapped = E.clone_model(model, iSigma_w=np.transpose(model.sets["best"]["iSigma_w"], (1, 0, 2)).copy())
    res = E.scaled_errors(out, E.ld_reference(swapped, Xs, Psi), scales)
    assert res["nu"][0] > 1e3 * E.DIAG_GATE and res["mu"][0] <= E.DIAG_GATE / 10


@pytest.mark.parametrize("pattern,noisy", [(None, True), ((1,), False), ((0, 3), True)])
def test_abs_model_returns_the_sums_of_absolute_terms(pattern, noisy):
    """term_scales (two oracle calls) against the same sums formed term by term in extended precision, at one small diagonal shape."""
    model = E.trained_like_model("VD", 4, 9, 2, seed=65)
    rng = np.random.default_rng(5)
    Xs = model.muX + model.sdX * rng.standard_normal((40, 4))
    if pattern:
        Xs[:, list(pattern)] = np.nan
    Psi = rng.gamma(1.0, 0.1, (40, 4)) if noisy else None
    out = E.oracle_outputs(model, Xs, Psi)
    scales = E.term_scales(model, out, E.oracle_outputs(E.abs_model(model), Xs, Psi))
    direct = E.ld_reference(model, Xs, Psi, want_terms=True)["scales"]
    for name in ("mu", "gamma", "nu", "beta_i", "sigma"):
        err = float(np.max(np.abs(scales[name] - direct[name]) / direct[name]))
        print(name, "%.1e" % err)
        assert err <= 1e-9, (name, err)
    canc = direct["gamma"] / np.abs(out["gamma"])
    assert np.median(canc) > 10.0                       # what the scales are there for: the pair sum of gamma cancels


def test_twin_is_the_same_predictor():
    """A GC / VC model with diagonal Gamma_j is the GD / VD model: the oracle's covariance code on the twin against the
    extended-precision reference of the diagonal model, with missing inputs and Psi (the missing dimensions last, see twin_case)."""
    for method in ("GD", "VD"):
        model = E.trained_like_model(method, 3, 7, 2, seed=12)
        rng = np.random.default_rng(8)
        Xs = model.muX + model.sdX * rng.standard_normal((9, 3))
        Xs[4:, 2] = np.nan
        Psi = rng.gamma(1.0, 0.1, (9, 3))
        tw = E.diag_twin(model)
        assert tw.method == ("GC" if method == "GD" else "VC")
        out = E.oracle_outputs(tw, Xs, E.twin_psi(Psi))
        scales = E.term_scales(tw, out, E.oracle_outputs(E.abs_model(tw), Xs, E.twin_psi(Psi)))
        res = E.scaled_errors(out, E.ld_reference(model, Xs, Psi), scales)
        assert E.worst_of(res) <= 1e-9, res


def test_fixtures_are_the_table():
    """One file per fixture case and none besides, each under the size limit, holding the inputs the table describes."""
    want = {os.path.basename(E.fixture_path(c)) for c in E.CASES if c["fixture"]}
    have = {os.path.basename(p) for p in glob.glob(os.path.join(E.GOLDEN, "pe_*.npz"))}
    assert want == have, (sorted(want - have), sorted(have - want))
    for c in E.CASES:
        if not c["fixture"]:
            continue
        assert os.path.getsize(E.fixture_path(c)) <= 400 * 1024, c["id"]          # "a few hundred KB at most each"
        fm, fX, fP, out, scales = E.load_fixture(c)
        model, Xs, Psi = E.run_inputs(c)
        assert (fm.method, fm.m, fm.d, fm.k) == (model.method, model.m, model.d, model.k) and out["PHI"].shape == (c["ns"], c["m"])
        assert np.array_equal(np.isnan(fX), np.isnan(Xs)) and np.allclose(np.nan_to_num(fX), np.nan_to_num(Xs), rtol=1e-12, atol=0)
        assert (fP is None) == (Psi is None) and (Psi is None or np.allclose(fP, Psi, rtol=1e-12, atol=0))
        assert np.allclose(fm.sets["best"]["theta"], model.sets["best"]["theta"], rtol=1e-9, atol=1e-12)
        assert all(np.all(scales[name] > 0) for name in scales)


FITNESS = {}


@pytest.mark.parametrize("case", [c for c in E.CASES if c["entry"] != "F"], ids=lambda c: c["id"])
def test_case_is_fit_to_judge_a_kernel(case):
    model = E.run_inputs(case)[0]
    gate = E.gate_of(model)
    if case["fixture"]:
        PHI = E.load_fixture(case)[3]["PHI"]
    else:
        PHI = E.oracle_outputs(*E.run_inputs(case))["PHI"]
    share = E.phi_share(PHI)
    if case["fixture"] and E.run_method(case)[1] == "C":
        e_ref = float(np.load(E.fixture_path(case))["e_ref_twin"])
    else:
        e_ref = E.reference_error(case)[0]
    FITNESS[case["id"]] = (e_ref, share, gate)
    print("%s: e_ref %.2e (gate %.1e), PHI share %.3f" % (case["id"], e_ref, gate, share))
    assert e_ref <= gate / 10, (e_ref, gate)
    assert share >= E.PHI_SHARE_MIN, share
    if model.method[1] == "C" and not case["twin"]:     # (phi_tol's rule with phi_tol's own constant for eps, 2.2e-16)
        assert 200.0 * E.cov_cond(model) * 2.2e-16 <= gate / 10, E.cov_cond(model)


def test_fitness_report():
    """Last in the file: the worst e_ref / gate and the smallest PHI share per entry (DESIGN.md records a run)."""
    for entry in ("N", "MD", "MC"):
        mine = {cid: v for cid, v in FITNESS.items() if E.CASE_BY_ID[cid]["entry"] == entry}
        if mine:
            worst = max(mine, key=lambda cid: mine[cid][0] / mine[cid][2])
            low = min(mine, key=lambda cid: mine[cid][1])
            print("%s: %d cases, worst e_ref %.2e at gate %.1e (%s), smallest PHI share %.3f (%s)" % (
                entry, len(mine), mine[worst][0], mine[worst][2], worst, mine[low][1], low))
