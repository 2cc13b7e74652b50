"""CPU-side checks of Predictor(model, large_m=True) / GPZ_PREDICT_LARGE_M: the flag's value in the header, the Python constant and
gpz_predictor_create's flags agree; the Python scope checks of the three forms of Psi (a variance per dimension on a diagonal kind, on
GC / VC, and the d x d x n cube) pass at m = 257, 300 and 1024 with the flag, refuse m = 1025 with large_m and 1024 in the text, and
refuse what they refused before without it, all before the library is loaded; the pair-chunk rules, stated here a second time, equal
the siblings' rules for every m <= 256 and the table of DESIGN.md section 36 beyond; and k_predict_noisy_phi compiles for gfx950
without scratch at every width, with the LDS it is documented to take."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from gpz_amd import predictor as P
from test_predictor_noisy_cov_cpu import cov_chunks_rule
from test_predictor_noisy_cpu import _model, _resource_records, chunks_rule
from test_predictor_stack_noisy_cpu import gamma_chunks_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
LIMIT = 1024


def large_chunks_rule(m):
    """The three chunk rules up to m = 1024, stated a second time on purpose: (predict_noisy_chunks = predict_noisy_cov_chunks,
    predict_gamma_chunks).  One chunk per 2048 (4096, rounded up) pairs, at most 4: the cap does not rise past m = 256."""
    npair = m * (m + 1) // 2
    return min(4, max(1, npair // 2048)), min(4, max(1, (npair + 4095) // 4096))


def test_the_flag_in_the_header_the_constant_and_create():
    h = open(HEADER).read()
    assert int(re.search(r"#define GPZ_PREDICT_LARGE_M (\d+)", h).group(1)) == P.GPZ_PREDICT_LARGE_M == gpz_amd.api.GPZ_PREDICT_LARGE_M == 2
    assert int(re.search(r"#define GPZ_PREDICT_FORCE_TILES (\d+)", h).group(1)) == P.GPZ_PREDICT_FORCE_TILES == 1
    k = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert int(re.search(r"#define GPZ_PREDICT_LARGE_M_MAX (\d+)", k).group(1)) == P.GPZ_PREDICT_LARGE_M_MAX == LIMIT
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "flags & ~(GPZ_PREDICT_FORCE_TILES | GPZ_PREDICT_LARGE_M)" in host
    assert "p->large_m = (flags & GPZ_PREDICT_LARGE_M) != 0;" in host


def test_the_flag_reaches_gpz_predictor_create(monkeypatch):
    seen = []

    class FakeLib:
        def gpz_predictor_create(self, desc, theta, w, iS, tile_rows, flags, out):
            seen.append((tile_rows, flags))
            return 0

        def gpz_predictor_destroy(self, h):
            pass

    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    for kw, want in (({}, 0), ({"force_tiles": True}, 1), ({"large_m": True}, 2), ({"large_m": True, "force_tiles": True}, 3),
                     ({"large_m": False}, 0)):
        p = gpz_amd.Predictor(_model(), tile_rows=512, **kw)
        p._handle()
        assert seen[-1] == (512, want), (kw, seen[-1])
        p.close()


def _forms(p, model, n=4):
    """One call of each question for each form of Psi that the model's kind has: (name, callable)."""
    d = model.d
    X, Pd = torch.zeros((n, d), dtype=torch.float64), torch.ones((n, d), dtype=torch.float64)
    e = np.linspace(0.0, 1.0, 5)
    if model.method[1] != "C":
        return [("predict_dev", lambda: p.predict_dev(X, Psi=Pd)), ("draws_dev", lambda: p.draws_dev(X, 3, Psi=Pd)),
                ("draws_dev gamma", lambda: p.draws_dev(X, 3, Psi=Pd, return_gamma=True)),
                ("stack_noisy_dev", lambda: p.stack_noisy_dev(X, Pd, e, n_draws=2))]
    cube = torch.zeros((d, d, n), dtype=torch.float64)
    return [("predict_noisy_cov_dev", lambda: p.predict_noisy_cov_dev(X, Pd)), ("draws_noisy_cov_dev", lambda: p.draws_noisy_cov_dev(X, Pd, 3)),
            ("draws_noisy_cov_dev gamma", lambda: p.draws_noisy_cov_dev(X, Pd, 3, return_gamma=True)),
            ("stack_noisy_cov_dev", lambda: p.stack_noisy_cov_dev(X, Pd, e, n_draws=2)),
            ("predict_psi_cube_dev", lambda: p.predict_psi_cube_dev(X, cube)), ("draws_psi_cube_dev", lambda: p.draws_psi_cube_dev(X, cube, 3)),
            ("draws_psi_cube_dev gamma", lambda: p.draws_psi_cube_dev(X, cube, 3, return_gamma=True)),
            ("stack_psi_cube_dev", lambda: p.stack_psi_cube_dev(X, cube, e, n_draws=2))]


def _host_forms(p, model, n=4):
    d = model.d
    X, Ph, e = np.zeros((n, d)), np.ones((n, d)), np.linspace(0.0, 1.0, 5)
    return [("draws", lambda: p.draws(X, 3, Psi=Ph)), ("stack_noisy", lambda: p.stack_noisy(X, Ph, e, n_draws=2))]


@pytest.mark.parametrize("method", ["VD", "GL", "VC", "GC"])
def test_scope_checks_with_and_without_the_flag(monkeypatch, method):
    """With the flag m = 257, 300 and 1024 pass every Python check of every method of the form: the CPU tensors reach the device check
    (the last one, "must be on cuda:0"), the host arrays reach the library load, which is made to fail.  m = 1025 is a ValueError that
    names large_m and 1024.  Without the flag the same models raise the text they raised before the flag existed."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    diag = method[1] != "C"
    fits = "predict_noisy_fits" if diag else "predict_noisy_cov_fits"
    old = ("k <= 8 and m <= 256; this one is" if diag else "GC or VC, d <= 10, k <= 8 and m <= 256; this one is")
    for m in (257, 300, 1024):
        model = _model(d=3, m=m, method=method)
        with gpz_amd.Predictor(model, large_m=True) as p:
            for name, call in _forms(p, model):
                with pytest.raises(ValueError, match="must be on cuda:0"):
                    call()
            for name, call in (_host_forms(p, model) if diag else []):
                with pytest.raises(RuntimeError, match="disabled"):
                    call()
        with gpz_amd.Predictor(model) as q:
            for name, call in _forms(q, model) + (_host_forms(q, model) if diag else []):
                with pytest.raises(ValueError, match=fits) as ei:
                    call()
                assert old in str(ei.value) and "large_m" not in str(ei.value), (name, str(ei.value))
    model = _model(d=3, m=1025, method=method)
    with gpz_amd.Predictor(model, large_m=True) as p:
        for name, call in _forms(p, model) + (_host_forms(p, model) if diag else []):
            with pytest.raises(ValueError, match=fits) as ei:
                call()
            assert "large_m" in str(ei.value) and "1024" in str(ei.value) and "m = 1025" in str(ei.value), (name, str(ei.value))
    # the other limits of the scope stay with the flag: d, k and the kind
    for kw in ({"d": 24} if diag else {"d": 11}, {"k": 9}):
        model = _model(**{"d": 3, "m": 300, "method": method, **kw})
        with gpz_amd.Predictor(model, large_m=True) as p:
            for name, call in _forms(p, model):
                with pytest.raises(ValueError, match=fits):
                    call()


def test_the_methods_for_missing_inputs_do_not_look_at_the_flag(monkeypatch):
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    X, Pd = torch.zeros((4, 3), dtype=torch.float64), torch.ones((4, 3), dtype=torch.float64)
    for flag in (False, True):
        with gpz_amd.Predictor(_model(d=3, m=257), large_m=flag) as p:
            for call in (lambda: p.predict_dev(X, missing=True), lambda: p.draws_dev(X, 3, missing=True),
                         lambda: p.predict_noisy_missing_dev(X, Pd), lambda: p.draws_noisy_missing_dev(X, Pd, 3)):
                with pytest.raises(ValueError, match="m <= 256, not m = 257"):
                    call()
        with gpz_amd.Predictor(_model(d=3, m=257, method="VC"), large_m=flag) as p:
            with pytest.raises(ValueError, match="m <= 256"):
                p.predict_missing_cov_dev(X)


def test_force_tiles_with_the_flag_takes_draws_with_psi(monkeypatch):
    """Without the flag the draws with Psi of a forced tile route are refused in Python (the sibling test); with it they pass."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    X, Pd = torch.zeros((4, 3), dtype=torch.float64), torch.ones((4, 3), dtype=torch.float64)
    with gpz_amd.Predictor(_model(), force_tiles=True) as p:
        with pytest.raises(ValueError, match="force_tiles"):
            p.draws_dev(X, 4, Psi=Pd)
    with gpz_amd.Predictor(_model(), force_tiles=True, large_m=True) as p:
        with pytest.raises(ValueError, match="must be on cuda:0"):
            p.draws_dev(X, 4, Psi=Pd)
        with pytest.raises(RuntimeError, match="disabled"):
            p.draws(np.zeros((4, 3)), 4, Psi=np.ones((4, 3)))


def test_chunk_rules_up_to_1024():
    """For m <= 256 the rules are the siblings' rules; beyond, the table of DESIGN.md section 36 row by row, and no change of either
    count above m = 256 (the GPU tests take m +- 1 of every change above 256: there is none)."""
    for m in range(1, 257):
        assert large_chunks_rule(m) == (chunks_rule(m, 5, 1), gamma_chunks_rule(m)), m
        assert chunks_rule(m, 5, 1) == cov_chunks_rule(m, 5, 1)
    assert [m for m in range(257, LIMIT + 1) if large_chunks_rule(m) != large_chunks_rule(m - 1)] == []
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 36."):]
    rows = re.findall(r"^\| (\d+) \| (\d+) \| (\d+) \| (\d+) \|$", sec, flags=re.M)
    assert [int(r[0]) for r in rows] == [256, 257, 272, 273, 512, 1000, 1024], rows
    for m, npair, c, g in ((int(v) for v in r) for r in rows):
        assert npair == m * (m + 1) // 2 and (c, g) == large_chunks_rule(m), (m, npair, c, g)
    for unit, name, body in (("k_predict_noisy.hip", "predict_noisy_chunks", "/ 2048"), ("k_predict_noisy_cov.hip", "predict_noisy_cov_chunks", "/ 2048"),
                             ("k_predict_noisy_gamma.hip", "predict_gamma_chunks", "+ 4095) / 4096")):
        src = open(os.path.join(CSRC, unit)).read()
        fn = re.search(r"int " + name + r"\([^)]*\) \{(.*?)\n\}", src, flags=re.S).group(1)
        assert body in fn and "(c > 4 ? 4 : c)" in fn, name
        assert not re.search(r"\b(ns|nt|tile|rows|large)\w*\b", fn), name   # the model's shape alone, and not the flag


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_phi_kernel_compiled_form(tmp_path):
    """k_predict_noisy_phi<1 .. 20>: no scratch, no spill, at most 256 vector registers, and the LDS of its header: a 64 x 33 tile of
    values and one stage of 32 records of 2 d doubles."""
    asm = tmp_path / "k_predict_noisy.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "k_predict_noisy.hip"), "-o",
                        str(asm)], check=True, capture_output=True, text=True, timeout=1800)
    phi = {n: q for n, q in _resource_records(r.stderr).items() if "k_predict_noisy_phi" in n}
    assert len(phi) == 20, sorted(phi)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 36."):]
    table = {int(d): (int(v), int(l)) for d, v, l in re.findall(r"^\| (\d+) \| (\d+) \| (\d+) \|$", sec, flags=re.M)}
    for name, q in phi.items():
        d = int(re.search(r"ILi(\d+)E", name).group(1))
        assert q["ScratchSize [bytes/lane]"] == 0 and q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
        assert q["LDS Size [bytes/block]"] == (64 * 33 + 32 * 2 * d) * 8, (name, q)
        assert table[d][1] == q["LDS Size [bytes/block]"], (d, table.get(d), q)   # (the table's registers are one compiler's figures)
