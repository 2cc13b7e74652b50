"""CPU-side checks of Predictor(model, large_m_missing=True) / GPZ_PREDICT_LARGE_M_MISSING: the flag's value in the header, the Python
constants and gpz_predictor_create's flags agree; the fits rule and the LDS rule of the panelled pair kernels, stated here a second
time, with the LDS rule inside 160 KB for every accepted shape; the Python refusals before the library is loaded (m = 1025 with the
flag, m = 257 without it in the old words, the covariance kinds' methods in their old words); and the two new units compile for gfx950
without scratch or spill, inside their launch bounds, with no static LDS, on the f64 MFMA and without a floating-point atomic."""
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
from test_predictor_noisy_cpu import _model, _resource_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
LIMIT, KP, GB, GB8 = 1024, 128, 4, 2


# ---- the rules, a second time -----------------------------------------------------------------------------------------------------------
def large_fits_rule(kind_diag, de, m, k):
    return kind_diag and de in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20) and 1 <= k <= 8 and 1 <= m and (m + 15) // 16 * 16 <= LIMIT


def large_lds_rule(d, k, psi, gamma=False):
    """One K panel of the Pio block, the 64 records of a group (gamma: their first 1 + 2 d doubles and 64 (a, b)), the block's rows of X
    and with psi of Psi; at least the sink's last reduction.  Bytes; m does not enter."""
    rec = 1 + 2 * d if gamma else 1 + 2 * d + 3 * k
    work = 32 * (KP + 2) + 64 * rec + (64 if psi else 32) * d + (64 if gamma else 0)
    red = 4 * 32 * 16 if gamma else 4 * 32 * 3 * (1 if k == 1 else 8)
    return 8 * max(work, red)


def test_the_flag_in_the_header_the_constants_and_create():
    h = open(HEADER).read()
    assert int(re.search(r"#define GPZ_PREDICT_LARGE_M_MISSING (\d+)", h).group(1)) == P.GPZ_PREDICT_LARGE_M_MISSING == \
        gpz_amd.api.GPZ_PREDICT_LARGE_M_MISSING == 4
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "flags & ~(GPZ_PREDICT_FORCE_TILES | GPZ_PREDICT_LARGE_M) & ~GPZ_PREDICT_LARGE_M_MISSING" in host
    assert "p->large_m_missing = (flags & GPZ_PREDICT_LARGE_M_MISSING) != 0;" in host
    k = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert int(re.search(r"#define GPZ_PML_KP (\d+)", k).group(1)) == KP
    assert int(re.search(r"#define GPZ_PML_GB (\d+)", k).group(1)) == GB and int(re.search(r"#define GPZ_PML_GB8 (\d+)", k).group(1)) == GB8


def test_the_flag_reaches_gpz_predictor_create(monkeypatch):
    seen = []

    class FakeLib:
        def gpz_predictor_create(self, desc, theta, w, iS, tile_rows, flags, out):
            seen.append((tile_rows, flags))
            return 0

        def gpz_predictor_destroy(self, h):
            pass

    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    for kw, want in (({}, 0), ({"large_m": True}, 2), ({"large_m_missing": True}, 6), ({"large_m_missing": True, "large_m": True}, 6),
                     ({"large_m_missing": True, "force_tiles": True}, 7), ({"large_m_missing": False}, 0)):
        p = gpz_amd.Predictor(_model(), tile_rows=512, **kw)
        p._handle()
        assert seen[-1] == (512, want), (kw, seen[-1])
        p.close()


def test_fits_and_lds_rules():
    src = open(os.path.join(CSRC, "k_pml_pairs.hip")).read()
    fits = re.search(r"bool predict_missing_large_fits\(int kind, int de, int m, int k\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "{1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20}" in fits
    assert "kind == GPZ_KIND_DIAG && width && k >= 1 && k <= 8 && m >= 1 && ((m + 15) / 16) * 16 <= GPZ_PREDICT_LARGE_M_MAX" in fits
    assert large_fits_rule(True, 3, 1024, 8) and large_fits_rule(True, 20, 1009, 1) and not large_fits_rule(True, 3, 1025, 1)
    assert not large_fits_rule(False, 3, 300, 1) and not large_fits_rule(True, 7, 300, 1) and not large_fits_rule(True, 3, 300, 9)
    lds = re.search(r"size_t predict_missing_large_lds\(int m, int d, int k, bool psi, bool gamma\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "32 * (GPZ_PML_KP + 2) + 64 * rec + (psi ? 64 : 32) * (size_t)d + (gamma ? 64 : 0)" in lds
    assert "gamma ? 1 + 2 * (size_t)d : (size_t)predict_missing_rec(d, k)" in lds and "gamma ? 4 * 32 * 16 : 4 * 32 * 3 * km" in lds
    assert not re.search(r"\b(ns|nt|n|tile|rows|nd|ncol)\b", fits + lds)    # the model's shape alone
    worst = 0
    for d in range(1, 21):
        for k in range(1, 9):
            for psi in (False, True):
                for gamma in (False, True):
                    b = large_lds_rule(d, k, psi, gamma)                  # the same for every m <= 1024: m is not an argument
                    assert 32 * (KP + 2) * 8 <= b <= 160 * 1024, (d, k, psi, gamma, b)
                    worst = max(worst, b)
    assert worst == large_lds_rule(20, 8, True) == 76_800
    assert large_lds_rule(10, 1, False) == 48_128 and 3 * large_lds_rule(10, 1, False) <= 160 * 1024   # the headline shape: three workgroups
    impl = open(os.path.join(CSRC, "k_predict_group_impl.h")).read()
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in impl and "lds > 65536" in impl
    assert "launch_predict_group<k_pml_pairs" in src and "launch_predict_group<k_pml_gamma" in open(os.path.join(CSRC, "k_pml_gamma.hip")).read()
    # the chunk count is the old rule, and the old rules are where they were
    old = open(os.path.join(CSRC, "k_predict_missing.hip")).read()
    assert "nchunk != predict_missing_chunks(m)" in src and "int predict_missing_chunks(int m) {" in old
    for name in ("k_predict_missing_pairs", "k_predict_noisy_missing_pairs", "k_predict_missing_gamma", "k_predict_noisy_missing_gamma"):
        for unit in ("k_pml_pairs.hip", "k_pml_gamma.hip"):
            code = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, unit)).read().splitlines())
            assert name not in code, (unit, name)


# ---- the Python refusals ----------------------------------------------------------------------------------------------------------------
def _calls(p, d=3, n=4):
    X, Pd = torch.zeros((n, d), dtype=torch.float64), torch.ones((n, d), dtype=torch.float64)
    e = np.linspace(0.0, 1.0, 5)
    return [("predict_dev", lambda: p.predict_dev(X, missing=True)), ("draws_dev", lambda: p.draws_dev(X, 3, missing=True)),
            ("draws_dev gamma", lambda: p.draws_dev(X, 3, missing=True, return_gamma=True)),
            ("stack_missing_dev", lambda: p.stack_missing_dev(X, e, n_draws=2)),
            ("predict_noisy_missing_dev", lambda: p.predict_noisy_missing_dev(X, Pd)),
            ("draws_noisy_missing_dev", lambda: p.draws_noisy_missing_dev(X, Pd, 3)),
            ("draws_noisy_missing_dev gamma", lambda: p.draws_noisy_missing_dev(X, Pd, 3, return_gamma=True)),
            ("stack_noisy_missing_dev", lambda: p.stack_noisy_missing_dev(X, Pd, e, n_draws=2))]


@pytest.mark.parametrize("method", ["VD", "GL"])
def test_scope_checks_with_and_without_the_flag(monkeypatch, method):
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    for m in (257, 300, 1024):
        with gpz_amd.Predictor(_model(d=3, m=m, method=method), large_m_missing=True) as p:
            for name, call in _calls(p):
                with pytest.raises(ValueError, match="must be on cuda:0"):   # the last check: every check of the shape has passed
                    call()
    with gpz_amd.Predictor(_model(d=3, m=1025, method=method), large_m_missing=True) as p:
        for name, call in _calls(p):
            with pytest.raises(ValueError, match="predict_missing_fits") as ei:
                call()
            assert "m <= 1024, not m = 1025" in str(ei.value), (name, str(ei.value))
    for flags in ({}, {"large_m": True}):                                 # without the flag: the old text, word for word
        with gpz_amd.Predictor(_model(d=3, m=257, method=method), **flags) as p:
            for name, call in _calls(p):
                with pytest.raises(ValueError) as ei:
                    call()
                how = "" if "noisy_missing" in name else " with missing=True"
                what = name.split(" ")[0]
                assert str(ei.value) == (f"{what}{how} needs a model inside predict_missing_fits: m <= 256, not m = 257 "
                                         "(Predictor.predict takes rows with missing values for every shape)"), (name, str(ei.value))
    # the other limits stay with the flag
    for kw, text in (({"d": 24}, "d <= 20, not d = 24"), ({"k": 9}, "k <= 8, not k = 9")):
        with gpz_amd.Predictor(_model(**{"d": 3, "m": 300, "method": method, **kw}), large_m_missing=True) as p:
            for name, call in _calls(p, d=kw.get("d", 3)):
                with pytest.raises(ValueError, match=text):
                    call()


def test_the_covariance_kinds_do_not_look_at_the_flag(monkeypatch):
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    X, Pd, e = torch.zeros((4, 3), dtype=torch.float64), torch.ones((4, 3), dtype=torch.float64), np.linspace(0.0, 1.0, 5)
    cube = torch.zeros((3, 3, 4), dtype=torch.float64)
    texts = []
    for flags in ({}, {"large_m_missing": True}):
        with gpz_amd.Predictor(_model(d=3, m=257, method="VC"), **flags) as p:
            got = []
            for call in (lambda: p.predict_missing_cov_dev(X), lambda: p.draws_missing_cov_dev(X, 3), lambda: p.stack_missing_cov_dev(X, e),
                         lambda: p.predict_noisy_missing_cov_dev(X, Pd), lambda: p.draws_noisy_missing_cov_dev(X, Pd, 3),
                         lambda: p.predict_psi_cube_missing_dev(X, cube)):
                with pytest.raises(ValueError) as ei:
                    call()
                got.append(str(ei.value))
            assert all("m <= 256" in t for t in got), got
            with pytest.raises(ValueError, match=r"a diagonal kind \(GL, VL, GD, VD\), not VC"):   # and the diagonal kinds' methods refuse VC
                p.predict_dev(X, missing=True)
            texts.append(got)
    assert texts[0] == texts[1]                                           # the old text, with the flag and without
    assert "predict_missing_cov_fits: GC or VC, d <= 10, k <= 8 and m <= 256; this one is VC with d = 3, m = 257, k = 1" in texts[1][0]


# ---- the compiled form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
@pytest.mark.parametrize("unit,kernels,counts", [("k_pml_pairs", ("k_pml_pairs", "k_pml_pairs_psi"), [1, 8]),
                                                 ("k_pml_gamma", ("k_pml_gamma", "k_pml_gamma_psi"), [1, 2, 3, 4])])
def test_the_new_units_compiled_form(tmp_path, unit, kernels, counts):
    """Every instantiation: no scratch, no spilled register, VGPRs + AGPRs <= 256 (__launch_bounds__(256, 2): two workgroups of four
    waves per compute unit), no static LDS (all of it is the dynamic block of predict_missing_large_lds), the f64 MFMA, no
    floating-point atomic."""
    asm = tmp_path / (unit + ".s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, unit + ".hip"), "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    assert len(recs) == 2 * len(counts), sorted(recs)
    for kname in kernels:
        mine = [n for n in recs if re.search(r"\d+" + kname + "ILi", n)]
        assert sorted(int(re.search(r"ILi(\d+)E", n).group(1)) for n in mine) == counts, (kname, sorted(recs))
    for name, q in recs.items():
        print(name, q["VGPRs"], q.get("AGPRs", 0))
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
        assert q["LDS Size [bytes/block]"] == 0, (name, q)
    text = asm.read_text()
    assert "v_mfma_f64_16x16x4" in text
    for word in ("atomic_add_f", "atomic_pk_add", "atomic_fadd", "atomic_fmin", "atomic_fmax", "ds_add_f", "ds_add_rtn_f", "cmpswap",
                 "scratch_"):
        assert word not in text, word
    src = open(os.path.join(CSRC, unit + ".hip")).read() + open(os.path.join(CSRC, "k_predict_group_large_impl.h")).read()
    assert "__launch_bounds__(256, 2)" in src and "atomic" not in src.replace("No atomics", "")
