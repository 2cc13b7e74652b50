"""CPU-side checks of rows with missing inputs on the predictor handle (Predictor.predict_dev / draws_dev with missing=True,
gpz_predictor_run_missing_dev / _draws_missing_dev of the C ABI): the keyword's refusals fire before the GPU is touched; the entries are
declared, bound and exported; k_predict_missing.hip compiles for gfx950 without scratch or spills, its pair kernel within 256 registers
and the LDS DESIGN.md section 17 states; the fit and chunk rules are functions of the model's shape alone."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
SRC = os.path.join(CSRC, "k_predict_missing.hip")
IMPL = os.path.join(CSRC, "k_predict_group_impl.h")              # the pair kernels' body and the helper that launches them
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_run_missing_dev": 17, "gpz_predictor_draws_missing_dev": 16}
# k_pnm_no: k_pmd_no for rows with Psi too, one body behind both (it came here from k_predict_noisy_missing.hip)
KERNELS = ("k_pmd_check", "k_pmd_basis", "k_pmd_pairs", "k_pmd_u", "k_pmd_no", "k_pnm_no", "k_pmd_phi", "k_predict_missing_pairs",
           "k_pmd_finish")


def _model(d=3, m=6, k=1, method="VD"):
    model = gpz_amd.Model(m=m, d=d, k=k, method=method)
    p = m * d + model.g_dim + m * k + k + 2 * m * k
    model.sets["best"] = {"theta": np.zeros(p), "w": np.zeros((m, k)), "iSigma_w": np.stack([np.eye(m)] * k, axis=2)}
    return model


# ---- the keyword's refusals ------------------------------------------------------------------------------------------------------------
def test_missing_keyword_validates_before_the_gpu(monkeypatch):
    """The library load is made to fail, so a call that got past the checks would raise RuntimeError instead of ValueError."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    p = gpz_amd.Predictor(_model())
    X = torch.zeros((4, 3), dtype=torch.float64)
    X[1, 2] = float("nan")
    for call in (lambda **kw: p.predict_dev(X, **kw), lambda **kw: p.draws_dev(X, 4, **kw)):
        with pytest.raises(ValueError, match="missing=True does not take Psi"):
            call(missing=True, Psi=torch.ones((4, 3), dtype=torch.float64))
        with pytest.raises(ValueError, match="must be on cuda:0"):        # past the checks of the keyword: the device, last
            call(missing=True)
        with pytest.raises(ValueError, match="must be on cuda:0"):        # and the default is the call as it was
            call(missing=False)
    with pytest.raises(ValueError, match="return_phi"):
        p.predict_dev(X, return_phi=True, missing=True)
    with pytest.raises(ValueError, match="X must be n x 3"):              # X's own checks come first
        p.predict_dev(torch.zeros((4, 2), dtype=torch.float64), missing=True)
    for kw, text in (({"m": 257}, "m <= 256, not m = 257"), ({"d": 21}, "d <= 20, not d = 21"), ({"k": 9}, "k <= 8, not k = 9"),
                     ({"method": "GC"}, "a diagonal kind .* not GC"), ({"method": "VC"}, "a diagonal kind .* not VC")):
        model = _model(**kw)
        q = gpz_amd.Predictor(model)
        Xd = torch.zeros((4, model.d), dtype=torch.float64)
        for call in (lambda: q.predict_dev(Xd, missing=True), lambda: q.draws_dev(Xd, 4, missing=True)):
            with pytest.raises(ValueError, match="predict_missing_fits.*" + text):
                call()
        with pytest.raises(ValueError, match="must be on cuda:0"):        # without the keyword these models are as before
            q.predict_dev(Xd)
    bad = _model()
    bad.sets["best"]["priors"] = np.ones(5) / 5                           # m = 6
    with pytest.raises(ValueError, match="priors"):
        gpz_amd.Predictor(bad).predict_dev(X, missing=True)
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.predict_dev(X, missing=True)
    # the host methods and the stacks have no such keyword
    p = gpz_amd.Predictor(_model())
    for call in (lambda: p.predict(np.zeros((4, 3)), missing=True), lambda: p.draws(np.zeros((4, 3)), 4, missing=True),
                 lambda: p.stack(np.zeros((4, 3)), np.linspace(0, 1, 5), missing=True),
                 lambda: p.stack_dev(X, np.linspace(0, 1, 5), missing=True)):
        with pytest.raises(TypeError, match="missing"):
            call()


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_missing_entries():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
        assert m, f"{name} is not declared in gpz_hip.h"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    # gpz_predictor_run_dev's / _draws_dev's arguments + the priors and the mask after muY (and no PHI)
    for name, base, drop in (("gpz_predictor_run_missing_dev", "gpz_predictor_run_dev", 1),
                             ("gpz_predictor_draws_missing_dev", "gpz_predictor_draws_dev", 0)):
        args = [a.strip() for a in re.search(r"\bint " + name + r"\(([^;]*)\);", h).group(1).split(",")]
        old = [a.strip() for a in re.search(r"\bint " + base + r"\(([^;]*)\);", h).group(1).split(",")]
        assert len(args) == len(old) + 2 - drop
        assert args[:9] == old[:9]
        assert args[9:11] == ["const double *priors", "uint32_t obs_mask"]
        assert not any("PHI" in a for a in args) and args[-1] == "void *stream"
        assert _lib.SYMBOLS[name][1][9:11] == [_lib.c_double_p, _lib.C.c_uint32]
        assert _lib.SYMBOLS[name][1][:9] == _lib.SYMBOLS[base][1][:9]
    full = open(HEADER).read()
    assert "the rows of a group must share one NaN pattern" in full and "Cost per row" in full
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert re.search(r'UNITS="[^"]*\bk_predict_missing\b', build)


# ---- the compiled form ---------------------------------------------------------------------------------------------------------------------
def _resource_records(stderr):
    recs, cur = {}, None
    for l in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = m.group(1)
            recs[cur] = {}
            continue
        m = re.search(r"(VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", l)
        if m and cur:
            recs[cur][m.group(1)] = int(m.group(2))
    return recs


def lds_rule(m, d, k):
    """predict_missing_lds of k_predict_missing.hip and DESIGN.md section 17, stated a second time on purpose: the Pio block of 32 rows
    (row stride ceil16(m) + 2), the 64 records of a pair group, the block's rows; at least the 4 x 32 x 3 KM doubles of the last
    reduction (KM = 1 for one output, else 8)."""
    nk = (m + 15) // 16 * 16
    return 8 * max(32 * (nk + 2) + 64 * (1 + 2 * d + 3 * k) + 32 * d, 4 * 32 * 3 * (1 if k == 1 else 8))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_missing_kernels_compiled_form(tmp_path):
    """Every kernel of the unit: no scratch, no spilled register.  The pair kernel: two instantiations (1 or 8 outputs in registers), at
    most 256 vector registers, no static LDS (all of it is the dynamic block of predict_missing_lds), the f64 MFMA, no floating-point
    atomic."""
    asm = tmp_path / "k_predict_missing.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    for kname in KERNELS:
        assert any(kname in n for n in recs), (kname, sorted(recs))
    for name, q in recs.items():
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
    pairs = {n: q for n, q in recs.items() if "k_predict_missing_pairs" in n}
    assert sorted(int(re.search(r"ILi(\d+)E", n).group(1)) for n in pairs) == [1, 8]
    for name, q in pairs.items():
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)           # two workgroups of 256 per compute unit
        assert q["LDS Size [bytes/block]"] == 0, (name, q)
    src = open(SRC).read()
    body = re.search(r"size_t predict_missing_lds\(int m, int d, int k, bool psi\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert ": 32 * (nk + 2) + 64 * (size_t)predict_missing_rec(d, k) + 32 * (size_t)d;" in body and "red = 4 * 32 * 3 * km" in body
    assert "int predict_missing_rec(int d, int k) { return 1 + 2 * d + 3 * k; }" in src
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in open(IMPL).read() and "launch_predict_group<k_predict_missing_pairs<" in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "32 (nk + 2) + 64 (1 + 2 d + 3 k) + 32 d" in design
    # what the rule gives at the shapes section 17 names: the benchmark shape fits two workgroups per compute unit, the largest one
    assert lds_rule(100, 5, 1) == 37_632 and 2 * lds_rule(100, 5, 1) <= 160 * 1024
    assert lds_rule(256, 20, 8) == 104_448 and lds_rule(256, 20, 8) <= 160 * 1024
    assert lds_rule(1, 1, 8) == 8 * 3072
    text = asm.read_text()
    assert "v_mfma_f64_16x16x4" in text
    for word in ("atomic_add_f", "atomic_pk_add", "atomic_fadd", "atomic_fmin", "atomic_fmax", "ds_add_f", "ds_add_rtn_f", "cmpswap",
                 "scratch_"):
        assert word not in text, word


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------
def fits_rule(kind_diag, de, m, k):
    return kind_diag and de in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20) and 1 <= k <= 8 and 1 <= m and (m + 15) // 16 * 16 <= 256


def chunks_rule(m):
    """predict_missing_chunks: one chunk per 16 groups of 64 pairs, at most 8 - m only."""
    return min(8, max(1, ((m * (m + 1) // 2 + 63) // 64) // 16))


def test_fit_and_chunk_rules_are_functions_of_the_model_shape():
    h = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert re.search(r"\bbool predict_missing_fits\(int kind, int de, int m, int k\);", h)
    assert re.search(r"\bint predict_missing_chunks\(int m\);", h)
    src = open(SRC).read()
    fits = re.search(r"bool predict_missing_fits\(int kind, int de, int m, int k\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "{1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20}" in fits
    assert "kind == GPZ_KIND_DIAG && width && k >= 1 && k <= 8 && m >= 1 && ((m + 15) / 16) * 16 <= 256" in fits
    groups = re.search(r"long predict_missing_groups\(int m\) \{(.*?)\}", src, flags=re.S).group(1)
    assert "((long)m * (m + 1) / 2 + 63) / 64" in groups
    body = re.search(r"int predict_missing_chunks\(int m\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "const long c = predict_missing_groups(m) / 16;" in body and "(c > 8 ? 8 : c)" in body
    for text in (fits, groups, body):
        for word in ("ns", "nt", "n", "tile", "rows"):
            assert not re.search(r"\b" + word + r"\b", text), word
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "predict_missing_fits(p->kind, p->de, p->m, p->k)" in host and "predict_missing_chunks(p->m)" in host
    # the Python check of the keyword is the same rule for the padded widths of d <= 20
    assert fits_rule(True, 20, 256, 8) and not fits_rule(True, 20, 257, 8) and not fits_rule(True, 20, 256, 9)
    assert not fits_rule(False, 5, 10, 1) and not fits_rule(True, 24, 10, 1) and not fits_rule(True, 7, 10, 1)
    # where the chunk rule changes: the block-edge test of the GPU suite walks m on both sides of several of these
    changes = [m for m in range(2, 257) if chunks_rule(m) != chunks_rule(m - 1)]
    assert changes == [63, 78, 90, 101, 110, 119, 128]
    assert [chunks_rule(m) for m in (1, 11, 62, 63, 100, 127, 128, 256)] == [1, 1, 1, 2, 4, 7, 8, 8]


# ---- the four units of the one pair-kernel body ----------------------------------------------------------------------------------------------
GROUP_UNITS = {"k_predict_missing": ("k_predict_missing_pairs", [1, 8]),
               "k_predict_noisy_missing": ("k_predict_noisy_missing_pairs", [1, 8]),
               "k_predict_missing_gamma": ("k_predict_missing_gamma", list(range(1, 9))),
               "k_predict_noisy_missing_gamma": ("k_predict_noisy_missing_gamma", list(range(1, 9)))}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_each_unit_holds_exactly_its_own_pair_kernels(tmp_path):
    """The four pair kernels are wrappers around predict_group_body<PSI, Sink> of k_predict_group_impl.h.  Each unit's listing holds the
    instantiations of its own kernel and of no other of the four, every one on the shared argument struct, and the unit's text names
    the body once, with the PSI and the sink of its name: a wrapper that named the wrong ones would still compile."""
    procs = {u: subprocess.Popen(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                                  "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, u + ".hip"),
                                  "-o", str(tmp_path / (u + ".s"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for u in GROUP_UNITS}
    for u, (kname, counts) in GROUP_UNITS.items():
        _, err = procs[u].communicate(timeout=1800)
        assert procs[u].returncode == 0, err[-2000:]
        recs = _resource_records(err)
        found = sorted((m.group(1), int(m.group(2))) for m in (re.match(r"_Z\d+(k_predict_\w+?)ILi(\d+)EEv", n) for n in recs) if m)
        assert found == [(kname, c) for c in counts], (u, found)
        assert not any("k_predict_" in n and not re.match(r"_Z\d+k_predict_\w+?ILi\d+EEv13PredGroupArgs$", n) for n in recs), sorted(recs)
        src = open(os.path.join(CSRC, u + ".hip")).read()
        psi, sink = "noisy" in u, "PredGammaSink<NB>" if "gamma" in u else "PredPairsSink<KM>"
        assert f"predict_group_body<{'true' if psi else 'false'}, {sink}>(a);" in src, u
        assert src.count("predict_group_body<") == 1, u
