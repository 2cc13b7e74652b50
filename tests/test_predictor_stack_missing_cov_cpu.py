"""CPU-side checks of the stacks of rows with missing inputs on a covariance kind and of gamma under every weight draw
(Predictor.stack_missing_cov_dev, draws_missing_cov_dev(..., return_gamma=True); gpz_predictor_stack_missing_cov_dev /
_draws_gamma_missing_cov_dev): the declarations against the binding, the library and the entry table with exactly the twins' arguments,
the compiled form of k_predict_missing_cov_gamma.hip and its LDS rule, every refusal of the two Python entries before the library is
loaded, and the definition of gamma_s as a quadratic form of the draw's weights, stated with the NumPy oracle alone."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, synth_model
from test_predictor_stack_missing_cpu import _model, _resource_records
from test_predictor_stack_noisy import with_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
SRC = os.path.join(CSRC, "k_predict_missing_cov_gamma.hip")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_draws_gamma_missing_cov_dev": "gpz_predictor_draws_gamma_missing_dev",
           "gpz_predictor_stack_missing_cov_dev": "gpz_predictor_stack_missing_dev"}
LDS_MAX = 160 * 1024


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_binding_library_and_entry_table_agree():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name, twin in ENTRIES.items():
        args = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
        assert args, f"{name} is not declared in gpz_hip.h"
        old = re.search(r"\bint " + twin + r"\(([^;]*)\);", h).group(1)
        assert [a.strip() for a in args.group(1).split(",")] == [a.strip() for a in old.split(",")]   # exactly the twin's arguments
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name] == _lib.SYMBOLS[twin], name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    E = gpz_amd.predictor._DEV_ENTRIES
    assert E["draws_gamma", "missing_cov"] == "gpz_predictor_draws_gamma_missing_cov_dev"
    assert E["stack", "missing_cov"] == "gpz_predictor_stack_missing_cov_dev"
    assert E["draws_gamma", "missing"] == "gpz_predictor_draws_gamma_missing_dev" and E["stack", "missing"] == "gpz_predictor_stack_missing_dev"
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert re.search(r'UNITS="[^"]*\bk_predict_missing_cov_gamma\b', build) and "k_pmcv_density.h" in build
    kh = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert "int launch_predict_missing_cov_gamma(" in kh and "size_t predict_missing_cov_gamma_lds(int m, int no);" in kh
    assert "int launch_pmc_triples(" in kh
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "&p->mcslab_kept, p->Wd, ldw, ncol, p->mchunks, p->gpart, nt))" in host    # the pair kernel's own chunks and slab state
    assert "; missing per draw: k_predict_missing_cov_gamma (%d pair chunks)" in host
    old = open(os.path.join(CSRC, "k_predict_missing_cov.hip")).read()
    assert old.count("void k_pmc_triples(") == 1 and "k_pmc_triples" not in open(SRC).read().replace("launch_pmc_triples", "")


# ---- the compiled form ---------------------------------------------------------------------------------------------------------------------
def gamma_cov_lds_rule(m, no):
    """predict_missing_cov_gamma_lds of k_predict_missing_cov_gamma.hip and DESIGN.md section 30, stated a second time on purpose: the
    Pio block of the workgroup's 64 rows and four stages of 16 records, an odd number of doubles apart."""
    rl = 1 + no + no * (no + 1) // 2
    return 8 * (64 * m + 4 * ((16 * rl) | 1))


def test_the_lds_rule_fits_the_compute_unit_for_every_shape():
    worst = max((gamma_cov_lds_rule(m, no), m, no) for m in range(1, 257) for no in range(10))
    assert worst == (159_264, 256, 9) and worst[0] <= LDS_MAX
    assert gamma_cov_lds_rule(100, 4) == 58_912 and 2 * gamma_cov_lds_rule(100, 4) <= LDS_MAX   # the timing shape: two workgroups
    assert gamma_cov_lds_rule(100, 9) == 79_392 and 2 * gamma_cov_lds_rule(100, 9) <= LDS_MAX
    for no in range(10):                                                 # four stages start in four different banks
        s = (16 * (1 + no + no * (no + 1) // 2)) | 1
        assert len({(g * s) % 32 for g in range(4)}) == 4, no
    src = open(SRC).read()
    body = re.search(r"size_t predict_missing_cov_gamma_lds\(int m, int no\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "((size_t)m * 64 + 4 * (size_t)pmcg_stride(predict_missing_cov_rec(no))) * sizeof(double)" in body
    assert "constexpr int pmcg_stride(int rl) { return (PMCV_SB * rl) | 1; }" in src
    assert "#define PMCV_SB 16" in open(os.path.join(CSRC, "k_pmcv_density.h")).read()
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in src and "nchunk != predict_missing_cov_chunks(m)" in src
    assert "(64 m + 4 ((16 RL) | 1))" in open(os.path.join(ROOT, "DESIGN.md")).read()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_missing_cov_gamma_kernel_compiled_form(tmp_path):
    """k_predict_missing_cov_gamma<NO>, NO = 0 .. 9, and no other kernel in the unit: no scratch, no spilled register, VGPRs + AGPRs <=
    256 (the kernel claims two workgroups of 256 per compute unit with its launch bound, for every NO), no static LDS (all of it is the
    dynamic block of predict_missing_cov_gamma_lds), the f64 MFMA and no atomic of any kind."""
    asm = tmp_path / "k_predict_missing_cov_gamma.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    assert len(recs) == 10 and all("k_predict_missing_cov_gamma" in n for n in recs), sorted(recs)
    assert sorted(int(re.search(r"ILi(\d+)E", n).group(1)) for n in recs) == list(range(10))
    assert "__launch_bounds__(256, 2) void k_predict_missing_cov_gamma" in open(SRC).read()
    print("NO  VGPRs  AGPRs")
    no_of = {name: int(re.search(r"ILi(\d+)E", name).group(1)) for name in recs}
    for name, q in sorted(recs.items(), key=lambda t: no_of[t[0]]):
        print(f"{no_of[name]:2d}  {q['VGPRs']:5d}  {q.get('AGPRs', 0):5d}")
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
        assert q["LDS Size [bytes/block]"] == 0, (name, q)
    text = asm.read_text()
    assert "v_mfma_f64_16x16x4" in text
    for word in ("global_atomic", "flat_atomic", "ds_add_f", "ds_add_rtn_f", "cmpswap", "scratch_"):
        assert word not in text, word


# ---- the refusals of the two Python entries ----------------------------------------------------------------------------------------------
def test_new_entries_validate_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of stack_missing_cov_dev and of draws_missing_cov_dev(return_gamma=True) is raised on the host: the
    library load is made to fail, so a call that got past the checks would raise RuntimeError instead.  Each refusal of the kind of
    rows or model says where such rows go."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    e = np.linspace(0.0, 1.0, 11)
    p = gpz_amd.Predictor(_model(method="VC"))
    X = torch.zeros((4, 3), dtype=torch.float64)
    X[1, 2] = float("nan")
    psi = torch.ones((4, 3), dtype=torch.float64)
    # ---- stack_missing_cov_dev
    with pytest.raises(TypeError, match="stack_missing_cov_dev takes a torch tensor.*Predictor.predict"):
        p.stack_missing_cov_dev(np.zeros((4, 3)), e)
    with pytest.raises(TypeError, match="X must be a torch.Tensor"):
        p.stack_missing_cov_dev([[0.0, 0.0, 0.0]] * 4, e)
    with pytest.raises(TypeError, match="X must be float64 or float32"):
        p.stack_missing_cov_dev(X.long(), e)
    with pytest.raises(ValueError, match="X must be n x 3"):
        p.stack_missing_cov_dev(torch.zeros((4, 2), dtype=torch.float64), e)
    with pytest.raises(TypeError, match="selection"):
        p.stack_missing_cov_dev(X, e, selection=torch.ones(4))
    with pytest.raises(ValueError, match="selection"):
        p.stack_missing_cov_dev(X, e, selection=torch.ones(3, dtype=torch.bool))
    for bad in (e[::-1], e[:1], np.array([0.0, np.nan, 1.0]), e.reshape(1, -1)):
        with pytest.raises(ValueError, match="edges"):
            p.stack_missing_cov_dev(X, bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="n_draws"):
            p.stack_missing_cov_dev(X, e, n_draws=bad)
    with pytest.raises(ValueError, match="over the limit"):
        p.stack_missing_cov_dev(X, e, n_draws=gpz_amd.api.GPZ_DRAWS_MAX_COLUMNS)
    with pytest.raises(ValueError, match="seed"):
        p.stack_missing_cov_dev(X, e, n_draws=2, seed=-1)
    with pytest.raises(ValueError, match="Z must be None"):
        p.stack_missing_cov_dev(X, e, Z=np.zeros((6, 1, 1)))
    with pytest.raises(ValueError, match="Z must have shape"):
        p.stack_missing_cov_dev(X, e, n_draws=2, Z=np.zeros((6, 3, 1)))
    for bad in (torch.zeros(4), torch.zeros(3, dtype=torch.int64), np.zeros(4, dtype=int), torch.zeros(4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="groups"):
            p.stack_missing_cov_dev(X, e, groups=bad)
    for bad in (torch.zeros(3), torch.zeros(4, dtype=torch.int64), np.ones(4)):
        with pytest.raises(ValueError, match="weights"):
            p.stack_missing_cov_dev(X, e, weights=bad)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="n_groups"):
            p.stack_missing_cov_dev(X, e, n_groups=bad)
    with pytest.raises(ValueError, match="n_groups \\* bins"):
        p.stack_missing_cov_dev(X, e, n_groups=gpz_amd.api.GPZ_STACK_MAX_GROUP_BINS)
    for ok in (X, X.float(), X.T.contiguous().T):
        with pytest.raises(ValueError, match="must be on cuda:0.*Predictor.predict takes a catalogue"):   # the device, last
            p.stack_missing_cov_dev(ok, e, n_draws=2, groups=torch.zeros(4, dtype=torch.int64), weights=torch.ones(4))
    with pytest.raises(TypeError, match="Psi"):                           # no Psi together with missing values, and no keyword for it
        p.stack_missing_cov_dev(X, e, Psi=psi)
    # ---- return_gamma
    with pytest.raises(ValueError, match="does not take Psi.*Predictor.predict"):
        p.draws_missing_cov_dev(X, 4, Psi=psi, return_gamma=True)
    with pytest.raises(ValueError, match="n_draws"):
        p.draws_missing_cov_dev(X, 0, return_gamma=True)
    with pytest.raises(ValueError, match="X must be n x 3"):
        p.draws_missing_cov_dev(torch.zeros((4, 2), dtype=torch.float64), 4, return_gamma=True)
    with pytest.raises(TypeError, match="draws_missing_cov_dev takes a torch tensor.*Predictor.predict"):
        p.draws_missing_cov_dev(np.zeros((4, 3)), 4, return_gamma=True)
    with pytest.raises(ValueError, match="must be on cuda:0.*Predictor.predict takes a catalogue"):
        p.draws_missing_cov_dev(X, 4, return_gamma=True)
    with pytest.raises(ValueError, match="must be on cuda:0"):            # the call without the keyword is the call as it was
        p.draws_missing_cov_dev(X, 4)
    # ---- the entries of the other kinds keep refusing a covariance kind, with the texts they have
    with pytest.raises(ValueError, match="stack_missing_dev.*predict_missing_fits.*a diagonal kind .* not VC"):
        p.stack_missing_dev(X, e)
    with pytest.raises(ValueError, match="predict_missing_fits.*a diagonal kind .* not VC"):
        p.draws_dev(X, 4, missing=True, return_gamma=True)
    with pytest.raises(ValueError, match="stack_noisy_cov_dev needs Psi"):
        p.stack_noisy_cov_dev(X, None, e)
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.stack_missing_cov_dev(X, e)
    with pytest.raises(RuntimeError, match="closed"):
        p.draws_missing_cov_dev(X, 4, return_gamma=True)
    # ---- models outside predict_missing_cov_fits, and a diagonal kind by name
    for kw, text in (({"m": 257}, "predict_missing_cov_fits.*m = 257"), ({"d": 11}, "predict_missing_cov_fits.*d = 11"),
                     ({"k": 9}, "predict_missing_cov_fits.*k = 9")):
        model = _model(**{"method": "GC", **kw})
        q = gpz_amd.Predictor(model)
        Xd = torch.zeros((4, model.d), dtype=torch.float64)
        with pytest.raises(ValueError, match="stack_missing_cov_dev.*" + text + ".*Predictor.predict"):
            q.stack_missing_cov_dev(Xd, e)
        with pytest.raises(ValueError, match="draws_missing_cov_dev.*" + text + ".*Predictor.predict"):
            q.draws_missing_cov_dev(Xd, 4, return_gamma=True)
        with pytest.raises(ValueError, match="must be on cuda:0"):        # without missing values these models are as before
            q.stack_dev(Xd, e)
    q = gpz_amd.Predictor(_model(method="VD"))
    with pytest.raises(ValueError, match=r"stack_missing_cov_dev is for the covariance kinds.*VD goes to stack_missing_dev\(X, edges\)"):
        q.stack_missing_cov_dev(X, e)
    with pytest.raises(ValueError, match=r"draws_missing_cov_dev is for the covariance kinds.*VD goes to draws_dev\(X, missing=True\)"):
        q.draws_missing_cov_dev(X, 4, return_gamma=True)
    bad = _model(method="VC")
    bad.sets["best"]["priors"] = np.ones(5) / 5                           # m = 6
    with pytest.raises(ValueError, match="priors"):
        gpz_amd.Predictor(bad).stack_missing_cov_dev(X, e)
    with pytest.raises(ValueError, match="priors"):
        gpz_amd.Predictor(bad).draws_missing_cov_dev(X, 4, return_gamma=True)


# ---- the definition ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["GC", "VC"])
def test_gamma_per_draw_is_a_quadratic_form_of_the_draws_weights(method):
    """gamma_s + mu_s^2 = sum_{a >= b} f_ab z_ab(x) w_s,a w_s,b is a quadratic form w_s' E w_s whose matrix E(x) does not depend on w.
    The oracle does not expose the pair quantities, so E is recovered from ``O.predict_any`` through ``with_weights`` by polarisation
    (E_aa from w = e_a, E_ab from w = e_a + e_b), and the form under a draw's weights reproduces predict_any's gamma of the w := w_s
    model at the project's oracle gate, rel <= 1e-8: the definition, fixed without any kernel.  m = 4, d = 3; one dimension missing,
    two missing, and complete rows."""
    m, d, k, n = 4, 3, 2, 10
    model = synth_model(method, m, d, k, True, seed=29)
    model.sets["best"]["priors"] = np.random.default_rng(30).dirichlet(np.full(m, 2.0))
    X = catalogue(model, n, seed=31)
    X[0:4, 1] = np.nan
    X[4:8, 0] = X[4:8, 2] = np.nan                                         # rows 8, 9 stay complete
    muY = np.asarray(model.muY).reshape(-1)

    def second_moment(w):
        out = O.predict_any(X, with_weights(model, w))
        return out[4] + (out[0] - muY) ** 2                                # gamma + mu^2, (n, k)

    eye = np.eye(m)
    E = np.zeros((n, k, m, m))
    for a in range(m):
        E[:, :, a, a] = second_moment(np.repeat(eye[:, a:a + 1], k, axis=1))
    for a in range(m):
        for b in range(a):
            both = second_moment(np.repeat((eye[:, a] + eye[:, b])[:, None], k, axis=1))
            E[:, :, a, b] = E[:, :, b, a] = 0.5 * (both - E[:, :, a, a] - E[:, :, b, b])
    rng = np.random.default_rng(32)
    for s in range(3):
        ws = model.sets["best"]["w"] + 0.3 * rng.standard_normal((m, k))
        out = O.predict_any(X, with_weights(model, ws))
        mu_s = out[0] - muY
        # f_ab = 2 off the diagonal: the sum over a >= b of f_ab E_ab w_a w_b
        tri = sum((1.0 if a == b else 2.0) * E[:, :, a, b] * ws[a] * ws[b] for a in range(m) for b in range(a + 1))
        gamma_s = tri - mu_s ** 2
        print(f"{method} draw {s}: rel of the form's gamma_s against the oracle's {rel(gamma_s[:8], out[4][:8]):.3e}")
        assert rel(gamma_s[:8], out[4][:8]) <= 1e-8, (s, rel(gamma_s[:8], out[4][:8]))
        assert np.all(out[4][8:] == 0.0) and np.all(np.abs(gamma_s[8:]) <= 1e-12 * np.max(np.abs(tri)))
        assert np.all(out[4][:8] > 0.0)
