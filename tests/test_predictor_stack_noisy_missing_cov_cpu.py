"""CPU-side checks of the stacks of rows with input noise and missing inputs on a covariance kind and of gamma under every weight draw
(Predictor.stack_noisy_missing_cov_dev, draws_noisy_missing_cov_dev(..., return_gamma=True); gpz_predictor_stack_noisy_missing_cov_dev /
_draws_gamma_noisy_missing_cov_dev): the declarations against the binding, the library and the entry table with exactly the diagonal
twins' arguments, the compiled form of k_predict_noisy_missing_cov_gamma.hip, its LDS rule and the rules it borrows, every refusal of the
two Python entries before the library is loaded, and the definition of gamma_s as a quadratic form of the draw's weights, stated with the
NumPy oracle alone."""
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
from test_predictor_noisy_cpu import _model, _resource_records
from test_predictor_noisy_missing_cov_cpu import rec_len
from test_predictor_stack_noisy import with_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
SRC = os.path.join(CSRC, "k_predict_noisy_missing_cov_gamma.hip")
OLD = os.path.join(CSRC, "k_predict_noisy_missing_cov.hip")
IMPL = os.path.join(CSRC, "k_predict_nmcov_impl.h")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_draws_gamma_noisy_missing_cov_dev": "gpz_predictor_draws_gamma_noisy_missing_dev",
           "gpz_predictor_stack_noisy_missing_cov_dev": "gpz_predictor_stack_noisy_missing_dev"}
LDS_MAX = 160 * 1024
# the instantiations DESIGN.md section 32 reports above 256 registers (one workgroup per compute unit by their launch bound)
OVER_256 = {8, 9}


# ---- 1. the ABI --------------------------------------------------------------------------------------------------------------------------
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
    assert E["draws_gamma", "noisy_missing_cov"] == "gpz_predictor_draws_gamma_noisy_missing_cov_dev"
    assert E["stack", "noisy_missing_cov"] == "gpz_predictor_stack_noisy_missing_cov_dev"
    assert E["draws_gamma", "noisy_missing"] == "gpz_predictor_draws_gamma_noisy_missing_dev"
    assert E["stack", "noisy_missing"] == "gpz_predictor_stack_noisy_missing_dev"
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert re.search(r'UNITS="[^"]*\bk_predict_noisy_missing_cov_gamma\b', build) and "k_pnmc_density.h" in build
    kh = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert "int launch_predict_noisy_missing_cov_gamma(" in kh and "int launch_pnmc_triples(" in kh
    assert "size_t predict_noisy_missing_cov_gamma_lds(int m, int d, int no);" in kh
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "; noisy missing per draw: k_predict_noisy_missing_cov_gamma (%d pair chunks)" in host
    assert "p->nmcslab, &p->nmcslab_kept, p->Wd" in host                  # the pair kernel's own slab and its state
    assert "} gam[8];" in open(os.path.join(CSRC, "gpz_predictor.h")).read()   # one slot per kind of rows with gamma per draw, this kind's the sixth
    for f in ("gpz_predictor.h", "gpz_predictor.hip", "gpz_predictor_host.hip", "gpz_predictor_dev.hip"):   # indexed by kind - 1, no accessor
        text = open(os.path.join(CSRC, f)).read()
        assert "gam_pcm" not in text and "rows_gamma_state" not in text, f
    old = open(OLD).read()                                               # one generation kernel, reached through its launcher
    assert old.count("void k_pnmc_triples(") == 1 and "k_pnmc_triples" not in open(SRC).read().replace("launch_pnmc_triples", "")
    assert "pnmc_density" not in old and "#define PNMC_CASES" not in old   # they moved to the header
    head = open(os.path.join(CSRC, "k_pnmc_density.h")).read()
    assert "double pnmc_density(" in head and "#define PNMC_CASES(MACRO)" in head


# ---- 2. the compiled form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_noisy_missing_cov_gamma_kernel_compiled_form(tmp_path):
    """The resource remarks only.  k_predict_noisy_missing_cov_gamma<NO>, NO = 1 .. 9, and no other kernel in the unit: no scratch, no
    spilled register, no static LDS (all of it is the dynamic block of predict_noisy_missing_cov_gamma_lds), VGPRs + AGPRs <= 512 and
    <= 256 for all but the two instantiations DESIGN.md section 32 names."""
    asm = tmp_path / "k_predict_noisy_missing_cov_gamma.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    assert len(recs) == 9 and all("k_predict_noisy_missing_cov_gamma" in n for n in recs), sorted(recs)
    no_of = {name: int(re.search(r"ILi(\d+)E", name).group(1)) for name in recs}
    assert sorted(no_of.values()) == list(range(1, 10))
    print("NO  VGPRs  AGPRs")
    for name, q in sorted(recs.items(), key=lambda t: no_of[t[0]]):
        regs = q["VGPRs"] + q.get("AGPRs", 0)
        print(f"{no_of[name]:2d}  {q['VGPRs']:5d}  {q.get('AGPRs', 0):5d}")
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert regs <= 512 and (regs <= 256 or no_of[name] in OVER_256), (name, q)
        assert q["LDS Size [bytes/block]"] == 0, (name, q)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_predict_noisy_missing_cov_gamma<8>" in design and "k_predict_noisy_missing_cov_gamma<9>" in design


# ---- 3. LDS and rules --------------------------------------------------------------------------------------------------------------------
def gamma_lds_rule(m, d, no):
    """predict_noisy_missing_cov_gamma_lds of the unit and DESIGN.md section 32, stated a second time on purpose: the Pio block of the
    workgroup's 64 rows and four stages of 4 records, an odd number of doubles apart."""
    return 8 * (64 * m + 4 * ((4 * rec_len(d, no)) | 1))


def test_the_lds_rule_fits_the_compute_unit_and_the_rules_are_borrowed():
    worst = max((gamma_lds_rule(256, d, no), d, no) for d in range(2, 11) for no in range(1, d))
    assert worst == (149_792, 10, 9) and worst[0] <= 163_840
    for d in range(2, 11):
        for no in range(1, d):
            assert (64 * 256 + 4 * ((4 * rec_len(d, no)) | 1)) * 8 <= 163_840, (d, no)
            s = (4 * rec_len(d, no)) | 1
            assert s % 2 == 1 and s >= 4 * rec_len(d, no)                   # odd, and a stage of 4 records fits under it
            assert len({(g * s) % 32 for g in range(4)}) == 4, (d, no)     # four stages start in four different banks
    assert gamma_lds_rule(100, 5, 4) == 55_840 and 2 * gamma_lds_rule(100, 5, 4) <= LDS_MAX   # the timing shape: two workgroups
    src = open(SRC).read()
    body = re.search(r"size_t predict_noisy_missing_cov_gamma_lds\(int m, int d, int no\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "((size_t)m * 64 + 4 * (size_t)nmcg_stride(predict_noisy_missing_cov_rec(d, no))) * sizeof(double)" in body
    for word in ("n", "ns", "nt", "tile", "rows", "k", "ncol"):            # m, d and no alone
        assert not re.search(r"\b" + word + r"\b", body), word
    impl = open(IMPL).read()                                             # the stride and the stage: one definition, beside the body
    assert "int nmcg_stride(int rl) { return (GPZ_NMCG_SB * rl) | 1; }" in impl and re.search(r"#define GPZ_NMCG_SB 4\b", impl)
    assert "nmcg_stride" not in src.replace("nmcg_stride(predict_noisy_missing_cov_rec(d, no))", "") and "GPZ_NMCG_SB" not in src
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in impl
    # the chunk and slab rules: not restated (tests/test_predictor_noisy_missing_cov_cpu.py holds their use by the launchers)
    for text in (src, impl):
        assert "int predict_missing_cov_chunks(" not in text and "int predict_noisy_missing_cov_slabs(" not in text
        assert "PNMC_SLAB_BYTES" not in text and "int predict_noisy_missing_cov_rec(" not in text
    # the blocks of a pass and the launch bound are functions of NO alone
    assert "constexpr int nmcg_nb(int no)" in src and "constexpr int nmcg_wg(int no)" in src
    assert "__launch_bounds__(256, nmcg_wg(NO)) void k_predict_noisy_missing_cov_gamma" in src
    assert "(64 m + 4 ((4 rl) | 1))" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- 4. the definition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["GC", "VC"])
def test_gamma_per_draw_is_a_quadratic_form_of_the_draws_weights(method):
    """gamma_s + mu_s^2 = sum_{a >= b} f_ab z_ab(x, psi) w_s,a w_s,b is a quadratic form w_s' E w_s whose matrix E(x, psi) does not depend
    on w.  The oracle does not expose the pair quantities, so E is recovered from ``O.predict_any(X, model, Psi=Psi)``
    (predictNoisyMissing) through ``with_weights`` by polarisation (E_aa from w = e_a, E_ab from w = e_a + e_b), and the form under a
    draw's weights reproduces the oracle's gamma of the w := w_s model at the project's oracle gate, rel <= 1e-8: the definition, fixed
    without any kernel.  m = 4, d = 3, Psi > 0; one dimension missing (dimension 1: [o u] = [0 2 1] is its own inverse; dimension 0:
    [1 2 0] is not) and two missing."""
    m, d, k, n = 4, 3, 2, 12
    model = synth_model(method, m, d, k, True, seed=29)
    model.sets["best"]["priors"] = np.random.default_rng(30).dirichlet(np.full(m, 2.0))
    X = catalogue(model, n, seed=31)
    X[0:4, 1] = np.nan
    X[4:8, 0] = np.nan
    X[8:12, 0] = X[8:12, 2] = np.nan
    Psi = 0.05 + 0.2 * np.random.default_rng(33).random((n, d)) * np.asarray(model.sdX).reshape(-1) ** 2
    muY = np.asarray(model.muY).reshape(-1)

    def second_moment(w):
        out = O.predict_any(X, with_weights(model, w), Psi=Psi)
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
        out = O.predict_any(X, with_weights(model, ws), Psi=Psi)
        mu_s = out[0] - muY
        # f_ab = 2 off the diagonal: the sum over a >= b of f_ab E_ab w_a w_b
        tri = sum((1.0 if a == b else 2.0) * E[:, :, a, b] * ws[a] * ws[b] for a in range(m) for b in range(a + 1))
        gamma_s = tri - mu_s ** 2
        print(f"{method} draw {s}: rel of the form's gamma_s against the oracle's {rel(gamma_s, out[4]):.3e}")
        assert rel(gamma_s, out[4]) <= 1e-8, (s, rel(gamma_s, out[4]))
        assert np.all(out[4] > 0.0)


# ---- 5. the refusals of the two Python entries ---------------------------------------------------------------------------------------------
def test_refusals_fire_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of stack_noisy_missing_cov_dev and of draws_noisy_missing_cov_dev(return_gamma=True) is raised on the
    host: the library load is made to fail, so a call that got past the checks would raise RuntimeError instead.  Each refusal of the
    kind of rows or model says where such rows go.  Type, dtype, shape, model, edges, draws, groups, weights; the device last."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    e = np.linspace(0.0, 1.0, 11)
    X = torch.zeros((4, 3), dtype=torch.float64)
    X[1, 2] = float("nan")
    Psi = torch.ones((4, 3), dtype=torch.float64)
    for method in ("VC", "GC"):
        p = gpz_amd.Predictor(_model(method=method))
        calls = {"stack": lambda x, psi, **kw: p.stack_noisy_missing_cov_dev(x, psi, e, **kw),
                 "draws": lambda x, psi, **kw: p.draws_noisy_missing_cov_dev(x, psi, 4, return_gamma=True, **kw)}
        for what, call in calls.items():
            with pytest.raises(TypeError, match=rf"{what}_noisy_missing_cov_dev takes a torch tensor.*Predictor.predict\(X, Psi=Psi\)"):
                call(np.zeros((4, 3)), Psi)
            with pytest.raises(TypeError, match="X must be a torch.Tensor"):
                call([[0.0] * 3] * 4, Psi)
            with pytest.raises(TypeError, match="X must be float64 or float32"):
                call(X.half(), Psi)
            with pytest.raises(ValueError, match="X must be n x 3"):
                call(torch.zeros((4, 2), dtype=torch.float64), Psi)
            with pytest.raises(TypeError, match="selection must be a bool torch tensor"):
                call(X, Psi, selection=np.ones(4, dtype=bool))
            with pytest.raises(ValueError, match=f"{what}_noisy_missing_cov_dev needs Psi.*{what}_missing_cov_dev"):
                call(X, None)
            with pytest.raises(ValueError, match=r"full d x d x n Psi stays on Predictor.predict\(X, Psi=Psi\)"):
                call(X, torch.ones((3, 3, 4), dtype=torch.float64))
            with pytest.raises(TypeError, match="Psi as a torch tensor"):
                call(X, np.ones((4, 3)))
            with pytest.raises(TypeError, match="Psi must be float64 or float32"):
                call(X, Psi.long())
            with pytest.raises(ValueError, match="Psi must be n x d, n x 1 or n"):
                call(X, torch.ones((4, 2), dtype=torch.float64))
            for okx, okp in ((X, Psi), (X.float(), Psi[:, :1]), (X.T.contiguous().T, Psi[:, 0]), (X[::2], Psi[::2].float())):
                with pytest.raises(ValueError, match="must be on cuda:0"):   # the device, last
                    call(okx, okp)
        # ---- what the stack alone takes
        for bad in (e[::-1], e[:1], np.array([0.0, np.nan, 1.0]), e.reshape(1, -1)):
            with pytest.raises(ValueError, match="edges"):
                p.stack_noisy_missing_cov_dev(X, Psi, bad)
        for bad in (-1, 1.5, True):
            with pytest.raises(ValueError, match="n_draws"):
                p.stack_noisy_missing_cov_dev(X, Psi, e, n_draws=bad)
        with pytest.raises(ValueError, match="over the limit"):
            p.stack_noisy_missing_cov_dev(X, Psi, e, n_draws=gpz_amd.api.GPZ_DRAWS_MAX_COLUMNS)
        with pytest.raises(ValueError, match="seed"):
            p.stack_noisy_missing_cov_dev(X, Psi, e, n_draws=2, seed=-1)
        with pytest.raises(ValueError, match="Z must have shape"):
            p.stack_noisy_missing_cov_dev(X, Psi, e, n_draws=2, Z=np.zeros((6, 3, 1)))
        for bad in (torch.zeros(4), torch.zeros(3, dtype=torch.int64), np.zeros(4, dtype=int), torch.zeros(4, dtype=torch.bool)):
            with pytest.raises(ValueError, match="groups"):
                p.stack_noisy_missing_cov_dev(X, Psi, e, groups=bad)
        for bad in (torch.zeros(3), torch.zeros(4, dtype=torch.int64), np.ones(4)):
            with pytest.raises(ValueError, match="weights"):
                p.stack_noisy_missing_cov_dev(X, Psi, e, weights=bad)
        for bad in (0, -2, 1.5, True):
            with pytest.raises(ValueError, match="n_groups"):
                p.stack_noisy_missing_cov_dev(X, Psi, e, n_groups=bad)
        with pytest.raises(ValueError, match="n_groups \\* bins"):
            p.stack_noisy_missing_cov_dev(X, Psi, e, n_groups=gpz_amd.api.GPZ_STACK_MAX_GROUP_BINS)
        with pytest.raises(ValueError, match="must be on cuda:0"):           # the default of 64 draws, labels and weights: the device, last
            p.stack_noisy_missing_cov_dev(X, Psi, e, groups=torch.zeros(4, dtype=torch.int64), weights=torch.ones(4))
        with pytest.raises(ValueError, match="n_draws"):
            p.draws_noisy_missing_cov_dev(X, Psi, 0, return_gamma=True)
        with pytest.raises(ValueError, match="must be on cuda:0"):           # the call without the keyword is the call as it was
            p.draws_noisy_missing_cov_dev(X, Psi, 4)
        # ---- the entries of the other kinds keep refusing, with the texts they have
        with pytest.raises(ValueError, match=r"predict_missing_fits: a diagonal kind"):
            p.stack_noisy_missing_dev(X, Psi, e)
        with pytest.raises(ValueError, match=r"predict_missing_fits: a diagonal kind"):
            p.draws_noisy_missing_dev(X, Psi, 4, return_gamma=True)
        with pytest.raises(ValueError, match=r"does not take Psi.*Predictor.predict\(X, Psi=Psi\)"):
            p.draws_missing_cov_dev(X, 4, Psi=Psi, return_gamma=True)
        p.close()
        with pytest.raises(RuntimeError, match="closed"):
            p.stack_noisy_missing_cov_dev(X, Psi, e)
        with pytest.raises(RuntimeError, match="closed"):
            p.draws_noisy_missing_cov_dev(X, Psi, 4, return_gamma=True)
    # a diagonal kind is sent to its own methods by name
    for method in ("GL", "VL", "GD", "VD"):
        q = gpz_amd.Predictor(_model(method=method))
        with pytest.raises(ValueError, match=r"diagonal kind.*stack_noisy_missing_dev\(X, Psi\)"):
            q.stack_noisy_missing_cov_dev(X, Psi, e)
        with pytest.raises(ValueError, match=r"diagonal kind.*draws_noisy_missing_dev\(X, Psi\)"):
            q.draws_noisy_missing_cov_dev(X, Psi, 4, return_gamma=True)
    # shapes outside predict_missing_cov_fits
    for kw, text in (({"m": 257}, "m = 257"), ({"d": 11}, "d = 11"), ({"k": 9}, "k = 9")):
        model = _model(method="VC", **kw)
        q = gpz_amd.Predictor(model)
        Xd, Pd = torch.zeros((4, model.d), dtype=torch.float64), torch.ones((4, model.d), dtype=torch.float64)
        with pytest.raises(ValueError, match="stack_noisy_missing_cov_dev.*predict_missing_cov_fits.*" + text + ".*Predictor.predict"):
            q.stack_noisy_missing_cov_dev(Xd, Pd, e)
        with pytest.raises(ValueError, match="draws_noisy_missing_cov_dev.*predict_missing_cov_fits.*" + text + ".*Predictor.predict"):
            q.draws_noisy_missing_cov_dev(Xd, Pd, 4, return_gamma=True)
    # the edges of the scope pass the shape check (and then stop at the device)
    for kw in ({"m": 256}, {"d": 10}, {"d": 1}, {"k": 8}):
        model = _model(method="GC", **kw)
        q = gpz_amd.Predictor(model, force_tiles=True)                        # (no route is refused)
        Xd, Pd = torch.zeros((4, model.d), dtype=torch.float64), torch.ones((4, model.d), dtype=torch.float64)
        with pytest.raises(ValueError, match="must be on cuda:0"):
            q.stack_noisy_missing_cov_dev(Xd, Pd, e, n_draws=2)
        with pytest.raises(ValueError, match="must be on cuda:0"):
            q.draws_noisy_missing_cov_dev(Xd, Pd, 4, return_gamma=True)
    bad = _model(method="VC")
    bad.sets["best"]["priors"] = np.ones(5) / 5                           # m = 6
    with pytest.raises(ValueError, match="priors of the set must be 6 values"):
        gpz_amd.Predictor(bad).stack_noisy_missing_cov_dev(X, Psi, e)
    with pytest.raises(ValueError, match="priors of the set must be 6 values"):
        gpz_amd.Predictor(bad).draws_noisy_missing_cov_dev(X, Psi, 4, return_gamma=True)
