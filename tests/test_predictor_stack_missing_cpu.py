"""CPU-side checks of the stacks of rows with missing inputs and of gamma under every weight draw (Predictor.stack_missing_dev,
draws_dev(..., missing=True, return_gamma=True); gpz_predictor_stack_missing_dev / _draws_gamma_missing_dev): every refusal of the two
Python entries before the library is loaded, the declarations against the binding, the compiled form of k_predict_missing_gamma.hip and
its LDS rule, and the definition of gamma_s as a quadratic form of the draw's weights, stated with the NumPy oracle alone."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from oracle import gpz_oracle as O
from test_predictor import catalogue, synth_model
from test_predictor_stack_noisy import with_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_draws_gamma_missing_dev": 17, "gpz_predictor_stack_missing_dev": 24}


def _model(d=3, m=6, k=1, method="VD"):
    model = gpz_amd.Model(m=m, d=d, k=k, method=method)
    p = m * d + model.g_dim + m * k + k + 2 * m * k
    model.sets["best"] = {"theta": np.zeros(p), "w": np.zeros((m, k)), "iSigma_w": np.stack([np.eye(m)] * k, axis=2)}
    return model


# ---- the refusals of the two Python entries ----------------------------------------------------------------------------------------------
def test_new_entries_validate_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of stack_missing_dev and of return_gamma with missing is raised on the host: the library load is
    made to fail, so a call that got past the checks would raise RuntimeError instead."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    e = np.linspace(0.0, 1.0, 11)
    p = gpz_amd.Predictor(_model())
    X = torch.zeros((4, 3), dtype=torch.float64)
    X[1, 2] = float("nan")
    # ---- stack_missing_dev
    with pytest.raises(TypeError, match="takes a torch tensor"):
        p.stack_missing_dev(np.zeros((4, 3)), e)
    with pytest.raises(TypeError, match="X must be a torch.Tensor"):
        p.stack_missing_dev([[0.0, 0.0, 0.0]] * 4, e)
    with pytest.raises(TypeError, match="X must be float64 or float32"):
        p.stack_missing_dev(X.long(), e)
    with pytest.raises(ValueError, match="X must be n x 3"):
        p.stack_missing_dev(torch.zeros((4, 2), dtype=torch.float64), e)
    with pytest.raises(TypeError, match="selection"):
        p.stack_missing_dev(X, e, selection=torch.ones(4))
    with pytest.raises(ValueError, match="selection"):
        p.stack_missing_dev(X, e, selection=torch.ones(3, dtype=torch.bool))
    for bad in (e[::-1], e[:1], np.array([0.0, np.nan, 1.0]), e.reshape(1, -1)):
        with pytest.raises(ValueError, match="edges"):
            p.stack_missing_dev(X, bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="n_draws"):
            p.stack_missing_dev(X, e, n_draws=bad)
    with pytest.raises(ValueError, match="over the limit"):
        p.stack_missing_dev(X, e, n_draws=gpz_amd.api.GPZ_DRAWS_MAX_COLUMNS)
    with pytest.raises(ValueError, match="seed"):
        p.stack_missing_dev(X, e, n_draws=2, seed=-1)
    with pytest.raises(ValueError, match="Z must be None"):
        p.stack_missing_dev(X, e, Z=np.zeros((6, 1, 1)))
    with pytest.raises(ValueError, match="Z must have shape"):
        p.stack_missing_dev(X, e, n_draws=2, Z=np.zeros((6, 3, 1)))
    for bad in (torch.zeros(4), torch.zeros(3, dtype=torch.int64), np.zeros(4, dtype=int), torch.zeros(4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="groups"):
            p.stack_missing_dev(X, e, groups=bad)
    for bad in (torch.zeros(3), torch.zeros(4, dtype=torch.int64), np.ones(4)):
        with pytest.raises(ValueError, match="weights"):
            p.stack_missing_dev(X, e, weights=bad)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="n_groups"):
            p.stack_missing_dev(X, e, n_groups=bad)
    with pytest.raises(ValueError, match="n_groups \\* bins"):
        p.stack_missing_dev(X, e, n_groups=gpz_amd.api.GPZ_STACK_MAX_GROUP_BINS)
    for ok in (X, X.float(), X.T.contiguous().T):
        with pytest.raises(ValueError, match="must be on cuda:0"):        # past every check of the call: the device, last
            p.stack_missing_dev(ok, e, n_draws=2, groups=torch.zeros(4, dtype=torch.int64), weights=torch.ones(4))
    with pytest.raises(TypeError, match="Psi"):                           # no Psi together with missing values, and no keyword for it
        p.stack_missing_dev(X, e, Psi=torch.ones((4, 3), dtype=torch.float64))
    with pytest.raises(TypeError, match="missing"):                       # stack_dev has no such keyword: the method is the entry
        p.stack_dev(X, e, missing=True)
    # ---- return_gamma
    with pytest.raises(ValueError, match="return_gamma=True needs Psi or missing=True, and not both"):
        p.draws_dev(X, 4, return_gamma=True)
    with pytest.raises(ValueError, match="return_gamma=True needs Psi or missing=True, and not both"):
        p.draws_dev(X, 4, Psi=torch.ones((4, 3), dtype=torch.float64), missing=True, return_gamma=True)
    with pytest.raises(ValueError, match="n_draws"):
        p.draws_dev(X, 0, missing=True, return_gamma=True)
    with pytest.raises(ValueError, match="X must be n x 3"):
        p.draws_dev(torch.zeros((4, 2), dtype=torch.float64), 4, missing=True, return_gamma=True)
    with pytest.raises(ValueError, match="must be on cuda:0"):
        p.draws_dev(X, 4, missing=True, return_gamma=True)
    with pytest.raises(ValueError, match="must be on cuda:0"):            # the call without the keyword is the call as it was
        p.draws_dev(X, 4, missing=True)
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.stack_missing_dev(X, e)
    # ---- models outside predict_missing_fits
    for kw, text in (({"m": 257}, "m <= 256, not m = 257"), ({"d": 21}, "d <= 20, not d = 21"), ({"k": 9}, "k <= 8, not k = 9"),
                     ({"method": "GC"}, "a diagonal kind .* not GC"), ({"method": "VC"}, "a diagonal kind .* not VC")):
        model = _model(**kw)
        q = gpz_amd.Predictor(model)
        Xd = torch.zeros((4, model.d), dtype=torch.float64)
        with pytest.raises(ValueError, match="stack_missing_dev.*predict_missing_fits.*" + text):
            q.stack_missing_dev(Xd, e)
        with pytest.raises(ValueError, match="predict_missing_fits.*" + text):
            q.draws_dev(Xd, 4, missing=True, return_gamma=True)
        with pytest.raises(ValueError, match="must be on cuda:0"):        # without missing values these models are as before
            q.stack_dev(Xd, e)
    bad = _model()
    bad.sets["best"]["priors"] = np.ones(5) / 5                           # m = 6
    with pytest.raises(ValueError, match="priors"):
        gpz_amd.Predictor(bad).stack_missing_dev(X, e)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_binding_library_and_build_agree_on_the_new_entries():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()

    def decl(name):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
        assert m, f"{name} is not declared in gpz_hip.h"
        return [a.strip() for a in m.group(1).split(",")]
    for name, nargs in ENTRIES.items():
        assert len(decl(name)) == nargs, (name, decl(name))
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    # the missing draws + Gam_d in front of the stream
    old, new = decl("gpz_predictor_draws_missing_dev"), decl("gpz_predictor_draws_gamma_missing_dev")
    assert new[:-2] == old[:-1] and new[-2] == "double *Gam_d" and new[-1] == old[-1] == "void *stream"
    so, sn = _lib.SYMBOLS["gpz_predictor_draws_missing_dev"][1], _lib.SYMBOLS["gpz_predictor_draws_gamma_missing_dev"][1]
    assert sn[:-2] == so[:-1] and sn[-2:] == [_lib.C.c_void_p, _lib.C.c_void_p]
    # the device stack + the priors and the mask behind the normalisation vectors, where the missing run has them behind muY
    old, new = decl("gpz_predictor_stack_dev"), decl("gpz_predictor_stack_missing_dev")
    assert new[:8] == old[:8] and new[8:10] == ["const double *priors", "uint32_t obs_mask"] and new[10:] == old[8:]
    so, sn = _lib.SYMBOLS["gpz_predictor_stack_dev"][1], _lib.SYMBOLS["gpz_predictor_stack_missing_dev"][1]
    assert sn[:8] == so[:8] and sn[8:10] == [_lib.c_double_p, _lib.C.c_uint32] and sn[10:] == so[8:]
    run = decl("gpz_predictor_run_missing_dev")
    assert run[9:11] == new[8:10]
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert re.search(r'UNITS="[^"]*\bk_predict_missing_gamma\b', build)
    kh = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert "int launch_predict_missing_gamma(" in kh and "size_t predict_missing_gamma_lds(int m, int d, bool psi);" in kh
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "p->mchunks, p->gpart, nt))" in host                          # the pair kernel's own chunk count: predict_missing_chunks(m)
    assert "; missing per draw: k_predict_missing_gamma (%d pair chunks)" in host


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


def gamma_lds_rule(m, d):
    """predict_missing_gamma_lds of k_predict_missing_gamma.hip and DESIGN.md section 19, stated a second time on purpose: the Pio block
    of 32 rows (row stride ceil16(m) + 2), [lnZ | c | 1 / C] of the 64 pairs of a group, the block's rows, (a, b) of the 64 pairs as 128
    ints; at least the 4 x 32 x 16 doubles of the last reduction, one column block at a time."""
    nk = (m + 15) // 16 * 16
    return 8 * max(32 * (nk + 2) + 64 * (1 + 2 * d) + 32 * d + 64, 4 * 32 * 16)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_missing_gamma_kernel_compiled_form(tmp_path):
    """k_predict_missing_gamma<NB>, NB = 1 .. 8 column blocks: no scratch, no spilled register, VGPRs + AGPRs <= 256 (two workgroups of
    256 per compute unit; the accumulators of 16 NB columns for two row halves among them), no static LDS (all of it is the dynamic
    block of predict_missing_gamma_lds), the f64 MFMA, no atomic of any kind and no other kernel in the unit."""
    src_path = os.path.join(CSRC, "k_predict_missing_gamma.hip")
    asm = tmp_path / "k_predict_missing_gamma.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src_path, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    assert len(recs) == 8 and all("k_predict_missing_gamma" in n for n in recs), sorted(recs)
    assert sorted(int(re.search(r"ILi(\d+)E", n).group(1)) for n in recs) == list(range(1, 9))
    for name, q in recs.items():
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
        assert q["LDS Size [bytes/block]"] == 0, (name, q)
    text = asm.read_text()
    assert "v_mfma_f64_16x16x4" in text
    for word in ("global_atomic", "flat_atomic", "ds_add_f", "ds_add_rtn_f", "cmpswap", "scratch_"):
        assert word not in text, word
    src = open(src_path).read()
    body = re.search(r"size_t predict_missing_gamma_lds\(int m, int d, bool psi\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert ": 32 * (nk + 2) + 64 * (1 + 2 * (size_t)d) + 32 * (size_t)d + 64;" in body and "red = 4 * 32 * 16" in body
    impl = open(os.path.join(CSRC, "k_predict_group_impl.h")).read()      # the helper that launches the four kernels
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in impl and "launch_predict_group<k_predict_missing_gamma<NBT>>" in src
    assert "nchunk != predict_missing_chunks(m)" in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "32 (nk + 2) + 64 (1 + 2 d) + 32 d + 64" in design
    # what the rule gives at the shapes section 19 names: the timing shape fits two workgroups per compute unit, the largest one
    assert gamma_lds_rule(100, 5) == 36_608 and 2 * gamma_lds_rule(100, 5) <= 160 * 1024
    assert gamma_lds_rule(256, 20) == 92_672 and gamma_lds_rule(256, 20) <= 160 * 1024
    assert gamma_lds_rule(1, 1) == 8 * 2048


# ---- the definition ------------------------------------------------------------------------------------------------------------------------
def test_gamma_per_draw_is_a_quadratic_form_of_the_draws_weights():
    """gamma_s + mu_s^2 = sum_{a >= b} f_ab EcC_ab w_s,a w_s,b is a quadratic form w_s' E w_s whose matrix E(x) does not depend on w.  The
    oracle does not expose the pair expectations, so E is recovered from ``O.predict_any`` through ``with_weights`` by polarisation
    (E_aa from w = e_a, E_ab from w = e_a + e_b), and the form under a draw's weights is compared with predict_any's gamma of the
    w := w_s model: the definition, fixed without any kernel.  Tiny model, three patterns; 1e-12 of the largest term for the sums of
    m (m + 1) / 2 products in another order."""
    m, d, k, n = 4, 3, 2, 12
    model = synth_model("VD", m, d, k, True, seed=19)
    model.sets["best"]["priors"] = np.random.default_rng(20).dirichlet(np.full(m, 2.0))
    X = catalogue(model, n, seed=21)
    X[0:4, 1] = np.nan
    X[4:8, 0] = X[4:8, 2] = np.nan
    X[8:10, :] = np.nan                                                    # rows 10, 11 stay complete
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
    rng = np.random.default_rng(22)
    for s in range(3):
        ws = model.sets["best"]["w"] + 0.3 * rng.standard_normal((m, k))
        out = O.predict_any(X, with_weights(model, ws))
        mu_s = out[0] - muY
        form = np.einsum("ao,noab,bo->no", ws, E, ws)
        # f_ab = 2 off the diagonal: the sum over a >= b of f_ab E_ab w_a w_b is the full symmetric form
        tri = sum((1.0 if a == b else 2.0) * E[:, :, a, b] * ws[a] * ws[b] for a in range(m) for b in range(a + 1))
        assert np.max(np.abs(tri - form)) <= 1e-12 * np.max(np.abs(form))
        gamma_s = tri - mu_s ** 2
        assert np.max(np.abs(gamma_s - out[4])) <= 1e-12 * np.max(np.abs(form)), s
        assert np.all(out[4][10:] == 0.0) and np.all(np.abs(gamma_s[10:]) <= 1e-12 * np.max(np.abs(form)))
        assert np.all(out[4][:10] > 0.0)
