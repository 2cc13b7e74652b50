"""CPU-side checks of the stacks of rows with input noise and of gamma under every weight draw (Predictor.stack_noisy / stack_noisy_dev /
draws_dev(..., Psi=, return_gamma=True); gpz_predictor_stack_noisy / _stack_noisy_dev / _draws_gamma_noisy_dev): every refusal of the
three Python entries before the library is loaded, the declarations against the binding, the chunk rule of k_predict_noisy_gamma, the
compiled form of the two new units, and the per-draw-width reference ``stack_reference_w`` that the GPU tests
(test_predictor_stack_noisy.py) take from here."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from scipy.special import ndtr

import gpz_amd
from gpz_amd import _lib
from test_predictor_stack_cpu import stack_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_stack_noisy": 17, "gpz_predictor_stack_noisy_dev": 27, "gpz_predictor_draws_gamma_noisy_dev": 20}


def stack_reference_w(mu0, s2_0, F, S2, edges, groups, weights, n_groups=None):
    """stack_reference with a width per (column, row): mu0, s2_0 (n, k) for column 0; F, S2 (S, n, k) the draws and their widths^2 (or
    None).  Built on stack_reference: one call per draw column with that column's width in the place of beta, column 1 of it taken."""
    h0, sw, m0, q0 = stack_reference(mu0, s2_0, None, s2_0, edges, groups, weights, n_groups=n_groups)
    S = 0 if F is None else len(F)
    hist, sum_mu, sum_mu2 = [h0[0]], [m0[0]], [q0[0]]
    for s in range(S):
        h, _, m1, q1 = stack_reference(mu0, s2_0, np.asarray(F)[s:s + 1], np.asarray(S2)[s], edges, groups, weights, n_groups=n_groups)
        hist.append(h[1]); sum_mu.append(m1[1]); sum_mu2.append(q1[1])
    return np.stack(hist), sw, np.stack(sum_mu), np.stack(sum_mu2)


def test_reference_with_a_width_per_draw_closed_form():
    """Three rows, two draw columns with their own widths: every bin against the normal CDF written out."""
    mu = np.array([[0.0], [1.0], [5.0]])
    s2 = np.array([[4.0], [1.0], [0.25]])
    F = np.stack([mu + 0.5, mu - 0.25])
    S2 = np.stack([np.array([[1.0], [9.0], [0.04]]), np.array([[0.01], [2.25], [16.0]])])
    e = np.array([-1.0, 0.0, 1.0, 2.0, 6.0])
    g = np.array([0, 1, 0])
    w = np.array([1.0, 2.0, 0.5])
    h, sw, sm, sm2 = stack_reference_w(mu, s2, F, S2, e, g, w, n_groups=2)
    assert h.shape == (3, 2, 1, 4) and np.array_equal(sw, [1.5, 2.0])
    for c in range(3):
        m_c = mu if c == 0 else F[c - 1]
        v_c = s2 if c == 0 else S2[c - 1]
        for gi in range(2):
            want = sum(w[i] * np.diff(ndtr((e - m_c[i, 0]) / np.sqrt(v_c[i, 0]))) for i in range(3) if g[i] == gi)
            assert np.allclose(h[c, gi, 0], want, rtol=0, atol=4e-16), (c, gi)
            assert sm[c, gi, 0] == sum(w[i] * m_c[i, 0] for i in range(3) if g[i] == gi)
            assert abs(sm2[c, gi, 0] - sum(w[i] * m_c[i, 0] ** 2 for i in range(3) if g[i] == gi)) <= 1e-15
    # a draw column whose widths equal beta is stack_reference's own column
    h2 = stack_reference(mu, s2, F[:1], S2[0], e, g, w, n_groups=2)[0]
    assert np.array_equal(h[:2], h2)


def test_header_binding_and_library_agree_on_the_new_entries():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    args = {}
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
        assert m, f"{name} is not declared in gpz_hip.h"
        args[name] = [a.strip() for a in m.group(1).split(",")]
        assert len(args[name]) == nargs, (name, args[name])
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported by the built library"

    def decl(name):
        return [a.strip() for a in re.search(r"\bint " + name + r"\(([^;]*)\);", h).group(1).split(",")]
    psi4 = ["const void *Psi_d", "int32_t psi_type", "int64_t psi_row_stride", "int64_t psi_col_stride"]
    # the host stack + Psi behind ns, as gpz_predictor_draws_noisy takes it
    old, new = decl("gpz_predictor_stack"), args["gpz_predictor_stack_noisy"]
    assert new[:3] == old[:3] and new[3] == "const double *Psi" and new[4:] == old[3:]
    # the device stack + Psi's pointer, type and strides behind X's, sd2 behind sdX
    old, new = decl("gpz_predictor_stack_dev"), args["gpz_predictor_stack_noisy_dev"]
    assert new[:6] == old[:6] and new[6:10] == psi4 and new[10:12] == old[6:8] and new[12] == "const double *sd2" and new[13:] == old[8:]
    # the noisy device draws + Gam_d in front of the stream
    old, new = decl("gpz_predictor_draws_noisy_dev"), args["gpz_predictor_draws_gamma_noisy_dev"]
    assert new[:-2] == old[:-1] and new[-2] == "double *Gam_d" and new[-1] == old[-1] == "void *stream"
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert " k_predict_stack_w " in build and " k_predict_noisy_gamma " in build


def gamma_chunks_rule(m):
    """predict_gamma_chunks of k_predict_noisy_gamma.hip, stated a second time on purpose: one chunk per 4096 pairs (rounded up), at most 4
    - the model's shape only."""
    return min(4, max(1, -(-(m * (m + 1) // 2) // 4096)))


def test_gamma_pair_chunks_are_a_function_of_the_model_shape():
    h = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert re.search(r"\bint predict_gamma_chunks\(int m\);", h)
    src = open(os.path.join(CSRC, "k_predict_noisy_gamma.hip")).read()
    body = re.search(r"int predict_gamma_chunks\(int m\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "const long c = ((long)m * (m + 1) / 2 + 4095) / 4096;" in body and "(c > 4 ? 4 : c)" in body
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "p->gchunks = predict_gamma_chunks(p->m);" in host
    changes = [m for m in range(2, 257) if gamma_chunks_rule(m) != gamma_chunks_rule(m - 1)]
    assert changes == [91, 128, 157]                                    # the values documented beside the C function
    assert "it changes at m = 91, 128, 157" in src
    assert [gamma_chunks_rule(m) for m in (1, 7, 17, 50, 90, 91, 127, 128, 156, 157, 250, 256)] == [1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 4]


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


def _compile(unit, tmp_path):
    asm = tmp_path / (unit + ".s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, unit + ".hip"), "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    return _resource_records(r.stderr), asm.read_text()


ATOMIC_WORDS = ("atomic_add_f", "atomic_pk_add", "atomic_fadd", "atomic_fmin", "atomic_fmax", "ds_add_f", "ds_add_rtn_f", "cmpswap", "scratch_")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_gamma_kernels_compiled_form(tmp_path):
    """k_predict_noisy_gamma<d>, d = 1 .. 20: the f64 MFMA in the loop, no scratch and no spill, VGPRs + AGPRs <= 256 (the accumulators
    of 128 columns among them), the LDS stage of 32 records of 1 + 2 d doubles; the two finish kernels; no floating-point atomic and no
    compare-and-swap loop in the unit."""
    recs, text = _compile("k_predict_noisy_gamma", tmp_path)
    for name, q in recs.items():
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
    hot = {n: q for n, q in recs.items() if "k_predict_noisy_gamma" in n}
    assert sorted(int(re.search(r"ILi(\d+)E", n).group(1)) for n in hot) == list(range(1, 21))
    for name, q in hot.items():
        d = int(re.search(r"ILi(\d+)E", name).group(1))
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
        assert q["LDS Size [bytes/block]"] == 32 * (1 + 2 * d) * 8, (name, q)
    assert len(recs) == 22 and any("k_gamma_finish_dev" in n for n in recs) and any("k_gamma_finish_s2" in n for n in recs)
    assert "v_mfma_f64_16x16x4" in text and "v_rsq_f64" in text
    for word in ATOMIC_WORDS + ("global_atomic", "flat_atomic"):
        assert word not in text, word


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_stack_w_kernel_compiled_form(tmp_path):
    """k_predict_stack_w.hip: exactly one kernel, k_stack_tile_w, within k_stack_tile's budget (DESIGN.md sections 14 and 18): at most 128
    vector registers, no scratch, no static LDS, no atomics."""
    recs, text = _compile("k_predict_stack_w", tmp_path)
    assert len(recs) == 1 and "k_stack_tile_w" in next(iter(recs)), sorted(recs)
    for name, q in recs.items():
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 128, (name, q)
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["LDS Size [bytes/block]"] == 0, (name, q)
    for word in ("global_atomic_add_f64", "cmpswap", "flat_atomic", "global_atomic", "ds_add_f64", "ds_add_rtn_f64", "scratch_"):
        assert word not in text, word


def _model(d=3, m=6, k=1, method="VD"):
    model = gpz_amd.Model(m=m, d=d, k=k, method=method)
    p = m * d + model.g_dim + m * k + k + 2 * m * k
    model.sets["best"] = {"theta": np.zeros(p), "w": np.zeros((m, k)), "iSigma_w": np.stack([np.eye(m)] * k, axis=2)}
    return model


def test_new_entries_validate_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of stack_noisy, stack_noisy_dev and return_gamma is raised on the host: the library load is made to
    fail, so a call that got past the checks would raise RuntimeError instead."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    e = np.linspace(0.0, 1.0, 11)
    p = gpz_amd.Predictor(_model())
    X = torch.zeros((4, 3), dtype=torch.float64)
    good = torch.ones((4, 3), dtype=torch.float64)
    Xh, Ph = np.zeros((4, 3)), np.ones((4, 3))
    # ---- stack_noisy (host arrays)
    with pytest.raises(ValueError, match="cube"):
        p.stack_noisy(Xh, np.ones((3, 3, 4)), e)
    for shape in ((5, 3), (4, 2), (3,)):
        with pytest.raises(ValueError, match="Psi must be"):
            p.stack_noisy(Xh, np.ones(shape), e)
    with pytest.raises(ValueError, match="X must be n x 3"):
        p.stack_noisy(np.zeros((4, 2)), Ph, e)
    for bad in (np.nan, np.inf, -1e-300):
        psi = Ph.copy()
        psi[2, 1] = bad
        with pytest.raises(ValueError, match="Psi must be finite"):
            p.stack_noisy(Xh, psi, e)
    with pytest.raises(ValueError, match="needs Psi"):
        p.stack_noisy(Xh, None, e)
    with pytest.raises(ValueError, match="edges"):
        p.stack_noisy(Xh, Ph, e[::-1])
    with pytest.raises(ValueError, match="n_draws"):
        p.stack_noisy(Xh, Ph, e, n_draws=-1)
    with pytest.raises(ValueError, match="groups"):
        p.stack_noisy(Xh, Ph, e, groups=np.zeros(3, dtype=int))
    with pytest.raises(ValueError, match="weights"):
        p.stack_noisy(Xh, Ph, e, weights=-np.ones(4))
    with pytest.raises(ValueError, match="missing values"):
        p.stack_noisy(np.full((4, 3), np.nan), Ph, e)
    for ok in (Ph, Ph[:, :1], Ph[:, 0]):
        with pytest.raises(RuntimeError, match="disabled"):              # past every check: the first GPU call
            p.stack_noisy(Xh, ok, e, n_draws=2)
    # ---- stack_noisy_dev (torch tensors)
    with pytest.raises(TypeError, match="Predictor.stack_noisy"):        # NumPy handed to _dev
        p.stack_noisy_dev(Xh, good, e)
    with pytest.raises(TypeError, match="Predictor.stack_noisy"):
        p.stack_noisy_dev(X, Ph, e)
    with pytest.raises(TypeError, match="Psi must be a torch.Tensor"):
        p.stack_noisy_dev(X, [[1.0, 1.0, 1.0]] * 4, e)
    for bad in (good.half(), good.long()):
        with pytest.raises(TypeError, match="Psi must be float64 or float32"):
            p.stack_noisy_dev(X, bad, e)
    with pytest.raises(TypeError, match="X must be float64 or float32"):
        p.stack_noisy_dev(X.long(), good, e)
    for shape in ((5, 3), (4, 2), (4, 3, 1), (3,), (3, 4)):
        with pytest.raises(ValueError, match="Psi must be n x d"):
            p.stack_noisy_dev(X, torch.ones(shape, dtype=torch.float64), e)
    with pytest.raises(ValueError, match="needs Psi"):
        p.stack_noisy_dev(X, None, e)
    with pytest.raises(ValueError, match="groups"):
        p.stack_noisy_dev(X, good, e, groups=torch.zeros(4))
    with pytest.raises(ValueError, match="weights"):
        p.stack_noisy_dev(X, good, e, weights=torch.zeros(3))
    for ok in (good, good.float(), good[:, :1], good[:, 0], good.T.contiguous().T):
        with pytest.raises(ValueError, match="must be on cuda:0"):        # past the checks of Psi: the device, last
            p.stack_noisy_dev(X, ok, e, n_draws=2)
    # ---- return_gamma
    with pytest.raises(ValueError, match="return_gamma=True needs Psi"):
        p.draws_dev(X, 4, return_gamma=True)
    with pytest.raises(ValueError, match="return_gamma=True needs Psi"):
        p.draws_dev(X, 4, Psi=good, missing=True, return_gamma=True)
    with pytest.raises(TypeError, match="Predictor.draws"):
        p.draws_dev(X, 4, Psi=Ph, return_gamma=True)
    with pytest.raises(ValueError, match="Psi must be n x d"):
        p.draws_dev(X, 4, Psi=torch.ones((4, 2), dtype=torch.float64), return_gamma=True)
    with pytest.raises(ValueError, match="must be on cuda:0"):
        p.draws_dev(X, 4, Psi=good, return_gamma=True)
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.stack_noisy(Xh, Ph, e)
    # ---- models outside predict_noisy_fits: a covariance kind, d = 21, k = 9, m = 257; and the forced tile route
    for kw in ({"method": "VC"}, {"method": "GC"}, {"d": 21}, {"k": 9}, {"m": 257}):
        model = _model(**kw)
        d = model.d
        p = gpz_amd.Predictor(model)
        Xd, Pd = torch.zeros((4, d), dtype=torch.float64), torch.ones((4, d), dtype=torch.float64)
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.stack_noisy(np.zeros((4, d)), np.ones((4, d)), e)
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.stack_noisy_dev(Xd, Pd, e)
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.draws_dev(Xd, 4, Psi=Pd, return_gamma=True)
        with pytest.raises(ValueError, match="must be on cuda:0"):        # without Psi these models are as before
            p.stack_dev(Xd, e)
    p = gpz_amd.Predictor(_model(), force_tiles=True)
    with pytest.raises(ValueError, match="force_tiles"):
        p.stack_noisy(Xh, Ph, e)
    with pytest.raises(ValueError, match="force_tiles"):
        p.stack_noisy_dev(X, good, e)
    with pytest.raises(ValueError, match="force_tiles"):
        p.draws_dev(X, 4, Psi=good, return_gamma=True)
