"""CPU-side checks of input noise on the predictor handle (Predictor.predict_dev / draws_dev / draws with Psi=, gpz_predictor_run_noisy_dev /
_draws_noisy_dev / _draws_noisy of the C ABI): the entries are declared, bound and exported; k_predict_noisy.hip compiles for gfx950
without scratch or spills and its draws kernels keep room for two workgroups per compute unit; the pair chunks are a function of the
model's shape; and the argument checks of the new keyword fire before the GPU is touched."""
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
SRC = os.path.join(CSRC, "k_predict_noisy.hip")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_run_noisy_dev": 20, "gpz_predictor_draws_noisy_dev": 19, "gpz_predictor_draws_noisy": 8}
KERNELS = ("k_predict_noisy_small", "k_predict_noisy_finish", "k_noisy_pair_coef", "k_predict_draws_psi", "k_pred_check_psi",
           "k_pred_stage_psi", "k_pred_finish_noisy_dev")
WIDTHS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20)


def test_header_binding_and_library_agree_on_the_noisy_entries():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
        assert m, f"{name} is not declared in gpz_hip.h"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    # the device entries: gpz_predictor_run_dev's / _draws_dev's arguments + Psi after the X strides + sd2 after sdX (and no PHI)
    for name, base, drop in (("gpz_predictor_run_noisy_dev", "gpz_predictor_run_dev", 1),
                             ("gpz_predictor_draws_noisy_dev", "gpz_predictor_draws_dev", 0)):
        args = [a.strip() for a in re.search(r"\bint " + name + r"\(([^;]*)\);", h).group(1).split(",")]
        old = [a.strip() for a in re.search(r"\bint " + base + r"\(([^;]*)\);", h).group(1).split(",")]
        assert len(args) == len(old) + 5 - drop
        assert args[:6] == old[:6]
        assert args[6:10] == ["const void *Psi_d", "int32_t psi_type", "int64_t psi_row_stride", "int64_t psi_col_stride"]
        assert args[10:12] == old[6:8] and args[12] == "const double *sd2"
        assert not any("PHI" in a for a in args) and args[-1] == "void *stream"
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert "k_predict_noisy" in build and "k_predict_draws_impl.h" in build


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


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_noisy_kernels_compiled_form(tmp_path):
    """Every kernel of the unit: no scratch, no spilled register.  The draws-with-Psi kernels: one per instantiated width, at most 256
    vector registers and 80 KB of LDS (static + the dynamic block of predict_draws_psi_lds), the bounds of the noise-free draws.  The
    hot kernel holds its LDS stage of pair records, adds no atomic and touches no scratch."""
    asm = tmp_path / "k_predict_noisy.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    for kname in KERNELS:
        assert any(kname in n for n in recs), (kname, sorted(recs))
    for name, q in recs.items():
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
    draws = {n: q for n, q in recs.items() if "k_predict_draws_psi" in n}
    assert len(draws) == 11, sorted(draws)
    lda = int(re.search(r"#define PS_LDA (\d+)", open(os.path.join(CSRC, "k_predict_draws_impl.h")).read()).group(1))
    assert lda == 262
    assert "return ((size_t)32 * PS_LDA + 2 * 32 * (size_t)de) * sizeof(double); }" in open(SRC).read()
    seen = set()
    for name, q in draws.items():
        d = int(re.search(r"ILi(\d+)E", name).group(1))
        seen.add(d)
        dynamic = (32 * lda + 2 * 32 * d) * 8                         # predict_draws_psi_lds(d)
        assert q["LDS Size [bytes/block]"] + dynamic <= 80 * 1024, (name, q, dynamic)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
    assert seen == set(WIDTHS)
    small = {n: q for n, q in recs.items() if "k_predict_noisy_small" in n}
    assert len(small) == 40, sorted(small)                            # d = 1 .. 20 x {1, 8} outputs in registers
    for name, q in small.items():
        d, km = (int(v) for v in re.search(r"ILi(\d+)ELi(\d+)E", name).groups())
        assert q["LDS Size [bytes/block]"] == 32 * (1 + 2 * d + 3 * km) * 8, (name, q)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)       # two workgroups of 256 per compute unit
    text = asm.read_text()
    for word in ("atomic_add_f", "atomic_pk_add", "atomic_fadd", "atomic_fmin", "atomic_fmax", "ds_add_f", "ds_add_rtn_f", "cmpswap",
                 "scratch_"):
        assert word not in text, word
    for word in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64"):   # Psi / sd2 is a correctly rounded f64 division
        assert word in text, word


def chunks_rule(m, d, k):
    """predict_noisy_chunks of k_predict_noisy.hip, stated a second time on purpose: one chunk per 2048 pairs, at most 4 - the model's
    shape only."""
    return min(4, max(1, (m * (m + 1) // 2) // 2048))


def test_pair_chunks_are_a_function_of_the_model_shape():
    h = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert re.search(r"\bint predict_noisy_chunks\(int m, int d, int k\);", h)
    src = open(SRC).read()
    body = re.search(r"int predict_noisy_chunks\(int m, int d, int k\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "const long c = ((long)m * (m + 1) / 2) / 2048;" in body and "(c > 4 ? 4 : c)" in body
    for word in ("ns", "nt", "tile", "rows"):
        assert not re.search(r"\b" + word + r"\b", body), word
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "predict_noisy_chunks(p->m, p->d, p->k)" in host
    # where the rule changes: the m the GPU edge test takes on each side
    changes = [m for m in range(2, 257) if chunks_rule(m, 5, 1) != chunks_rule(m - 1, 5, 1)]
    assert changes == [91, 111, 128]
    assert [chunks_rule(m, 5, 1) for m in (1, 90, 91, 110, 111, 127, 128, 256)] == [1, 1, 2, 2, 3, 3, 4, 4]


def _model(d=3, m=6, k=1, method="VD"):
    model = gpz_amd.Model(m=m, d=d, k=k, method=method)
    p = m * d + model.g_dim + m * k + k + 2 * m * k
    model.sets["best"] = {"theta": np.zeros(p), "w": np.zeros((m, k)), "iSigma_w": np.stack([np.eye(m)] * k, axis=2)}
    return model


def test_psi_keyword_validates_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of the Psi keyword is raised on the host: the library load is made to fail, so a call that got past
    the checks would raise RuntimeError instead.  Type, dtype, shape, return_phi and the model's shape come first, the device last."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    for k in (1, 2):
        p = gpz_amd.Predictor(_model(k=k))
        X = torch.zeros((4, 3), dtype=torch.float64)
        good = torch.ones((4, 3), dtype=torch.float64)
        calls = {"predict": lambda x, **kw: p.predict_dev(x, **kw), "draws": lambda x, **kw: p.draws_dev(x, 4, **kw)}
        for what, call in calls.items():
            with pytest.raises(TypeError, match=f"Predictor.{what}"):                 # a NumPy Psi: pointed at the host method
                call(X, Psi=np.ones((4, 3)))
            with pytest.raises(TypeError, match="Psi must be a torch.Tensor"):
                call(X, Psi=[[1.0, 1.0, 1.0]] * 4)
            for bad in (good.half(), good.long()):
                with pytest.raises(TypeError, match="Psi must be float64 or float32"):
                    call(X, Psi=bad)
            for shape in ((5, 3), (4, 2), (4, 3, 1), (3,), (3, 4)):
                with pytest.raises(ValueError, match="Psi must be n x d"):
                    call(X, Psi=torch.ones(shape, dtype=torch.float64))
            for ok in (good, good.float(), good[:, :1], good[:, 0], good.T.contiguous().T):
                with pytest.raises(ValueError, match="must be on cuda:0"):            # past the checks of Psi: the device, last
                    call(X, Psi=ok)
            with pytest.raises(ValueError, match="X must be n x 3"):                  # X's own checks come before Psi's
                call(torch.zeros((4, 2), dtype=torch.float64), Psi=np.ones((4, 3)))
        with pytest.raises(ValueError, match="return_phi"):
            p.predict_dev(X, return_phi=True, Psi=good)
        # the host draws: Psi as predict takes it
        Xh = np.zeros((4, 3))
        for shape in ((5, 3), (4, 2), (2, 2, 4)):
            with pytest.raises(ValueError, match="Psi must be"):
                p.draws(Xh, 4, Psi=np.ones(shape))
        for bad in (np.nan, np.inf, -1e-300):
            psi = np.ones((4, 3))
            psi[2, 1] = bad
            with pytest.raises(ValueError, match="Psi must be finite"):
                p.draws(Xh, 4, Psi=psi)
        with pytest.raises(ValueError, match="n_draws"):
            p.draws(Xh, 0, Psi=np.ones((4, 3)))
        with pytest.raises(RuntimeError, match="disabled"):                           # past every check: the first GPU call
            p.draws(Xh, 4, Psi=np.ones((4, 1)))
        p.close()
        with pytest.raises(RuntimeError, match="closed"):
            p.predict_dev(X, Psi=good)
    # models outside predict_noisy_fits: m = 300, d = 24, k = 9, a covariance kind; and the forced tile route for the draws
    X = torch.zeros((4, 3), dtype=torch.float64)
    for kw in ({"m": 300}, {"d": 24}, {"k": 9}, {"method": "VC"}, {"method": "GC"}):
        model = _model(**kw)
        d = model.d
        p = gpz_amd.Predictor(model)
        Xd, Pd = torch.zeros((4, d), dtype=torch.float64), torch.ones((4, d), dtype=torch.float64)
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.predict_dev(Xd, Psi=Pd)
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.draws_dev(Xd, 4, Psi=Pd)
        with pytest.raises(ValueError, match="predict_noisy_fits"):
            p.draws(np.zeros((4, d)), 4, Psi=np.ones((4, d)))
        with pytest.raises(ValueError, match="must be on cuda:0"):                    # without Psi these models are as before
            p.predict_dev(Xd)
    p = gpz_amd.Predictor(_model(), force_tiles=True)
    with pytest.raises(ValueError, match="force_tiles"):
        p.draws_dev(X, 4, Psi=torch.ones((4, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="force_tiles"):
        p.draws(np.zeros((4, 3)), 4, Psi=np.ones((4, 3)))
    # stack and stack_dev still have no Psi
    p = gpz_amd.Predictor(_model())
    e = np.linspace(0.0, 1.0, 11)
    with pytest.raises(TypeError, match="Psi"):
        p.stack(np.zeros((4, 3)), e, Psi=np.ones((4, 3)))
    with pytest.raises(TypeError, match="Psi"):
        p.stack_dev(X, e, Psi=torch.ones((4, 3), dtype=torch.float64))
