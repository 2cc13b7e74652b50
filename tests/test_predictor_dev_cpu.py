"""CPU-side checks of the device-resident predictor entries (Predictor.predict_dev / draws_dev / stack_dev, gpz_predictor_*_dev of the C
ABI): the entries are declared, bound and exported; k_predict_dev.hip compiles for gfx950 without scratch, spills or floating-point
atomics and with the LDS tile of the transposing stage kernel; and the argument checks fire before the GPU is touched."""
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
SRC = os.path.join(ROOT, "gpz_amd", "csrc", "k_predict_dev.hip")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_run_dev": 16, "gpz_predictor_draws_dev": 14, "gpz_predictor_stack_dev": 22}
KERNELS = ("k_pred_check_dev", "k_pred_stage", "k_pred_finish_dev", "k_pred_phi_dev", "k_draws_finish_dev")


def test_header_binding_and_library_agree_on_the_device_entries():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
        assert m, f"{name} is not declared in gpz_hip.h"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert m.group(1).lstrip().startswith("gpz_predictor *p, const void *X_d, int32_t x_type, int64_t ns, int64_t row_stride, "
                                              "int64_t col_stride,"), name
        assert m.group(1).rstrip().endswith("void *stream"), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert re.search(r"#define GPZ_X_F64 0\b", h) and re.search(r"#define GPZ_X_F32 1\b", h)
    assert "k_predict_dev" in open(os.path.join(ROOT, "build.sh")).read()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_dev_kernels_compiled_form(tmp_path):
    """Bandwidth kernels: no scratch, no spilled register, no floating-point atomic (the only atomic is the integer OR of the check
    kernel's record), and the stage kernel holds the LDS tile it transposes row-major input through."""
    asm = tmp_path / "k_predict_dev.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "gpz_amd", "csrc"), "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=900)
    recs, cur = {}, None
    for l in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = m.group(1)
            recs[cur] = {}
            continue
        m = re.search(r"(VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", l)
        if m and cur:
            recs[cur][m.group(1)] = int(m.group(2))
    for kname in KERNELS:
        assert any(kname in n for n in recs), (kname, sorted(recs))
    assert sum("k_pred_stage" in n for n in recs) == 2, sorted(recs)   # f64 and f32 rows
    for name, q in recs.items():
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        if "k_pred_stage" in name:
            assert 0 < q["LDS Size [bytes/block]"] <= 64 * 1024, (name, q)
        else:
            assert q["LDS Size [bytes/block]"] == 0, (name, q)
    text = asm.read_text()
    assert "ds_write_b64" in text or "ds_store_b64" in text or "ds_write2" in text       # the tile is written ...
    for word in ("atomic_add_f", "atomic_pk_add", "atomic_fadd", "atomic_fmin", "atomic_fmax", "atomic_min_f", "atomic_max_f",
                 "ds_add_f", "ds_add_rtn_f", "cmpswap", "scratch_"):
        assert word not in text, word
    # the normalisation is a correctly rounded f64 division, not a reciprocal multiply
    for word in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64"):
        assert word in text, word


def _model(d=3, m=6, k=1):
    model = gpz_amd.Model(m=m, d=d, k=k, method="VD")
    p = m * d + model.g_dim + m * k + k + 2 * m * k
    model.sets["best"] = {"theta": np.zeros(p), "w": np.zeros((m, k)), "iSigma_w": np.stack([np.eye(m)] * k, axis=2)}
    return model


def test_dev_methods_validate_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of the *_dev methods is raised on the host: the library load is made to fail, so a call that got
    past the checks would raise RuntimeError instead.  Type, dtype, shapes and the scalar arguments come first and the device check
    last, so all of them can be shown with CPU tensors on a machine without a GPU."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    e = np.linspace(0.0, 1.0, 11)
    for k in (1, 2):
        p = gpz_amd.Predictor(_model(k=k))
        X = torch.zeros((4, 3), dtype=torch.float64)
        calls = {"predict": lambda x, **kw: p.predict_dev(x, **kw), "draws": lambda x, **kw: p.draws_dev(x, 4, **kw),
                 "stack": lambda x, **kw: p.stack_dev(x, e, **kw)}
        for what, call in calls.items():
            with pytest.raises(TypeError, match=f"Predictor.{what}"):                 # a NumPy array: pointed at the host method
                call(np.zeros((4, 3)))
            with pytest.raises(TypeError, match="torch.Tensor"):
                call([[0.0, 0.0, 0.0]])
            with pytest.raises(ValueError, match="must be on cuda:0"):                # a CPU tensor
                call(X)
            with pytest.raises(ValueError, match="must be on cuda:0"):
                call(X.float())
            with pytest.raises(TypeError, match="float64 or float32"):
                call(X.half())
            with pytest.raises(TypeError, match="float64 or float32"):
                call(X.long())
            with pytest.raises(ValueError, match="X must be n x 3"):                  # wrong d
                call(torch.zeros((4, 2), dtype=torch.float64))
            with pytest.raises(ValueError, match="X must be n x 3"):
                call(torch.zeros(4, dtype=torch.float64))
            with pytest.raises(ValueError, match="selection"):
                call(X, selection=torch.ones(5, dtype=torch.bool))
            with pytest.raises(TypeError, match="selection"):
                call(X, selection=np.ones(4, dtype=bool))
        for bad in (0, -1, 2.5, True, None):
            with pytest.raises(ValueError, match="n_draws"):
                p.draws_dev(X, bad)
        with pytest.raises(ValueError, match="limit"):
            p.draws_dev(X, 16384 // k + 1)
        for bad in (-1, 2 ** 64, 1.5, True):
            with pytest.raises(ValueError, match="seed"):
                p.draws_dev(X, 4, seed=bad)
        with pytest.raises(ValueError, match="Z must"):
            p.draws_dev(X, 4, Z=np.zeros((6, 5, k)))
        for bad in ([0.0], 1.0, np.zeros((2, 3)), [0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, 1.0, np.inf]):
            with pytest.raises(ValueError, match="edges"):
                p.stack_dev(X, bad)
        for bad in (-1, 2.5, True):
            with pytest.raises(ValueError, match="n_draws"):
                p.stack_dev(X, e, n_draws=bad)
        with pytest.raises(ValueError, match="limit"):
            p.stack_dev(X, e, n_draws=16384 // k)
        with pytest.raises(ValueError, match="Z must"):
            p.stack_dev(X, e, n_draws=0, Z=np.zeros((6, 4, k)))
        for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros(4), np.zeros(4, dtype=int), torch.zeros((4, 1), dtype=torch.int32)):
            with pytest.raises(ValueError, match="groups"):
                p.stack_dev(X, e, groups=bad)
        for bad in (torch.ones(5), torch.ones(4, dtype=torch.int32), np.ones(4)):
            with pytest.raises(ValueError, match="weights"):
                p.stack_dev(X, e, weights=bad)
        for bad in (0, -3, 1.5, True):
            with pytest.raises(ValueError, match="n_groups"):
                p.stack_dev(X, e, n_groups=bad)
        with pytest.raises(ValueError, match="limit of 4096"):
            p.stack_dev(X, e, n_groups=410)
        with pytest.raises(ValueError, match="must be on cuda:0"):                    # past every other check: the device check
            p.stack_dev(X, e, n_draws=4, seed=2 ** 64 - 1, Z=np.zeros((6, 4, k)), groups=torch.tensor([0, -1, 2, 1]), n_groups=4,
                        weights=torch.tensor([0.0, 1.0, 2.0, 0.5]), selection=torch.tensor([True, True, False, True]))
        p.close()
        for call in (lambda: p.predict_dev(X), lambda: p.draws_dev(X, 2), lambda: p.stack_dev(X, e)):
            with pytest.raises(RuntimeError, match="closed"):
                call()
