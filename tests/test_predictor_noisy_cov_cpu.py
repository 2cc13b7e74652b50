"""CPU-side checks of input noise for the covariance kinds on the predictor handle (Predictor.predict_noisy_cov_dev / draws_noisy_cov_dev,
gpz_predictor_run_noisy_cov_dev / _draws_noisy_cov_dev of the C ABI): the entries are declared, bound, exported and in the entry table;
k_predict_noisy_cov.hip compiles for gfx950 without scratch or spills and every instantiation keeps room for two workgroups per compute
unit; the chunks are a function of the model's shape; and the refusals of the two methods fire before the GPU is touched."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from test_predictor_noisy_cpu import _model, _resource_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
SRC = os.path.join(CSRC, "k_predict_noisy_cov.hip")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_run_noisy_cov_dev": "gpz_predictor_run_noisy_dev", "gpz_predictor_draws_noisy_cov_dev": "gpz_predictor_draws_noisy_dev"}


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
    assert E["run", "noisy_cov"] == "gpz_predictor_run_noisy_cov_dev" and E["draws", "noisy_cov"] == "gpz_predictor_draws_noisy_cov_dev"
    assert E["run", "noisy"] == "gpz_predictor_run_noisy_dev" and E["draws", "noisy"] == "gpz_predictor_draws_noisy_dev"
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert "k_predict_noisy_cov " in build and "$SRC/k_predict_ncov_impl.h" in build   # the unit and the header that holds its kernels' bodies


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_noisy_cov_kernels_compiled_form(tmp_path):
    """Every kernel of the unit: no scratch, no spilled register.  The tile kernel: d = 1 .. 10 x {GC, VC} x {1, 8} outputs in registers,
    each holding its LDS stage of 32 records; every KM = 1 instantiation within 256 registers, two workgroups of 256 per compute unit.
    No atomic anywhere: every sum runs in one fixed order."""
    asm = tmp_path / "k_predict_noisy_cov.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    for kname in ("k_predict_noisy_cov_small", "k_predict_noisy_cov_phi", "k_noisy_cov_records"):
        assert any(kname in n for n in recs), (kname, sorted(recs))
    for name, q in recs.items():
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
    small = {n: q for n, q in recs.items() if "k_predict_noisy_cov_small" in n}
    assert len(small) == 40, sorted(small)
    seen = set()
    for name, q in small.items():
        d, shared, km = (int(v) for v in re.search(r"ILi(\d+)ELb(\d)ELi(\d+)E", name).groups())
        seen.add((d, shared, km))
        assert q["LDS Size [bytes/block]"] == 32 * (1 + d + d * (d + 1) // 2 + 3 * km) * 8, (name, q)
        if km == 1:
            assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
    assert seen == {(d, s, km) for d in range(1, 11) for s in (0, 1) for km in (1, 8)}
    phi = {n: q for n, q in recs.items() if "k_predict_noisy_cov_phi" in n}
    assert len(phi) == 20, sorted(phi)
    for name, q in phi.items():
        d = int(re.search(r"ILi(\d+)ELb", name).group(1))
        assert q["LDS Size [bytes/block]"] == 32 * (1 + d + d * (d + 1) // 2) * 8, (name, q)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
    text = asm.read_text()
    for word in ("atomic_add_f", "atomic_pk_add", "atomic_fadd", "atomic_fmin", "atomic_fmax", "ds_add_f", "ds_add_rtn_f", "cmpswap",
                 "scratch_"):
        assert word not in text, word


def cov_chunks_rule(m, d, k):
    """predict_noisy_cov_chunks of k_predict_noisy_cov.hip, stated a second time on purpose: one chunk per 2048 pairs, at most 4 - the
    model's shape only."""
    return min(4, max(1, (m * (m + 1) // 2) // 2048))


def test_chunks_are_a_function_of_the_model_shape():
    h = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert re.search(r"\bint predict_noisy_cov_chunks\(int m, int d, int k\);", h)
    body = re.search(r"int predict_noisy_cov_chunks\(int m, int d, int k\) \{(.*?)\n\}", open(SRC).read(), flags=re.S).group(1)
    assert "const long c = ((long)m * (m + 1) / 2) / 2048;" in body and "(c > 4 ? 4 : c)" in body
    for word in ("n", "ns", "nt", "tile", "rows"):
        assert not re.search(r"\b" + word + r"\b", body), word
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "predict_noisy_cov_chunks(p->m, p->d, p->k)" in host
    changes = [m for m in range(2, 257) if cov_chunks_rule(m, 3, 1) != cov_chunks_rule(m - 1, 3, 1)]
    assert changes == [91, 111, 128]
    assert [cov_chunks_rule(m, 5, 8) for m in (1, 90, 91, 110, 111, 127, 128, 256)] == [1, 1, 2, 2, 3, 3, 4, 4]


def test_refusals_fire_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of the two methods is raised on the host: the library load is made to fail, so a call that got past
    the checks would raise RuntimeError instead.  Each refusal says where such rows go."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    X = torch.zeros((4, 3), dtype=torch.float64)
    good = torch.ones((4, 3), dtype=torch.float64)

    def calls(p):
        return {"predict": lambda x, psi, **kw: p.predict_noisy_cov_dev(x, psi, **kw),
                "draws": lambda x, psi, **kw: p.draws_noisy_cov_dev(x, psi, 4, **kw)}

    for method in ("VC", "GC"):
        for k in (1, 2):
            p = gpz_amd.Predictor(_model(k=k, method=method))
            for what, call in calls(p).items():
                with pytest.raises(ValueError, match=f"needs Psi.*{what}_dev\\(X\\)"):
                    call(X, None)
                for cube in (torch.ones((3, 3, 4), dtype=torch.float64), np.ones((3, 3, 4))):
                    with pytest.raises(ValueError, match=r"full d x d x n Psi stays on Predictor.predict"):
                        call(X, cube)
                with pytest.raises(TypeError, match=f"Predictor.{what}"):                 # a NumPy Psi: pointed at the host method
                    call(X, np.ones((4, 3)))
                for bad in (good.half(), good.long()):
                    with pytest.raises(TypeError, match="Psi must be float64 or float32"):
                        call(X, bad)
                for shape in ((5, 3), (4, 2), (3,), (3, 4)):
                    with pytest.raises(ValueError, match="Psi must be n x d"):
                        call(X, torch.ones(shape, dtype=torch.float64))
                with pytest.raises(ValueError, match="X must be n x 3"):                  # X's own checks come first
                    call(torch.zeros((4, 2), dtype=torch.float64), good)
                for ok in (good, good.float(), good[:, :1], good[:, 0], good.T.contiguous().T):
                    with pytest.raises(ValueError, match="must be on cuda:0"):            # past the checks: the device, last
                        call(X, ok)
            with pytest.raises(ValueError, match="n_draws"):
                p.draws_noisy_cov_dev(X, good, 0)
            p.close()
            with pytest.raises(RuntimeError, match="closed"):
                p.predict_noisy_cov_dev(X, good)
    # a diagonal kind is sent to the Psi keyword
    for method in ("GL", "VL", "GD", "VD"):
        p = gpz_amd.Predictor(_model(method=method))
        with pytest.raises(ValueError, match=r"diagonal kind.*predict_dev\(X, Psi=Psi\)"):
            p.predict_noisy_cov_dev(X, good)
        with pytest.raises(ValueError, match=r"diagonal kind.*draws_dev\(X, Psi=Psi\)"):
            p.draws_noisy_cov_dev(X, good, 4)
    # shapes outside predict_noisy_cov_fits
    for kw in ({"m": 300}, {"d": 12}, {"d": 11}, {"k": 9}):
        model = _model(method="VC", **kw)
        d = model.d
        p = gpz_amd.Predictor(model)
        Xd, Pd = torch.zeros((4, d), dtype=torch.float64), torch.ones((4, d), dtype=torch.float64)
        with pytest.raises(ValueError, match="predict_noisy_cov_fits.*Predictor.predict"):
            p.predict_noisy_cov_dev(Xd, Pd)
        with pytest.raises(ValueError, match="predict_noisy_cov_fits.*Predictor.predict"):
            p.draws_noisy_cov_dev(Xd, Pd, 4)
    # the edges of the scope pass the shape check (and then stop at the device)
    for kw in ({"m": 256}, {"d": 10}, {"d": 1}, {"k": 8}):
        model = _model(method="GC", **kw)
        d = model.d
        p = gpz_amd.Predictor(model, force_tiles=True)                                    # (no route is refused)
        with pytest.raises(ValueError, match="must be on cuda:0"):
            p.draws_noisy_cov_dev(torch.zeros((4, d), dtype=torch.float64), torch.ones((4, d), dtype=torch.float64), 4)
