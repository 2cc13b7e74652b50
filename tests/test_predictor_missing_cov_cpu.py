"""CPU-side checks of rows with missing inputs for the covariance kinds on the predictor handle (Predictor.predict_missing_cov_dev /
draws_missing_cov_dev, gpz_predictor_run_missing_cov_dev / _draws_missing_cov_dev of the C ABI): the entries are declared, bound,
exported and in the entry table, each with exactly its twin's arguments; k_predict_missing_cov.hip compiles for gfx950 with all 20
instantiations of the pair kernel inside the register file and without scratch or spills; the chunk rule and the slab rule are
functions of m and no alone; and the refusals of the two methods fire before the GPU is touched."""
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
SRC = os.path.join(CSRC, "k_predict_missing_cov.hip")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_run_missing_cov_dev": "gpz_predictor_run_missing_dev",
           "gpz_predictor_draws_missing_cov_dev": "gpz_predictor_draws_missing_dev"}
SLAB_BYTES = 64 << 20


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
    assert E["run", "missing_cov"] == "gpz_predictor_run_missing_cov_dev"
    assert E["draws", "missing_cov"] == "gpz_predictor_draws_missing_cov_dev"
    assert E["run", "missing"] == "gpz_predictor_run_missing_dev" and E["draws", "missing"] == "gpz_predictor_draws_missing_dev"
    assert "k_predict_missing_cov " in open(os.path.join(ROOT, "build.sh")).read()
    kh = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    for fn in ("predict_missing_cov_fits", "predict_missing_cov_chunks", "predict_missing_cov_slab_pairs", "launch_predict_missing_cov_pairs"):
        assert re.search(r"\b" + fn + r"\(", kh), fn


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_missing_cov_kernels_compiled_form(tmp_path):
    """The resource remarks only.  k_predict_missing_cov_pairs<NO, KM>: all of NO = 0 .. 9 x KM in {1, 8}, no scratch, no spill, VGPRs +
    AGPRs <= 256.  The Ex, PHI and dot kernels: no scratch, no spill.  The generation kernels run d x d temporaries through scratch
    memory on purpose (off the hot path): reported, not gated."""
    asm = tmp_path / "k_predict_missing_cov.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    pairs = {n: q for n, q in recs.items() if "k_predict_missing_cov_pairs" in n}
    assert len(pairs) == 20, sorted(pairs)
    seen = set()
    for name, q in pairs.items():
        no, km = (int(v) for v in re.search(r"ILi(\d+)ELi(\d+)E", name).groups())
        seen.add((no, km))
        assert q["ScratchSize [bytes/lane]"] == 0 and q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
        assert q["LDS Size [bytes/block]"] == 0, (name, q)                            # all of it dynamic: predict_missing_cov_lds
    assert seen == {(no, km) for no in range(10) for km in (1, 8)}
    for kname, count in (("k_pmcv_ex", 10), ("k_pmcv_phi", 10), ("k_pmcv_hd", 1), ("k_pmcv_coef", 1)):
        mine = {n: q for n, q in recs.items() if kname in n and "k_pmcv_phirec" not in n}
        assert len(mine) == count, (kname, sorted(mine))
        for name, q in mine.items():
            assert q["ScratchSize [bytes/lane]"] == 0 and q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
            assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
    for kname in ("k_pmc_triples", "k_pmcv_basis", "k_pmcv_phirec"):                  # reported, not gated
        (name, q), = [(n, q) for n, q in recs.items() if kname in n]
        print(f"{kname}: {q['VGPRs']} VGPRs, {q['ScratchSize [bytes/lane]']} bytes of scratch per lane")
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)


def chunks_rule(m):
    """predict_missing_cov_chunks of k_predict_missing_cov.hip, stated a second time on purpose: the largest power of two <= pairs / 32,
    between 1 and 16."""
    c = 1
    while c < 16 and 2 * c * 32 <= m * (m + 1) // 2:
        c *= 2
    return c


def rec_len(no):
    return 1 + no + no * (no + 1) // 2


def slabs_rule(m, no):
    """predict_missing_cov_slabs, stated a second time: the smallest power of two S such that ceil(pairs / S) pairs of m records of
    rec_len(no) doubles are at most 64 MB."""
    npair, s = m * (m + 1) // 2, 1
    while -(-npair // s) * m * rec_len(no) * 8 > SLAB_BYTES:
        s *= 2
    return s


def slab_pairs_rule(m, no):
    return -(-(m * (m + 1) // 2) // slabs_rule(m, no))


def test_chunks_and_slabs_are_functions_of_m_and_no_alone():
    src = open(SRC).read()
    body = re.search(r"int predict_missing_cov_chunks\(int m\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "while (c < 16 && 2L * c * 32 <= npair) c *= 2;" in body and "npair = (long)m * (m + 1) / 2" in body
    sbody = re.search(r"int predict_missing_cov_slabs\(int m, int no\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "while (((npair + s - 1) / s) * per > PMCV_SLAB_BYTES) s *= 2;" in sbody
    assert "per = (long)m * predict_missing_cov_rec(no) * (long)sizeof(double)" in sbody
    pbody = re.search(r"long predict_missing_cov_slab_pairs\(int m, int no\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "return (npair + s - 1) / s;" in pbody and "s = predict_missing_cov_slabs(m, no)" in pbody
    assert re.search(r"#define PMCV_SLAB_BYTES \(64L << 20\)", src)
    assert "int predict_missing_cov_rec(int no) { return 1 + no + no * (no + 1) / 2; }" in src
    for b in (body, sbody, pbody):
        for word in ("n", "ns", "nt", "tile", "rows", "d", "k"):
            assert not re.search(r"\b" + word + r"\b", b), word
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "p->mchunks = predict_missing_cov_chunks(p->m);" in host
    assert [m for m in range(2, 257) if chunks_rule(m) != chunks_rule(m - 1)] == [11, 16, 23, 32]
    assert [chunks_rule(m) for m in (1, 10, 11, 15, 16, 22, 23, 31, 32, 256)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [m for m in range(2, 257) if slabs_rule(m, 2) != slabs_rule(m - 1, 2)] == [141, 178, 224]
    assert slabs_rule(100, 4) == 1 and slab_pairs_rule(100, 4) == 5050                # 61 MB: the whole table is one slab
    assert slabs_rule(256, 9) == 64 and slab_pairs_rule(256, 9) == 514                # 3.7 GB in 64 slabs of 58 MB
    for m in (1, 7, 100, 141, 256):
        for no in range(10):
            assert slab_pairs_rule(m, no) * m * rec_len(no) * 8 <= SLAB_BYTES
            assert slabs_rule(m, no) * slab_pairs_rule(m, no) >= m * (m + 1) // 2


def test_refusals_fire_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of the two methods is raised on the host: the library load is made to fail, so a call that got past
    the checks would raise RuntimeError instead.  Each refusal says where such rows go.  Type, dtype, shape, model, device last."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    X = torch.zeros((4, 3), dtype=torch.float64)

    def calls(p):
        return {"predict": lambda x, **kw: p.predict_missing_cov_dev(x, **kw), "draws": lambda x, **kw: p.draws_missing_cov_dev(x, 4, **kw)}

    for method in ("VC", "GC"):
        for k in (1, 2):
            p = gpz_amd.Predictor(_model(k=k, method=method))
            for what, call in calls(p).items():
                with pytest.raises(TypeError, match="NumPy catalogue with missing values goes to Predictor.predict"):
                    call(np.zeros((4, 3)))
                with pytest.raises(TypeError, match="X must be a torch.Tensor"):
                    call([[0.0] * 3] * 4)
                for bad in (X.half(), X.long()):
                    with pytest.raises(TypeError, match="X must be float64 or float32"):
                        call(bad)
                with pytest.raises(ValueError, match="X must be n x 3"):
                    call(torch.zeros((4, 2), dtype=torch.float64))
                with pytest.raises(TypeError, match="selection must be a bool torch tensor"):
                    call(X, selection=np.ones(4, dtype=bool))
                for psi in (torch.ones((4, 3), dtype=torch.float64), np.ones((4, 3))):   # a Psi argument
                    with pytest.raises(ValueError, match=r"does not take Psi.*Predictor.predict\(X, Psi=Psi\)"):
                        call(X, Psi=psi)
                for ok in (X, X.float(), X.T.contiguous().T, X[::2]):
                    with pytest.raises(ValueError, match=r"must be on cuda:0.*Predictor.predict takes a catalogue"):   # the device, last
                        call(ok)
            with pytest.raises(ValueError, match="n_draws"):
                p.draws_missing_cov_dev(X, 0)
            p.close()
            with pytest.raises(RuntimeError, match="closed"):
                p.predict_missing_cov_dev(X)
    # a wrong device: the catalogue on the meta device is no CUDA tensor either
    p = gpz_amd.Predictor(_model(method="VC"), device=0)
    with pytest.raises(ValueError, match=r"must be on cuda:0.*Predictor.predict"):
        p.predict_missing_cov_dev(torch.zeros((4, 3), dtype=torch.float64, device="meta"))
    # a diagonal kind is sent to the missing keyword, and keeps refusing the covariance kinds there with the text it has
    for method in ("GL", "VL", "GD", "VD"):
        p = gpz_amd.Predictor(_model(method=method))
        with pytest.raises(ValueError, match=r"diagonal kind.*predict_dev\(X, missing=True\)"):
            p.predict_missing_cov_dev(X)
        with pytest.raises(ValueError, match=r"diagonal kind.*draws_dev\(X, missing=True\)"):
            p.draws_missing_cov_dev(X, 4)
    for method in ("GC", "VC"):
        p = gpz_amd.Predictor(_model(method=method))
        with pytest.raises(ValueError, match=r"predict_missing_fits: a diagonal kind.*Predictor.predict takes rows with missing values"):
            p.predict_dev(X, missing=True)
        with pytest.raises(ValueError, match=r"predict_missing_fits: a diagonal kind.*Predictor.predict takes rows with missing values"):
            p.draws_dev(X, 4, missing=True)
    # shapes outside predict_missing_cov_fits
    for kw in ({"d": 11}, {"k": 9}, {"m": 257}):
        model = _model(method="VC", **kw)
        p = gpz_amd.Predictor(model)
        Xd = torch.zeros((4, model.d), dtype=torch.float64)
        with pytest.raises(ValueError, match="predict_missing_cov_fits.*Predictor.predict"):
            p.predict_missing_cov_dev(Xd)
        with pytest.raises(ValueError, match="predict_missing_cov_fits.*Predictor.predict"):
            p.draws_missing_cov_dev(Xd, 4)
    # the edges of the scope pass the shape check (and then stop at the device)
    for kw in ({"m": 256}, {"d": 10}, {"d": 1}, {"k": 8}):
        model = _model(method="GC", **kw)
        p = gpz_amd.Predictor(model, force_tiles=True)                                    # (no route is refused)
        with pytest.raises(ValueError, match="must be on cuda:0"):
            p.draws_missing_cov_dev(torch.zeros((4, model.d), dtype=torch.float64), 4)
    # priors of the wrong length
    model = _model(method="VC")
    model.sets["best"]["priors"] = np.ones(5) / 5
    with pytest.raises(ValueError, match="priors of the set must be 6 values"):
        gpz_amd.Predictor(model).predict_missing_cov_dev(X)
