"""CPU-side checks of rows with both input noise and missing inputs on the predictor handle (Predictor.predict_noisy_missing_dev /
draws_noisy_missing_dev, gpz_predictor_run_noisy_missing_dev / _draws_noisy_missing_dev of the C ABI): the methods refuse in order before
the GPU is touched and the old spelling keeps its refusal; the entries are declared, bound and exported; k_predict_noisy_missing.hip
compiles for gfx950 without scratch or spills, its pair kernel within 256 registers and the LDS DESIGN.md section 22 states; and the
calls the methods make on the library, recorded behind the stand-in of test_predictor_calls_cpu.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
import test_predictor_calls_cpu as calls
from test_predictor_calls_cpu import CODES, D, N, SEL, rig, run, _rows   # noqa: F401  (rig is a fixture)
from test_predictor_missing_cpu import _model, _resource_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
SRC = os.path.join(CSRC, "k_predict_noisy_missing.hip")
LAUNCH = os.path.join(CSRC, "k_predict_missing.hip")               # the pair launcher and the LDS rule, with and without Psi
IMPL = os.path.join(CSRC, "k_predict_group_impl.h")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_run_noisy_missing_dev": ("gpz_predictor_run_noisy_dev", 22),
           "gpz_predictor_draws_noisy_missing_dev": ("gpz_predictor_draws_noisy_dev", 21)}
# k_pnm_no sits beside k_pmd_no in k_predict_missing.hip (one body), k_pnm_check_psi became k_pred_check_psi with a mask (k_predict_noisy.hip):
# test_predictor_missing_cpu.py and test_predictor_noisy_cpu.py hold them
KERNELS = ("k_pnm_records", "k_predict_noisy_missing_pairs")

# where include/gpz_hip.h puts the arguments of the two entries (the stand-in checks the vectors behind the pointers there)
calls.POS.setdefault("gpz_predictor_run_noisy_missing_dev",
                     dict(rows=3, muX=10, sdX=11, sd2=12, muY=13, priors=14, mask=15, out=16, stream=21))
calls.POS.setdefault("gpz_predictor_draws_noisy_missing_dev",
                     dict(rows=3, muX=10, sdX=11, sd2=12, muY=13, priors=14, mask=15, n_draws=16, seed=17, out=19, stream=20))


# ---- the methods' refusals ---------------------------------------------------------------------------------------------------------------
def test_methods_validate_in_order_before_the_gpu(monkeypatch):
    """The library load is made to fail, so a call that got past the checks would raise RuntimeError instead of ValueError.  Two things
    wrong at once: the text of the first.  Order: X and Psi by type, dtype and shape; the model's shape; the priors; the device."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    p = gpz_amd.Predictor(_model())
    X = torch.zeros((4, 3), dtype=torch.float64)
    X[1, 2] = float("nan")
    Psi = torch.ones((4, 3), dtype=torch.float64)
    big, cov = gpz_amd.Predictor(_model(m=257)), gpz_amd.Predictor(_model(method="GC"))
    bad = _model(m=257)
    bad.sets["best"]["priors"] = np.ones(5) / 5
    both = gpz_amd.Predictor(bad)                                          # outside the shapes AND the wrong number of priors
    pri = _model()
    pri.sets["best"]["priors"] = np.ones(5) / 5                           # m = 6
    pp = gpz_amd.Predictor(pri)
    for name, call in (("predict", lambda q, x, psi, **kw: q.predict_noisy_missing_dev(x, psi, **kw)),
                       ("draws", lambda q, x, psi, **kw: q.draws_noisy_missing_dev(x, psi, 4, **kw))):
        with pytest.raises(TypeError, match=f"{name}_dev takes a torch tensor"):             # 1. X, then Psi
            call(big, X.numpy(), Psi.numpy())
        with pytest.raises(TypeError, match="X must be float64 or float32"):
            call(big, X.to(torch.float16), Psi[:, :2])
        with pytest.raises(ValueError, match="X must be n x 3"):
            call(big, X[:, :2], Psi[:, :2])
        with pytest.raises(TypeError, match="selection must be a bool torch tensor"):
            call(big, X, Psi[:, :2], selection=torch.ones(4))
        with pytest.raises(ValueError, match="needs Psi"):
            call(big, X, None)
        with pytest.raises(TypeError, match="takes Psi as a torch tensor"):
            call(big, X, Psi.numpy())
        with pytest.raises(TypeError, match="Psi must be float64 or float32"):
            call(big, X, Psi.to(torch.int64))
        with pytest.raises(ValueError, match=r"Psi must be n x d, n x 1 or n \(n = 4, d = 3\), got shape \(4, 2\)"):
            call(big, X, Psi[:, :2])
        with pytest.raises(ValueError, match=r"Psi must be n x d, n x 1 or n \(n = 4, d = 3\), got shape \(3, 1\)"):
            call(big, X, Psi[:3, 0])
        for q, text in ((big, "m <= 256, not m = 257"), (cov, "a diagonal kind .* not GC"), (both, "m <= 256, not m = 257"),   # 2. the model
                        (gpz_amd.Predictor(_model(d=21)), "d <= 20, not d = 21"), (gpz_amd.Predictor(_model(k=9)), "k <= 8, not k = 9"),
                        (gpz_amd.Predictor(_model(method="VC")), "a diagonal kind .* not VC")):
            d = q._d
            with pytest.raises(ValueError, match=f"{name}_noisy_missing_dev needs a model inside predict_missing_fits.*"
                                                 + text):
                call(q, torch.zeros((4, d), dtype=torch.float64), torch.ones((4, d), dtype=torch.float64))
        with pytest.raises(ValueError, match="the priors of the set must be 6 values, got 5"):   # 3. the priors
            call(pp, X, Psi)
        for psi in (Psi, Psi[:, :1], Psi[:, 0], Psi.float()):                                    # 4. the device, last
            with pytest.raises(ValueError, match="X must be on cuda:0"):
                call(p, X, psi)
        with pytest.raises(ValueError, match="X must be on cuda:0"):
            call(p, X.float(), Psi, selection=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="n_draws must be a positive integer"):
        p.draws_noisy_missing_dev(X, Psi, 0)
    with pytest.raises(ValueError, match="needs the fused draws route"):
        gpz_amd.Predictor(_model(), force_tiles=True).draws_noisy_missing_dev(X, Psi, 4)
    with pytest.raises(ValueError, match="X must be on cuda:0"):          # the moments do not need that route
        gpz_amd.Predictor(_model(), force_tiles=True).predict_noisy_missing_dev(X, Psi)
    # the old spelling keeps its refusal and now names the methods
    for spell in (lambda **kw: p.predict_dev(X, **kw), lambda **kw: p.draws_dev(X, 4, **kw)):
        with pytest.raises(ValueError, match="missing=True does not take Psi.*predict_noisy_missing_dev / draws_noisy_missing_dev"):
            spell(missing=True, Psi=Psi)
    with pytest.raises(ValueError, match="return_gamma=True needs Psi or missing=True, and not both"):
        p.draws_dev(X, 4, missing=True, Psi=Psi, return_gamma=True)
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.predict_noisy_missing_dev(X, Psi)
    with pytest.raises(RuntimeError, match="closed"):
        p.draws_noisy_missing_dev(X, Psi, 4)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_entries():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name, (base, nargs) in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
        assert m, f"{name} is not declared in gpz_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        old = [a.strip() for a in re.search(r"\bint " + base + r"\(([^;]*)\);", h).group(1).split(",")]
        assert len(args) == nargs == len(old) + 2
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        # the noisy entry's arguments with the priors and the mask behind muY
        assert args[:14] == old[:14] and args[13] == "const double *muY"
        assert args[14:16] == ["const double *priors", "uint32_t obs_mask"]
        assert args[16:] == old[14:] and args[-1] == "void *stream"
        types, told = _lib.SYMBOLS[name][1], _lib.SYMBOLS[base][1]
        assert types[:14] == told[:14] and types[14:16] == [_lib.c_double_p, _lib.C.c_uint32] and types[16:] == told[14:]
        assert calls.POS[name]["priors"] == 14 and calls.POS[name]["mask"] == 15 and calls.POS[name]["stream"] == nargs - 1
    full = open(HEADER).read()
    assert "noisy missing: k_predict_noisy_missing_pairs (C pair chunks)" in full
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert re.search(r'UNITS="[^"]*\bk_predict_noisy_missing\b', build)
    kh = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert re.search(r"\bint launch_predict_missing_pairs\(hipStream_t st, const double \*Xc, const double \*Psic,", kh)
    assert re.search(r"\bsize_t predict_missing_lds\(int m, int d, int k, bool psi\);", kh)


# ---- the compiled form ---------------------------------------------------------------------------------------------------------------------
def lds_rule(m, d, k):
    """predict_missing_lds with psi (k_predict_missing.hip) and DESIGN.md section 22, stated a second time on purpose: the Pio block
    of 32 rows (row stride ceil16(m) + 2), the 64 records of a pair group, the block's rows of X and of Psi; at least the 4 x 32 x 3 KM
    doubles of the last reduction (KM = 1 for one output, else 8)."""
    nk = (m + 15) // 16 * 16
    return 8 * max(32 * (nk + 2) + 64 * (1 + 2 * d + 3 * k) + 64 * d, 4 * 32 * 3 * (1 if k == 1 else 8))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_kernels_compiled_form(tmp_path):
    """Every kernel of the unit: no scratch, no spilled register.  The pair kernel: two instantiations (1 or 8 outputs in registers), at
    most 256 vector registers, no static LDS (all of it is the dynamic block of predict_missing_lds), the f64 MFMA, no
    floating-point atomic."""
    asm = tmp_path / "k_predict_noisy_missing.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    for kname in KERNELS:
        assert any(kname in n for n in recs), (kname, sorted(recs))
    for name, q in recs.items():
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
    pairs = {n: q for n, q in recs.items() if "k_predict_noisy_missing_pairs" in n}
    assert sorted(int(re.search(r"ILi(\d+)E", n).group(1)) for n in pairs) == [1, 8]
    for name, q in pairs.items():
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)           # two workgroups of 256 per compute unit
        assert q["LDS Size [bytes/block]"] == 0, (name, q)
    src = open(LAUNCH).read()
    body = re.search(r"size_t predict_missing_lds\(int m, int d, int k, bool psi\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "psi ? 32 * (nk + 2) + 64 * (size_t)predict_missing_rec(d, k) + 64 * (size_t)d\n" in body and "red = 4 * 32 * 3 * km" in body
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in open(IMPL).read()
    assert "launch_predict_group<k_predict_noisy_missing_pairs<" in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "32 (nk + 2) + 64 (1 + 2 d + 3 k) + 64 d" in design
    # the benchmark shape fits two workgroups per compute unit, the largest shape one (opted in above 64 KB)
    assert lds_rule(100, 5, 1) == 38_912 and 2 * lds_rule(100, 5, 1) <= 160 * 1024
    assert lds_rule(256, 20, 8) == 109_568 and lds_rule(256, 20, 8) <= 160 * 1024
    assert lds_rule(1, 1, 8) == 8 * 3072
    text = asm.read_text()
    assert "v_mfma_f64_16x16x4" in text
    for word in ("atomic_add_f", "atomic_pk_add", "atomic_fadd", "atomic_fmin", "atomic_fmax", "ds_add_f", "ds_add_rtn_f", "cmpswap",
                 "scratch_"):
        assert word not in text, word


# ---- the calls the methods make ------------------------------------------------------------------------------------------------------------
def test_methods_reach_their_entries(rig):
    """Complete rows reach the _noisy_dev entries; every other group the new entry once, in ascending code order (0, 4, 6, 7), with the
    mask 7 & ~code; the stand-in checks the priors, sd2 and the other vectors at the header's positions and the binding's types."""
    p, rec, lookups = rig
    Xc, Xn = torch.from_numpy(_rows([0] * N)), torch.from_numpy(_rows())
    Psi, sel = (0.01 * torch.arange(1, N + 1, dtype=torch.float64))[:, None].repeat(1, D), torch.from_numpy(SEL)   # told apart by value
    seen = []
    orig = p._psi_args

    def psi_args(P, n):
        seen.append(P[:, 0].tolist())
        return orig(P, n)
    p._psi_args = psi_args
    out = p.predict_noisy_missing_dev(Xn, Psi)
    assert rec.take() == [run("gpz_predictor_run_noisy_dev", 3), run("gpz_predictor_run_noisy_missing_dev", 3, mask=3),
                          run("gpz_predictor_run_noisy_missing_dev", 2, mask=1), run("gpz_predictor_run_noisy_missing_dev", 2, mask=0)]
    assert out[0].data_ptr() not in rec.out[-4:]                           # every group has results of its own, scattered back
    want = [[i for i, c in enumerate(CODES) if c == code] for code in (0, 4, 6, 7)]
    assert seen == [Psi[idx, 0].tolist() for idx in want]                  # the gathered Psi of each group, in its rows' order
    del seen[:]
    p.predict_noisy_missing_dev(Xn, Psi[:, 1], selection=sel)              # one variance per row; codes 0, 4, 0, 6, 4, 7 stay
    assert rec.take() == [run("gpz_predictor_run_noisy_dev", 2), run("gpz_predictor_run_noisy_missing_dev", 2, mask=3),
                          run("gpz_predictor_run_noisy_missing_dev", 1, mask=1), run("gpz_predictor_run_noisy_missing_dev", 1, mask=0)]
    assert len(lookups) == 2                                               # one stream lookup per Python call, however many groups
    nd = dict(n_draws=3, seed=5)
    F = p.draws_noisy_missing_dev(Xn, Psi, 3, seed=5)
    assert rec.take() == [run("gpz_predictor_draws_noisy_dev", 3, **nd), run("gpz_predictor_draws_noisy_missing_dev", 3, mask=3, **nd),
                          run("gpz_predictor_draws_noisy_missing_dev", 2, mask=1, **nd),
                          run("gpz_predictor_draws_noisy_missing_dev", 2, mask=0, **nd)]
    assert F.data_ptr() not in rec.out[-4:] and tuple(F.shape) == (3, N, p._k)
    # one pattern: the whole call, on the caller's own result tensors
    out = p.predict_noisy_missing_dev(Xc, Psi)
    assert rec.take() == [run("gpz_predictor_run_noisy_dev", 10)] and rec.out[-1] == out[0].data_ptr()
    out = p.predict_noisy_missing_dev(torch.from_numpy(_rows([4] * N)), Psi.float())
    assert rec.take() == [run("gpz_predictor_run_noisy_missing_dev", 10, mask=3)] and rec.out[-1] == out[0].data_ptr()
    F = p.draws_noisy_missing_dev(torch.from_numpy(_rows([7] * N)), Psi[:, :1], 3, seed=5)
    assert rec.take() == [run("gpz_predictor_draws_noisy_missing_dev", 10, mask=0, **nd)] and rec.out[-1] == F.data_ptr()
    # no rows: no entry
    none = torch.zeros(N, dtype=torch.bool)
    assert tuple(p.predict_noisy_missing_dev(Xn, Psi, selection=none)[0].shape) == (0, p._k)
    assert tuple(p.draws_noisy_missing_dev(Xn, Psi, 3, selection=none).shape) == (3, 0, p._k)
    assert rec.take() == [] and rec.created == 1
