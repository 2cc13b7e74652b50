"""CPU-side checks of the stacked n(z) and gamma under every weight draw for rows with input noise on a covariance kind
(Predictor.stack_noisy_cov_dev / draws_noisy_cov_dev(..., return_gamma=True), gpz_predictor_stack_noisy_cov_dev /
_draws_gamma_noisy_cov_dev of the C ABI): the entries are declared with their twins' arguments, bound, exported and in the entry table;
k_predict_noisy_cov_gamma.hip compiles for gfx950 to 20 instantiations without scratch, spills or floating-point atomics inside the
register bounds of DESIGN.md section 27; and the refusals of the two Python spellings fire before the GPU is touched."""
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
SRC = os.path.join(CSRC, "k_predict_noisy_cov_gamma.hip")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_stack_noisy_cov_dev": "gpz_predictor_stack_noisy_dev",
           "gpz_predictor_draws_gamma_noisy_cov_dev": "gpz_predictor_draws_gamma_noisy_dev"}


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
    assert E["draws_gamma", "noisy_cov"] == "gpz_predictor_draws_gamma_noisy_cov_dev"
    assert E["stack", "noisy_cov"] == "gpz_predictor_stack_noisy_cov_dev"
    assert E["draws_gamma", "noisy"] == "gpz_predictor_draws_gamma_noisy_dev" and E["stack", "noisy"] == "gpz_predictor_stack_noisy_dev"
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert " k_predict_noisy_cov_gamma " in build and "k_ncov_density.h" in build


def test_the_density_is_shared_and_the_chunks_are_the_existing_function():
    """Both units take ncov_factor / ncov_density from one header and define neither (the tile kernels through the bodies of
    k_predict_ncov_impl.h, the gamma kernel through the one policy GammaNcov, each with PsiDiag, which is where ncov_factor is called);
    the gamma unit has no chunk rule of its own and the host takes this kind's chunks from predict_gamma_chunks."""
    head = open(os.path.join(CSRC, "k_ncov_density.h")).read()
    assert len(re.findall(r"__device__[^;{]*\bncov_factor\s*\(", head)) == 1 and len(re.findall(r"__device__[^;{]*\bncov_density\s*\(", head)) == 1
    diag = re.search(r"struct PsiDiag \{.*?\n\};", head, flags=re.S).group(0)
    assert "ncov_factor<DD>(S, ps, M, rd, prd)" in diag and "W = DD;" in diag
    for unit in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, unit)).read()
        if unit != "k_ncov_density.h":
            assert not re.search(r"__device__[^;{]*\bncov_(factor|density)\s*\(", text), unit   # no second definition
            if re.match(r"k_predict_(noisy_cov|psi_cube|ncov_impl)", unit):                       # these reach it through PsiDiag alone
                assert "ncov_factor<" not in re.sub(r"//.*", "", text), unit
    impl = open(os.path.join(CSRC, "k_predict_ncov_impl.h")).read()
    assert re.search(r'#include\s+"k_ncov_density\.h"', impl)
    tile = re.sub(r"//.*", "", open(os.path.join(CSRC, "k_predict_noisy_cov.hip")).read())
    assert '#include "k_predict_ncov_impl.h"' in tile
    assert "predict_ncov_small_body<PsiDiag<D>, SHARED, KM>(a)" in tile and "predict_ncov_phi_body<PsiDiag<D>, SHARED>(a)" in tile
    code = re.sub(r"//.*", "", open(SRC).read())
    assert re.search(r'#include\s+"k_ncov_density\.h"', code)
    assert "predict_gamma_body<GammaNcov<PsiDiag<D>, SHARED, ncg_blocks(D)>>(a)" in code
    assert "__launch_bounds__(256, D == 9 ? 2 : 1) void k_predict_noisy_cov_gamma(" in code
    assert "predict_gamma_chunks" not in code and not re.search(r"\bint\s+\w*chunks\s*\(", code)
    host = re.sub(r"//.*", "", open(os.path.join(CSRC, "gpz_predictor.hip")).read())
    prep = re.search(r"int rows_gamma_prepare\(.*?\n\}", host, flags=re.S).group(0)
    assert re.search(r"r\.ncov\(\)[^;]*gchunks\s*=\s*predict_gamma_chunks\(p->m\)", prep)
    assert re.search(r"bool ncov\(\) const \{ return kind == ROWS_NOISY_COV \|\|", open(os.path.join(CSRC, "gpz_predictor.h")).read())
    form = re.search(r"static NcovForm ncov_form\(.*?\n\}", host, flags=re.S).group(0)
    assert re.search(r"return \{p->Psic, launch_predict_noisy_cov_small, launch_predict_noisy_cov_phi, launch_predict_noisy_cov_gamma, "
                     r"\"noisy_cov\"\}", form)
    tile = re.search(r"int rows_gamma_tile\(.*?\n\}", host, flags=re.S).group(0)
    assert re.search(r"\bf\.gamma\([^;]*f\.Psi\[s\][^;]*p->gchunks[^;]*p->gpart", tile, flags=re.S)
    assert '"%s: k_predict_%s_gamma launch failed", who, f.name' in tile


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_gamma_kernel_compiled_form(tmp_path):
    """k_predict_noisy_cov_gamma<D, SHARED>, D = 1 .. 10 x {GC, VC}: the f64 MFMA in the loop, no scratch and no spill; VGPRs + AGPRs <=
    256 for D <= 8 (two workgroups of 256 per compute unit) and <= 512 above; the static LDS stage of 32 record heads of 1 + D +
    D (D + 1) / 2 doubles; at least 4 accumulator blocks (64 columns) per pass at every D; no floating-point atomic and no
    compare-and-swap loop in the unit."""
    asm = tmp_path / "k_predict_noisy_cov_gamma.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    assert len(recs) == 20 and all("k_predict_noisy_cov_gamma" in n for n in recs), sorted(recs)
    seen = set()
    for name, q in recs.items():
        d, shared = (int(v) for v in re.search(r"ILi(\d+)ELb(\d)E", name).groups())
        seen.add((d, shared))
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert q["LDS Size [bytes/block]"] == 32 * (1 + d + d * (d + 1) // 2) * 8, (name, q)
        regs = q["VGPRs"] + q.get("AGPRs", 0)
        print(f"d {d} {'GC' if shared else 'VC'}: {q['VGPRs']} + {q.get('AGPRs', 0)} registers")
        assert regs <= (256 if d <= 8 else 512), (name, q)
    assert seen == {(d, s) for d in range(1, 11) for s in (0, 1)}
    text = asm.read_text()
    assert "v_mfma_f64_16x16x4" in text and "v_rsq_f64" in text
    for word in ("atomic_add_f", "atomic_pk_add", "atomic_fadd", "atomic_fmin", "atomic_fmax", "ds_add_f", "ds_add_rtn_f", "cmpswap",
                 "scratch_", "global_atomic", "flat_atomic"):
        assert word not in text, word
    # the blocks per pass, from the compiled kernels: the K loop is not unrolled and holds one MFMA per 16-column block of accumulators
    per = {}
    for part in re.split(r"\t\.type\t(?=_Z\d+k_predict_noisy_cov_gamma)", text)[1:]:
        name = part.split(",", 1)[0]
        body = part.split("\t.size\t" + name, 1)[0]
        d, shared = (int(v) for v in re.search(r"ILi(\d+)ELb(\d)E", name).groups())
        per[d, shared] = body.count("v_mfma_f64_16x16x4")
    assert set(per) == seen, sorted(per)
    print("MFMAs (= 16-column blocks per pass) per kernel:", sorted(per.items()))
    assert all(n >= 4 for n in per.values()), per                       # at least 64 columns per pass at every D
    assert all(per[d, 0] == per[d, 1] for d in range(1, 11)), per       # a function of D alone


def test_refusals_fire_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of draws_noisy_cov_dev(..., return_gamma=True) and stack_noisy_cov_dev is raised on the host: the
    library load is made to fail, so a call that got past the checks would raise RuntimeError instead.  Each refusal says where such
    rows go, and the old spellings keep theirs."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    e = np.linspace(0.0, 1.0, 11)
    X = torch.zeros((4, 3), dtype=torch.float64)
    good = torch.ones((4, 3), dtype=torch.float64)

    def calls(p):
        return {"draws": lambda x, psi, **kw: p.draws_noisy_cov_dev(x, psi, 4, return_gamma=True, **kw),
                "stack": lambda x, psi, **kw: p.stack_noisy_cov_dev(x, psi, e, n_draws=2, **kw)}

    for method in ("VC", "GC"):
        for k in (1, 2):
            p = gpz_amd.Predictor(_model(k=k, method=method))
            for what, call in calls(p).items():
                with pytest.raises(ValueError, match=f"{what}_noisy_cov_dev needs Psi.*{what}_dev\\(X"):
                    call(X, None)
                for cube in (torch.ones((3, 3, 4), dtype=torch.float64), np.ones((3, 3, 4))):
                    with pytest.raises(ValueError, match=r"full d x d x n Psi stays on Predictor.predict"):
                        call(X, cube)
                with pytest.raises(TypeError, match="Predictor.draws" if what == "draws" else r"Predictor.predict\(X, Psi=Psi\)"):
                    call(X, np.ones((4, 3)))                                              # a NumPy Psi: pointed at a host method
                with pytest.raises(TypeError, match="Psi must be a torch.Tensor"):
                    call(X, [[1.0, 1.0, 1.0]] * 4)
                with pytest.raises(TypeError, match=f"Predictor.{what}"):                 # a NumPy X
                    call(np.zeros((4, 3)), good)
                for bad in (good.half(), good.long()):
                    with pytest.raises(TypeError, match="Psi must be float64 or float32"):
                        call(X, bad)
                with pytest.raises(TypeError, match="X must be float64 or float32"):
                    call(X.long(), good)
                for shape in ((5, 3), (4, 2), (3,), (3, 4)):
                    with pytest.raises(ValueError, match="Psi must be n x d"):
                        call(X, torch.ones(shape, dtype=torch.float64))
                with pytest.raises(ValueError, match="X must be n x 3"):                  # X's own checks come first
                    call(torch.zeros((4, 2), dtype=torch.float64), good)
                with pytest.raises(TypeError, match="selection must be a bool"):
                    call(X, good, selection=torch.zeros(4))
                with pytest.raises(ValueError, match="selection must be a mask of length 4"):
                    call(X, good, selection=torch.zeros(3, dtype=torch.bool))
                for ok in (good, good.float(), good[:, :1], good[:, 0], good.T.contiguous().T):
                    with pytest.raises(ValueError, match="must be on cuda:0"):            # past the checks: the device, last
                        call(X, ok)
            # the draws' own arguments
            for nd in (0, -1, 2.0, True):
                with pytest.raises(ValueError, match="n_draws"):
                    p.draws_noisy_cov_dev(X, good, nd, return_gamma=True)
            with pytest.raises(ValueError, match="seed"):
                p.draws_noisy_cov_dev(X, good, 4, seed=-1, return_gamma=True)
            with pytest.raises(ValueError, match="Z must have shape"):
                p.draws_noisy_cov_dev(X, good, 4, Z=np.zeros((5, 4, k)), return_gamma=True)
            # the stack's own arguments
            with pytest.raises(ValueError, match="edges"):
                p.stack_noisy_cov_dev(X, good, e[::-1])
            with pytest.raises(ValueError, match="edges"):
                p.stack_noisy_cov_dev(X, good, [0.0])
            with pytest.raises(ValueError, match="n_draws"):
                p.stack_noisy_cov_dev(X, good, e, n_draws=-1)
            with pytest.raises(ValueError, match="Z must be None when n_draws is 0"):
                p.stack_noisy_cov_dev(X, good, e, Z=np.zeros((6, 1, k)))
            with pytest.raises(ValueError, match="groups"):
                p.stack_noisy_cov_dev(X, good, e, groups=torch.zeros(4))
            with pytest.raises(ValueError, match="groups"):
                p.stack_noisy_cov_dev(X, good, e, groups=torch.zeros(3, dtype=torch.int64))
            with pytest.raises(ValueError, match="weights"):
                p.stack_noisy_cov_dev(X, good, e, weights=torch.zeros(3))
            with pytest.raises(ValueError, match="weights"):
                p.stack_noisy_cov_dev(X, good, e, weights=torch.zeros(4, dtype=torch.int64))
            with pytest.raises(ValueError, match="n_groups"):
                p.stack_noisy_cov_dev(X, good, e, n_groups=0)
            with pytest.raises(ValueError, match="over the limit"):
                p.stack_noisy_cov_dev(X, good, e, n_groups=1000)
            with pytest.raises(ValueError, match="must be on cuda:0"):                    # n_draws = 0 passes the checks too
                p.stack_noisy_cov_dev(X, good, e)
            # the old spellings keep their refusals and texts for a covariance kind
            with pytest.raises(ValueError, match="predict_noisy_fits"):
                p.stack_noisy_dev(X, good, e)
            with pytest.raises(ValueError, match="predict_noisy_fits"):
                p.draws_dev(X, 4, Psi=good, return_gamma=True)
            p.close()
            with pytest.raises(RuntimeError, match="closed"):
                p.stack_noisy_cov_dev(X, good, e)
            with pytest.raises(RuntimeError, match="closed"):
                p.draws_noisy_cov_dev(X, good, 4, return_gamma=True)
    # a diagonal kind is sent to the other spelling
    for method in ("GL", "VL", "GD", "VD"):
        p = gpz_amd.Predictor(_model(method=method))
        with pytest.raises(ValueError, match=r"diagonal kind.*draws_dev\(X, Psi=Psi\)"):
            p.draws_noisy_cov_dev(X, good, 4, return_gamma=True)
        with pytest.raises(ValueError, match=r"diagonal kind.*stack_noisy_dev\(X, Psi, edges\)"):
            p.stack_noisy_cov_dev(X, good, e)
    # shapes outside predict_noisy_cov_fits
    for kw in ({"m": 300}, {"d": 12}, {"d": 11}, {"k": 9}):
        model = _model(method="VC", **kw)
        d = model.d
        p = gpz_amd.Predictor(model)
        Xd, Pd = torch.zeros((4, d), dtype=torch.float64), torch.ones((4, d), dtype=torch.float64)
        with pytest.raises(ValueError, match="draws_noisy_cov_dev needs.*predict_noisy_cov_fits.*Predictor.predict"):
            p.draws_noisy_cov_dev(Xd, Pd, 4, return_gamma=True)
        with pytest.raises(ValueError, match="stack_noisy_cov_dev needs.*predict_noisy_cov_fits.*Predictor.predict"):
            p.stack_noisy_cov_dev(Xd, Pd, e)
    # the edges of the scope pass the shape check (and then stop at the device), on either route of the handle
    for kw in ({"m": 256}, {"d": 10}, {"d": 1}, {"k": 8}):
        model = _model(method="GC", **kw)
        d = model.d
        for force in (False, True):
            p = gpz_amd.Predictor(model, force_tiles=force)
            Xd, Pd = torch.zeros((4, d), dtype=torch.float64), torch.ones((4, d), dtype=torch.float64)
            with pytest.raises(ValueError, match="must be on cuda:0"):
                p.draws_noisy_cov_dev(Xd, Pd, 4, return_gamma=True)
            with pytest.raises(ValueError, match="must be on cuda:0"):
                p.stack_noisy_cov_dev(Xd, Pd, e, n_draws=3)
