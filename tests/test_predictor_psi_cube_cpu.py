"""CPU-side checks of rows with a full input-noise covariance on the predictor handle (Predictor.predict_psi_cube_dev /
draws_psi_cube_dev / stack_psi_cube_dev; gpz_predictor_run_psi_cube_dev, _draws_psi_cube_dev, _draws_gamma_psi_cube_dev and
_stack_psi_cube_dev of the C ABI): the entries are declared with their twins' arguments but three Psi strides and the divisor triangle,
bound, exported and in the entry table; the factor step, the Psi policy and each kernel body have one definition and the units no
chunk rule; k_predict_psi_cube.hip and k_predict_psi_cube_gamma.hip compile for gfx950 to complete instantiation sets without scratch,
spills or atomics, inside the register bounds of DESIGN.md section 33; and every refusal of the three methods fires before the GPU is
touched."""
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
UNITS = ("k_predict_psi_cube.hip", "k_predict_psi_cube_gamma.hip")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_run_psi_cube_dev": "gpz_predictor_run_noisy_cov_dev",
           "gpz_predictor_draws_psi_cube_dev": "gpz_predictor_draws_noisy_cov_dev",
           "gpz_predictor_draws_gamma_psi_cube_dev": "gpz_predictor_draws_gamma_noisy_cov_dev",
           "gpz_predictor_stack_psi_cube_dev": "gpz_predictor_stack_noisy_cov_dev"}
# The largest d at which every instantiation of a kernel stays within 256 registers (VGPRs + AGPRs: two workgroups of 256 per compute
# unit), read from the compile of this file's third test; above it a kernel takes one workgroup per compute unit (<= 512)
LAST_D_WITHIN_256 = {"k_predict_psi_cube_small": 8, "k_predict_psi_cube_phi": 9, "k_predict_psi_cube_gamma": 7}


def _args(h, name):
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
    assert m, f"{name} is not declared in gpz_hip.h"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_header_binding_library_and_entry_table_agree():
    """Each entry has its noisy_cov twin's arguments with (matrix row, matrix column, catalogue row) strides where the twin has two and
    the divisor triangle where the twin has sd2."""
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name, twin in ENTRIES.items():
        want = []
        for a in _args(h, twin):
            if a == "int64_t psi_row_stride":
                want += ["int64_t psi_mrow_stride"]
            elif a == "int64_t psi_col_stride":
                want += ["int64_t psi_mcol_stride", "int64_t psi_row_stride"]
            else:
                want.append("const double *div" if a == "const double *sd2" else a)
        assert _args(h, name) == want, name
        res, args = _lib.SYMBOLS[name]
        tres, targs = _lib.SYMBOLS[twin]
        at = targs.index(_lib.C.c_int64, 6)                               # the twin's first Psi stride (behind Psi_d and psi_type)
        assert res == tres and list(args) == list(targs[:at]) + [_lib.C.c_int64] + list(targs[at:]), name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    E = gpz_amd.predictor._DEV_ENTRIES
    assert {q: E[q, "psi_cube"] for q in ("run", "draws", "draws_gamma", "stack")} == dict(zip(("run", "draws", "draws_gamma", "stack"),
                                                                                              ENTRIES))
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert " k_predict_psi_cube " in build and " k_predict_psi_cube_gamma " in build and "k_ncov_density.h" in build
    assert "$SRC/k_predict_ncov_impl.h" in build                          # a change to the shared bodies rebuilds the units
    for m in ("predict_psi_cube_dev", "draws_psi_cube_dev", "stack_psi_cube_dev"):
        assert callable(getattr(gpz_amd.Predictor, m))


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))}


def test_the_factor_has_one_definition_and_the_units_no_chunk_rule():
    """The factor, the density and the Psi policy live in k_ncov_density.h alone; both units take their kernels from the bodies of
    k_predict_ncov_impl.h (the tile kernels) and from GammaNcov (the gamma kernel) with PsiTri, which is where ncov_factor_tri is
    called; neither has a chunk rule; and the host passes the handle's chunk counts to the form's launchers."""
    src = _sources()
    head = src["k_ncov_density.h"]
    assert len(re.findall(r"__device__[^;{]*\bncov_factor_tri\s*\(", head)) == 1
    for f, text in src.items():
        if f != "k_ncov_density.h":
            assert not re.search(r"__device__[^;{]*\bncov_factor_tri\s*\(", text), f
            assert "ncov_factor_tri<" not in re.sub(r"//.*", "", text), f     # reached through PsiTri alone
    tri = re.search(r"struct PsiTri \{.*?\n\};", head, flags=re.S).group(0)
    assert "ncov_factor_tri<DD>(S, ps, 1, M, rd, prd)" in tri and "W = DD * (DD + 1) / 2" in tri
    impl = re.sub(r"//.*", "", src["k_predict_ncov_impl.h"])
    assert re.search(r'#include\s+"k_ncov_density\.h"', impl) and "Psi::factor(" in impl and "ncov_density<" in impl
    policy = re.search(r"struct GammaNcov \{.*?\n\};", head, flags=re.S).group(0)
    assert "Psi::factor(" in policy and "ncov_density<" in policy
    for unit, needs in ((UNITS[0], ('#include "k_predict_ncov_impl.h"', "predict_ncov_small_body<PsiTri<D>, SHARED, KM>(a)",
                                    "predict_ncov_phi_body<PsiTri<D>, SHARED>(a)")),
                        (UNITS[1], ('#include "k_ncov_density.h"', "predict_gamma_body<GammaNcov<PsiTri<D>, SHARED, pcg_blocks(D)>>(a)"))):
        code = re.sub(r"//.*", "", src[unit])
        for word in needs:
            assert word in code, (unit, word)
        assert not re.search(r"__device__[^;{]*\b(ncov_(factor|density)|chol_packed_rd)\s*\(", code), unit
        assert not re.search(r"\bint\s+\w*chunks\s*\(", code) and "predict_gamma_chunks" not in code, unit
        assert "predict_noisy_cov_chunks" not in code, unit
    assert not re.search(r"\bint\s+\w*chunks\s*\(", impl) and "predict_noisy_cov_chunks" not in impl
    host = re.sub(r"//.*", "", src["gpz_predictor.hip"])
    form = re.search(r"static NcovForm ncov_form\(.*?\n\}", host, flags=re.S).group(0)
    assert re.search(r"r\.cube\(\)\) return \{p->Psiq, launch_predict_psi_cube_small, launch_predict_psi_cube_phi, "
                     r"launch_predict_psi_cube_gamma, \"psi_cube\"\}", form)
    assert re.search(r"\bf\.small\([^;]*f\.Psi\[s\][^;]*p->cchunks", host, flags=re.S)
    assert re.search(r"\bf\.phi\([^;]*f\.Psi\[s\][^;]*p->cchunks", host, flags=re.S)
    assert re.search(r"\bf\.gamma\([^;]*f\.Psi\[s\][^;]*p->gchunks[^;]*p->gpart", host, flags=re.S)
    prep = re.search(r"int rows_gamma_prepare\(.*?\n\}", host, flags=re.S).group(0)
    assert re.search(r"r\.ncov\(\)[^;]*gchunks\s*=\s*predict_gamma_chunks\(p->m\)", prep)
    assert re.search(r"bool ncov\(\) const \{ return kind == ROWS_NOISY_COV \|\| kind == ROWS_PSI_CUBE; \}", src["gpz_predictor.h"])


def test_each_body_has_one_definition_and_the_host_no_cube_flag():
    """The record loops of the four tile kernels are the two bodies of k_predict_ncov_impl.h and the two gamma policies are GammaNcov:
    each is defined once in the tree, the four units hold wrappers only, and the host tells the two forms apart by the kind of rows."""
    src = _sources()
    code = {f: re.sub(r"//.*", "", t) for f, t in src.items()}
    for body, home in (("predict_ncov_small_body", "k_predict_ncov_impl.h"), ("predict_ncov_phi_body", "k_predict_ncov_impl.h"),
                       ("struct GammaNcov", "k_ncov_density.h"), ("struct PsiDiag", "k_ncov_density.h"), ("struct PsiTri", "k_ncov_density.h")):
        pat = re.escape(body) + (r"\s*\{" if body.startswith("struct") else r"\s*\(const PredNcovArgs &a\)\s*\{")
        assert [f for f, t in code.items() if re.search(pat, t)] == [home], body
    # the record loops themselves: the calls that form a density per record stand in the two headers and nowhere else
    assert sorted(f for f, t in code.items() if "Psi::factor(" in t) == ["k_ncov_density.h", "k_predict_ncov_impl.h"]
    assert not [f for f, t in code.items() if "ncov_density<" in t and re.match(r"k_predict_(noisy_cov|psi_cube)", f)]
    for unit, kernels in (("k_predict_noisy_cov.hip", ("k_predict_noisy_cov_small", "k_predict_noisy_cov_phi")),
                          ("k_predict_psi_cube.hip", ("k_predict_psi_cube_small", "k_predict_psi_cube_phi")),
                          ("k_predict_noisy_cov_gamma.hip", ("k_predict_noisy_cov_gamma",)),
                          ("k_predict_psi_cube_gamma.hip", ("k_predict_psi_cube_gamma",))):
        for kname in kernels:
            m = re.search(r"__global__[^{;]*\bvoid " + kname + r"\((?:PredNcovArgs|PredGammaArgs) a\) \{\s*(.*?)\s*\}", code[unit], flags=re.S)
            assert m and re.fullmatch(r"predict_\w+_body<[^;]*>\(a\);", m.group(1)), (unit, kname)   # a wrapper: one call
        assert "__syncthreads" not in code[unit] and "__shared__" not in code[unit], unit   # no staging loop of its own
        for word in ("struct GammaCov", "struct GammaCube", "PredNoisyCovArgs", "PredPsiCubeArgs"):
            assert word not in code[unit], (unit, word)
    for f, t in code.items():
        for word in ("GPZ_PSI_CUBE_REG_D", "psi_cube_regs", "gamq", "per_draw("):
            assert word not in t, (f, word)
        assert not re.search(r"\bbool cube\b(?!\()", t), f              # no flag parameter (Rows::cube() and cube_used are not one)
    assert "den.bind(" not in code["k_predict_gamma_impl.h"] and "gamma_psi_width" not in code["k_predict_gamma_impl.h"]
    host = code["gpz_predictor.hip"]
    assert len(re.findall(r"ROWS_NOISY_COV\s*\|\|", host + code["gpz_predictor_dev.hip"] + code["gpz_predictor_host.hip"])) == 0
    assert "} gam[8];" in src["gpz_predictor.h"] and "p->gam[r.kind - 1]" in host


def _compile(unit, tmp_path):
    asm = tmp_path / (unit + ".s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, unit), "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    return _resource_records(r.stderr), asm.read_text()


NO_ATOMICS = ("atomic_add_f", "atomic_pk_add", "atomic_fadd", "atomic_fmin", "atomic_fmax", "ds_add_f", "ds_add_rtn_f", "cmpswap",
              "scratch_")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_psi_cube_kernels_compiled_form(tmp_path):
    """Every kernel of both units: no scratch, no spilled register, VGPRs + AGPRs <= 512.  d = 1 .. 10 x {GC, VC} (x {1, 8} outputs for
    the moments), each with its twin's LDS stage; the largest d within 256 registers per kernel as pinned above.  The gamma unit has the
    f64 MFMA in its loop, at least 4 accumulator blocks per pass at every d.  No floating-point atomic and no compare-and-swap loop."""
    recs, text = _compile(UNITS[0], tmp_path)
    grecs, gtext = _compile(UNITS[1], tmp_path)
    for kname in ("k_predict_psi_cube_small", "k_predict_psi_cube_phi", "k_pred_check_psi_cube", "k_pred_stage_psi_cube"):
        assert any(kname in n for n in recs), (kname, sorted(recs))
    assert len(grecs) == 20 and all("k_predict_psi_cube_gamma" in n for n in grecs), sorted(grecs)
    for name, q in list(recs.items()) + list(grecs.items()):
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 512, (name, q)
    worst = {}                                                            # kernel -> d -> most registers over its instantiations
    small = {n: q for n, q in recs.items() if "k_predict_psi_cube_small" in n}
    assert len(small) == 40, sorted(small)
    seen = set()
    for name, q in small.items():
        d, shared, km = (int(v) for v in re.search(r"ILi(\d+)ELb(\d)ELi(\d+)E", name).groups())
        seen.add((d, shared, km))
        assert q["LDS Size [bytes/block]"] == 32 * (1 + d + d * (d + 1) // 2 + 3 * km) * 8, (name, q)
        w = worst.setdefault("k_predict_psi_cube_small", {})
        w[d] = max(w.get(d, 0), q["VGPRs"] + q.get("AGPRs", 0))
    assert seen == {(d, s, km) for d in range(1, 11) for s in (0, 1) for km in (1, 8)}
    for kname, rr in (("k_predict_psi_cube_phi", recs), ("k_predict_psi_cube_gamma", grecs)):
        mine = {n: q for n, q in rr.items() if kname in n}
        assert len(mine) == 20, sorted(mine)
        seen = set()
        for name, q in mine.items():
            d, shared = (int(v) for v in re.search(r"ILi(\d+)ELb(\d)E", name).groups())
            seen.add((d, shared))
            assert q["LDS Size [bytes/block]"] == 32 * (1 + d + d * (d + 1) // 2) * 8, (name, q)
            w = worst.setdefault(kname, {})
            w[d] = max(w.get(d, 0), q["VGPRs"] + q.get("AGPRs", 0))
        assert seen == {(d, s) for d in range(1, 11) for s in (0, 1)}
    for kname, w in worst.items():
        print(kname, "most registers per d:", sorted(w.items()))
        last = max(d for d in range(1, 11) if all(w[e] <= 256 for e in range(1, d + 1)))
        assert last == LAST_D_WITHIN_256[kname], (kname, last, sorted(w.items()))
    assert "v_mfma_f64_16x16x4" in gtext and "v_rsq_f64" in gtext
    for word in NO_ATOMICS + ("global_atomic", "flat_atomic"):
        assert word not in gtext, word
    for word in NO_ATOMICS:
        assert word not in text, word
    # (the unit's one atomic is the integer OR of the scan's verdict word)
    assert set(re.findall(r"\b(?:global|flat)_atomic_\w+", text)) <= {"global_atomic_or", "flat_atomic_or"}
    per = {}
    for part in re.split(r"\t\.type\t(?=_Z\d+k_predict_psi_cube_gamma)", gtext)[1:]:
        name = part.split(",", 1)[0]
        body = part.split("\t.size\t" + name, 1)[0]
        d, shared = (int(v) for v in re.search(r"ILi(\d+)ELb(\d)E", name).groups())
        per[d, shared] = body.count("v_mfma_f64_16x16x4")
    assert set(per) == {(d, s) for d in range(1, 11) for s in (0, 1)}, sorted(per)
    print("MFMAs (= 16-column blocks per pass) per kernel:", sorted(per.items()))
    assert all(n >= 4 for n in per.values()), per
    assert all(per[d, 0] == per[d, 1] for d in range(1, 11)), per


def test_refusals_fire_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of the three methods is raised on the host: the library load is made to fail, so a call that got past
    the checks would raise RuntimeError instead.  Each refusal says where such rows go, and the old spellings keep their texts on a cube."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    e = np.linspace(0.0, 1.0, 11)
    X = torch.zeros((4, 3), dtype=torch.float64)
    good = torch.ones((3, 3, 4), dtype=torch.float64)

    def calls(p):
        return {"predict": lambda x, psi, **kw: p.predict_psi_cube_dev(x, psi, **kw),
                "draws": lambda x, psi, **kw: p.draws_psi_cube_dev(x, psi, 4, return_gamma=True, **kw),
                "stack": lambda x, psi, **kw: p.stack_psi_cube_dev(x, psi, e, n_draws=2, **kw)}

    for method in ("VC", "GC"):
        for k in (1, 2):
            p = gpz_amd.Predictor(_model(k=k, method=method))
            for what, call in calls(p).items():
                with pytest.raises(ValueError, match=f"{what}_psi_cube_dev needs Psi.*{what}_dev\\(X"):
                    call(X, None)
                for flat in (torch.ones((4, 3), dtype=torch.float64), np.ones((4, 3)), torch.ones(4, dtype=torch.float64)):
                    with pytest.raises(ValueError, match=f"d x d x n cube.*{what}_noisy_cov_dev"):
                        call(X, flat)
                with pytest.raises(TypeError, match=r"host arrays stay on Predictor.predict\(X, Psi=Psi\)"):
                    call(X, np.ones((3, 3, 4)))
                with pytest.raises(TypeError, match="Psi must be a torch.Tensor"):
                    call(X, [[[1.0] * 4] * 3] * 3)
                with pytest.raises(TypeError, match=f"Predictor.{what}"):                 # a NumPy X
                    call(np.zeros((4, 3)), good)
                for bad in (good.half(), good.long()):
                    with pytest.raises(TypeError, match="Psi must be float64 or float32"):
                        call(X, bad)
                for shape in ((4, 3, 3), (3, 3, 5), (3, 2, 4), (2, 3, 4), (3, 3, 4, 1)):
                    with pytest.raises(ValueError, match=r"Psi must be d x d x n.*permute\(1, 2, 0\)"):
                        call(X, torch.ones(shape, dtype=torch.float64))
                with pytest.raises(ValueError, match="X must be n x 3"):                  # X's own checks come first
                    call(torch.zeros((4, 2), dtype=torch.float64), good)
                with pytest.raises(ValueError, match="selection must be a mask of length 4"):
                    call(X, good, selection=torch.zeros(3, dtype=torch.bool))
                for ok in (good, good.float(), torch.ones((4, 3, 3), dtype=torch.float64).permute(1, 2, 0), good[:, :, :]):
                    with pytest.raises(ValueError, match="must be on cuda:0"):            # past the checks: the device, last
                        call(X, ok)
                with pytest.raises(ValueError, match="must be on cuda:0"):
                    call(X, good, selection=torch.ones(4, dtype=torch.bool))
            with pytest.raises(ValueError, match="n_draws"):
                p.draws_psi_cube_dev(X, good, 0)
            with pytest.raises(ValueError, match="edges"):
                p.stack_psi_cube_dev(X, good, [0.0])
            # the old spellings keep their texts on a cube
            with pytest.raises(ValueError, match=r"full d x d x n Psi stays on Predictor.predict"):
                p.predict_noisy_cov_dev(X, good)
            with pytest.raises(ValueError, match=r"full d x d x n Psi stays on Predictor.predict"):
                p.draws_noisy_cov_dev(X, good, 4)
            with pytest.raises(ValueError, match=r"full d x d x n Psi stays on Predictor.predict"):
                p.stack_noisy_cov_dev(X, good, e)
            p.close()
            with pytest.raises(RuntimeError, match="closed"):
                p.predict_psi_cube_dev(X, good)
    # a diagonal kind is sent to the Psi keyword with the cube's diagonal
    for method in ("GL", "VL", "GD", "VD"):
        p = gpz_amd.Predictor(_model(method=method))
        with pytest.raises(ValueError, match=r"diagonal kind.*cube's diagonal.*predict_dev\(X, Psi=Psi\)"):
            p.predict_psi_cube_dev(X, good)
        with pytest.raises(ValueError, match=r"diagonal kind.*cube's diagonal.*draws_dev\(X, Psi=Psi\)"):
            p.draws_psi_cube_dev(X, good, 4)
        with pytest.raises(ValueError, match=r"diagonal kind.*cube's diagonal.*stack_noisy_dev\(X, Psi, edges\)"):
            p.stack_psi_cube_dev(X, good, e)
    # shapes outside predict_noisy_cov_fits
    for kw in ({"m": 300}, {"d": 12}, {"d": 11}, {"k": 9}):
        model = _model(method="VC", **kw)
        d = model.d
        p = gpz_amd.Predictor(model)
        Xd, Pd = torch.zeros((4, d), dtype=torch.float64), torch.ones((d, d, 4), dtype=torch.float64)
        for call in calls(p).values():
            with pytest.raises(ValueError, match="predict_noisy_cov_fits.*Predictor.predict"):
                call(Xd, Pd)
    # the edges of the scope pass the shape check (and then stop at the device)
    for kw in ({"m": 256}, {"d": 10}, {"d": 1}, {"k": 8}):
        model = _model(method="GC", **kw)
        d = model.d
        p = gpz_amd.Predictor(model, force_tiles=True)                                    # (no route is refused)
        for call in calls(p).values():
            with pytest.raises(ValueError, match="must be on cuda:0"):
                call(torch.zeros((4, d), dtype=torch.float64), torch.ones((d, d, 4), dtype=torch.float64))
