"""CPU-side checks of rows with a full input-noise covariance and missing inputs on the predictor handle
(Predictor.predict_psi_cube_missing_dev / draws_psi_cube_missing_dev / stack_psi_cube_missing_dev; gpz_predictor_run_psi_cube_missing_dev,
_draws_, _draws_gamma_ and _stack_psi_cube_missing_dev of the C ABI): the entries are declared with their noisy_missing_cov twins'
arguments but three Psi strides and the divisor triangle, bound, exported and in the entry table; the identity that reduces each density
of predictNoisyMissing to nu squares and one no x no form holds for a full Psi_oo; gamma under a draw is a quadratic form of the
draw's weights with a cube; k_predict_psi_cube_missing.hip and k_predict_psi_cube_missing_gamma.hip compile for gfx950 without scratch,
spills or static LDS, with the instantiations above 256 registers pinned; and every refusal of the three methods fires before the GPU
is touched."""
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
from predict_edges import psi_cube
from test_predictor import catalogue, synth_model
from test_predictor_noisy_cpu import _model, _resource_records
from test_predictor_stack_noisy import with_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
UNITS = ("k_predict_psi_cube_missing.hip", "k_predict_psi_cube_missing_gamma.hip")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_run_psi_cube_missing_dev": "gpz_predictor_run_noisy_missing_cov_dev",
           "gpz_predictor_draws_psi_cube_missing_dev": "gpz_predictor_draws_noisy_missing_cov_dev",
           "gpz_predictor_draws_gamma_psi_cube_missing_dev": "gpz_predictor_draws_gamma_noisy_missing_cov_dev",
           "gpz_predictor_stack_psi_cube_missing_dev": "gpz_predictor_stack_noisy_missing_cov_dev"}
# The instantiations above 256 registers (VGPRs + AGPRs: one workgroup of 256 per compute unit), as the compile of this file's fourth
# test reports them and DESIGN.md section 34 records them; every other one is within 256
OVER_256 = {"k_pcm_ex": {9}, "k_pcm_phi": {8, 9}, "k_predict_psi_cube_missing_pairs": {(7, 8), (8, 1), (8, 8), (9, 1), (9, 8)},
            "k_predict_psi_cube_missing_gamma": {7, 8, 9}}


def _args(h, name):
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
    assert m, f"{name} is not declared in gpz_hip.h"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


# ---- 1. the entry table and the ABI --------------------------------------------------------------------------------------------------------
def test_header_binding_library_and_entry_table_agree():
    """Each entry has its noisy_missing_cov twin's arguments with (matrix row, matrix column, catalogue row) strides where the twin has
    two and the divisor triangle where the twin has sd2 - the way section 33's entries take a cube."""
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
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == list(args), name
    E = gpz_amd.predictor._DEV_ENTRIES
    questions = ("run", "draws", "draws_gamma", "stack")
    assert {q: E[q, "psi_cube_missing"] for q in questions} == dict(zip(questions, ENTRIES))
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert " k_predict_psi_cube_missing " in build and " k_predict_psi_cube_missing_gamma " in build and "k_pnmc_density.h" in build
    for m in ("predict_psi_cube_missing_dev", "draws_psi_cube_missing_dev", "stack_psi_cube_missing_dev"):
        assert callable(getattr(gpz_amd.Predictor, m))
    kh = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    for fn in ("launch_pcm_check_psi", "launch_pcm_stage_psi", "launch_pcm_rows", "launch_predict_psi_cube_missing_pairs",
               "launch_predict_psi_cube_missing_gamma"):
        assert f"int {fn}(" in kh, fn
    ph = open(os.path.join(CSRC, "gpz_predictor.h")).read()
    assert "ROWS_PSI_CUBE_MISSING = 8" in ph and "bool cube_obs() const" in ph
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert '"; noise cube missing: k_predict_psi_cube_missing_pairs (%d pair chunks)"' in host
    assert '"; noise cube missing per draw: k_predict_psi_cube_missing_gamma (%d pair chunks)"' in host
    # the density has one definition and one spelling, the Psi policy its parameter, and both units' kernels are the shared bodies with
    # PsiTri (the chunk, slab and LDS rules those bodies' launchers use: tests/test_predictor_noisy_missing_cov_cpu.py)
    head = re.sub(r"//.*", "", open(os.path.join(CSRC, "k_pnmc_density.h")).read())
    assert len(re.findall(r"P::factor\(", head)) == 1 and len(re.findall(r"double pnmc_density\(", head)) == 1
    assert "double pnmc_density(const double *t, int nu, const double (&x)[P::D], const double (&ps)[P::W])" in head
    for unit, bodies in zip(UNITS, (("nmcov_ex_body<PsiTri<NO>, true>(a)", "nmcov_phi_body<PsiTri<NO>, true>(a)", "nmcov_pairs_body<PsiTri<NO>, KM>(a)"),
                                    ("nmcov_gamma_body<PsiTri<NO>, pcmg_nb(NO)>(a)",))):
        code = re.sub(r"//.*", "", open(os.path.join(CSRC, unit)).read())
        for body in bodies:
            assert body in code, (unit, body)
        assert "ncov_factor" not in code and "int predict_missing_cov_chunks(" not in code, unit
    impl = open(os.path.join(CSRC, "k_predict_nmcov_impl.h")).read()
    assert "predict_noisy_missing_cov_gamma_lds(m, d, pt.no)" in impl                                             # LDS is unchanged


def test_each_body_has_one_definition_and_the_host_one_form_table():
    """The tile and gamma kernels of a group with Psi, a variance per observed input or a full matrix per row, are the four bodies of
    k_predict_nmcov_impl.h: each body, both argument structs and the row loader are defined once in the tree, the four units hold
    wrappers only, the names of the copies are gone, and the host reaches the launchers of either form through group_psi_form alone."""
    code = {f: re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read()) for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}
    home = "k_predict_nmcov_impl.h"
    for what, pat in (("nmcov_ex_body", r"void nmcov_ex_body\(const PredNmcovArgs &a\)\s*\{"),
                      ("nmcov_phi_body", r"void nmcov_phi_body\(PredNmcovArgs a\)\s*\{"),
                      ("nmcov_pairs_body", r"void nmcov_pairs_body\(PredNmcovArgs a\)\s*\{"),
                      ("nmcov_gamma_body", r"void nmcov_gamma_body\(PredNmcovGammaArgs a\)\s*\{"),
                      ("PredNmcovArgs", r"struct PredNmcovArgs\s*\{"), ("PredNmcovGammaArgs", r"struct PredNmcovGammaArgs\s*\{"),
                      ("nmcov_load", r"void nmcov_load\(const A &a, long ic, double \(&x\)\[P::D\], double \(&ps\)\[P::W\]\)\s*\{")):
        assert [f for f, t in code.items() if re.search(pat, t)] == [home], what
    impl = code[home]
    for body in ("nmcov_ex_body", "nmcov_phi_body", "nmcov_pairs_body", "nmcov_gamma_body"):   # by value, its own LDS, one density
        text = re.search(r"__device__ __forceinline__ void " + body + r"\(.*?\n\}", impl, flags=re.S).group(0)
        stage = "double *sT = nmcov_stage<DYNAMIC>();" if body in ("nmcov_ex_body", "nmcov_phi_body") else "extern __shared__ double sm[];"
        assert text.count(stage) == 1 and len(re.findall(r"__shared__", text)) == (stage[0] == "e"), body
        assert "nmcov_load<P>(a, ic, x, ps);" in text, body
        assert len(re.findall(r"\w*density\w*[<(]", text)) == 1 and "pnmc_density<P>(" in text, body
    # the record stage of the Ex and PHI bodies: one helper, static (k_pnmc_*, as it was) or the launch's dynamic LDS (k_pcm_*, as it was)
    stage = re.search(r"double \*nmcov_stage\(\) \{.*?\n\}", impl, flags=re.S).group(0)
    assert "extern __shared__ double dyn[];" in stage and "__shared__ double fix[PNMC_STD];" in stage and impl.count("__shared__") == 4
    assert "nmcov_ex_body<PsiDiag<NO>, false>(a)" in code["k_predict_noisy_missing_cov.hip"]
    assert "nmcov_phi_body<PsiDiag<NO>, false>(a)" in code["k_predict_noisy_missing_cov.hip"]
    assert "stage_lds = 0;" in code["k_predict_noisy_missing_cov.hip"]
    assert "stage_lds = PNMC_STD * sizeof(double);" in code["k_predict_psi_cube_missing.hip"] and impl.count("K::stage_lds, st") == 2
    assert "bool" not in re.search(r"void nmcov_load_psi\(.*?void nmcov_load\([^{]*\{", impl, flags=re.S).group(0)   # by policy, no flag
    assert "nmcov_load_psi(PsiDiag<NO>, const A &a" in impl and "nmcov_load_psi(PsiTri<NO>, const A &a" in impl
    assert "ps[c] = a.Psi[(size_t)a.oidx[c] * a.ldx + ic];" in impl and "ncov_psi_load(a.Psi + ic, a.ldx, ps);" in impl
    assert len(re.findall(r"P::factor\(", code["k_pnmc_density.h"])) == 1
    for unit in ("k_predict_noisy_missing_cov.hip", "k_predict_psi_cube_missing.hip", "k_predict_noisy_missing_cov_gamma.hip",
                 "k_predict_psi_cube_missing_gamma.hip"):
        for word in ("__shared__", "__syncthreads", "pnmc_density"):
            assert word not in code[unit], (unit, word)
        assert '#include "k_predict_nmcov_impl.h"' in code[unit], unit
    for f, t in code.items():
        for word in ("PnmcArgs", "PcmArgs", "PcmgArgs", "NmcgArgs", "PCM_STD", "PCM_SB", "GPZ_PCMG_SB", "GPZ_PCMG_PF", "pcmg_stride",
                     "gam_pcm", "rows_gamma_state"):
            assert word not in t, (f, word)
    for name in ("PNMC_STD", "PNMC_SB", "GPZ_NMCG_SB", "GPZ_NMCG_PF"):                   # one definition of each stage size
        assert [f for f, t in code.items() if re.search(r"#define " + name + r"\b", t)] == [home], name
    assert [f for f, t in code.items() if re.search(r"\bint nmcg_stride\(", t)] == [home]
    assert "ldx < n" in re.search(r"static int nmcov_launch_rows\(.*?\n\}", impl, flags=re.S).group(0)   # both forms refuse it now
    assert "ldx < n" in re.search(r"static int nmcov_launch_pairs\(.*?\n\}", impl, flags=re.S).group(0)
    assert "ldx < n" in re.search(r"static int nmcov_launch_gamma\(.*?\n\}", impl, flags=re.S).group(0)
    host = code["gpz_predictor.hip"]
    form = re.search(r"static GroupPsiForm group_psi_form\(.*?\n\}", host, flags=re.S).group(0)
    for fn in ("launch_pnmc_rows", "launch_predict_noisy_missing_cov_pairs", "launch_predict_noisy_missing_cov_gamma", "launch_pcm_rows",
               "launch_predict_psi_cube_missing_pairs", "launch_predict_psi_cube_missing_gamma"):
        assert len(re.findall(r"\b" + fn + r"\b(?!\))", host)) == 1 and re.search(r"\b" + fn + r"\b", form), fn   # (decltype(&fn) aside)
    assert '"k_pcm"' in form and '"psi_cube_missing"' in form and '"k_pnmc"' in form and '"noisy_missing_cov"' in form
    assert "p->Psiq, launch_pcm_rows" in form and "p->Psic, launch_pnmc_rows" in form
    tile = re.search(r"static int predictor_missing_cov_tile\(.*?\n\}", host, flags=re.S).group(0)
    assert len(re.findall(r"\bf\.rows\(", tile)) == 1 and len(re.findall(r"\bf\.pairs\(", tile)) == 1 and "launch_pmcv_rows(" in tile
    assert '"%s: %s launch failed", who, f.rows_name' in tile and '"%s: k_predict_%s_pairs launch failed", who, f.name' in tile
    gtile = re.search(r"int rows_gamma_tile\(.*?\n\}", host, flags=re.S).group(0)
    assert len(re.findall(r"\bg\.gamma\(", gtile)) == 1 and len(re.findall(r"launch_predict_missing_cov_gamma\(", gtile)) == 1
    assert "} gam[8];" in code["gpz_predictor.h"] and "p->gam[i]" in host
    assert "k_predict_nmcov_impl.h" in open(os.path.join(ROOT, "build.sh")).read()


# ---- 2. the identity with a full Psi_oo ----------------------------------------------------------------------------------------------------
def _random_psd(rng, n, rank):
    a = rng.standard_normal((n, rank))
    return a @ a.T


def _identity_error(rng, d, obs, Psi):
    """One density of predictNoisyMissing, two ways.  S: the covariance in [o u] order, C + CU on (u, u); T = [I; R']; G: the rows of T
    moved where predictCov.m:271-273's `unshuffle` (the inverse of the permutation [find(o) find(~o)], applied as an assignment) puts
    them; mean T x_o + s.  Direct: the quadratic form and log-determinant of S + G Psi_oo G'.  Section 31: whitening by S = L L', the
    Householder QR of L^-1 G, nu squares plus w' (M + Psi_oo)^-1 w, and |S| |R_B|^2 |M + Psi_oo|."""
    o = [c for c in range(d) if obs[c]]
    u = [c for c in range(d) if not obs[c]]
    no, nu = len(o), len(u)
    perm = np.array(o + u)
    inv = np.argsort(perm)                                                # inv[dimension] = its index in [o u]
    S = _random_psd(rng, d, d + 2) + 0.1 * np.eye(d)
    R = rng.standard_normal((no, nu))
    T = np.vstack([np.eye(no), R.T])
    G = np.zeros((d, no))
    for a in range(d):
        G[inv[inv[a]]] = T[a]                                             # row a of T Psi T' lands on dimension unshuffle(a)
    s, x = rng.standard_normal(d), rng.standard_normal(no)
    v = T @ x + s
    cov = S + G @ Psi @ G.T
    q_direct = v @ np.linalg.solve(cov, v)
    ld_direct = np.linalg.slogdet(cov)[1]
    L = np.linalg.cholesky(S)
    A, B, b = np.linalg.solve(L, T), np.linalg.solve(L, G), np.linalg.solve(L, s)
    Q, RB = np.linalg.qr(B, mode="complete")
    RB = RB[:no]
    y = Q.T @ (A @ x + b)
    w = np.linalg.solve(RB, y[:no])
    M = np.linalg.inv(RB.T @ RB)
    q_form = y[no:] @ y[no:] + w @ np.linalg.solve(M + Psi, w)
    ld_form = 2.0 * np.log(np.diag(L)).sum() + 2.0 * np.log(np.abs(np.diag(RB))).sum() + np.linalg.slogdet(M + Psi)[1]
    involution = bool(np.array_equal(inv[inv], np.arange(d)))
    return abs(q_form - q_direct) / abs(q_direct), abs(ld_form - ld_direct) / max(abs(ld_direct), 1.0), involution


def test_the_identity_holds_for_a_full_psi_oo():
    """d = 2 .. 6, every no < d (the first no dimensions observed, the last no observed, and scattered patterns), dimension 1 of 5
    missing among them ([o u] = [0 2 3 4 1] is no involution), Psi_oo random positive definite, singular (rank 1), and zero.  The gate
    is the project's oracle gate, 1e-8."""
    rng = np.random.default_rng(3401)
    worst, seen_non_involution = 0.0, False
    for d in range(2, 7):
        pats = set()
        for no in range(1, d):
            pats.add(tuple([1] * no + [0] * (d - no)))
            pats.add(tuple([0] * (d - no) + [1] * no))
            pats.add(tuple(int(b) for b in rng.permutation([1] * no + [0] * (d - no))))
        if d == 5:
            pats.add((1, 0, 1, 1, 1))
        for obs in sorted(pats):
            no = sum(obs)
            for Psi in (_random_psd(rng, no, no + 1), _random_psd(rng, no, 1), np.zeros((no, no))):
                eq, el, invol = _identity_error(rng, d, obs, Psi)
                worst = max(worst, eq, el)
                if obs == (1, 0, 1, 1, 1):
                    assert not invol
                    seen_non_involution = True
                assert eq <= 1e-8 and el <= 1e-8, (d, obs, eq, el)
    print(f"the identity with a full Psi_oo: largest relative difference {worst:.3e}")
    assert seen_non_involution


# ---- 3. gamma under a draw -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["GC", "VC"])
def test_gamma_per_draw_is_a_quadratic_form_of_the_draws_weights_with_a_cube(method):
    """tests/test_predictor_stack_noisy_missing_cov_cpu.py's definition of gamma_s with a cube: the matrix E(x, Psi) of the quadratic form
    gamma_s + mu_s^2, recovered from ``O.predict_any(X, model, Psi=cube)`` by polarisation, reproduces the oracle's gamma of the
    w := w_s model at rel <= 1e-8.  m = 4, d = 3; dimension 1 missing, dimension 0 missing ([1 2 0] is no involution), two missing."""
    m, d, k, n = 4, 3, 2, 12
    model = synth_model(method, m, d, k, True, seed=29)
    model.sets["best"]["priors"] = np.random.default_rng(30).dirichlet(np.full(m, 2.0))
    X = catalogue(model, n, seed=31)
    X[0:4, 1] = np.nan
    X[4:8, 0] = np.nan
    X[8:12, 0] = X[8:12, 2] = np.nan
    sd = np.asarray(model.sdX).reshape(-1)
    rng = np.random.default_rng(33)
    cube = psi_cube((0.05 + 0.2 * rng.random((n, d))) * sd ** 2, 0.3 * rng.standard_normal((n, d)) * sd)
    muY = np.asarray(model.muY).reshape(-1)

    def second_moment(w):
        out = O.predict_any(X, with_weights(model, w), Psi=cube)
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
        out = O.predict_any(X, with_weights(model, ws), Psi=cube)
        mu_s = out[0] - muY
        tri = sum((1.0 if a == b else 2.0) * E[:, :, a, b] * ws[a] * ws[b] for a in range(m) for b in range(a + 1))
        gamma_s = tri - mu_s ** 2
        print(f"{method} draw {s}: rel of the form's gamma_s against the oracle's {rel(gamma_s, out[4]):.3e}")
        assert rel(gamma_s, out[4]) <= 1e-8, (s, rel(gamma_s, out[4]))
        assert np.all(out[4] > 0.0)


# ---- 4. the compiled form ------------------------------------------------------------------------------------------------------------------
def _compile(unit, tmp_path):
    asm = tmp_path / (unit + ".s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, unit), "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    return _resource_records(r.stderr), asm.read_text()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_psi_cube_missing_kernels_compiled_form(tmp_path):
    """Every kernel of both units: no scratch, no spilled register, no static LDS (all of it is dynamic: the twins' figures),
    VGPRs + AGPRs <= 512, and the set above 256 registers is the pinned one.  NO = 1 .. 9 (x {1, 8} outputs for the pair kernel).  The
    gamma kernel has the f64 MFMA in its loop; no floating-point atomic and no compare-and-swap loop anywhere."""
    recs, text = _compile(UNITS[0], tmp_path)
    grecs, gtext = _compile(UNITS[1], tmp_path)
    assert len(grecs) == 9 and all("k_predict_psi_cube_missing_gamma" in n for n in grecs), sorted(grecs)
    for name, q in list(recs.items()) + list(grecs.items()):
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 512, (name, q)
        assert q["LDS Size [bytes/block]"] == 0, (name, q)
    over = {}
    for kname, rr, count in (("k_pcm_ex", recs, 9), ("k_pcm_phi", recs, 9), ("k_predict_psi_cube_missing_pairs", recs, 18),
                             ("k_predict_psi_cube_missing_gamma", grecs, 9)):
        mine = {n: q for n, q in rr.items() if kname in n}
        assert len(mine) == count, (kname, sorted(mine))
        seen = set()
        for name, q in sorted(mine.items()):
            key = tuple(int(v) for v in re.search(r"ILi(\d+)E(?:Li(\d+)E)?", name).groups() if v is not None)
            key = key if len(key) > 1 else key[0]
            seen.add(key)
            regs = q["VGPRs"] + q.get("AGPRs", 0)
            print(f"{kname}<{key}>: {q['VGPRs']} VGPRs + {q.get('AGPRs', 0)} AGPRs")
            if regs > 256:
                over.setdefault(kname, set()).add(key)
        want = {(no, km) for no in range(1, 10) for km in (1, 8)} if count == 18 else set(range(1, 10))
        assert seen == want, (kname, sorted(seen))
    assert over == OVER_256, over
    for kname in ("k_pcm_check_psi", "k_pcm_stage_psi"):
        assert any(kname in n for n in recs), kname
    assert "v_mfma_f64_16x16x4" in gtext and "v_rsq_f64" in gtext
    atomics = ("atomic_add_f", "atomic_pk_add", "atomic_fadd", "atomic_fmin", "atomic_fmax", "ds_add_f", "ds_add_rtn_f", "cmpswap", "scratch_")
    for word in atomics + ("global_atomic", "flat_atomic"):
        assert word not in gtext, word
    for word in atomics:
        assert word not in text, word
    # (the unit's one atomic is the integer OR of the scan's verdict word)
    assert set(re.findall(r"\b(?:global|flat)_atomic_\w+", text)) <= {"global_atomic_or", "flat_atomic_or"}
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_predict_psi_cube_missing_gamma<7>" in design and "k_predict_psi_cube_missing_pairs<9, 8>" in design


# ---- 5. the refusals of the three Python methods ---------------------------------------------------------------------------------------------
def test_refusals_fire_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of the three methods is raised on the host: the library load is made to fail, so a call that got past
    the checks would raise RuntimeError instead.  Each refusal says where such rows go, and the sibling methods keep their texts."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    e = np.linspace(0.0, 1.0, 11)
    X = torch.zeros((4, 3), dtype=torch.float64)
    X[1, 2] = float("nan")
    good = torch.ones((3, 3, 4), dtype=torch.float64)

    def calls(p):
        return {"predict": lambda x, psi, **kw: p.predict_psi_cube_missing_dev(x, psi, **kw),
                "draws": lambda x, psi, **kw: p.draws_psi_cube_missing_dev(x, psi, 4, return_gamma=True, **kw),
                "stack": lambda x, psi, **kw: p.stack_psi_cube_missing_dev(x, psi, e, n_draws=2, **kw)}

    for method in ("VC", "GC"):
        for k in (1, 2):
            p = gpz_amd.Predictor(_model(k=k, method=method))
            for what, call in calls(p).items():
                with pytest.raises(TypeError, match=rf"{what}_psi_cube_missing_dev takes a torch tensor.*Predictor.predict\(X, Psi=Psi\)"):
                    call(np.zeros((4, 3)), good)
                with pytest.raises(ValueError, match=f"{what}_psi_cube_missing_dev needs Psi.*{what}_missing_cov_dev"):
                    call(X, None)
                for flat in (torch.ones((4, 3), dtype=torch.float64), np.ones((4, 3)), torch.ones(4, dtype=torch.float64)):
                    with pytest.raises(ValueError, match=f"d x d x n cube.*{what}_noisy_missing_cov_dev"):
                        call(X, flat)
                with pytest.raises(TypeError, match=r"host arrays stay on Predictor.predict\(X, Psi=Psi\)"):
                    call(X, np.ones((3, 3, 4)))
                with pytest.raises(TypeError, match="Psi must be a torch.Tensor"):
                    call(X, [[[1.0] * 4] * 3] * 3)
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
                for ok in (good, good.float(), torch.ones((4, 3, 3), dtype=torch.float64).permute(1, 2, 0)):
                    with pytest.raises(ValueError, match="must be on cuda:0"):            # past the checks: the device, last
                        call(X, ok)
            with pytest.raises(ValueError, match="n_draws"):
                p.draws_psi_cube_missing_dev(X, good, 0)
            with pytest.raises(ValueError, match="edges"):
                p.stack_psi_cube_missing_dev(X, good, [0.0])
            # the siblings keep their texts on a cube
            with pytest.raises(ValueError, match=r"full d x d x n Psi stays on Predictor.predict\(X, Psi=Psi\)"):
                p.predict_noisy_missing_cov_dev(X, good)
            with pytest.raises(ValueError, match=r"full d x d x n Psi stays on Predictor.predict\(X, Psi=Psi\)"):
                p.stack_noisy_missing_cov_dev(X, good, e)
            p.close()
            with pytest.raises(RuntimeError, match="closed"):
                p.predict_psi_cube_missing_dev(X, good)
    for method in ("GL", "VL", "GD", "VD"):                                               # a diagonal kind: the cube's diagonal
        p = gpz_amd.Predictor(_model(method=method))
        for what, call in calls(p).items():
            with pytest.raises(ValueError, match=rf"diagonal kind.*cube's diagonal.*{what}_noisy_missing_dev\(X, Psi\)"):
                call(X, good)
    for kw in ({"m": 257}, {"d": 11}, {"k": 9}):                                          # shapes outside predict_missing_cov_fits
        model = _model(method="VC", **kw)
        d = model.d
        p = gpz_amd.Predictor(model)
        for call in calls(p).values():
            with pytest.raises(ValueError, match="predict_missing_cov_fits.*Predictor.predict"):
                call(torch.zeros((4, d), dtype=torch.float64), torch.ones((d, d, 4), dtype=torch.float64))
    for kw in ({"m": 256}, {"d": 10}, {"d": 2}, {"k": 8}):                                # the edges of the scope pass (and stop at the device)
        model = _model(method="GC", **kw)
        d = model.d
        p = gpz_amd.Predictor(model, force_tiles=True)
        for call in calls(p).values():
            with pytest.raises(ValueError, match="must be on cuda:0"):
                call(torch.zeros((4, d), dtype=torch.float64), torch.ones((d, d, 4), dtype=torch.float64))
    model = _model(method="VC")
    model.sets["best"]["priors"] = np.ones(5) / 5
    with pytest.raises(ValueError, match="priors of the set must be 6 values"):
        gpz_amd.Predictor(model).predict_psi_cube_missing_dev(X, good)
