"""CPU-side checks of the stacks of rows with input noise and missing inputs and of gamma under every weight draw
(Predictor.stack_noisy_missing_dev, draws_noisy_missing_dev(..., return_gamma=True); gpz_predictor_stack_noisy_missing_dev /
_draws_gamma_noisy_missing_dev): the definition of gamma_s as a quadratic form of the draw's weights, stated with the NumPy oracle alone;
the declarations against the binding, the library and build.sh; the calls the methods make on the library, recorded behind the stand-in of
test_predictor_calls_cpu.py, and their refusals in order; the compiled form of k_predict_noisy_missing_gamma.hip and its LDS rule."""
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
import test_predictor_calls_cpu as calls
from test_predictor import catalogue, synth_model
from test_predictor_calls_cpu import CODES, D, EDGES, LABELS, N, SEL, raises, rig, run, _rows   # noqa: F401  (rig is a fixture)
from test_predictor_stack_missing_cpu import _resource_records
from test_predictor_stack_noisy import noise, with_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
SRC = os.path.join(CSRC, "k_predict_noisy_missing_gamma.hip")
LAUNCH = os.path.join(CSRC, "k_predict_missing_gamma.hip")         # the gamma launcher and the LDS rule, with and without Psi
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
NB_MAX = 8                                                                # column blocks per launch
GAMMA, STACK = "gpz_predictor_draws_gamma_noisy_missing_dev", "gpz_predictor_stack_noisy_missing_dev"

# where include/gpz_hip.h puts the arguments of the two entries (the stand-in checks the vectors behind the pointers there)
calls.POS.setdefault(GAMMA, dict(rows=3, muX=10, sdX=11, sd2=12, muY=13, priors=14, mask=15, n_draws=16, seed=17, out=19, gam=20,
                                 stream=21))
calls.POS.setdefault(STACK, dict(rows=3, muX=10, sdX=11, sd2=12, priors=13, mask=14, n_draws=15, seed=16, bins=19, groups=21, out=23,
                                 muY=27, stream=28))
calls.POS.setdefault("gpz_predictor_draws_noisy_missing_dev",
                     dict(rows=3, muX=10, sdX=11, sd2=12, muY=13, priors=14, mask=15, n_draws=16, seed=17, out=19, stream=20))


# ---- the definition ------------------------------------------------------------------------------------------------------------------------
def test_gamma_per_draw_is_a_quadratic_form_of_the_draws_weights():
    """gamma_s + mu_s^2 = sum_{a >= b} f_ab EcC_ab(x, psi) w_s,a w_s,b is a quadratic form w_s' E w_s whose matrix E(x, psi) does not
    depend on w.  The oracle does not expose the pair expectations, so E is recovered from ``O.predict_any(X, model, Psi=Psi)`` through
    ``with_weights`` by polarisation (E_aa from w = e_a, E_ab from w = e_a + e_b), and the form under a draw's weights must reproduce the
    oracle's gamma of the w := w_s model at rel <= 1e-8: the definition, fixed without any kernel.  m = 6, d = 3, k = 2, three patterns
    with missing values, among them nothing observed, and complete rows, whose gamma is the input noise's and not zero."""
    m, d, k, n = 6, 3, 2, 12
    model = synth_model("VD", m, d, k, True, seed=23)
    model.sets["best"]["priors"] = np.random.default_rng(24).dirichlet(np.full(m, 2.0))
    X = catalogue(model, n, seed=25)
    Psi = noise(n, d, seed=26)
    X[0:4, 1] = np.nan
    X[4:8, 0] = X[4:8, 2] = np.nan
    X[8:10, :] = np.nan                                                    # rows 10, 11 stay complete
    muY = np.asarray(model.muY).reshape(-1)

    def second_moment(w):
        out = O.predict_any(X, with_weights(model, w), Psi=Psi)
        return out[4] + (out[0] - muY) ** 2                                # gamma + mu^2, (n, k)

    eye = np.eye(m)
    E = np.zeros((n, k, m, m))
    for a in range(m):
        E[:, :, a, a] = second_moment(np.repeat(eye[:, a:a + 1], k, axis=1))
    for a in range(m):
        for b in range(a):
            both = second_moment(np.repeat((eye[:, a] + eye[:, b])[:, None], k, axis=1))
            E[:, :, a, b] = E[:, :, b, a] = 0.5 * (both - E[:, :, a, a] - E[:, :, b, b])
    rng = np.random.default_rng(27)
    for s in range(3):
        ws = model.sets["best"]["w"] + 0.3 * rng.standard_normal((m, k))
        out = O.predict_any(X, with_weights(model, ws), Psi=Psi)
        mu_s = out[0] - muY
        tri = sum((1.0 if a == b else 2.0) * E[:, :, a, b] * ws[a] * ws[b] for a in range(m) for b in range(a + 1))
        gamma_s = tri - mu_s ** 2
        assert rel(gamma_s, out[4]) <= 1e-8, (s, rel(gamma_s, out[4]))
        assert np.all(out[4] > 0.0)                                        # the complete rows too: the variance over their input noise


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_binding_library_and_build_agree_on_the_new_entries():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()

    def decl(name):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
        assert m, f"{name} is not declared in gpz_hip.h"
        return [a.strip() for a in m.group(1).split(",")]
    for name, nargs in ((GAMMA, 22), (STACK, 29)):
        assert len(decl(name)) == nargs, (name, decl(name))
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert calls.POS[name]["stream"] == nargs - 1
    # the draws of such a group + Gam_d between F_d and the stream
    old, new = decl("gpz_predictor_draws_noisy_missing_dev"), decl(GAMMA)
    assert new[:-2] == old[:-1] and new[-3] == "double *F_d" and new[-2] == "double *Gam_d" and new[-1] == old[-1] == "void *stream"
    so, sn = _lib.SYMBOLS["gpz_predictor_draws_noisy_missing_dev"][1], _lib.SYMBOLS[GAMMA][1]
    assert sn[:-2] == so[:-1] and sn[-2:] == [_lib.C.c_void_p, _lib.C.c_void_p]
    # the noisy stack + the priors and the mask behind sd2 (no muY in a stack's prefix), as the missing stack has them behind sdX
    old, new = decl("gpz_predictor_stack_noisy_dev"), decl(STACK)
    assert new[:13] == old[:13] and new[12] == "const double *sd2"
    assert new[13:15] == ["const double *priors", "uint32_t obs_mask"] and new[15:] == old[13:]
    so, sn = _lib.SYMBOLS["gpz_predictor_stack_noisy_dev"][1], _lib.SYMBOLS[STACK][1]
    assert sn[:13] == so[:13] and sn[13:15] == [_lib.c_double_p, _lib.C.c_uint32] and sn[15:] == so[13:]
    assert decl("gpz_predictor_stack_missing_dev")[8:] == new[13:]
    full = open(HEADER).read()
    assert "noisy missing: k_predict_noisy_missing_pairs (C pair chunks)" in full
    assert "noisy missing per draw: k_predict_noisy_missing_gamma (C pair chunks)" in full and "No stack, no gamma per draw" not in full
    build = open(os.path.join(ROOT, "build.sh")).read()
    assert re.search(r'UNITS="[^"]*\bk_predict_noisy_missing_gamma\b', build)
    kh = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    assert "int launch_predict_missing_gamma(hipStream_t st, const double *Xc, const double *Psic," in kh
    assert "size_t predict_missing_gamma_lds(int m, int d, bool psi);" in kh
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert "; noisy missing per draw: k_predict_noisy_missing_gamma (%d pair chunks)" in host
    assert "are not there for rows with input noise and missing inputs" not in host
    assert ("draws_gamma", "noisy_missing") in gpz_amd.predictor._DEV_ENTRIES and ("stack", "noisy_missing") in gpz_amd.predictor._DEV_ENTRIES


# ---- the calls the methods make ------------------------------------------------------------------------------------------------------------
def test_methods_reach_their_entries(rig):
    """Complete rows reach the _noisy_dev entries (gamma of complete rows is the input noise's: an entry, not zeros); every other group
    the new entry once, in ascending code order (0, 4, 6, 7), with the mask 7 & ~code and its gathered Psi; the stand-in checks the
    priors, sd2 and the other vectors at the header's positions and the binding's types."""
    p, rec, lookups = rig
    Xc, Xn = torch.from_numpy(_rows([0] * N)), torch.from_numpy(_rows())
    Psi, sel = (0.01 * torch.arange(1, N + 1, dtype=torch.float64))[:, None].repeat(1, D), torch.from_numpy(SEL)   # told apart by value
    lab, wt = torch.from_numpy(LABELS), torch.ones(N)
    seen = []
    orig = p._psi_args

    def psi_args(P, n):
        seen.append(P[:, 0].tolist())
        return orig(P, n)
    p._psi_args = psi_args
    want = [[i for i, c in enumerate(CODES) if c == code] for code in (0, 4, 6, 7)]
    nd = dict(n_draws=3, seed=5)
    F, Gam = p.draws_noisy_missing_dev(Xn, Psi, 3, seed=5, return_gamma=True)
    assert rec.take() == [run("gpz_predictor_draws_gamma_noisy_dev", 3, **nd), run(GAMMA, 3, mask=3, **nd), run(GAMMA, 2, mask=1, **nd),
                          run(GAMMA, 2, mask=0, **nd)]
    assert F.data_ptr() not in rec.out[-4:] and Gam.data_ptr() not in rec.gam[-4:] and None not in rec.gam[-4:]
    assert tuple(F.shape) == tuple(Gam.shape) == (3, N, p._k)
    assert seen == [Psi[idx, 0].tolist() for idx in want]                  # the gathered Psi of each group, in its rows' order
    del seen[:]
    p.draws_noisy_missing_dev(Xn, Psi[:, 1], 3, seed=5, selection=sel, return_gamma=True)   # codes 0, 4, 0, 6, 4, 7 stay
    assert rec.take() == [run("gpz_predictor_draws_gamma_noisy_dev", 2, **nd), run(GAMMA, 2, mask=3, **nd), run(GAMMA, 1, mask=1, **nd),
                          run(GAMMA, 1, mask=0, **nd)]
    F = p.draws_noisy_missing_dev(Xn, Psi, 3, seed=5)                      # without the keyword: the call as it was
    assert [c[0] for c in rec.take()] == ["gpz_predictor_draws_noisy_dev"] + ["gpz_predictor_draws_noisy_missing_dev"] * 3
    assert len(lookups) == 3                                               # one stream lookup per Python call, however many groups
    del seen[:]
    # the stack: n_groups over all rows (label 2 sits on one row of the last pattern), the parts in ascending code order
    st = dict(n_draws=2, seed=7, bins=4)
    r = p.stack_noisy_missing_dev(Xn, Psi, EDGES, n_draws=2, seed=7, groups=lab, weights=wt)
    assert rec.take() == [run("gpz_predictor_stack_noisy_dev", 3, groups=3, **st), run(STACK, 3, mask=3, groups=3, **st),
                          run(STACK, 2, mask=1, groups=3, **st), run(STACK, 2, mask=0, groups=3, **st)]
    assert r.hist.ctypes.data not in rec.out[-4:] and r.hist.shape == (3, 3, p._k, 4)
    assert seen == [Psi[idx, 0].tolist() for idx in want]
    p.stack_noisy_missing_dev(Xn, Psi[:, :1], EDGES, n_draws=2, seed=7, groups=lab, selection=sel)   # label 2 is outside the selection
    assert rec.take() == [run("gpz_predictor_stack_noisy_dev", 2, groups=2, **st), run(STACK, 2, mask=3, groups=2, **st),
                          run(STACK, 1, mask=1, groups=2, **st), run(STACK, 1, mask=0, groups=2, **st)]
    assert len(lookups) == 5
    # one pattern: the whole call, on the caller's own arrays
    F, Gam = p.draws_noisy_missing_dev(Xc, Psi, 3, seed=5, return_gamma=True)
    assert rec.take() == [run("gpz_predictor_draws_gamma_noisy_dev", 10, **nd)]
    assert (rec.out[-1], rec.gam[-1]) == (F.data_ptr(), Gam.data_ptr())
    F, Gam = p.draws_noisy_missing_dev(torch.from_numpy(_rows([7] * N)), Psi.float(), 3, seed=5, return_gamma=True)
    assert rec.take() == [run(GAMMA, 10, mask=0, **nd)] and (rec.out[-1], rec.gam[-1]) == (F.data_ptr(), Gam.data_ptr())
    r = p.stack_noisy_missing_dev(Xc, Psi, EDGES, n_draws=2, seed=7, weights=wt)
    assert rec.take() == [run("gpz_predictor_stack_noisy_dev", 10, groups=1, **st)] and rec.out[-1] == r.hist.ctypes.data
    r = p.stack_noisy_missing_dev(torch.from_numpy(_rows([4] * N)), Psi[:, 0], EDGES, n_draws=2, seed=7)
    assert rec.take() == [run(STACK, 10, mask=3, groups=1, **st)] and rec.out[-1] == r.hist.ctypes.data
    # no rows: no entry
    none = torch.zeros(N, dtype=torch.bool)
    assert tuple(p.draws_noisy_missing_dev(Xn, Psi, 3, selection=none, return_gamma=True)[1].shape) == (3, 0, p._k)
    assert not p.stack_noisy_missing_dev(Xn, Psi, EDGES, n_draws=2, selection=none).hist.any()
    assert rec.take() == [] and rec.created == 1


def test_methods_refuse_in_order_before_the_gpu(monkeypatch):
    """stack_noisy_missing_dev with two things wrong at once: the text of the first.  Order: X and Psi by type, dtype and shape, the
    model's shape, the priors, the draws route of the complete rows (_check_noisy_missing's), then stack_dev's own ladder, the device
    last.  The library load is made to fail, so a call that got past the checks would raise RuntimeError.  draws_dev keeps refusing
    Psi with missing=True, with its text."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    mk = calls._model
    p, pt = gpz_amd.Predictor(mk()), gpz_amd.Predictor(mk(), force_tiles=True)
    pc, pm = gpz_amd.Predictor(mk(method="GC")), gpz_amd.Predictor(mk(m=257))
    pp = gpz_amd.Predictor(mk(priors=np.ones(5) / 5))
    X = _rows([0, 0, 0, 4, 0, 0, 0, 0])
    T, Tp = torch.from_numpy(X), torch.full((8, D), 0.01, dtype=torch.float64)
    ints, ones = torch.zeros(8, dtype=torch.int64), torch.ones(8)
    with raises(TypeError, "stack_dev takes a torch tensor on cuda:0; a NumPy array goes to Predictor.stack"):
        pm.stack_noisy_missing_dev(X, None, [0.0])
    with raises(ValueError, "X must be n x 3, got shape (8, 2)"):
        pm.stack_noisy_missing_dev(T[:, :2], None, [0.0])
    with raises(TypeError, "selection must be a bool torch tensor on the same device as X"):
        pm.stack_noisy_missing_dev(T, None, [0.0], selection=ones)
    with raises(ValueError, "stack_noisy_missing_dev needs Psi: rows without input noise go to stack_missing_dev"):
        pm.stack_noisy_missing_dev(T, None, [0.0])
    with raises(TypeError, "stack_dev takes Psi as a torch tensor on cuda:0; a NumPy array goes to Predictor.stack"):
        pm.stack_noisy_missing_dev(T, Tp.numpy(), [0.0])
    with raises(TypeError, "Psi must be float64 or float32"):
        pm.stack_noisy_missing_dev(T, Tp.long(), [0.0])
    with raises(ValueError, "Psi must be n x d, n x 1 or n (n = 8, d = 3), got shape (8, 2)"):
        pm.stack_noisy_missing_dev(T, Tp[:, :2], [0.0])
    with raises(ValueError, "stack_noisy_missing_dev needs a model inside predict_missing_fits: m <= 256, not m = 257"):
        pm.stack_noisy_missing_dev(T, Tp, [0.0])
    with raises(ValueError, "stack_noisy_missing_dev needs a model inside predict_missing_fits: a diagonal kind"):
        pc.stack_noisy_missing_dev(T, Tp, [0.0])
    with raises(ValueError, "the priors of the set must be 6 values, got 5"):
        pp.stack_noisy_missing_dev(T, Tp, [0.0])
    with raises(ValueError, "stack_noisy_missing_dev needs the fused draws route for its complete rows"):
        pt.stack_noisy_missing_dev(T, Tp, [0.0])
    with raises(ValueError, "edges must be a vector of at least 2 values, got shape (1,)"):
        p.stack_noisy_missing_dev(T, Tp, [0.0], n_draws=-1)
    with raises(ValueError, "n_draws must be a non-negative integer, got -1"):
        p.stack_noisy_missing_dev(T, Tp, [0.0, 1.0], n_draws=-1, groups=ones)
    with raises(ValueError, "groups must be a tensor of 8 integer labels"):
        p.stack_noisy_missing_dev(T, Tp, [0.0, 1.0], groups=ones, weights=ints)
    with raises(ValueError, "weights must be a float tensor of 8 values"):
        p.stack_noisy_missing_dev(T, Tp, [0.0, 1.0], weights=ints, n_groups=0)
    with raises(ValueError, "n_groups must be a positive integer, got 0"):
        p.stack_noisy_missing_dev(T, Tp, np.arange(4098.0), n_groups=0)
    with raises(ValueError, "n_groups * bins = 8194 is over the limit of 4096 per call"):
        p.stack_noisy_missing_dev(T, Tp, np.arange(4098.0), n_groups=2)
    for psi in (Tp, Tp[:, :1], Tp[:, 0], Tp.float()):
        with raises(ValueError, "X must be on cuda:0, it is on cpu: the host methods take host arrays"):
            p.stack_noisy_missing_dev(T, psi, [0.0, 1.0], n_draws=2, groups=ints, weights=ones)
    # return_gamma: the draws method's own ladder, unchanged by the keyword
    with raises(ValueError, "draws_noisy_missing_dev needs a model inside predict_missing_fits: m <= 256, not m = 257"):
        pm.draws_noisy_missing_dev(T, Tp, 0, return_gamma=True)
    with raises(ValueError, "draws_noisy_missing_dev needs the fused draws route for its complete rows"):
        pt.draws_noisy_missing_dev(T, Tp, 0, return_gamma=True)
    with raises(ValueError, "n_draws must be a positive integer, got 0"):
        p.draws_noisy_missing_dev(T, Tp, 0, return_gamma=True)
    with raises(ValueError, "X must be on cuda:0, it is on cpu: the host methods take host arrays"):
        p.draws_noisy_missing_dev(T, Tp, 3, return_gamma=True)
    # the old spelling keeps its refusals and their texts
    with raises(ValueError, "return_gamma=True needs Psi or missing=True, and not both: gamma under a draw is the variance over the "
                            "input noise or over the missing dimensions"):
        p.draws_dev(T, 3, Psi=Tp, missing=True, return_gamma=True)
    with pytest.raises(ValueError, match="missing=True does not take Psi.*predict_noisy_missing_dev / draws_noisy_missing_dev"):
        p.draws_dev(T, 3, Psi=Tp, missing=True)
    with pytest.raises(TypeError, match="missing"):                       # stack_noisy_dev has no such keyword: the method is the entry
        p.stack_noisy_dev(T, Tp, [0.0, 1.0], missing=True)
    p.close()
    with pytest.raises(RuntimeError, match="closed"):
        p.stack_noisy_missing_dev(T, Tp, [0.0, 1.0])


# ---- the compiled form ---------------------------------------------------------------------------------------------------------------------
def gamma_lds_rule(m, d):
    """predict_missing_gamma_lds with psi (k_predict_missing_gamma.hip) and DESIGN.md section 23, stated a second time on purpose: the
    Pio block of 32 rows (row stride ceil16(m) + 2), [lnZ | c | C] of the 64 pairs of a group, the block's rows of X and of Psi, (a, b) of
    the 64 pairs as 128 ints; at least the 4 x 32 x 16 doubles of the last reduction, one column block at a time."""
    nk = (m + 15) // 16 * 16
    return 8 * max(32 * (nk + 2) + 64 * (1 + 2 * d) + 64 * d + 64, 4 * 32 * 16)


def test_lds_rule_at_the_three_shapes():
    assert gamma_lds_rule(100, 5) == 37_888 and 2 * gamma_lds_rule(100, 5) <= 160 * 1024   # two workgroups per compute unit
    assert gamma_lds_rule(256, 20) == 97_792 and gamma_lds_rule(256, 20) <= 160 * 1024     # one, opted in per launch
    assert gamma_lds_rule(1, 1) == 16_384
    src = open(LAUNCH).read()
    body = re.search(r"size_t predict_missing_gamma_lds\(int m, int d, bool psi\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "psi ? 32 * (nk + 2) + 64 * (1 + 2 * (size_t)d) + 64 * (size_t)d + 64\n" in body and "red = 4 * 32 * 16" in body
    impl = open(os.path.join(CSRC, "k_predict_group_impl.h")).read()      # the helper that launches the four kernels
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in impl and "launch_predict_group<k_predict_noisy_missing_gamma<NBT>>" in src
    assert "nchunk != predict_missing_chunks(m)" in src
    assert f"#define GPZ_MGAMMA_NB {NB_MAX}" in src                         # one count for the kernels with and without Psi
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "32 (nk + 2) + 64 (1 + 2 d) + 64 d + 64" in design


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_noisy_missing_gamma_kernel_compiled_form(tmp_path):
    """k_predict_noisy_missing_gamma<NB>, NB = 1 .. NB_MAX column blocks: no scratch, no spilled register, VGPRs + AGPRs <= 256 (two
    workgroups of 256 per compute unit), no static LDS (all of it is the dynamic block of predict_missing_gamma_lds), the f64
    MFMA, no atomic of any kind and no other kernel in the unit."""
    asm = tmp_path / "k_predict_noisy_missing_gamma.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    assert len(recs) == NB_MAX and all("k_predict_noisy_missing_gamma" in n for n in recs), sorted(recs)
    assert sorted(int(re.search(r"ILi(\d+)E", n).group(1)) for n in recs) == list(range(1, NB_MAX + 1))
    for name, q in recs.items():
        print(name, q)
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
        assert q["LDS Size [bytes/block]"] == 0, (name, q)
    text = asm.read_text()
    assert "v_mfma_f64_16x16x4" in text
    for word in ("global_atomic", "flat_atomic", "ds_add_f", "ds_add_rtn_f", "cmpswap", "scratch_"):
        assert word not in text, word
