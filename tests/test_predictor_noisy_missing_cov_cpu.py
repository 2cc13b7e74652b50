"""CPU-side checks of rows with input noise and missing inputs for the covariance kinds on the predictor handle
(Predictor.predict_noisy_missing_cov_dev / draws_noisy_missing_cov_dev, gpz_predictor_run_noisy_missing_cov_dev /
_draws_noisy_missing_cov_dev of the C ABI): the entries are declared, bound, exported and in the entry table, each with exactly its twin's
arguments; k_predict_noisy_missing_cov.hip compiles for gfx950 with every instantiation of the pair, Ex and PHI kernels free of scratch
and spills; the chunk rule is the missing_cov entries' own and the slab rule is theirs at this unit's record length; and every refusal of
the two methods fires before the GPU is touched."""
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
SRC = os.path.join(CSRC, "k_predict_noisy_missing_cov.hip")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")
ENTRIES = {"gpz_predictor_run_noisy_missing_cov_dev": "gpz_predictor_run_noisy_missing_dev",
           "gpz_predictor_draws_noisy_missing_cov_dev": "gpz_predictor_draws_noisy_missing_dev"}
SLAB_BYTES = 64 << 20
LDS_BYTES = 160 << 10
# the pair kernels DESIGN.md section 31 reports above 256 registers (one workgroup per compute unit, which LDS allows them anyway)
OVER_256 = {(8, 8), (9, 8)}


def rec_len(d, no):
    """predict_noisy_missing_cov_rec, stated a second time: [lnw | -j (no) | M (no (no + 1) / 2) | J (no no) | A2 (nu no) | b2 (nu)]."""
    return 1 + no + no * (no + 1) // 2 + no * no + (d - no) * (no + 1)


def slabs_rule(m, d, no):
    """predict_noisy_missing_cov_slabs, stated a second time: the smallest power of two S such that ceil(pairs / S) pairs of m records of
    rec_len(d, no) doubles are at most 64 MB."""
    npair, s = m * (m + 1) // 2, 1
    while -(-npair // s) * m * rec_len(d, no) * 8 > SLAB_BYTES:
        s *= 2
    return s


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
    assert E["run", "noisy_missing_cov"] == "gpz_predictor_run_noisy_missing_cov_dev"
    assert E["draws", "noisy_missing_cov"] == "gpz_predictor_draws_noisy_missing_cov_dev"
    assert E["run", "noisy_missing"] == "gpz_predictor_run_noisy_missing_dev" and E["run", "missing_cov"] == "gpz_predictor_run_missing_cov_dev"
    assert re.search(r'UNITS="[^"]*\bk_predict_noisy_missing_cov\b', open(os.path.join(ROOT, "build.sh")).read())
    kh = open(os.path.join(CSRC, "gpz_kernels.h")).read()
    for fn in ("predict_noisy_missing_cov_rec", "predict_noisy_missing_cov_slabs", "launch_pnmc_tables", "launch_pnmc_rows",
               "launch_predict_noisy_missing_cov_pairs", "launch_pmcv_hd"):
        assert re.search(r"\b" + fn + r"\(", kh), fn
    host = open(os.path.join(CSRC, "gpz_predictor.hip")).read()
    assert '"; noisy missing: k_predict_noisy_missing_cov_pairs (%d pair chunks)"' in host
    assert "ROWS_NOISY_MISSING_COV = 6" in open(os.path.join(CSRC, "gpz_predictor.h")).read()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_noisy_missing_cov_kernels_compiled_form(tmp_path):
    """The resource remarks only.  k_predict_noisy_missing_cov_pairs<NO, KM>, NO = 1 .. 9 x KM in {1, 8}, k_pnmc_ex<NO> and k_pnmc_phi<NO>:
    no scratch, no spill; registers printed, and VGPRs + AGPRs <= 256 asserted for all but the two pair kernels DESIGN.md names.  The
    generation kernels run their d x d temporaries through scratch memory on purpose (off the hot path): reported, not gated."""
    asm = tmp_path / "k_predict_noisy_missing_cov.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=1800)
    recs = _resource_records(r.stderr)
    pairs = {n: q for n, q in recs.items() if "k_predict_noisy_missing_cov_pairs" in n}
    assert len(pairs) == 18, sorted(pairs)
    seen = set()
    for name, q in sorted(pairs.items()):
        no, km = (int(v) for v in re.search(r"ILi(\d+)ELi(\d+)E", name).groups())
        seen.add((no, km))
        regs = q["VGPRs"] + q.get("AGPRs", 0)
        print(f"k_predict_noisy_missing_cov_pairs<{no}, {km}>: {regs} registers")
        assert q["ScratchSize [bytes/lane]"] == 0 and q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
        assert regs <= 512 and (regs <= 256 or (no, km) in OVER_256), (name, q)
        assert q["LDS Size [bytes/block]"] == 0, (name, q)                            # all of it dynamic: predict_noisy_missing_cov_lds
    assert seen == {(no, km) for no in range(1, 10) for km in (1, 8)}
    for kname in ("k_pnmc_ex", "k_pnmc_phi"):
        mine = {n: q for n, q in recs.items() if kname in n and "k_pnmc_phirec" not in n}
        assert len(mine) == 9, (kname, sorted(mine))
        for name, q in sorted(mine.items()):
            no = re.search(r"ILi(\d+)E", name).group(1)
            print(f"{kname}<{no}>: {q['VGPRs'] + q.get('AGPRs', 0)} registers")
            assert q["ScratchSize [bytes/lane]"] == 0 and q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)
            assert q["VGPRs"] + q.get("AGPRs", 0) <= 256, (name, q)
    for kname in ("k_pnmc_triples", "k_pnmc_basis", "k_pnmc_phirec"):                 # reported, not gated
        (name, q), = [(n, q) for n, q in recs.items() if kname in n]
        print(f"{kname}: {q['VGPRs']} VGPRs, {q['ScratchSize [bytes/lane]']} bytes of scratch per lane")
        assert q["SGPRs Spill"] == 0 and q["VGPRs Spill"] == 0, (name, q)


def test_chunks_slabs_and_lds_are_functions_of_the_model_and_the_pattern_alone():
    src = open(SRC).read()
    impl = open(os.path.join(CSRC, "k_predict_nmcov_impl.h")).read()                   # the launchers of both forms of Psi
    # the chunk rule: used by the pair launcher and the gamma launcher, not restated
    assert impl.count("nchunk != predict_missing_cov_chunks(m)") == 2 and "int predict_missing_cov_chunks(" not in src + impl
    # the slab rule and the one generation kernel: one loop, which the pair launcher and the gamma launcher both go through
    loop = re.search(r"static int nmcov_slabs\(.*?\n\}", impl, flags=re.S).group(0)
    assert "predict_noisy_missing_cov_slabs(m, d, pt.no)" in loop and "predict_noisy_missing_cov_slab_pairs(m, d, pt.no)" in loop
    assert "if (!(nslab == 1 && *slab_kept) && launch_pnmc_triples(st, d, obs, q0, cnt, m, raw, bas, slab)) return -1;" in loop
    assert "*slab_kept = nslab == 1;" in loop and impl.count("launch_pnmc_triples(st") == 1
    assert len(re.findall(r"\bnmcov_slabs\(st, pt, obs, m, raw, bas, slab, slab_kept, nchunk, a, launch\)", impl)) == 2
    assert ("int predict_noisy_missing_cov_rec(int d, int no) { return 1 + no + no * (no + 1) / 2 + no * no + (d - no) * (no + 1); }"
            in src)
    sbody = re.search(r"int predict_noisy_missing_cov_slabs\(int m, int d, int no\) \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "while (((npair + s - 1) / s) * per > PNMC_SLAB_BYTES) s *= 2;" in sbody
    assert "per = (long)m * predict_noisy_missing_cov_rec(d, no) * (long)sizeof(double)" in sbody
    assert re.search(r"#define PNMC_SLAB_BYTES \(64L << 20\)", src) and re.search(r"#define PNMC_SB 4\b", impl)
    assert "PNMC_SB" not in src.replace("4 * (size_t)PNMC_SB * predict_noisy_missing_cov_rec(d, no)", "")   # counted by the LDS figure alone
    assert re.search(r"#define PNMC_STD 2048\b", impl) and "predict_noisy_missing_cov_lds(m, d, pt.no, k)" in impl
    for word in ("n", "ns", "nt", "tile", "rows", "k"):
        assert not re.search(r"\b" + word + r"\b", sbody), word
    old = open(os.path.join(CSRC, "k_predict_missing_cov.hip")).read()                 # the records the other entries read keep their form
    assert "int predict_missing_cov_rec(int no) { return 1 + no + no * (no + 1) / 2; }" in old
    assert slabs_rule(100, 5, 4) == 4 and slabs_rule(250, 5, 4) > 1 and slabs_rule(7, 5, 4) == 1
    for d in range(2, 11):
        for no in range(1, d):
            assert rec_len(d, no) >= 1 + no + no * (no + 1) // 2 and rec_len(d, no) <= 2048 // 13   # whole records in a stage of the Ex kernel
            assert (256 * 64 + 4 * 4 * rec_len(d, no)) * 8 <= LDS_BYTES                  # the pair kernel's LDS at the widest model
            for m in (1, 100, 256):
                assert -(-(m * (m + 1) // 2) // slabs_rule(m, d, no)) * m * rec_len(d, no) * 8 <= SLAB_BYTES


def test_refusals_fire_before_the_gpu(monkeypatch):
    """Every TypeError / ValueError of the two methods is raised on the host: the library load is made to fail, so a call that got past
    the checks would raise RuntimeError instead.  Each refusal says where such rows go.  Type, dtype, shape, model, device last."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    X = torch.zeros((4, 3), dtype=torch.float64)
    Psi = torch.ones((4, 3), dtype=torch.float64)

    def calls(p):
        return {"predict": lambda x, psi, **kw: p.predict_noisy_missing_cov_dev(x, psi, **kw),
                "draws": lambda x, psi, **kw: p.draws_noisy_missing_cov_dev(x, psi, 4, **kw)}

    for method in ("VC", "GC"):
        for k in (1, 2):
            p = gpz_amd.Predictor(_model(k=k, method=method))
            for what, call in calls(p).items():
                with pytest.raises(TypeError, match=r"NumPy catalogue.*Predictor.predict\(X, Psi=Psi\)"):
                    call(np.zeros((4, 3)), Psi)
                with pytest.raises(TypeError, match="X must be a torch.Tensor"):
                    call([[0.0] * 3] * 4, Psi)
                with pytest.raises(TypeError, match="X must be float64 or float32"):
                    call(X.half(), Psi)
                with pytest.raises(ValueError, match="X must be n x 3"):
                    call(torch.zeros((4, 2), dtype=torch.float64), Psi)
                with pytest.raises(TypeError, match="selection must be a bool torch tensor"):
                    call(X, Psi, selection=np.ones(4, dtype=bool))
                with pytest.raises(ValueError, match=f"needs Psi.*{what}_missing_cov_dev"):
                    call(X, None)
                with pytest.raises(ValueError, match=r"full d x d x n Psi stays on Predictor.predict\(X, Psi=Psi\)"):
                    call(X, torch.ones((3, 3, 4), dtype=torch.float64))
                with pytest.raises(TypeError, match="Psi as a torch tensor"):
                    call(X, np.ones((4, 3)))
                with pytest.raises(TypeError, match="Psi must be float64 or float32"):
                    call(X, Psi.long())
                with pytest.raises(ValueError, match="Psi must be n x d, n x 1 or n"):
                    call(X, torch.ones((4, 2), dtype=torch.float64))
                for okx, okp in ((X, Psi), (X.float(), Psi[:, :1]), (X.T.contiguous().T, Psi[:, 0]), (X[::2], Psi[::2].float())):
                    with pytest.raises(ValueError, match="must be on cuda:0"):   # the device, last
                        call(okx, okp)
            with pytest.raises(ValueError, match="n_draws"):
                p.draws_noisy_missing_cov_dev(X, Psi, 0)
            p.close()
            with pytest.raises(RuntimeError, match="closed"):
                p.predict_noisy_missing_cov_dev(X, Psi)
    # a diagonal kind is sent to its own methods, which keep refusing the covariance kinds with the texts they have
    for method in ("GL", "VL", "GD", "VD"):
        p = gpz_amd.Predictor(_model(method=method))
        with pytest.raises(ValueError, match=r"diagonal kind.*predict_noisy_missing_dev\(X, Psi\)"):
            p.predict_noisy_missing_cov_dev(X, Psi)
        with pytest.raises(ValueError, match=r"diagonal kind.*draws_noisy_missing_dev\(X, Psi\)"):
            p.draws_noisy_missing_cov_dev(X, Psi, 4)
    for method in ("GC", "VC"):
        p = gpz_amd.Predictor(_model(method=method))
        with pytest.raises(ValueError, match=r"predict_missing_fits: a diagonal kind.*Predictor.predict takes rows with missing values"):
            p.predict_noisy_missing_dev(X, Psi)
        with pytest.raises(ValueError, match=r"does not take Psi.*Predictor.predict\(X, Psi=Psi\)"):
            p.predict_missing_cov_dev(X, Psi=Psi)
        with pytest.raises(ValueError, match=r"does not take Psi.*Predictor.predict\(X, Psi=Psi\)"):
            p.draws_missing_cov_dev(X, 4, Psi=Psi)
    # shapes outside predict_missing_cov_fits
    for kw in ({"d": 11}, {"k": 9}, {"m": 257}):
        model = _model(method="VC", **kw)
        p = gpz_amd.Predictor(model)
        Xd, Pd = torch.zeros((4, model.d), dtype=torch.float64), torch.ones((4, model.d), dtype=torch.float64)
        with pytest.raises(ValueError, match="predict_missing_cov_fits.*Predictor.predict"):
            p.predict_noisy_missing_cov_dev(Xd, Pd)
        with pytest.raises(ValueError, match="predict_missing_cov_fits.*Predictor.predict"):
            p.draws_noisy_missing_cov_dev(Xd, Pd, 4)
    # the edges of the scope pass the shape check (and then stop at the device)
    for kw in ({"m": 256}, {"d": 10}, {"d": 1}, {"k": 8}):
        model = _model(method="GC", **kw)
        p = gpz_amd.Predictor(model, force_tiles=True)                                    # (no route is refused)
        with pytest.raises(ValueError, match="must be on cuda:0"):
            p.draws_noisy_missing_cov_dev(torch.zeros((4, model.d), dtype=torch.float64), torch.ones((4, model.d), dtype=torch.float64), 4)
    # priors of the wrong length
    model = _model(method="VC")
    model.sets["best"]["priors"] = np.ones(5) / 5
    with pytest.raises(ValueError, match="priors of the set must be 6 values"):
        gpz_amd.Predictor(model).predict_noisy_missing_cov_dev(X, Psi)
