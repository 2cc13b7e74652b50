"""CPU-side checks of the streaming predictor (gpz_amd.Predictor, gpz_predictor_* of the C ABI): the fused kernel's compiled form (no
scratch traffic in a basic block that issues MFMAs; registers and LDS that leave room for two workgroups per compute unit) and the
argument checks that must fire before the GPU is touched."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gpz_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gpz_amd", "csrc", "k_predict_small.hip")


def _compile(tmp_path, extra=()):
    asm = tmp_path / "k_predict_small.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "gpz_amd", "csrc"), "-S", "--cuda-device-only", *extra, SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=900)
    return asm.read_text().splitlines(), r.stderr


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_no_scratch_traffic_inside_the_fused_predict_kernel(tmp_path):
    lines, _ = _compile(tmp_path)
    kernel = block = None
    nmfma = nscratch = 0
    bad, seen = [], set()

    def close():
        if kernel and nmfma and nscratch:
            bad.append((kernel, block, nmfma, nscratch))

    for l in lines:
        m = re.match(r"^(_Z\w*k_predict_small\w*):", l)
        if m:
            close()
            kernel, block, nmfma, nscratch = m.group(1), "entry", 0, 0
            seen.add(kernel)
            continue
        if kernel is None:
            continue
        if l.startswith(".Lfunc_end"):
            close()
            kernel = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            close()
            block, nmfma, nscratch = m.group(1), 0, 0
            continue
        t = l.strip()
        if t.startswith("v_mfma"):
            nmfma += 1
        elif t.startswith("scratch_"):
            nscratch += 1
    assert len(seen) == 22, sorted(seen)          # 11 input widths x {diagonal, covariance} kinds
    assert not bad, bad


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_fused_predict_kernel_leaves_room_for_two_workgroups_per_cu(tmp_path):
    """Two workgroups of 256 lanes per compute unit: at most 80 KB of LDS each (static + the dynamic block the launcher asks for,
    160 KB per CU) and at most 256 vector registers per lane (eight waves on four SIMDs)."""
    _, err = _compile(tmp_path, ("-Rpass-analysis=kernel-resource-usage",))
    src = open(SRC).read()
    lda = int(re.search(r"#define PS_LDA (\d+)", src).group(1))
    recs, cur = {}, None
    for l in err.splitlines():
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = m.group(1)
            recs[cur] = {}
            continue
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", l)
        if m and cur:
            recs[cur][m.group(1)] = int(m.group(2))
    ks = {k: v for k, v in recs.items() if "k_predict_small" in k}
    assert len(ks) == 22, sorted(recs)
    for name, r in ks.items():
        d = int(re.search(r"ILi(\d+)E", name).group(1))
        dynamic = (32 * lda + 32 * d + 4 * 32) * 8                    # predict_small_lds(d)
        assert r["LDS Size [bytes/block]"] + dynamic <= 80 * 1024, (name, r, dynamic)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 256, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)


def _model(method="VD", d=3, m=6, k=1):
    model = gpz_amd.Model(m=m, d=d, k=k, method=method)
    p = m * d + model.g_dim + m * k + k + 2 * m * k
    model.sets["best"] = {"theta": np.zeros(p), "w": np.zeros((m, k)), "iSigma_w": np.eye(m)}
    return model


def test_predictor_validates_before_the_gpu():
    """Wrong widths, Psi shapes and set names are ValueErrors raised on the host, with no GPU call (this holds on a machine without
    one: the handle is only created once the inputs have passed)."""
    model = _model()
    p = gpz_amd.Predictor(model)
    with pytest.raises(ValueError):
        p.predict(np.zeros((4, 2)))                          # d = 3
    with pytest.raises(ValueError):
        p.predict(np.zeros((4, 3)), Psi=np.zeros((5, 3)))    # Psi rows != X rows
    with pytest.raises(ValueError):
        p.predict(np.zeros((4, 3)), Psi=np.zeros((3, 3, 3)))
    with pytest.raises(ValueError):
        p.predict(np.zeros((4, 3)), selection=np.ones(5, dtype=bool))
    with pytest.raises(ValueError):
        gpz_amd.Predictor(model, whichSet="last")
    with pytest.raises(ValueError):
        gpz_amd.Predictor(model, tile_rows=0)
    bad = _model()
    bad.sets["best"]["theta"] = np.zeros(5)
    with pytest.raises(ValueError):
        gpz_amd.Predictor(bad)
    p.close()
    with pytest.raises(RuntimeError):
        p.predict(np.zeros((4, 3)))
