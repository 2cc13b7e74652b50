"""CPU-side checks of the posterior draws (gpz_amd.Predictor.draws, gpz_predictor_draws): a NumPy Philox4x32-10 with the library's
normal mapping against Random123's known answers and the normal moments, the argument checks that must fire before any GPU call, and the
compiled form of k_predict_draws (MFMAs, no scratch traffic in a basic block that issues them, LDS and registers for two workgroups per
compute unit).  The GPU tests (test_predictor_draws.py) take philox4x32 / philox_normals from here."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gpz_amd
from gpz_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gpz_amd", "csrc", "k_predict_draws.hip")

M32 = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Random123's round and key schedule) on arrays of uint32 counters, one key."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & M32
            k1 = (k1 + np.uint64(0xBB67AE85)) & M32
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return c


def normals_of(x):
    """z = sqrt(-2 ln u1) cos(2 pi u2), u1 = (((x1 << 32 | x0) >> 11) + 1) 2^-53, u2 = ((x3 << 32 | x2) >> 11) 2^-53."""
    x0, x1, x2, x3 = x
    u1 = ((((x1 << np.uint64(32)) | x0) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (((x3 << np.uint64(32)) | x2) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def philox_normals(seed, m, n_draws, k):
    """The library's z[j, s, o] for seed (m x n_draws x k): counter (j, s, o, 0), key (seed & 0xffffffff, seed >> 32)."""
    j, s, o = np.meshgrid(np.arange(m), np.arange(n_draws), np.arange(k), indexing="ij")
    x = philox4x32(j.ravel(), s.ravel(), o.ravel(), np.zeros(j.size, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)
    return normals_of(x).reshape(m, n_draws, k)


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = philox4x32(*[np.array([v], dtype=np.uint64) for v in ctr], *key)
    assert tuple(int(v[0]) for v in got) == want


def test_normal_mapping_moments():
    """1e6 normals of one seed: mean, variance, skew and excess kurtosis within 5 standard errors of N(0, 1)'s."""
    z = philox_normals(12345, 1000, 1000, 1).ravel()
    n = z.size
    mean, var = z.mean(), z.var()
    c = z - mean
    skew = (c ** 3).mean() / var ** 1.5
    kurt = (c ** 4).mean() / var ** 2 - 3.0
    assert abs(mean) < 5 / np.sqrt(n), mean
    assert abs(var - 1) < 5 * np.sqrt(2 / n), var
    assert abs(skew) < 5 * np.sqrt(6 / n), skew
    assert abs(kurt) < 5 * np.sqrt(24 / n), kurt
    assert np.all(np.isfinite(z))
    # draw s of a seed is the same for any n_draws > s, and a different seed gives other values
    assert np.array_equal(philox_normals(7, 5, 3, 2), philox_normals(7, 5, 8, 2)[:, :3])
    assert not np.array_equal(philox_normals(7, 5, 3, 2), philox_normals(8, 5, 3, 2))


def _model(d=3, m=6, k=1):
    model = gpz_amd.Model(m=m, d=d, k=k, method="VD")
    p = m * d + model.g_dim + m * k + k + 2 * m * k
    model.sets["best"] = {"theta": np.zeros(p), "w": np.zeros((m, k)), "iSigma_w": np.stack([np.eye(m)] * k, axis=2)}
    return model


def test_draws_validates_before_the_gpu(monkeypatch):
    """Every ValueError of Predictor.draws is raised on the host: the library load is made to fail, so a call that got past the checks
    would raise RuntimeError instead."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    X = np.zeros((4, 3))
    for model, k in ((_model(), 1), (_model(k=2), 2)):
        p = gpz_amd.Predictor(model)
        with pytest.raises(ValueError, match="X must be"):
            p.draws(np.zeros((4, 2)), 4)                                 # d = 3
        Xn = X.copy()
        Xn[[1, 3], 2] = np.nan
        with pytest.raises(ValueError, match="2 rows"):
            p.draws(Xn, 4)
        for bad in (0, -1, 2.5, True, "4", None):
            with pytest.raises(ValueError, match="n_draws"):
                p.draws(X, bad)
        with pytest.raises(ValueError, match="limit"):
            p.draws(X, 16384 // k + 1)
        for bad in (-1, 2 ** 64, 1.5, True):
            with pytest.raises(ValueError, match="seed"):
                p.draws(X, 4, seed=bad)
        with pytest.raises(ValueError, match="Z must"):
            p.draws(X, 4, Z=np.zeros((6, 5, k)))
        with pytest.raises(ValueError, match="Z must"):
            p.draws(X, 4, Z=np.zeros((5, 4, k)))
        if k == 2:
            with pytest.raises(ValueError, match="Z must"):
                p.draws(X, 4, Z=np.zeros((6, 4)))                        # (m, n_draws) only when k = 1
        with pytest.raises(ValueError, match="selection"):
            p.draws(X, 4, selection=np.ones(5, dtype=bool))
        with pytest.raises(RuntimeError, match="disabled"):              # past every check: the first GPU call
            p.draws(X, 4, seed=2 ** 64 - 1, Z=np.zeros((6, 4, k)))
        p.close()
        with pytest.raises(RuntimeError, match="closed"):
            p.draws(X, 4)


def _compile(tmp_path, extra=()):
    asm = tmp_path / "k_predict_draws.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "gpz_amd", "csrc"), "-S", "--cuda-device-only", *extra, SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=900)
    return asm.read_text().splitlines(), r.stderr


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_draws_kernel_issues_mfma_without_scratch_in_its_blocks(tmp_path):
    lines, _ = _compile(tmp_path)
    kernel = block = None
    nmfma = nscratch = 0
    bad, seen, total = [], set(), {}

    def close():
        if kernel and nmfma and nscratch:
            bad.append((kernel, block, nmfma, nscratch))

    for l in lines:
        m = re.match(r"^(_Z\w*k_predict_draws\w*):", l)
        if m:
            close()
            kernel, block, nmfma, nscratch = m.group(1), "entry", 0, 0
            seen.add(kernel)
            total[kernel] = 0
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
        if t.startswith("v_mfma_f64_16x16x4"):
            nmfma += 1
            total[kernel] += 1
        elif t.startswith("scratch_"):
            nscratch += 1
    assert len(seen) == 22, sorted(seen)          # 11 input widths x {diagonal, covariance} kinds
    assert all(v > 0 for v in total.values()), total
    assert not bad, bad


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_draws_kernel_leaves_room_for_two_workgroups_per_cu(tmp_path):
    """At most 80 KB of LDS per workgroup (static + the dynamic block of predict_draws_lds) and at most 256 vector registers per lane."""
    _, err = _compile(tmp_path, ("-Rpass-analysis=kernel-resource-usage",))
    lda = int(re.search(r"#define PS_LDA (\d+)", open(SRC).read()).group(1))
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
    ks = {k: v for k, v in recs.items() if "k_predict_draws" in k}
    assert len(ks) == 22, sorted(recs)
    for name, r in ks.items():
        d = int(re.search(r"ILi(\d+)E", name).group(1))
        dynamic = (32 * lda + 32 * d) * 8                             # predict_draws_lds(d)
        assert r["LDS Size [bytes/block]"] + dynamic <= 80 * 1024, (name, r, dynamic)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 256, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
