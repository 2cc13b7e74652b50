"""CPU-side checks of the stacked predictive densities (gpz_amd.Predictor.stack, gpz_predictor_stack): the argument checks that must fire
before any GPU call, the C declaration and its limits against api.py, the compiled form of k_predict_stack.hip (no scratch, registers and
LDS within the budget of DESIGN.md section 14, no floating-point atomics to global memory and no compare-and-swap loop), and the NumPy /
SciPy reference ``stack_reference`` against closed forms.  The GPU tests (test_predictor_stack.py) take stack_reference from here."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.special import ndtr

import gpz_amd
from gpz_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gpz_amd", "csrc", "k_predict_stack.hip")
HEADER = os.path.join(ROOT, "include", "gpz_hip.h")


def stack_reference(mu0, sigma2, F, beta, edges, groups, weights, n_groups=None):
    """hist (1 + S, G, k, B), sum_w (G,), sum_mu and sum_mu2 (1 + S, G, k) of the issue's definition: mu0, sigma2, beta (n, k) as
    ``predict`` returns mu, sigma and beta_i, F (S, n, k) as ``draws`` returns it or None, edges (B + 1,), groups (n,) labels in
    [-1, G) or None, weights (n,) or None.  Column 0: N(mu0, sigma2); column 1 + s: N(F[s], beta)."""
    mu0 = np.asarray(mu0, dtype=np.float64)
    n, k = mu0.shape
    edges = np.asarray(edges, dtype=np.float64)
    B = edges.size - 1
    g = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    G = n_groups if n_groups is not None else (int(g.max()) + 1 if n and g.max() >= 0 else 1)
    S = 0 if F is None else len(F)
    hist = np.zeros((1 + S, G, k, B))
    sum_w = np.zeros(G)
    sum_mu = np.zeros((1 + S, G, k))
    sum_mu2 = np.zeros((1 + S, G, k))
    for gi in range(G):
        rows = np.nonzero(g == gi)[0]
        wg = w[rows]
        sum_w[gi] = wg.sum()
        for c in range(1 + S):
            mu = mu0[rows] if c == 0 else np.asarray(F[c - 1])[rows]
            s = np.sqrt(np.asarray(sigma2 if c == 0 else beta, dtype=np.float64)[rows])
            for o in range(k):
                cdf = ndtr((edges[None, :] - mu[:, o, None]) / s[:, o, None])
                hist[c, gi, o] = wg @ (cdf[:, 1:] - cdf[:, :-1])
                sum_mu[c, gi, o] = wg @ mu[:, o]
                sum_mu2[c, gi, o] = wg @ (mu[:, o] * mu[:, o])
    return hist, sum_w, sum_mu, sum_mu2


def test_reference_closed_forms():
    one = np.ones((1, 1))
    # one row, edges over +-40 widths: all of its weight
    mu, s2 = 0.3 * one, 0.04 * one
    e = 0.3 + 0.2 * np.linspace(-40, 40, 161)
    h, sw, sm, sm2 = stack_reference(mu, s2, None, s2, e, None, np.array([2.5]))
    assert h.shape == (1, 1, 1, 160) and abs(h.sum() - 2.5) <= 4 * np.finfo(float).eps * 2.5
    assert sw[0] == 2.5 and sm[0, 0, 0] == 2.5 * 0.3 and abs(sm2[0, 0, 0] - 2.5 * 0.09) <= 1e-16
    # a row on an edge: half of its mass on each side
    h = stack_reference(one, one, None, one, np.array([-50.0, 1.0, 50.0]), None, None)[0]
    assert np.array_equal(h.ravel(), [0.5, 0.5])
    # label -1 contributes nothing; a draw column uses beta as its width
    mu = np.array([[0.0], [1.0], [5.0]])
    s2 = np.full((3, 1), 4.0)
    be = np.full((3, 1), 1.0)
    F = mu[None] + 0.5
    e = np.array([-1.0, 0.0, 1.0, 2.0])
    h, sw, sm, _ = stack_reference(mu, s2, F, be, e, np.array([0, 1, -1]), None)
    assert h.shape == (2, 2, 1, 3) and np.array_equal(sw, [1.0, 1.0])
    assert np.allclose(h[0, 0, 0], np.diff(ndtr((e - 0.0) / 2.0)), rtol=0, atol=1e-16)
    assert np.allclose(h[1, 1, 0], np.diff(ndtr((e - 1.5) / 1.0)), rtol=0, atol=1e-16)
    assert np.array_equal(sm[:, :, 0], [[0.0, 1.0], [0.5, 1.5]])
    h2 = stack_reference(mu[:2], s2[:2], F[:, :2], be[:2], e, np.array([0, 1]), None)[0]
    assert np.array_equal(h, h2)


def test_stack_tail_polynomial_against_high_precision():
    """The constants of stack_tail (k_predict_stack.hip), parsed from the source and evaluated as the kernel does (Horner in f64), against
    mpmath at 50 digits.  p(u) is stated to be within 2 ulp of exp(x^2) erfc(x) for x <= 7 and 7 ulp for x <= 27: asserted at 3 and 8 eps
    (eps per ulp at worst, rounded up).  The whole tail Q(t) = p exp(-x^2) / 2 with x = t / sqrt 2 as the kernel forms it: 3 eps of p,
    1 of exp, 1.5 of three rounded products, and 2 x^2 eps from x itself: x carries two roundings of eps / 2 each (the constant
    1 / sqrt 2 and the product with t) and d ln erfc / d ln x is about -2 x^2.  So (6 + 2 x^2) eps relative for t <= 9.9 - the relative
    accuracy the far tails keep; any erfc(t / sqrt 2) formed in f64 shares the x^2 term."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    src = open(SRC).read()
    body = src[src.index("const double c[25] = {"):]
    c = [float.fromhex(v) for v in re.findall(r"-?0x1\.[0-9a-f]+p[-+]?\d+", body[:body.index("};")])]
    assert len(c) == 25
    eps = np.finfo(np.float64).eps
    t = np.concatenate([np.linspace(0.0, 9.9, 1500), np.linspace(9.9, 38.0, 500)])
    x = np.minimum(t * 0.70710678118654752440, 40.0)
    u = (x - 3.0) / (x + 3.0)
    p = np.full_like(x, c[24])
    for i in range(23, -1, -1):
        p = p * u + c[i]
    ref_p = np.array([float(mp.exp(mp.mpf(float(v)) ** 2) * mp.erfc(mp.mpf(float(v)))) for v in x])
    rel_p = np.abs(p - ref_p) / ref_p / eps
    near = x <= 7.0
    print(f"p(u): worst relative error {rel_p[near].max():.2f} eps for x <= 7, {rel_p[x <= 27].max():.2f} eps for x <= 27")
    assert rel_p[near].max() <= 3.0 and rel_p[x <= 27].max() <= 8.0
    s = x * x
    e = np.array([float(mp.mpf(float(v)) ** 2 - mp.mpf(float(w))) for v, w in zip(x, s)])   # fma(x, x, -s): the exact remainder
    ex = np.exp(-s)
    q = 0.5 * p * (ex - ex * e)
    ref_q = np.array([float(mp.erfc(mp.mpf(float(v)) / mp.sqrt(2)) / 2) for v in t])
    tail = t <= 9.9
    rel_q = np.abs(q - ref_q)[tail] / ref_q[tail] / eps
    print(f"Q(t): worst relative error / (6 + 2 x^2) eps for t <= 9.9: {np.max(rel_q / (6.0 + 2.0 * s[tail])):.3f} "
          f"(at t = {t[tail][np.argmax(rel_q / (6.0 + 2.0 * s[tail]))]:.2f})")
    assert np.all(rel_q <= 6.0 + 2.0 * s[tail])
    assert np.all(np.isfinite(q)) and np.all(q[t > 38.0 - 1e-9] < 1e-300)


def _model(d=3, m=6, k=1):
    model = gpz_amd.Model(m=m, d=d, k=k, method="VD")
    p = m * d + model.g_dim + m * k + k + 2 * m * k
    model.sets["best"] = {"theta": np.zeros(p), "w": np.zeros((m, k)), "iSigma_w": np.stack([np.eye(m)] * k, axis=2)}
    return model


def test_stack_validates_before_the_gpu(monkeypatch):
    """Every ValueError of Predictor.stack is raised on the host: the library load is made to fail, so a call that got past the checks
    would raise RuntimeError instead."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    X = np.zeros((4, 3))
    e = np.linspace(0.0, 1.0, 11)
    for model, k in ((_model(), 1), (_model(k=2), 2)):
        p = gpz_amd.Predictor(model)
        with pytest.raises(ValueError, match="X must be"):
            p.stack(np.zeros((4, 2)), e)
        Xn = X.copy()
        Xn[[1, 3], 2] = np.nan
        with pytest.raises(ValueError, match="2 rows"):
            p.stack(Xn, e)
        for bad in ([0.0], 1.0, np.zeros((2, 3)), [0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, 1.0, np.inf]):
            with pytest.raises(ValueError, match="edges"):
                p.stack(X, bad)
        for bad in (-1, 2.5, True, "4", None):
            with pytest.raises(ValueError, match="n_draws"):
                p.stack(X, e, n_draws=bad)
        with pytest.raises(ValueError, match="limit"):
            p.stack(X, e, n_draws=16384 // k)                            # (1 + n_draws) * k over GPZ_DRAWS_MAX_COLUMNS
        for bad in (-1, 2 ** 64, 1.5, True):
            with pytest.raises(ValueError, match="seed"):
                p.stack(X, e, n_draws=4, seed=bad)
        with pytest.raises(ValueError, match="Z must"):
            p.stack(X, e, n_draws=4, Z=np.zeros((6, 5, k)))
        with pytest.raises(ValueError, match="Z must"):
            p.stack(X, e, n_draws=0, Z=np.zeros((6, 4, k)))
        for bad in (np.zeros(5, dtype=int), np.zeros(4), np.array([0, 1, -2, 0]), np.zeros((4, 1), dtype=int)):
            with pytest.raises(ValueError, match="groups"):
                p.stack(X, e, groups=bad)
        with pytest.raises(ValueError, match="groups"):
            p.stack(X, e, groups=np.array([0, 1, 2, 0]), n_groups=2)
        for bad in (0, -3, 1.5, True):
            with pytest.raises(ValueError, match="n_groups"):
                p.stack(X, e, n_groups=bad)
        for bad in (np.ones(5), np.array([1.0, -0.5, 1.0, 1.0]), np.array([1.0, np.nan, 1.0, 1.0]), np.array([1.0, np.inf, 1.0, 1.0])):
            with pytest.raises(ValueError, match="weights"):
                p.stack(X, e, weights=bad)
        with pytest.raises(ValueError, match="selection"):
            p.stack(X, e, selection=np.ones(5, dtype=bool))
        with pytest.raises(ValueError, match="limit of 4096"):
            p.stack(X, e, n_groups=410)                                  # 410 groups x 10 bins
        with pytest.raises(ValueError, match="limit of 4096"):
            p.stack(X, np.linspace(0, 1, 4098))                          # one group x 4097 bins
        with pytest.raises(RuntimeError, match="disabled"):              # past every check: the first GPU call
            p.stack(X, e, n_draws=4, seed=2 ** 64 - 1, Z=np.zeros((6, 4, k)), groups=np.array([0, -1, 2, 1]), n_groups=4,
                    weights=np.array([0.0, 1.0, 2.0, 0.5]), selection=np.array([True, True, False, True]))
        r = p.stack(X[:0], e, n_draws=2, n_groups=3)                     # no rows: zeros, and no GPU call either
        assert r.hist.shape == (3, 3, k, 10) and not r.hist.any() and r.sum_w.shape == (3,)
        assert r.sum_mu.shape == r.sum_mu2.shape == (3, 3, k) and np.array_equal(r.edges, e)
        p.close()
        with pytest.raises(RuntimeError, match="closed"):
            p.stack(X, e)


def test_header_declares_the_entry_and_its_limits():
    h = open(HEADER).read()
    assert re.search(r"\bint gpz_predictor_stack\(gpz_predictor \*p, const double \*Xs, int64_t ns, int32_t ndraws, uint64_t seed,", h)
    assert int(re.search(r"#define GPZ_STACK_MAX_GROUP_BINS (\d+)", h).group(1)) == api.GPZ_STACK_MAX_GROUP_BINS == 4096
    assert "gpz_predictor_stack" in _lib.SYMBOLS and len(_lib.SYMBOLS["gpz_predictor_stack"][1]) == 16


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_stack_kernels_compiled_form(tmp_path):
    """at most 128 vector registers per lane (four waves per SIMD by registers), no scratch, no static LDS and at
    most 128 KiB of dynamic LDS at the size limit; sums that cross workgroups go through slabs, never through atomics."""
    asm = tmp_path / "k_predict_stack.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "gpz_amd", "csrc"), "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(asm)],
                       check=True, capture_output=True, text=True, timeout=900)
    recs, cur = {}, None
    for l in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = m.group(1)
            recs[cur] = {}
            continue
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", l)
        if m and cur:
            recs[cur][m.group(1)] = int(m.group(2))
    assert sorted(n for n in recs if "k_stack" in n) == sorted(recs) and len(recs) == 2, sorted(recs)
    for name, q in recs.items():
        assert q["VGPRs"] + q.get("AGPRs", 0) <= 128, (name, q)
        assert q["ScratchSize [bytes/lane]"] == 0, (name, q)
        assert q["LDS Size [bytes/block]"] == 0, (name, q)
    gb = api.GPZ_STACK_MAX_GROUP_BINS
    assert (gb + 3 * gb) * 8 <= 128 * 1024                               # predict_stack_lds at G = 4096, B = 1
    text = asm.read_text()
    for word in ("global_atomic_add_f64", "cmpswap", "flat_atomic", "global_atomic", "ds_add_f64", "ds_add_rtn_f64", "scratch_"):
        assert word not in text, word
