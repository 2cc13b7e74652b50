"""An independent extended-precision restatement of predictFull for complete, noise-free rows, per-element error gates for what the
streaming predictor (gpz_amd.Predictor) returns, and the table of shapes that test_predictor_sweep.py runs on the GPU and
test_predictor_reference_cpu.py checks on the host.  A helper, not a test module.

The reference (``predict_reference``) works in np.longdouble (64-bit mantissa, ``LONGDOUBLE_OK``) straight from theta:

    q_ij   = sum_c Gamma_jc^2 (x_ic - p_jc)^2            diagonal kinds (GL, VL, GD, VD)
    q_ij   = |Gamma_j (x_i - p_j)|^2                      covariance kinds (GC, VC): the direct form, no inverse and no solve
    PHI_ij = exp(-q_ij / 2)
    mu     = PHI w + muY,   nu_o = rowsum(PHI .* (PHI iSigma_o)),   ln beta = b (+ PHI v),   sigma = nu + beta

Only the layout of theta (unpack_theta, expand_gamma) is taken from oracle/gpz_oracle.py; the arithmetic is stated here.  X is
normalised in float64 exactly as api.py does it, (X - muX) / sdX, and only then cast up, so both sides start from the same bits.

The gates (``gates``) - derived, not tuned
------------------------------------------
eps = 2^-52 throughout: twice the unit roundoff u of float64, so every term below carries a factor 2 over its first-order bound.
de = pad_dim(d) is the width the kernels sum over (the zero padding adds exact zeros), nk = ceil16(m) the length of the products.

PHI, diagonal kinds.  q is a sum of de non-negative terms fma(dl * dl, g, q) with dl = x - p rounded once: each term carries at most
3 u relative (dl twice, its square), the running sum de u more (Higham, Accuracy and Stability, section 3.1: gamma_n for a recursive
sum, the same for every order of non-negative terms), in all (de + 3) u q <= (de + 4) eps q / 2.  An absolute error in the exponent
is a relative error of the exponential, and the gate takes the error of q, not of q / 2: dPHI = PHI eps (4 + (de + 4) q / 2), 4 eps
for exp itself (a few ulp) and the rounding of its argument.  One unit in the last place of the subnormal range (2^-1074) is added,
so that a PHI that underflows gradually is held to its format, not to a relative error it cannot have.

PHI, covariance kinds.  The device factors Gamma_j = Q_j R_j once (Householder) and forms s = R_j x - c_j with c_j = R_j p_j, then
q = sum_a s_a^2.  Its error follows |R||x| + |R||p|, not |s|: with T_a = sum_b |R_j|_ab (|x_b| + |p_jb|),

    |ds_a| <= 2 de u T_a          two dot products of at most de fma terms each (section 3.1)       ->  2 |s_a| |ds_a| <= 2 de eps |s_a| T_a
    dq     <= (de + 1) u q        the sum of de squares by fma                                      ->  (de + 1) eps q / 2
    R_j, c_j                      de reflectors applied to every column of Gamma_j (chapter 19, lemma 19.3: r gamma~ per column
                                  for r reflectors).  The lemma's gamma~ holds the reflector's length as well, which makes the worst
                                  case quadratic in de; a gate quadratic in de would pass a kernel that loses a whole term at d = 20,
                                  so the allowance here is linear: 5 eps = 10 u per reflector, 5 de eps (|s_a| T_a).  This is the one
                                  place where a worst-case bound is not taken in full.  A kernel that fails here is to be looked at.

    C = 8 de >= 2 de + (de + 1) / 2 + 5 de:   dPHI = PHI eps (4 + C (q + sum_a |s_a| T_a)) (+ 2^-1074)

|R_j| is NumPy's QR of Gamma_j (unique up to the signs of its rows, which the absolute values drop).

mu.   sum_j |w_jo| (PHI_ij (nk + 4) eps + dPHI_ij): a product of nk terms in any order (nk u, MFMA chains included), the rounding of
      the result, plus eps |mu| for the addition of muY in float64.  That rounding is u |mu|, and for a row that no basis function
      covers (mu -> muY) |mu| exceeds sum_j |w_j| PHI_ij by orders of magnitude, so the first term cannot carry it: without the
      second the float64 restatement itself misses the gate 5.8e3 times over (GL, d = 20, m = 33; the CPU module asserts that it
      does, so the term is not there for comfort).
nu.   sum_jl |iS_jlo| (PHI_ij PHI_il (2 nk + 8) eps + dPHI_ij PHI_il + PHI_ij dPHI_il): two nested sums of nk terms.
ln beta.  The mu bound with v in place of w (none for a homoscedastic model) plus eps |b_o|.
beta.  Relative: the ln beta bound plus 4 eps (exp).
sigma.  The sum of the nu and beta bounds (the addition's own u sigma is inside the 8 eps and 4 eps of its terms).

``assert_within`` checks every element, never a norm, and names the worst one."""
import os
import re

import numpy as np

from oracle import gpz_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpz_amd", "csrc")
EPS = 2.0 ** -52
LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 2e-19)
LONGDOUBLE_WHY = (f"the reference needs a 64-bit mantissa: np.longdouble has eps = {float(np.finfo(np.longdouble).eps):.3g} here "
                  "(need < 2e-19); no fall-back to float64")
QUANTITIES = ("PHI", "mu", "nu", "beta", "sigma")


# ---- the routes, stated a second time (test_predictor_reference_cpu.py holds them against the sources) ---------------------------------
PS_WIDTHS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20)


def ceil16(v):
    return (v + 15) // 16 * 16


def pad_dim(d):
    for s in PS_WIDTHS:
        if d <= s:
            return s
    return d


def ps_width_instantiated(de):
    return de in PS_WIDTHS


def phi_is_wide(de, k):
    return de > 20 or k > 8


def predict_small_fits(de, m, k):
    if phi_is_wide(de, k) or not ps_width_instantiated(de):
        return False
    return ceil16(m + 2 * k) <= 256 and (32 * 262 + 32 * de + 4 * 32) * 8 <= 80 * 1024


def predict_draws_fits(de, m):
    if phi_is_wide(de, 1) or not ps_width_instantiated(de):
        return False
    return ceil16(m) <= 256 and (32 * 262 + 32 * de) * 8 <= 80 * 1024


def draws_splits(ncol):
    """The values the fused draws kernel's ``split`` takes over the 16-block chunks of ncol columns (k_predict_draws.hip)."""
    nbw = ceil16(ncol) // 16
    return {min(nbw - cb, 16) < 4 for cb in range(0, nbw, 16)}


def parsed_cases(filename, function):
    """The ``case N:`` labels inside ``function`` of a source file under gpz_amd/csrc."""
    src = open(os.path.join(CSRC, filename)).read()
    body = src[src.index(function):]
    body = body[:body.index("\n}\n")]
    return sorted(int(v) for v in re.findall(r"case (\d+):", body))


# ---- the table of the sweep ---------------------------------------------------------------------------------------------------------
KINDS = ("GL", "VD", "GC", "VC")
WIDTH_N, WIDTH_TILE = 203, 64
EDGE_KS = (1, 3, 8)
EDGE_FAMILIES = (("VD", 5), ("VC", 7))
ROW_TILES = (64, 1024)
ROW_MODELS = (("VD", 50, 5, 2), ("GC", 50, 5, 2))          # (method, m, d, k)
STACK_MODEL = ("VD", 5, 60, 2)                                # (method, d, m, k)
STACK_N = 3000
STACK_BINS = (63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000, 4096)


def width_cases():
    """A: (method, d, m, k) for d = 1 .. 20, four kinds, m on both sides of the fused predict kernel's limit at k = 2."""
    return [(method, d, m, 2) for d in range(1, 21) for method in KINDS for m in (33, 254)]


def edge_ms(k):
    ms = {1, 2, 256 - 2 * k}
    for t in range(1, 17):
        ms |= {16 * t - 1, 16 * t, 16 * t + 1}
    return sorted(ms)


def edge_cases():
    """B: (method, d, m, k), m around every multiple of 16 up to 257, k = 1, 3, 8, and a few k = 9 (the runtime-d route: tiles)."""
    cases = [(method, d, m, k) for method, d in EDGE_FAMILIES for k in EDGE_KS for m in edge_ms(k)]
    cases += [(method, d, m, 9) for method, d in EDGE_FAMILIES for m in (40, 200)]
    return cases


def row_counts(T):
    return [1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5]


def case_seed(method, d, m, k):
    return 100003 * ("GL", "VL", "GD", "VD", "GC", "VC").index(method) + 5003 * d + 17 * m + k


def case_id(case):
    return "-".join(str(v) for v in case)


def routes(method, d, m, k):
    """(predict fused, draws fused) of an unforced handle."""
    de = pad_dim(d)
    return predict_small_fits(de, m, k), predict_draws_fits(de, m)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def normalised(model, X):
    """(X - muX) / sdX in float64, as api.py forms it."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    Xn = np.empty(X.shape)
    np.subtract(X, model.muX, out=Xn)
    np.divide(Xn, model.sdX, out=Xn)
    return Xn


def parameters(model, whichSet="best"):
    st = model.sets[whichSet]
    P, G, _, b, v, _ = O.unpack_theta(st["theta"], model)
    Gam = O.expand_gamma(G, model)
    m, k = model.m, model.k
    return {"P": P, "Gamma": Gam, "b": b, "v": v, "w": np.asarray(st["w"], dtype=np.float64).reshape(m, k),
            "iS": np.asarray(st["iSigma_w"], dtype=np.float64).reshape(m, m, k)}


def quadratic_form(model, par, Xn, dt):
    """q (n x m) in the number format dt, the direct forms of the module docstring."""
    X = Xn.astype(dt)
    P = par["P"].astype(dt)
    Gam = par["Gamma"].astype(dt)
    n, m = X.shape[0], model.m
    if model.method[1] == "C":
        q = np.empty((n, m), dtype=dt)
        for j in range(m):
            s = (X - P[j]) @ Gam[:, :, j].T
            q[:, j] = np.sum(s * s, axis=1)
        return q
    D = X[:, None, :] - P[None, :, :]
    return np.sum((Gam * Gam)[None, :, :] * (D * D), axis=2)


def outputs_from_phi(model, par, PHI, dt, w=None, v=None, b=None, use_v=None):
    """mu, nu, lnbeta, beta, sigma from PHI in the number format dt (w, v, b: replacements, for the mutants of the CPU tests)."""
    k, n = model.k, PHI.shape[0]
    w = (par["w"] if w is None else w).astype(dt)
    b = (par["b"] if b is None else b).astype(dt)
    v = par["v"] if v is None else v
    iS = par["iS"].astype(dt)
    mu = PHI @ w + np.asarray(model.muY, dtype=np.float64).reshape(-1).astype(dt)
    nu = np.stack([np.sum(PHI * (PHI @ iS[:, :, o]), axis=1) for o in range(k)], axis=1)
    lnbeta = np.tile(b.reshape(1, k), (n, 1))
    if model.heteroscedastic if use_v is None else use_v:
        lnbeta = lnbeta + PHI @ v.astype(dt)
    beta = np.exp(lnbeta)
    return {"mu": mu, "nu": nu, "lnbeta": lnbeta, "beta": beta, "sigma": nu + beta}


def predict_direct(model, X, whichSet="best", dt=np.float64):
    par = parameters(model, whichSet)
    Xn = normalised(model, X)
    q = quadratic_form(model, par, Xn, dt)
    PHI = np.exp(-q / 2)
    out = {"q": q, "PHI": PHI}
    out.update(outputs_from_phi(model, par, PHI, dt))
    out["_Xn"], out["_par"] = Xn, par
    return out


def predict_reference(model, X, whichSet="best"):
    """q, PHI, mu, nu, lnbeta, beta, sigma (np.longdouble) of the complete, noise-free rows of X."""
    if not LONGDOUBLE_OK:
        raise RuntimeError(LONGDOUBLE_WHY)
    return predict_direct(model, X, whichSet, LD)


def rows_of(ref, rows):
    """The reference of a subset of its rows (every row is computed on its own)."""
    return {key: (val[rows] if isinstance(val, np.ndarray) else val) for key, val in ref.items()}


def gates(ref, model):
    """Per-element error bounds of PHI, mu, nu, lnbeta, beta, sigma (float64 arrays): the module docstring."""
    par, Xn = ref["_par"], ref["_Xn"]
    m, k, d = model.m, model.k, model.d
    de, nk = pad_dim(d), ceil16(m)
    q = np.asarray(ref["q"], dtype=np.float64)
    PHI = np.asarray(ref["PHI"], dtype=np.float64)
    if model.method[1] == "C":
        C = 8.0 * de
        sT = np.empty_like(q)
        for j in range(m):
            R = np.linalg.qr(par["Gamma"][:, :, j], mode="r")
            s = (Xn - par["P"][j]) @ R.T
            T = (np.abs(Xn) + np.abs(par["P"][j])) @ np.abs(R).T
            sT[:, j] = np.sum(np.abs(s) * T, axis=1)
        dPHI = PHI * EPS * (4.0 + C * (q + sT))
    else:
        dPHI = PHI * EPS * (4.0 + (de + 4.0) * q / 2.0)
    dPHI = dPHI + 2.0 ** -1074
    aw, aS = np.abs(par["w"]), np.abs(par["iS"])
    g = {"PHI": dPHI}
    g["mu"] = (PHI * ((nk + 4.0) * EPS) + dPHI) @ aw + EPS * np.abs(np.asarray(ref["mu"], dtype=np.float64))
    g["nu"] = np.stack([np.sum((PHI @ aS[:, :, o]) * PHI, axis=1) * ((2.0 * nk + 8.0) * EPS)
                        + np.sum((dPHI @ aS[:, :, o]) * PHI, axis=1) + np.sum((PHI @ aS[:, :, o]) * dPHI, axis=1) for o in range(k)], axis=1)
    g["lnbeta"] = np.tile(EPS * np.abs(par["b"]).reshape(1, k), (q.shape[0], 1))
    if model.heteroscedastic:
        g["lnbeta"] = g["lnbeta"] + (PHI * ((nk + 4.0) * EPS) + dPHI) @ np.abs(par["v"])
    beta = np.asarray(ref["beta"], dtype=np.float64)
    g["beta"] = beta * (g["lnbeta"] + 4.0 * EPS)
    g["sigma"] = g["nu"] + g["beta"]
    return g


def named(out):
    """What Predictor.predict(..., return_phi=True) returns, by name."""
    d = {"mu": out[0], "sigma": out[1], "nu": out[2], "beta": out[3]}
    if len(out) > 5 and out[5] is not None:
        d["PHI"] = out[5]
    return d


def ratios(out, ref, gate):
    """{quantity: (worst |out - ref| / gate, its index)} over the quantities that out, ref and gate share."""
    res = {}
    for key, val in out.items():
        if key not in gate or key.startswith("_"):
            continue
        val = np.asarray(val)
        assert val.shape == ref[key].shape, (key, val.shape, ref[key].shape)
        if val.size == 0:
            continue
        err = np.abs(val.astype(LD) - ref[key].astype(LD)).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / gate[key])
        r = np.where(np.isfinite(val), r, np.inf)
        at = np.unravel_index(int(np.argmax(r)), r.shape)
        res[key] = (float(r[at]), tuple(int(i) for i in at))
    return res


def assert_within(out, ref, gate, what=""):
    """Every element of every quantity of ``out`` (a dict) within its gate of the reference; -> {quantity: worst ratio}."""
    res = ratios(out, ref, gate)
    assert res, (what, "nothing to compare")
    bad = {key: r for key, r in res.items() if not r[0] <= 1.0}
    assert not bad, (what, "worst error / gate and its (row, column): " +
                     ", ".join(f"{key} {r[0]:.3g} at {r[1]}" for key, r in sorted(bad.items())))
    return {key: r[0] for key, r in res.items()}


class Worst:
    """The worst error-to-gate ratio per quantity over a run, for the report at its end."""

    def __init__(self):
        self.worst = {}

    def add(self, res, what):
        for key, r in res.items():
            if r > self.worst.get(key, (-1.0, ""))[0]:
                self.worst[key] = (r, what)

    def __str__(self):
        return "; ".join(f"{key} {r:.3g} ({what})" for key, (r, what) in sorted(self.worst.items()))
