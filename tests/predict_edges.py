"""The one-shot prediction entries (gpz_predict_full / _noisy / _missing behind gpz_amd.predict) at the chunk and row edges of their
host-side rules: the rules stated a second time, the table of cases placed by them, the scale every output is judged against, and an
extended-precision reference of the diagonal kinds.  A helper, not a test module: test_predict_edges_cpu.py checks the table, the
reference and the fitness of every case on the host, test_predict_edges.py runs the cases on the GPU.

Term scales
-----------
The pair sums cancel: gamma = sum_ab Z_ab w_a w_b - mu^2 is 1e2 ... 1e5 times smaller than the sum of the absolute values of its terms
on the models used here, so neither |gamma| nor the largest element of the array says what a rounding error of the sum looks like.
Every Z_ab >= 0 and every PHI_ij >= 0, so one more call of the oracle on the model with w -> |w|, v -> |v|, iSigma_w -> |iSigma_w|
and muY = 0 (``abs_model``) returns those sums (primes: the second call; mu without muY):

    s_mu    = PHI |w| + |muY|                                  = mu' + |muY|
    s_gamma = sum Z |w_a| |w_b| + mu^2                         = (gamma' + mu'^2) + mu^2
    s_nu    = sum Z |iS_ab|                                    = nu'
    s_sigma = s_nu + s_beta + s_gamma

beta_i = exp(E) (1 + V / 2) with E = b + sum_j PHI_j v_j and V = sum Z v_a v_b - (PHI v)^2.  A relative perturbation eps of every term
moves E by at most eps s_E, s_E = |b| + PHI |v|, and V by at most eps s_V, s_V = sum Z |v_a| |v_b| + (PHI v)^2, and to first order
d beta = exp(E) ((1 + V / 2) dE + dV / 2); the rounding of exp and of the product adds eps |beta|:

    s_beta  = exp(E) (|1 + V / 2| (1 + s_E) + s_V / 2)

PHI |v| is a product with the oracle's own PHI, and sum Z |v_a| |v_b| comes back out of beta' = exp(b + PHI |v|) (1 + V' / 2):
sum Z |v||v| = 2 (beta' / exp(b + PHI |v|) - 1) + (PHI |v|)^2.  (``term_scales``; test_predict_edges_cpu.py forms the same sums term
by term and compares.)

PHI has no sum: an element is judged relative to its own value where that is at least 1e-30 of the largest of its row, and against
1e-30 of that largest below (``PHI_FLOOR``); a case is fit only if at least 90 % of its PHI are judged relatively (``phi_share``).

The measure (``scaled_errors``) is |out - ref| / scale per element, never a norm.  The gates are the project's constants: 1e-9 for the
diagonal kinds, max(1e-8, 10 phi_tol) for GC / VC (``gate_of``; phi_tol as tests/test_gpu_parity.py states it), predictor_reference.gates
for predictFull.

The extended-precision reference (``ld_reference``), diagonal kinds
--------------------------------------------------------------------
Sigma_j = diag(Gamma_j^-2), phi_j(x) = exp(-1/2 (x - p_j)' inv(Sigma_j) (x - p_j)) = (2 pi)^(d/2) |Sigma_j|^(1/2) N(x; p_j, Sigma_j).  A row
is a density over x: the observed dimensions o are N(x_o, Psi_o) (Psi = 0 without input noise), the missing dimensions u follow the
mixture of the basis functions conditioned on x_o, which for diagonal Sigma is  sum_l pi_l N(x_u; p_lu, Sigma_lu)  with
pi_l ~ prior_l N(x_o; p_lo, Sigma_lo + Psi_o) (Pio).  With g(D, V) = exp(-1/2 sum D^2 / V - 1/2 sum ln V) over the named dimensions
(the powers of 2 pi cancel throughout):

    E[phi_i]       = |Sigma_i|^(1/2) g(x_o - p_io, Sigma_io + Psi_o) sum_l pi_l g(p_iu - p_lu, Sigma_iu + Sigma_lu)
    phi_i phi_j    = (2 pi)^d |Sigma_i Sigma_j|^(1/2) N(p_i; p_j, Sigma_i + Sigma_j) N(x; c_ij, C_ij),
                     C_ij = inv(inv(Sigma_i) + inv(Sigma_j)),  c_ij = C_ij (inv(Sigma_i) p_i + inv(Sigma_j) p_j)
    E[phi_i phi_j] = |Sigma_i Sigma_j|^(1/2) g(p_i - p_j, Sigma_i + Sigma_j) g(x_o - c_o, C_o + Psi_o) sum_l pi_l g(c_u - p_lu, C_u + Sigma_lu)

    mu = E[phi] w + muY,  gamma = sum_ij w_i w_j E[phi_i phi_j] - (E[phi] w)^2,  V likewise with v,  nu = sum_ij L_ij E[phi_i phi_j],
    beta_i = exp(b + E[phi] v) (1 + V / 2)

L is inv(Sigma_w) as the reference reads it: the pair loop runs over i >= j, takes iSigma_w(i, j) and counts it twice for i > j, so
L = tril(iS) + tril(iS, -1)'.  A complete row without Psi is predictFull (gamma = 0, nu = sum PHI .* (PHI iS) with iS as given).  X and Psi
are normalised in float64 as the API does and only then cast up; everything after that is np.longdouble, vectorised over rows and
pairs.  Only the layout of theta is taken from the oracle."""
import os
import re
import zlib

import numpy as np

from oracle import gpz_oracle as O
from helpers import GOLDEN, make_problem, recondition_gamma
from predictor_reference import CSRC, LD, LONGDOUBLE_OK, LONGDOUBLE_WHY  # noqa: F401

EPS = 2.0 ** -52
PHI_FLOOR = 1e-30
PHI_SHARE_MIN = 0.9
NAMES = ("mu", "sigma", "nu", "beta_i", "gamma", "PHI")
DIAG_GATE = 1e-9


# ---- the host rules, stated a second time (test_predict_edges_cpu.py holds the quoted lines against the sources) ------------------------
def rup(v, q):
    return (v + q - 1) // q * q


def npairs(m):
    return m * (m + 1) // 2


def n_pad_min(ns):
    """gpz_ctx.hip:52: rows padded to 1024 (the general path adds one more unit of 1024)."""
    return rup(max(ns, 1), 1024)


def n_pad_rule(ns, method, psi, missing):
    """gpz_ctx.hip:52 with :314,323: a covariance kind with input noise or missing inputs takes the general path, whose row set
    carries one more unit of 1024 rows."""
    return n_pad_min(ns) + (1024 if method[1] == "C" and (psi or missing) else 0)


def noisy_chunks(m, ns):
    """gpz_predict.hip:197-202 (gpz_predict_noisy): as many pair chunks as make ~1024 workgroups with ceil(ns / 64) row blocks, at most
    npair and at most 256; then pairs per chunk and the final count.  -> dict(npair, nchunk, ppc, last)."""
    npair = npairs(m)
    q = (ns + 63) // 64
    nchunk = (1024 + q - 1) // q
    nchunk = max(1, min(nchunk, npair, 256))
    ppc = -(-npair // nchunk)
    nchunk = -(-npair // ppc)
    return dict(npair=npair, nchunk=nchunk, ppc=ppc, last=npair - (nchunk - 1) * ppc, row_blocks=q)


def cpsi4_available(d):
    """k_cpsi4.hip:27."""
    return 10 < d <= 32


def cpsi4w_available(d):
    """k_cpsi4w.hip:7."""
    return 32 < d <= 48


def pmc4_available(d):
    """k_pmc4.hip:151."""
    return 10 < d <= 32


def pmc_fast(d, k):
    """k_pmiss_cov.hip:617."""
    return d >= 2 and (d <= 10 or pmc4_available(d)) and k <= 8


def noisy_diag_width(d):
    """k_psi.hip:480,492: launch_predict_noisy_diag's ladder of widths."""
    return 4 if d <= 4 else 8 if d <= 8 else 12 if d <= 12 else 16 if d <= 16 else 20


def noisy_family(method, d, k):
    """k_gen.hip:740-749 launch_predict_noisy -> k_psi.hip:386-392 launch_predict_noisy_cov / :480 launch_predict_noisy_diag: the family token of the route."""
    km = 1 if k == 1 else 8
    if method[1] == "C":
        if k <= 8:
            if cpsi4_available(d):
                return "cpsi4<%d,%d>" % ((d + 3) // 4, km)
            if cpsi4w_available(d) and k == 1:
                return "cpsi4w<%d,1>" % ((d + 3) // 4)
            if 2 <= d <= 10:
                return "psi<%d,%d>" % (d, km)
    elif d <= 20 and k <= 8:
        return "noisy_diag<%d,%d>" % (noisy_diag_width(d), km)
    return "gen<20>" if d <= 20 else "gen_rt"


def missing_cov_rule(m, d, k, n):
    """gpz_predict.hip:340-351 (predict_missing_cov) and k_pmiss_cov.hip:650,655,687 (launch_pmc): rows per block 2^26 / (m d^2), at most n,
    at most 64 on the register-resident route, 1 for d > 64; 2048 (register-resident) or 64 pair chunks; the PHI pass of the
    register-resident route in min(m, 256) chunks.  -> dict(family, rows_blk, blocks, last_rows, npair, nchunk, ppc, last, phi_chunks)."""
    rb = (1 << 26) // (m * d * d)
    rb = max(1, min(rb, n))
    fast = pmc_fast(d, k)
    if fast and rb > 64:
        rb = 64
    if d > 64:
        rb = 1
    want = 2048 if fast else 64
    npair = npairs(m)
    nchunk = min(npair, want)
    ppc = -(-npair // nchunk)
    nchunk = -(-npair // ppc)
    if d > 64:
        family = "pmc_generic"
    elif d > 32:
        family = "pmc_wide"
    elif fast:
        family = ("pmc_fast<%d>" if d <= 10 else "pmc4<%d>") % d
    else:
        family = "pmc_scratch"
    blocks = -(-n // rb)
    return dict(family=family, rows_blk=rb, blocks=blocks, last_rows=n - (blocks - 1) * rb, npair=npair, nchunk=nchunk, ppc=ppc,
                last=npair - (nchunk - 1) * ppc, phi_chunks=m if m < 256 else 256)


PM_MAXD_DIAG = 144          # gpz_kernels.h: GPZ_PM_MAXD_DIAG
PM_ACCUM_SPLITS = 16        # k_pmiss.hip:293


def missing_diag_rule(m, k, n, d=1, n_pad=None):
    """gpz_predict.hip:466-468,497,506 (predict_missing_diag): chunks of cw * mp pairs, cw = 32 halved while n_pad x width doubles pass
    2e9 bytes, width rounded up to 64; the GEMMs over npg = rup(n, 128) rows; one q0 pass per `width` pairs.
    -> dict(family, mp, cw, width, passes, last, npg, splits)."""
    mp = rup(m + k, 16)
    n_pad = n_pad_min(n) if n_pad is None else n_pad
    cw = 32
    while cw > 1 and float(n_pad) * float(cw * mp) * 8.0 > 2e9:
        cw >>= 1
    width = rup(cw * mp, 64)
    npair = npairs(m)
    passes = -(-npair // width)
    return dict(family="pm_diag_flags" if d > PM_MAXD_DIAG else "pm_diag", mp=mp, cw=cw, width=width, passes=passes,
                last=npair - (passes - 1) * width, npg=rup(n, 128), splits=PM_ACCUM_SPLITS)


def full_rule(m, k, ns):
    """gpz_ctx.hip:249 and gpz_predict.hip:142-143: PHI is n_pad x mp, one T-GEMM per output over 128-row tiles."""
    return dict(family="tgemm", mp=rup(m + k, 16), tiles=-(-ns // 128))


def parse_route(text):
    """'predict_noisy: nchunk=138 ppc=2 n_pad=1024 noisy_diag<8,1>' -> ('predict_noisy', {'nchunk': 138, ...}, ['noisy_diag<8,1>'])."""
    entry, _, rest = text.partition(":")
    nums, words = {}, []
    for tok in rest.split():
        if "=" in tok:
            key, val = tok.split("=")
            nums[key] = int(val)
        else:
            words.append(tok)
    return entry, nums, words


# ---- the two model families and the diagonal-Gamma twin -------------------------------------------------------------------------------
def f32_valued(a):
    """The float64 array of a's values rounded to float32: a fixture keeps such inputs in half the bytes and gives back the same bits."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def trained_like_model(method, d, m, k, seed, hetero=True):
    """make_problem + O.GPz(nargout = 4), as test_gpu_parity._trained_like_model: broad bases, w and inv(Sigma_w) of a real solve, heavy
    cancellation in the pair sums.  GC / VC: Gamma redrawn by recondition_gamma.  theta is rounded to float32
    values before the solve (f32_valued)."""
    model, theta, X, Y, _, rng = make_problem(300, d, m, k, method, hetero, seed=seed)
    theta = f32_valued(recondition_gamma(model, theta, rng))
    model.muX = rng.standard_normal(d) * 0.1
    model.sdX = 1.0 + rng.random(d)
    model.muY = rng.standard_normal(k)
    r4 = O.GPz(theta, model, X, Y, nargout=4)
    pri = rng.random(m) + 0.2
    model.sets["best"] = {"theta": theta, "w": r4.w, "iSigma_w": r4.iSigma_w, "priors": pri / pri.sum()}
    return model


def synth_model(method, d, m, k, seed, hetero=True):
    """test_predictor.synth_model restated on the oracle's Model (that module imports the product): narrower bases, and an inv(Sigma_w)
    that is NOT symmetric, so a transposed operand or a swapped (a, b) shows.  Priors are drawn too."""
    rng = np.random.default_rng(seed)
    model = O.Model(m=m, d=d, k=k, method=method, heteroscedastic=hetero)
    P = rng.standard_normal((m, d))
    if method[1] == "C":
        blocks = 1 if method == "GC" else m
        G = np.concatenate([(0.6 * np.eye(d) + 0.08 * rng.standard_normal((d, d))).ravel(order="F") for _ in range(blocks)])
    else:
        G = rng.uniform(0.4, 0.9, model.g_dim)
    parts = [P.ravel(order="F"), G, rng.uniform(-1, 1, m * k), rng.uniform(-3, -1, k)]
    if hetero:
        parts += [0.05 * rng.standard_normal(m * k), rng.uniform(-1, 1, m * k)]
    theta = np.concatenate(parts)
    A = rng.standard_normal((m, m)) / np.sqrt(m)
    iS = np.stack([0.05 * (A @ A.T) + 0.02 * np.eye(m) + 1e-3 * rng.standard_normal((m, m)) for _ in range(k)], axis=2)
    model.muX = rng.standard_normal(d)
    model.sdX = rng.uniform(0.5, 2.0, d)
    model.muY = rng.standard_normal(k)
    pri = rng.random(m) + 0.2
    model.sets["best"] = {"theta": theta, "w": rng.standard_normal((m, k)), "iSigma_w": iS, "priors": pri / pri.sum()}
    return model


def clone_model(model, method=None, theta=None, **sets):
    new = O.Model(m=model.m, d=model.d, k=model.k, method=method or model.method, heteroscedastic=model.heteroscedastic)
    new.muX, new.sdX, new.muY = np.array(model.muX), np.array(model.sdX), np.array(model.muY)
    st = dict(model.sets["best"])
    if theta is not None:
        st["theta"] = theta
    st.update(sets)
    new.sets["best"] = st
    return new


def diag_twin(model):
    """The GC / VC model whose Gamma_j are the diagonal matrices of a diagonal-kind model (GL, GD -> GC; VL, VD -> VC): the same
    predictor, computed by the covariance code."""
    assert model.method[1] != "C", model.method
    m, d = model.m, model.d
    theta = np.asarray(model.sets["best"]["theta"], dtype=np.float64)
    _, G, *_ = O.unpack_theta(theta, model)
    Gam = O.expand_gamma(G, model)
    shared = model.method[0] == "G"
    blocks = np.concatenate([np.diag(Gam[j]).reshape(-1, order="F") for j in range(1 if shared else m)])
    new_theta = np.concatenate([theta[:m * d], blocks, theta[m * d + model.g_dim:]])
    return clone_model(model, method="GC" if shared else "VC", theta=new_theta)


def twin_psi(Psi):
    """n x d variances -> the d x d x n cube of diagonal matrices."""
    if Psi is None:
        return None
    n, d = Psi.shape
    cube = np.zeros((d, d, n))
    cube[np.arange(d), np.arange(d), :] = Psi.T
    return cube


def v_slice(model):
    o = model.m * model.d + model.g_dim + model.m * model.k + model.k
    return slice(o, o + model.m * model.k)


def abs_model(model):
    """w -> |w|, v -> |v|, iSigma_w -> |iSigma_w|, muY = 0: the model whose prediction is the sum of absolute terms (module docstring)."""
    st = model.sets["best"]
    theta = np.array(st["theta"], dtype=np.float64)
    if model.heteroscedastic:
        theta[v_slice(model)] = np.abs(theta[v_slice(model)])
    new = clone_model(model, theta=theta, w=np.abs(st["w"]), iSigma_w=np.abs(st["iSigma_w"]))
    new.muY = np.zeros(model.k)
    return new


def cov_cond(model):
    """max_j cond(Gamma_j' Gamma_j) of a GC / VC model (1 for a diagonal kind)."""
    if model.method[1] != "C":
        return 1.0
    _, G, *_ = O.unpack_theta(model.sets["best"]["theta"], model)
    Gam = O.expand_gamma(G, model)
    return float(max(np.linalg.cond(Gam[:, :, j].T @ Gam[:, :, j]) for j in range(1 if model.method == "GC" else model.m)))


def phi_tol(model):
    """test_gpu_parity.phi_tol: the reference's own loss through inv(Gamma' Gamma) for a covariance kind."""
    if model.method[1] != "C":
        return 1e-12
    return max(1e-12, 200.0 * cov_cond(model) * 2.2e-16)


def gate_of(model):
    return DIAG_GATE if model.method[1] != "C" else max(1e-8, 10.0 * phi_tol(model))


# ---- scales and the measure -----------------------------------------------------------------------------------------------------------
def oracle_outputs(model, Xs, Psi):
    return dict(zip(NAMES, O.predict_any(Xs, model, Psi=Psi)))


def term_scales(model, out, out_abs):
    """Scales of mu, sigma, nu, beta_i, gamma from the oracle's outputs on the model and on abs_model(model): the module docstring."""
    st = model.sets["best"]
    k = model.k
    muY = np.asarray(model.muY, dtype=np.float64).reshape(1, -1)
    mu0 = out["mu"] - muY
    s = {"mu": out_abs["mu"] + np.abs(muY), "nu": out_abs["nu"],
         "gamma": (out_abs["gamma"] + out_abs["mu"] ** 2) + mu0 ** 2}
    _, _, _, b, v, _ = O.unpack_theta(st["theta"], model)
    v = np.zeros((model.m, k)) if v is None else v
    E = out["PHI"] @ v + b
    Ea = out["PHI"] @ np.abs(v)
    szz = 2.0 * (out_abs["beta_i"] / np.exp(Ea + b) - 1.0) + Ea ** 2
    s_V = np.maximum(szz, 0.0) + (E - b) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        one_half_V = np.abs(out["beta_i"] / np.exp(E))                         # |1 + V / 2|
    s["beta_i"] = np.exp(E) * (one_half_V * (1.0 + np.abs(b) + Ea) + 0.5 * s_V)
    s["sigma"] = s["nu"] + s["beta_i"] + s["gamma"]
    return s


def phi_scale(PHI):
    """Per element: its own value where that is at least PHI_FLOOR of its row's largest, PHI_FLOOR of that largest below."""
    PHI = np.abs(np.asarray(PHI, dtype=np.float64))
    top = PHI.max(axis=1, keepdims=True)
    return np.maximum(PHI, PHI_FLOOR * top)


def phi_share(PHI):
    """The share of PHI's entries that are judged relative to their own value."""
    PHI = np.abs(np.asarray(PHI, dtype=np.float64))
    return float(np.mean(PHI >= PHI_FLOOR * PHI.max(axis=1, keepdims=True)))


def scaled_errors(out, ref, scales):
    """{name: (worst |out - ref| / scale, its index)} over the six outputs; a non-finite output counts as infinite."""
    res = {}
    for name in NAMES:
        a, r = np.asarray(out[name]), np.asarray(ref[name])
        assert a.shape == r.shape, (name, a.shape, r.shape)
        sc = phi_scale(r) if name == "PHI" else np.asarray(scales[name], dtype=np.float64)
        err = np.abs(a.astype(LD) - r.astype(LD)).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / sc)
        q = np.where(np.isfinite(a.astype(np.float64)), q, np.inf)
        q = np.where(np.isnan(q), np.inf, q)
        at = np.unravel_index(int(np.argmax(q)), q.shape)
        res[name] = (float(q[at]), tuple(int(i) for i in at))
    return res


def worst_of(res):
    return max(v[0] for v in res.values())


# ---- the extended-precision reference of the diagonal kinds ----------------------------------------------------------------------------
def _g(D, V):
    """exp(-1/2 sum D^2 / V - 1/2 sum ln V) over the last axis (1 for no dimensions)."""
    return np.exp(-(np.sum(D * D / V, axis=-1) + np.sum(np.log(V), axis=-1)) / 2)


def _ld_group(X, Psi, o, P, S, w, v, b, iS, prior, pair_block=256, want_terms=False):
    """One group of rows sharing the pattern o (True = observed) with input noise Psi (n x d or None): the module docstring."""
    n, m, k = X.shape[0], P.shape[0], w.shape[1]
    u = ~o
    half = LD(1) / 2
    if o.all() and Psi is None:                                                    # predictFull
        PHI = np.exp(-np.sum((X[:, None, :] - P[None]) ** 2 / S[None], axis=2) / 2)
        nu = np.stack([np.sum(PHI * (PHI @ iS[:, :, q]), axis=1) for q in range(k)], axis=1)
        E = PHI @ v
        out = {"mu0": PHI @ w, "nu": nu, "gamma": np.zeros((n, k), dtype=LD), "beta_i": np.exp(E + b), "PHI": PHI}
        if want_terms:
            out["terms"] = {"s_mu0": PHI @ np.abs(w), "s_zww": np.zeros((n, k), dtype=LD), "s_zvv": np.zeros((n, k), dtype=LD),
                            "s_nu": np.stack([np.sum(PHI * (PHI @ np.abs(iS[:, :, q])), axis=1) for q in range(k)], axis=1),
                            "E": E, "Ea": PHI @ np.abs(v)}
        return out
    Po = np.zeros((n, int(o.sum())), dtype=LD) if Psi is None else Psi[:, o]
    Xo = X[:, o]
    lnz = np.sum(np.log(S), axis=1) / 2
    Go = _g(Xo[:, None, :] - P[None, :, o], S[None, :, o] + Po[:, None, :])       # n x m: g(x_o - p_lo, Sigma_lo + Psi_o)
    pi = Go * prior[None, :]
    pi = pi / np.sum(pi, axis=1, keepdims=True)
    Nij = _g(P[:, None, u] - P[None, :, u], S[:, None, u] + S[None, :, u])        # m x m over the missing dimensions
    PHI = np.exp(lnz)[None, :] * Go * (pi @ Nij.T)
    ii, jj = np.tril_indices(m)
    c2 = np.where(ii == jj, LD(1), LD(2))
    acc = {key: np.zeros((n, k), dtype=LD) for key in ("zww", "zvv", "znu", "s_zww", "s_zvv", "s_nu")}
    for p0 in range(0, ii.size, pair_block):
        a, c = ii[p0:p0 + pair_block], jj[p0:p0 + pair_block]
        Sa, Sc = S[a], S[c]
        C = Sa * Sc / (Sa + Sc)
        cen = (P[a] / Sa + P[c] / Sc) * C
        lnZ = lnz[a] + lnz[c] + np.log(_g(P[a] - P[c], Sa + Sc))
        A = _g(Xo[:, None, :] - cen[None, :, o], C[None, :, o] + Po[:, None, :])   # n x pairs
        B = _g(cen[:, None, u] - P[None, :, u], C[:, None, u] + S[None, :, u])     # pairs x m
        Z = np.exp(lnZ)[None, :] * A * (pi @ B.T) * c2[None, p0:p0 + pair_block]
        ww, vv, ss = w[a] * w[c], v[a] * v[c], iS[a, c, :]
        acc["zww"] += Z @ ww
        acc["zvv"] += Z @ vv
        acc["znu"] += Z @ ss
        if want_terms:
            acc["s_zww"] += Z @ np.abs(ww)
            acc["s_zvv"] += Z @ np.abs(vv)
            acc["s_nu"] += Z @ np.abs(ss)
    mu0, E = PHI @ w, PHI @ v
    V = acc["zvv"] - E * E
    out = {"mu0": mu0, "nu": acc["znu"], "gamma": acc["zww"] - mu0 * mu0, "beta_i": np.exp(E + b) * (1 + half * V), "PHI": PHI}
    if want_terms:
        out["terms"] = {"s_mu0": PHI @ np.abs(w), "s_zww": acc["s_zww"], "s_zvv": acc["s_zvv"], "s_nu": acc["s_nu"], "E": E,
                        "Ea": PHI @ np.abs(v)}
    return out


def ld_reference(model, Xs, Psi=None, whichSet="best", want_terms=False):
    """mu (with muY), sigma, nu, beta_i, gamma, PHI of predict(Xs, model, Psi) for a DIAGONAL kind in np.longdouble, every branch:
    rows grouped by NaN pattern, with or without input noise.  want_terms: also "scales", the sums of absolute terms formed term by
    term (s_mu, s_gamma, s_nu, s_beta, s_sigma of the module docstring)."""
    if not LONGDOUBLE_OK:
        raise RuntimeError(LONGDOUBLE_WHY)
    assert model.method[1] != "C", "the extended-precision reference covers the diagonal kinds (a GC / VC case is judged on its twin)"
    st = model.sets[whichSet]
    Xs = np.asarray(Xs, dtype=np.float64)
    n, m, k = Xs.shape[0], model.m, model.k
    Xn = (Xs - model.muX) / model.sdX
    PsiN = O.fixPsi(Psi, n, model.sdX, model.method)
    P, G, _, b, v, _ = O.unpack_theta(st["theta"], model)
    Gam = O.expand_gamma(G, model).astype(LD)
    S = 1 / (Gam * Gam)
    v = np.zeros((m, k)) if v is None else v
    w = np.asarray(st["w"], dtype=np.float64).reshape(m, k).astype(LD)
    iS = np.asarray(st["iSigma_w"], dtype=np.float64).reshape(m, m, k).astype(LD)
    L = np.stack([np.tril(iS[:, :, q]) + np.tril(iS[:, :, q], -1).T for q in range(k)], axis=2)
    prior = np.asarray(st.get("priors", np.ones(m) / m), dtype=np.float64).ravel().astype(LD)
    muY = np.asarray(model.muY, dtype=np.float64).reshape(1, k).astype(LD)
    res = {name: np.zeros((n, m if name == "PHI" else k), dtype=LD) for name in NAMES}
    terms = {key: np.zeros((n, k), dtype=LD) for key in ("s_mu0", "s_zww", "s_zvv", "s_nu", "E", "Ea")}
    miss = np.isnan(Xn)
    bl = b.astype(LD).reshape(1, k)
    for pat in np.unique(miss, axis=0):
        rows = np.flatnonzero((miss == pat).all(axis=1))
        full = not pat.any() and PsiN is None
        g = _ld_group(Xn[rows].astype(LD), None if PsiN is None else PsiN[rows].astype(LD), ~pat, P.astype(LD), S, w, v.astype(LD), bl,
                      iS if full else L, prior, want_terms=want_terms)
        res["mu"][rows] = g["mu0"] + muY
        for name in ("nu", "gamma", "beta_i", "PHI"):
            res[name][rows] = g[name]
        if want_terms:
            for key in terms:
                terms[key][rows] = g["terms"][key]
    res["sigma"] = res["nu"] + res["beta_i"] + res["gamma"]
    if want_terms:
        mu0 = res["mu"] - muY
        E = terms["E"]
        s_V = terms["s_zvv"] + E * E
        sc = {"mu": terms["s_mu0"] + np.abs(muY), "nu": terms["s_nu"], "gamma": terms["s_zww"] + mu0 * mu0}
        sc["beta_i"] = np.exp(E + bl) * (np.abs(res["beta_i"] / np.exp(E + bl)) * (1 + np.abs(bl) + terms["Ea"]) + s_V / 2)
        sc["sigma"] = sc["nu"] + sc["beta_i"] + sc["gamma"]
        res["scales"] = {key: val.astype(np.float64) for key, val in sc.items()}
    return res


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _case(id, entry, method, d, m, ns, k=1, psi=None, family="trained", pattern=None, twin=False, edge="", pred=None, fixture=False):
    """entry: N (gpz_predict_noisy), MD / MC (gpz_predict_missing, diagonal / covariance kinds), F (gpz_predict_full).  psi: None, "var"
    (n x d variances) or "cube".  pattern: the missing dimensions of every row.  twin: the diagonal-Gamma twin of a GD / VD model, run
    as GC / VC.  edge / pred: what the case is there for, in words and as a predicate on the restated rule's dict."""
    return dict(id=id, entry=entry, method=method, d=d, m=m, ns=ns, k=k, psi=psi, family=family, pattern=pattern, twin=twin, edge=edge,
                pred=pred, fixture=fixture)


N_MS = {22: ("253 pairs, one per chunk", lambda r: r["ppc"] == 1 and r["nchunk"] == 253),
        23: ("ppc == 2 and npair % ppc == 0", lambda r: r["ppc"] == 2 and r["npair"] % 2 == 0 and r["nchunk"] == 138),
        34: ("ppc == 3, the last chunk holds one pair", lambda r: r["ppc"] == 3 and r["last"] == 1 and r["nchunk"] == 199),
        60: ("ppc == 8, a chunk crosses several rows of the triangle, short last chunk", lambda r: r["ppc"] == 8 and 0 < r["last"] < 8)}
# (method, d, k, psi) of predictNoisy: one representative per kernel family
N_REPS = [("VD", 5, 1, "var"), ("GL", 20, 3, "var"), ("VC", 5, 1, "cube"), ("GC", 10, 3, "var"), ("VC", 12, 2, "cube"),
          ("GC", 36, 1, "cube"), ("VD", 6, 9, "var"), ("VC", 1, 1, "cube"), ("VL", 24, 1, "var"), ("VC", 50, 1, "cube")]
N_ROWS = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)


def _families(method, d=2):
    """Both families for a diagonal kind; trained-like for GC / VC - except at d = 1, where init_theta turns a covariance kind into
    its diagonal equivalent and only the synthetic model stays VC."""
    if method[1] != "C":
        return ("trained", "synth")
    return ("trained",) if d > 1 else ("synth",)


def _slow_noisy_cov(method, d, ns, m):
    """The oracle's predictNoisy of a covariance kind loops over (pair, row) in Python: beyond ~20 000 such steps a case takes more
    than 2 s and its expected outputs come from a fixture (measured: 1.4 s at 253 x 70, 3 s at 595 x 70, 1.7 s at 21 x 1024)."""
    return method[1] == "C" and npairs(m) * ns > 17000


def _build_cases():
    cases = []
    # N: predictNoisy, pairs per chunk
    for method, d, k, psi in N_REPS:
        for m, (edge, pred) in N_MS.items():
            if d == 50 and m > 34:
                continue
            for fam in _families(method, d):
                cases.append(_case("N-%s-d%d-k%d-m%d-%s" % (method, d, k, m, fam), "N", method, d, m, 70, k=k, psi=psi, family=fam,
                                   edge=edge, pred=pred, fixture=_slow_noisy_cov(method, d, 70, m)))
    # the diagonal-Gamma twins of the covariance representatives at m = 34
    for method, d, k, psi in N_REPS:
        if method[1] == "C":
            edge, pred = N_MS[34]
            cases.append(_case("N-twin-%s-d%d-k%d-m34" % (method, d, k), "N", "GD" if method == "GC" else "VD", d, 34, 70, k=k,
                               psi="var", twin=True, edge="diagonal-Gamma twin: " + edge, pred=pred, fixture=True))
    # N: rows, at m = 6 (21 pairs, one per chunk), k = 2: the wave edges and the 1024-row padding unit (pitch n_pad, not ns, at k = 2)
    for method, d, psi in (("VD", 5, "var"), ("VC", 5, "cube"), ("VC", 12, "cube")):
        for ns in N_ROWS:
            for fam in _families(method):
                cases.append(_case("N-rows-%s-d%d-n%d-%s" % (method, d, ns, fam), "N", method, d, 6, ns, k=2, psi=psi, family=fam,
                                   fixture=_slow_noisy_cov(method, d, ns, 6),
                                   edge="%d rows: %d row blocks of 64, %d padding units of 1024, one pair per chunk" % (
                                       ns, (ns + 63) // 64, (ns + 1023) // 1024),
                                   pred=lambda r, ns=ns: r["ppc"] == 1 and r["nchunk"] == 21 and r["row_blocks"] == -(-ns // 64)
                                   and r["n_pad"] - r["n_pad_min"] in (0, 1024) and r["n_pad_min"] == (2048 if ns > 1024 else 1024)))
    # MD: predictMissing / predictNoisyMissing of the diagonal kinds
    md_edges = {63: ("mp = 64, width 2048: 2016 pairs in one pass", lambda r: r["width"] == 2048 and r["passes"] == 1),
                64: ("mp steps to 80, width 2560: one pass", lambda r: r["width"] == 2560 and r["passes"] == 1),
                65: ("m one past the 64-column tile", lambda r: r["width"] == 2560 and r["passes"] == 1),
                71: ("2556 pairs against a width of 2560: the last pass-free m", lambda r: r["passes"] == 1 and r["width"] - r["last"] == 4),
                72: ("2628 pairs against 2560: a second q0 pass of 68 pairs", lambda r: r["passes"] == 2 and r["last"] == 68),
                73: ("a second pass of 141 pairs", lambda r: r["passes"] == 2 and r["last"] == 141)}
    for method, d, pats in (("VD", 5, ((4,), (0, 2))), ("GL", 3, ((2,), (0,)))):
        for m, (edge, pred) in md_edges.items():
            for pi, pat in enumerate(pats):
                for psi in (None, "var"):
                    for fam in _families(method):
                        cases.append(_case("MD-%s-m%d-p%d-%s-%s" % (method, m, pi, "psi" if psi else "nopsi", fam), "MD", method, d, m, 40,
                                           psi=psi, family=fam, pattern=pat, edge=edge, pred=pred))
        for ns in (1, 127, 128, 129, 1025):
            for psi in (None, "var"):
                for fam in _families(method):
                    cases.append(_case("MD-%s-rows%d-%s-%s" % (method, ns, "psi" if psi else "nopsi", fam), "MD", method, d, 10, ns, k=2,
                                       psi=psi, family=fam, pattern=pats[0], edge="a group of %d rows: npg = %d" % (ns, rup(ns, 128)),
                                       pred=lambda r, ns=ns: r["npg"] == rup(ns, 128) and r["passes"] == 1))
    for fam in _families("VD"):
        cases.append(_case("MD-VD-d150-m64-" + fam, "MD", "VD", 150, 64, 40, family=fam, pattern=tuple(range(3, 150, 7)),
                           edge="d > 144: the device-flag instantiations", pred=lambda r: r["family"] == "pm_diag_flags"))
    # MC: GC / VC with missing inputs
    mc_edges = {63: ("2016 pairs in 2016 chunks", lambda r: r["ppc"] == 1 and r["nchunk"] == 2016),
                64: ("ppc == 2 exactly", lambda r: r["ppc"] == 2 and r["npair"] % 2 == 0 and r["nchunk"] == 1040),
                65: ("ppc == 2 with a short last chunk", lambda r: r["ppc"] == 2 and r["last"] == 1)}
    for method, d, pat in (("VC", 5, (1, 3)), ("GC", 3, (2,))):
        for m, (edge, pred) in mc_edges.items():
            cases.append(_case("MC-%s-d%d-m%d-nopsi" % (method, d, m), "MC", method, d, m, 70, pattern=pat, fixture=True,
                               edge=edge + "; 70 rows: two row blocks of the register-resident route, the second of 6",
                               pred=lambda r, pred=pred: pred(r) and r["rows_blk"] == 64 and r["blocks"] == 2 and r["last_rows"] == 6))
            cases.append(_case("MC-%s-d%d-m%d-psi" % (method, d, m), "MC", method, d, m, 3, psi="cube", pattern=pat, fixture=True,
                               edge=edge + "; cube Psi", pred=pred))
        for ns in (1, 63, 64, 65, 129):
            for psi in (None, "cube"):
                cases.append(_case("MC-%s-d%d-rows%d-%s" % (method, d, ns, "psi" if psi else "nopsi"), "MC", method, d, 6, ns, k=2, psi=psi,
                                   pattern=pat, edge="a group of %d rows in blocks of 64" % ns,
                                   pred=lambda r, ns=ns: r["rows_blk"] == min(ns, 64) and r["blocks"] == -(-ns // 64)))
    cases.append(_case("MC-VC-d5-unshuffle", "MC", "VC", 5, 6, 5, psi="cube", pattern=(0, 1),
                       edge="[o u] = [2 3 4 0 1] is not an involution: the kept unshuffle quirk", pred=lambda r: r["family"] == "pmc_fast<5>"))
    for ns in (64, 65):
        cases.append(_case("MC-VC-d12-rows%d" % ns, "MC", "VC", 12, 5, ns, pattern=(2, 7), edge="pmc4, a group of %d rows" % ns,
                           pred=lambda r, ns=ns: r["family"] == "pmc4<12>" and r["blocks"] == -(-ns // 64)))
    for m, (edge, pred) in mc_edges.items():
        cases.append(_case("MC-VC-d12-m%d" % m, "MC", "VC", 12, m, 8, pattern=(2, 7), fixture=True, edge="pmc4: " + edge,
                           pred=lambda r, pred=pred: pred(r) and r["family"] == "pmc4<12>"))
    sc_edges = {10: ("55 pairs in 55 chunks", lambda r: r["ppc"] == 1 and r["nchunk"] == 55),
                11: ("66 pairs at ppc 2, exact", lambda r: r["ppc"] == 2 and r["last"] == 2),
                12: ("78 pairs at ppc 2, exact", lambda r: r["ppc"] == 2 and r["last"] == 2),
                13: ("91 pairs at ppc 2, the last chunk holds one", lambda r: r["ppc"] == 2 and r["last"] == 1)}
    # (VC d = 1 takes the scratch route too, but a row whose only input is missing has no observed dimension to condition on: the
    # narrowest covariance model with a missing input is d = 2, which k = 9 keeps off the register-resident route)
    for method, d, k, pat in (("GC", 4, 9, (1,)), ("VC", 2, 9, (0,))):
        for m, (edge, pred) in sc_edges.items():
            cases.append(_case("MC-%s-d%d-k%d-m%d" % (method, d, k, m), "MC", method, d, m, 20, k=k, pattern=pat, edge="scratch route: " + edge,
                               pred=lambda r, pred=pred: pred(r) and r["family"] == "pmc_scratch"))
    cases.append(_case("MC-VC-d40-rowblocks", "MC", "VC", 40, 8, 5250, pattern=(5, 17, 30),
                       edge="rows_blk = 5242: two row blocks, the second of 8 rows",
                       pred=lambda r: r["family"] == "pmc_wide" and r["rows_blk"] == 5242 and r["blocks"] == 2 and r["last_rows"] == 8))
    # F: predictFull
    for method in ("VD", "VC"):
        for m in (255, 256, 257, 300):
            for ns in (1, 1023, 1024, 1025):
                cases.append(_case("F-%s-m%d-n%d" % (method, m, ns), "F", method, 5, m, ns, k=2, family="synth",
                                   edge="mp = %d, %d tiles of 128 rows, n_pad %d" % (rup(m + 2, 16), -(-ns // 128), n_pad_min(ns)),
                                   pred=lambda r, m=m: r["mp"] == rup(m + 2, 16)))
    return cases


CASES = _build_cases()
CASE_BY_ID = {c["id"]: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def case_rule(case):
    """The restated rule's dict for a case (what its predicate reads and what the route must report)."""
    m, d, k, ns = case["m"], case["d"], case["k"], case["ns"]
    method = run_method(case)
    if case["entry"] == "N":
        r = noisy_chunks(m, ns)
        r["family"] = noisy_family(method, d, k)
    elif case["entry"] == "MD":
        r = missing_diag_rule(m, k, ns, d)
    elif case["entry"] == "MC":
        r = missing_cov_rule(m, d, k, ns)
    else:
        r = full_rule(m, k, ns)
    r["n_pad_min"] = n_pad_min(ns)
    r["n_pad"] = n_pad_rule(ns, method, bool(case["psi"]), case["pattern"] is not None)
    return r


def run_method(case):
    """The method the GPU runs: the covariance kind of a twin."""
    if case["twin"]:
        return "GC" if case["method"][0] == "G" else "VC"
    return case["method"]


def case_seed(case):
    return zlib.crc32(case["id"].encode()) % (2 ** 31)


_MODELS = {}


def case_model(case):
    """The model of a case (shared by the cases of one (family, method, d, m, k): the edges differ in rows, Psi and pattern)."""
    key = (case["family"], case["method"], case["d"], case["m"], case["k"])
    if key not in _MODELS:
        seed = zlib.crc32(repr(key).encode()) % (2 ** 31)
        make = trained_like_model if case["family"] == "trained" else synth_model
        _MODELS[key] = make(case["method"], case["d"], case["m"], case["k"], seed)
    return _MODELS[key]


def case_inputs(case):
    """-> (model, Xs, Psi) in the method of the case (a twin: the GD / VD model with n x d variances; ``run_inputs`` turns it)."""
    model = case_model(case)
    rng = np.random.default_rng(case_seed(case))
    ns, d = case["ns"], case["d"]
    Xs = f32_valued(model.muX + model.sdX * rng.standard_normal((ns, d)))
    if case["pattern"] is not None:
        Xs[:, list(case["pattern"])] = np.nan
    Psi = None
    if case["psi"] == "var":
        Psi = f32_valued(rng.gamma(1.0, 0.1, (ns, d)))
    elif case["psi"] == "cube":
        Psi = psi_cube(f32_valued(rng.gamma(1.0, 0.05, (ns, d))), f32_valued(0.3 * rng.standard_normal((ns, d))))
    return model, Xs, Psi


def psi_cube(g, u):
    """Psi_i = diag(g_i) + u_i u_i': full, positive definite, and formed element by element, so a fixture that keeps g and u (2 n d
    numbers, not n d^2) gives back the same bits everywhere."""
    n, d = g.shape
    cube = u.T[:, None, :] * u.T[None, :, :]
    cube[np.arange(d), np.arange(d), :] += g.T
    return cube


def run_inputs(case):
    """-> (model, Xs, Psi) as gpz_amd.predict and the oracle take them (a twin: the covariance model and the cube of diagonals)."""
    model, Xs, Psi = case_inputs(case)
    if case["twin"]:
        return diag_twin(model), Xs, twin_psi(Psi)
    return model, Xs, Psi


def fixture_path(case):
    return os.path.join(GOLDEN, "pe_" + case["id"].replace("<", "").replace(">", "") + ".npz")


def compute_expected(case):
    """The oracle's six outputs and the term scales of a case, computed here (two oracle calls)."""
    model, Xs, Psi = run_inputs(case)
    out = oracle_outputs(model, Xs, Psi)
    out_abs = oracle_outputs(abs_model(model), Xs, Psi)
    return out, term_scales(model, out, out_abs)


def model_from_arrays(g):
    model = O.Model(m=int(g["m"]), d=int(g["d"]), k=int(g["k"]), method=str(g["method"]), heteroscedastic=bool(int(g["heteroscedastic"])))
    model.muX, model.sdX, model.muY = g["muX"], g["sdX"], g["muY"]
    model.sets["best"] = {"theta": g["theta"], "w": g["w"], "iSigma_w": g["iSigma_w"], "priors": g["priors"]}
    return model


def load_fixture(case):
    """-> (model, Xs, Psi, out, scales) of a fixture case, from tests/golden/pe_<id>.npz alone."""
    z = np.load(fixture_path(case))
    g = {key: (z[key].astype(np.float64) if z[key].dtype == np.float32 else z[key]) for key in z.files}
    g["sigma"] = g["nu"] + g["beta_i"] + g["gamma"]                                      # predict.m:72, as the oracle forms it
    g["s_sigma"] = g["s_nu"] + g["s_beta_i"] + g["s_gamma"]
    Psi = None
    if int(g["has_psi"]) == 1:
        Psi = g["Psi"]
    elif int(g["has_psi"]) == 2:
        Psi = psi_cube(g["Psi_g"], g["Psi_u"])
    return (model_from_arrays(g), g["Xs"], Psi, {name: g[name] for name in NAMES},
            {name: g["s_" + name] for name in NAMES if name != "PHI"})


def fixture_arrays(case):
    """What tests/golden/make_golden_predict_edges.py freezes for a case: the model and the inputs as the GPU runs them, the oracle's
    six outputs and the term scales."""
    model, Xs, Psi = run_inputs(case)
    out, scales = compute_expected(case)
    st = model.sets["best"]
    arr = dict(d=model.d, m=model.m, k=model.k, method=model.method, heteroscedastic=int(model.heteroscedastic), theta=st["theta"],
               w=st["w"], iSigma_w=st["iSigma_w"], priors=st["priors"], muX=model.muX, sdX=model.sdX, muY=model.muY, Xs=Xs)
    if Psi is None:
        arr["has_psi"] = 0
    elif case["psi"] == "cube" and not case["twin"]:
        rng = np.random.default_rng(case_seed(case))        # the draws of case_inputs, in its order
        rng.standard_normal((case["ns"], case["d"]))
        g, u = f32_valued(rng.gamma(1.0, 0.05, (case["ns"], case["d"]))), f32_valued(0.3 * rng.standard_normal((case["ns"], case["d"])))
        assert np.array_equal(psi_cube(g, u), Psi)
        arr.update(has_psi=2, Psi_g=g, Psi_u=u)
    elif case["twin"]:
        arr.update(has_psi=2, Psi_g=case_inputs(case)[2], Psi_u=np.zeros((case["ns"], case["d"])))
        assert np.array_equal(psi_cube(arr["Psi_g"], arr["Psi_u"]), Psi)
    else:
        arr.update(has_psi=1, Psi=Psi)
    arr.update({name: val for name, val in out.items() if name != "sigma"})             # sigma = nu + beta_i + gamma on loading
    arr.update({"s_" + name: val for name, val in scales.items() if name != "sigma"})
    for key in ("theta", "Xs", "Psi", "Psi_g", "Psi_u"):                                 # float32-valued inputs in half the bytes
        if key in arr:
            small = np.asarray(arr[key]).astype(np.float32)
            if np.array_equal(small.astype(np.float64), arr[key], equal_nan=True):       # (the synthetic family's theta is not)
                arr[key] = small
    return arr


def expected(case):
    """-> (model, Xs, Psi, out, scales): from the fixture where the case has one, else computed."""
    if case["fixture"]:
        return load_fixture(case)
    model, Xs, Psi = run_inputs(case)
    out, scales = compute_expected(case)
    return model, Xs, Psi, out, scales


# ---- fitness: the oracle against the extended-precision reference ----------------------------------------------------------------------
def twin_case(case):
    """The diagonal-Gamma twin of a GC / VC case: the same m, d, k, rows and pair count, the Gamma_j of a GD / VD model, Psi as
    variances (run as the cube of diagonals).  With Psi the missing dimensions move to the end, where [o u] is the identity: the
    reference's unshuffle scatter (predictCov.m:266-268) equals the intended one only for an involution, and the twin is there to
    judge the oracle's arithmetic, not to restate the quirk."""
    if case["twin"]:
        return case
    assert case["method"][1] == "C"
    tw = dict(case, id="twin-of-" + case["id"], method="GD" if case["method"] == "GC" else "VD", twin=True, family="trained", fixture=False,
              psi="var" if case["psi"] else None)
    if case["pattern"] is not None and case["psi"]:
        tw["pattern"] = tuple(range(case["d"] - len(case["pattern"]), case["d"]))
    return tw


def reference_error(case):
    """e_ref: the oracle against the extended-precision reference in the per-element scaled measure - of the case itself for a
    diagonal kind or a twin, of its diagonal-Gamma twin for GC / VC.  -> (worst ratio, {name: (ratio, index)})."""
    c = case if case["method"][1] != "C" else twin_case(case)
    out, scales = compute_expected(c)
    dm, dX, dP = case_inputs(c)
    ref = ld_reference(dm, dX, dP)
    res = scaled_errors(out, ref, scales)
    return worst_of(res), res
