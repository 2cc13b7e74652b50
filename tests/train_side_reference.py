"""Extended-precision restatements of what train() runs AROUND the objective - the L-BFGS memory (lbfgsAdd.m / lbfgsProd.m), the
fixed point of getPrior.m, the normalised densities N of getPHI.m and Dxy.m - with the inputs and case tables that
test_lbfgs_edges.py and test_prior_edges.py run on the GPU and test_train_side_reference_cpu.py checks on the host.  A helper, not a
test module.  Plain NumPy in np.longdouble (64-bit mantissa, ``LONGDOUBLE_OK``); only the layout of theta (unpack_theta, expand_gamma)
comes from oracle/gpz_oracle.py, and the package under test is never imported here.

The L-BFGS memory
-----------------
lbfgsAdd.m receives y = g - g_old and s = t*d as minFunc.m:553 forms them, in float64; the ring (``Ring``) takes them so and does the
rest - y's, y'y, Hdiag, the two-loop product - in long double.  ``gram_direction_f64`` restates the coefficient recursion of
gpz_lbfgs_direction (k_lbfgs.hip: every vector of the two-loop is a combination of [S Y g], the recursion runs on the Gram matrix)
in float64 NumPy; it exists only to measure how much a float64 evaluation of THAT form loses against the long-double two-loop, next
to the float64 two-loop of host._LBFGS.  The larger of the two is e_ref of a case:

    fitness   e_ref <= 1e-13                          (else the inputs cannot be judged)
    gate      rel(d_gpu, d_ld) <= 32 max(e_ref, 2^-52)

32: the device sums each p-term dot in 4096-row chunks of fma chains, NumPy sums pairwise, each error is one sample under the same
p eps bound.  A dropped row or column shows at 1e-6 or more.

getPrior
--------
``prior_fixed_point`` is the loop of getPrior.m:5-20 on a given N.  The cases move the centres of the last eight basis functions onto
rows of X: as make_problem draws them, the highest columns can have a prior of 1e-104 and a column the kernel never wrote would pass
a max-norm comparison.  Fitness: the largest reference prior among the last eight columns is at least 0.01 of the largest overall.
For the cases whose iteration count is compared, the reference's convergence ratio at the stopping iteration and at the one before
differ from 1e-10 by at least 1 %, so that no float64 rounding decides on which side of the test of getPrior.m:18 they fall.

Dxy
---
Dxy.m's own formula |xx + yy - 2 xy| cancels, so the gate is relative to the size of its terms, per element:

    |D - D_ld| <= (d + 4) 2^-52 (xx + yy)             d fma roundings in each of the three sums plus the final combination
"""
import functools

import numpy as np

from helpers import make_problem
from oracle import gpz_oracle as O

LD = np.longdouble
EPS = 2.0 ** -52
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 2e-19)
LONGDOUBLE_WHY = (f"the reference needs a 64-bit mantissa: np.longdouble has eps = {float(np.finfo(np.longdouble).eps):.3g} here "
                  "(need < 2e-19); no fall-back to float64")


def rel_ld(a, b):
    """max|a - b| / max|b|, the difference taken in long double."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), LD(1e-300)))


# ---- the L-BFGS memory ---------------------------------------------------------------------------------------------------------------
# (p, corrections, steps).  The first three rows were planned with 4, 8 and 6 steps; with every fifth step rejected (and, at p = 1, every
# pair whose one product y*s comes out negative) those cannot give corrections + 5 accepted pairs, which the wrap condition asks of every
# row with steps > corrections.  11, 13 and 7 are the smallest step counts that do.
LBFGS_CASES = [(1, 1, 11), (1, 3, 13), (63, 1, 7), (64, 2, 9), (65, 3, 12), (255, 5, 12), (257, 5, 12), (4095, 7, 20), (4096, 7, 20),
               (4097, 128, 175), (8193, 100, 30), (12289, 4, 12)]
LBFGS_FITNESS = 1e-13
LBFGS_WRAP_MARGIN = 5


def lbfgs_gate(e_ref):
    return 32.0 * max(e_ref, EPS)


def lbfgs_steps(p, steps):
    """The generator of test_host.py::test_device_lbfgs_direction_matches_two_loop: rng = default_rng(p), every fifth step a pair with
    y's < 0.  -> [(g, g_old, t, d)]"""
    rng = np.random.default_rng(p)
    out = []
    g_old = rng.standard_normal(p)
    for it in range(steps):
        d = rng.standard_normal(p)
        t = float(rng.random() + 0.1)
        g = g_old + (0.3 * t) * d + 0.05 * rng.standard_normal(p)
        if it % 5 == 3:
            g = g_old - 0.2 * t * d
        out.append((g, g_old, t, d))
        g_old = g
    return out


def two_loop(pairs, g, hdiag):
    """lbfgsProd.m:19-32 in long double.  pairs: [(s, y)], oldest first."""
    d = -np.asarray(g, dtype=LD)
    pairs = [(np.asarray(s, dtype=LD), np.asarray(y, dtype=LD)) for s, y in pairs]
    ys = [y @ s for s, y in pairs]
    al = [LD(0)] * len(pairs)
    for i in range(len(pairs) - 1, -1, -1):
        al[i] = (pairs[i][0] @ d) / ys[i]
        d = d - al[i] * pairs[i][1]
    d = LD(hdiag) * d
    for i in range(len(pairs)):
        be = (pairs[i][1] @ d) / ys[i]
        d = d + pairs[i][0] * (al[i] - be)
    return d


class Ring:
    """lbfgsAdd.m: the pair is skipped when y's <= 1e-10, the newest `corrections` accepted pairs are kept, Hdiag = y's / y'y of the
    newest."""

    def __init__(self, corrections):
        self.cap, self.pairs, self.hdiag, self.accepted = int(corrections), [], LD(1), 0

    def add(self, y, s):
        y, s = np.asarray(y, dtype=LD), np.asarray(s, dtype=LD)
        ys = y @ s
        if ys <= 1e-10:
            return False
        self.pairs = (self.pairs + [(s, y)])[-self.cap:]
        self.hdiag = ys / (y @ y)
        self.accepted += 1
        return True

    def add_step(self, g, g_old, t, d):
        return self.add(g - g_old, t * d)                     # float64, as minFunc.m hands them to lbfgsAdd

    def direction(self, g):
        return two_loop(self.pairs, g, self.hdiag)


class GramMemory64:
    """The coefficient form of gpz_lbfgs_direction in float64 NumPy: the Gram blocks S'S, S'Y, Y'Y grow by a row and a column per
    accepted pair (the old entries are kept, as on the device), the recursion of lbfgsProd.m runs on the coefficients of
    q = dg g + sum_c ds_c s_c + dy_c y_c, and the direction is one combination of [S Y g] at the end."""

    def __init__(self, corrections):
        self.cap, self.S, self.Y = int(corrections), [], []
        self.SS = self.SY = self.YY = np.zeros((0, 0))          # SY[a, b] = s_a . y_b

    def add(self, y, s):
        """an ACCEPTED pair (the ring decides)"""
        if len(self.S) == self.cap:
            self.S.pop(0); self.Y.pop(0)
            self.SS, self.SY, self.YY = self.SS[1:, 1:], self.SY[1:, 1:], self.YY[1:, 1:]
        self.S.append(np.asarray(s, dtype=np.float64)); self.Y.append(np.asarray(y, dtype=np.float64))
        Sm, Ym = np.array(self.S), np.array(self.Y)
        k = len(self.S)

        def grown(old, row, col):
            new = np.empty((k, k))
            new[:k - 1, :k - 1] = old
            new[k - 1, :], new[:, k - 1] = row, col
            return new
        ss, sy, ys, yy = Sm @ s, Sm @ y, Ym @ s, Ym @ y
        self.SS, self.SY, self.YY = grown(self.SS, ss, ss), grown(self.SY, ys, sy), grown(self.YY, yy, yy)

    def direction(self, g, hdiag):
        g = np.asarray(g, dtype=np.float64)
        k = len(self.S)
        if k == 0:
            return -g
        Sm, Ym, SS, SY, YY = np.array(self.S), np.array(self.Y), self.SS, self.SY, self.YY
        sg, yg = Sm @ g, Ym @ g
        ds, dy, al = np.zeros(k), np.zeros(k), np.zeros(k)
        dg = -1.0
        for i in range(k - 1, -1, -1):
            al[i] = (dg * sg[i] + ds @ SS[i] + dy @ SY[i]) / SY[i, i]
            dy[i] -= al[i]
        hd = float(hdiag)
        dg *= hd; ds *= hd; dy *= hd
        for i in range(k):
            be = (dg * yg[i] + ds @ SY[:, i] + dy @ YY[i]) / SY[i, i]
            ds[i] += al[i] - be
        return dg * g + ds @ Sm + dy @ Ym


def gram_direction_f64(pairs, g, hdiag):
    """The same on a list of pairs [(s, y)] (float64, oldest first)."""
    mem = GramMemory64(max(1, len(pairs)))
    for s, y in pairs:
        mem.add(y, s)
    return mem.direction(g, hdiag)


@functools.lru_cache(maxsize=None)
def lbfgs_case(p, corrections, steps, f64_memory=None):
    """One row of the table, replayed on the reference.  f64_memory: a class with host._LBFGS's interface (the test modules pass
    host._LBFGS itself), whose float64 two-loop enters e_ref.  -> dict: steps [(g, g_old, t, d)], added [bool], d_ld [long double
    direction after every step], accepted, e_two_loop, e_gram, e_ref, and the three memories as the last step left them (ring,
    two_loop_f64, gram_f64: read them, never add to them - the result is shared)."""
    ring = Ring(corrections)
    mem = f64_memory(p, corrections) if f64_memory is not None else None
    gram = GramMemory64(corrections)
    seq = lbfgs_steps(p, steps)
    added, d_ld, e_tl, e_gr = [], [], 0.0, 0.0
    for g, g_old, t, d in seq:
        a = ring.add_step(g, g_old, t, d)
        added.append(a)
        if a:
            gram.add(g - g_old, t * d)
        ref = ring.direction(g)
        d_ld.append(ref)
        e_gr = max(e_gr, rel_ld(gram.direction(g, ring.hdiag), ref))
        if mem is not None:
            assert mem.add_step(g, g_old, t, d) == a
            e_tl = max(e_tl, rel_ld(mem.direction(g), ref))
    return dict(steps=seq, added=added, d_ld=d_ld, accepted=ring.accepted, e_two_loop=e_tl, e_gram=e_gr, e_ref=max(e_tl, e_gr),
                ring=ring, two_loop_f64=mem, gram_f64=gram)


# ---- getPrior ------------------------------------------------------------------------------------------------------------------------
def prior_fixed_point(N, dtype=LD):
    """getPrior.m:5-20 on the densities N (n x m).  -> (prior, iterations, [convergence ratio of every iteration])"""
    N = np.asarray(N, dtype=dtype)
    m = N.shape[1]
    prior = np.ones(m, dtype=dtype) / dtype(m)
    ratios, it = [], 0
    for it in range(1, 101):
        old = prior
        w = N * prior
        w = w / w.sum(axis=1, keepdims=True)
        prior = w.mean(axis=0)
        r = np.sqrt(np.sum((old - prior) ** 2)) / np.sqrt(np.sum((old + prior) ** 2))
        ratios.append(float(r))
        if r < 1e-10:
            break
    return prior, it, ratios


def _abs_det_ld(A):
    """|det A| of a small matrix by elimination with partial pivoting, in long double."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    det = LD(1)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        if piv != c:
            A[[c, piv]] = A[[piv, c]]
        det = det * A[c, c]
        if A[c, c] != 0:
            A[c + 1:] = A[c + 1:] - np.outer(A[c + 1:, c] / A[c, c], A[c])
    return abs(det)


def norm_densities(model, theta, X):
    """N of getPHI.m:77,87,98 for complete rows without input noise, from the parameters directly:
        N_ij = exp(-1/2 |Gamma_j (x_i - p_j)|^2) |det Gamma_j| (2 pi)^(-d/2)
    (diagonal kinds: Gamma_j = diag(gamma_j.)), in long double."""
    P, G, *_ = O.unpack_theta(np.asarray(theta, dtype=np.float64), model)
    Gam = O.expand_gamma(G, model)
    X = np.asarray(X, dtype=LD)
    P = np.asarray(P, dtype=LD)
    n, d, m = X.shape[0], model.d, model.m
    cn = (8 * np.arctan(LD(1))) ** (-LD(d) / 2)                  # (2 pi)^(-d/2), pi to the full mantissa
    N = np.empty((n, m), dtype=LD)
    for j in range(m):
        D = X - P[j]
        if model.method[1] == "C":
            Gj = np.asarray(Gam[:, :, j], dtype=LD)
            q = np.sum((D @ Gj.T) ** 2, axis=1)
            det = _abs_det_ld(Gj)
        else:
            gj = np.asarray(Gam[j], dtype=LD)
            q = np.sum((D * gj) ** 2, axis=1)
            det = np.prod(np.abs(gj))
        N[:, j] = np.exp(-q / 2) * det * cn
    return N


def _case(id, method, d, m, n, nan=False, psi=False, gamma_scale=1.0):
    return dict(id=id, method=method, d=d, m=m, n=n, nan=nan, psi=psi, gamma_scale=gamma_scale)


PRIOR_CASES = (
    [_case("wave-m%d" % m, "VD", 2, m, 300) for m in (1, 63, 64, 65, 128, 129, 192, 193, 255, 256)]
    + [_case("wave-n%d" % n, "VD", 2, 65, n) for n in (4095, 4096, 4097, 8195)]
    + [_case("strip-m%d" % m, "VD", 2, m, 130) for m in (257, 512, 513, 1024, 2048, 2049, 4096)]
    + [_case("strip-n%d" % n, "VD", 2, 257, n) for n in (1023, 1024, 1025, 2050)]
    + [_case("strip-VC-m1025", "VC", 3, 1025, 130), _case("strip-GL-m513", "GL", 2, 513, 130)]
    + [_case("beyond16-m%d" % m, "VD", 2, m, 130) for m in (4097, 4500)]              # more than 16 strips of 256 columns
    # gamma_scale = 3: at d = 3 and 4 make_problem's 300 basis functions are so wide that the fixed point collapses onto one or two of
    # them whatever their centres (tail weight 1.5e-24 and 8.2e-7 as drawn); three times narrower, 145 and 207 columns keep weight
    + [_case("nan-VD-m300", "VD", 4, 300, 300, nan=True, gamma_scale=3.0), _case("psi-VD-m300", "VD", 3, 300, 300, psi=True, gamma_scale=3.0)])
PRIOR_BY_ID = {c["id"]: c for c in PRIOR_CASES}
PRIOR_TOL = 1e-8
PRIOR_TAIL_FITNESS = 0.01

# getPHI(..., want_N=True) on complete rows: (n, m) for VD (d = 2) and VC (d = 3); the NaN and Psi rows of PRIOR_CASES go against O.getPHI
N_CASES = [(method, d, n, m) for method, d in (("VD", 2), ("VC", 3)) for n, m in ((2047, 257), (2049, 513), (130, 4097))]


def prior_problem(case):
    """make_problem(n, d, m, 1, method, True, seed=900 + m) with the centres of the last eight basis functions (all of them when
    m < 8) moved onto the first eight rows of X that have no missing value, and Gamma multiplied by the case's gamma_scale.
    -> (model, theta, X, Psi)"""
    model, theta, X, _, Psi, _ = make_problem(case["n"], case["d"], case["m"], 1, case["method"], True, seed=900 + case["m"],
                                              psi=case["psi"], nanfrac=0.3 if case["nan"] else 0.0)
    m, d = model.m, model.d
    rows = np.flatnonzero(~np.isnan(X).any(axis=1))[:min(8, m)]
    P = theta[:m * d].reshape((m, d), order="F").copy()
    P[m - rows.size:] = X[rows]
    theta = theta.copy()
    theta[:m * d] = P.ravel(order="F")
    theta[m * d:m * d + model.g_dim] *= case["gamma_scale"]
    return model, theta, X, Psi


def n_problem(method, d, n, m):
    return prior_problem(_case("", method, d, m, n))[:3]


@functools.lru_cache(maxsize=None)
def prior_reference(case_id):
    """-> (prior_ld, iterations, ratios, N_ld).  Complete rows without input noise: N from the parameters (norm_densities); the NaN
    and Psi cases: the oracle's float64 N cast up."""
    case = PRIOR_BY_ID[case_id]
    model, theta, X, Psi = prior_problem(case)
    if case["nan"] or case["psi"]:
        N = np.asarray(O.getPHI(X, Psi, theta, model, None, want_N=True)[3], dtype=LD)
    else:
        N = norm_densities(model, theta, X)
    return prior_fixed_point(N, LD) + (N,)


def tail_weight(prior, m):
    """largest prior among the last eight columns / largest overall"""
    return float(np.max(prior[max(0, m - 8):]) / np.max(prior))


# cases whose ITERATION COUNT is compared
def counted_problem(which):
    """-> (model, theta, X).  "first-batch": three basis functions far apart, every row next to exactly one of them, unequal shares -
    converges within the first batch of ten; "later-batch": test_get_prior's problem on all rows, stops at 61; "limit": a table case
    that runs into the limit of 100."""
    if which == "first-batch":
        model, theta, X, _, _, _ = make_problem(60, 2, 3, 1, "VD", True, seed=5)
        centres = np.array([[-5.0, 0.0], [0.0, 5.0], [5.0, 0.0]])
        rng = np.random.default_rng(5)
        X = np.repeat(centres, [10, 20, 30], axis=0) + 0.1 * rng.standard_normal((60, 2))
        theta = theta.copy()
        theta[:6] = centres.ravel(order="F")
        return model, theta, X
    if which == "later-batch":
        model, theta, X, _, _, _ = make_problem(400, 3, 7, 1, "VD", True, seed=77)
        return model, theta, X
    return prior_problem(PRIOR_BY_ID["wave-m65"])[:3]


COUNTED = {"first-batch": (2, 10), "later-batch": (11, 99), "limit": (100, 100)}          # where the reference's count has to fall


@functools.lru_cache(maxsize=None)
def counted_reference(which):
    model, theta, X = counted_problem(which)
    return prior_fixed_point(norm_densities(model, theta, X), LD)


def count_is_decidable(it, ratios):
    """The ratio at the stopping iteration and the one before differ from 1e-10 by at least 1 %."""
    last = ratios[it - 1:it] + ratios[it - 2:it - 1] if it >= 2 else ratios[:1]
    return all(abs(r - 1e-10) >= 1e-12 for r in last)


# ---- Dxy -----------------------------------------------------------------------------------------------------------------------------
def _dxy_case(id, nx, ny, d, shift=0.0, coincident=False):
    return dict(id=id, nx=nx, ny=ny, d=d, shift=shift, coincident=coincident)


DXY_CASES = ([_dxy_case("%dx%dx%d" % s, *s) for s in ((1, 1, 1), (255, 1, 3), (256, 2, 3), (257, 3, 1), (1000, 77, 10), (513, 300, 20),
                                                        (3, 70000, 2))]
             + [_dxy_case("1000x77x10-shifted", 1000, 77, 10, shift=1e4), _dxy_case("1000x77x10-coincident", 1000, 77, 10, coincident=True)])
DXY_BY_ID = {c["id"]: c for c in DXY_CASES}


def dxy_inputs(case):
    rng = np.random.default_rng(1000 * case["nx"] + case["ny"] + case["d"])
    X = rng.standard_normal((case["nx"], case["d"])) + case["shift"]
    Y = X[:case["ny"]].copy() if case["coincident"] else rng.standard_normal((case["ny"], case["d"])) + case["shift"]
    return X, Y


def dxy(X, Y):
    """Dxy.m:3-7 in long double.  -> (D, xx + yy per element)"""
    X, Y = np.asarray(X, dtype=LD), np.asarray(Y, dtype=LD)
    xx = np.sum(X * X, axis=1)[:, None]
    yy = np.sum(Y * Y, axis=1)[None, :]
    xy = np.zeros((X.shape[0], Y.shape[0]), dtype=LD)
    for c in range(X.shape[1]):
        xy += X[:, c][:, None] * Y[:, c][None, :]
    return np.abs(yy + (xx - 2 * xy)), xx + yy


@functools.lru_cache(maxsize=None)
def dxy_reference(case_id):
    return dxy(*dxy_inputs(DXY_BY_ID[case_id]))


def dxy_worst(D, D_ld, T, d):
    """-> the largest |D - D_ld| / ((d + 4) 2^-52 (xx + yy)) over the elements; the gate is <= 1."""
    return float(np.max(np.abs(np.asarray(D, dtype=LD) - D_ld) / ((d + 4) * LD(EPS) * T)))
