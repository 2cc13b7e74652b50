"""The covariance-kind PHI build on the f64 MFMA (k_phi_quad.hip: ln PHI = F C over centred row monomials, chosen per evaluation by a
bound on the product's rounding error) against the kernel it stands in for (k_phi_cov: developer build, GPZ_PHI_QUAD_OFF), against
the oracle, and against a long-double evaluation of PHI itself.

Bounds.  Both routes pass the gate of tests/helpers.py (grad_tol) and FTOL = 1e-8 against the oracle.  Between the routes f agrees
to 1e-10 relative and g to 1e-10 of max|g| - ROUTE_TOL, one hundredth of the gate, so that no parity figure moves visibly.  An
evaluation whose bound exceeds 2^-33 must BE the old route: the same bits.  Measured figures: DESIGN.md section 8."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpz_amd
from oracle import gpz_oracle as O
from helpers import DEV_LIB, ROOT, grad_tol, make_problem, rel

pytestmark = pytest.mark.gpu
FTOL = 1e-8
ROUTE_TOL = 1e-10
TAU = 2.0 ** -33


def _mk(model, X, Y, om, tr, va, shards):
    if shards > 1:
        return gpz_amd.GPzMulti(model, X, Y, None, om, tr, va, n_gpus=shards, reducer="loopback")
    return gpz_amd.GPzContext(model, X, Y, None, om, tr, va)


def _route(ctx, shards):
    return ctx.route(0) if shards > 1 else ctx.route()


def _last_phi(ctx, shards):
    """(some rank fell back, the largest bound over the ranks)"""
    if shards > 1:
        lp = [ctx.last_phi(r) for r in range(shards)]
        return any(fb for fb, _ in lp), max(b for _, b in lp)
    return ctx.last_phi()


def _old_route(tmp_path, model, thetas, X, Y, om=None, tr=None, va=None, shards=1, env_extra=None, want_phi=False):
    """The same evaluations in a FRESH process on the developer build with GPZ_PHI_QUAD_OFF -> (f[], g[], PHI of the last or None)"""
    if not os.path.exists(DEV_LIB):
        subprocess.run(["bash", os.path.join(ROOT, "build.sh"), "--dev"], cwd=ROOT, check=True, capture_output=True, timeout=1800)
    np.savez(tmp_path / "in.npz", thetas=np.stack(thetas), X=X, Y=Y, om=(om if om is not None else np.zeros(0)),
             tr=(tr if tr is not None else np.zeros(0, bool)), va=(va if va is not None else np.zeros(0, bool)))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import gpz_amd\n"
            "z = np.load(%r)\n"
            "model = gpz_amd.Model(m=%d, d=%d, k=%d, method=%r, heteroscedastic=True)\n"
            "om = z['om'] if z['om'].size else None; tr = z['tr'] if z['tr'].size else None; va = z['va'] if z['va'].size else None\n"
            "S = %d\n"
            "ctx = gpz_amd.GPzMulti(model, z['X'], z['Y'], None, om, tr, va, n_gpus=S, reducer='loopback') if S > 1 else "
            "gpz_amd.GPzContext(model, z['X'], z['Y'], None, om, tr, va)\n"
            "out = [ctx.eval(t) for t in z['thetas']]\n"
            "route = ctx.route(0) if S > 1 else ctx.route()\n"
            "phi = ctx.phi() if %d else np.zeros(0)\n"
            "ctx.close()\n"
            "np.savez(%r, f=np.array([o[0] for o in out]), g=np.stack([o[1] for o in out]), route=route, phi=phi)\n"
            ) % (ROOT, str(tmp_path / "in.npz"), model.m, model.d, model.k, model.method, shards, int(want_phi), str(tmp_path / "out.npz"))
    env = dict(os.environ, GPZ_HIP_LIB=DEV_LIB, GPZ_PHI_QUAD_OFF="1", **(env_extra or {}))
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=900)
    o = np.load(tmp_path / "out.npz")
    assert "k_phi_quad" not in str(o["route"]), str(o["route"])
    return o["f"], o["g"], (o["phi"] if want_phi else None)


def _scale_gamma(model, theta, s):
    """theta with every Gamma_j multiplied by s (the basis functions s times narrower)"""
    t = theta.copy()
    md = model.m * model.d
    gdim = model.d * model.d * (model.m if model.method == "VC" else 1)
    t[md:md + gdim] *= s
    return t


def _compare(tmp_path, monkeypatch, method, d, m, n, k=1, omega=None, masks=False, shards=1, tile=0, seed=0, quad=True):
    model, theta, X, Y, _, rng = make_problem(n, d, m, k, method, True, seed=9900 + seed + m + d)
    om = None
    if omega == "n1":
        om = rng.random((n, 1)) + 0.5
    tr = va = None
    if masks:
        tr = rng.random(n) < 0.8
        va = ~tr
    env_extra = {}
    if tile:
        monkeypatch.setenv("GPZ_ROW_TILE", str(tile))
        env_extra["GPZ_ROW_TILE"] = str(tile)
    ref = O.GPz(theta, model, X, Y, None, om, tr, va)
    ctx = _mk(model, X, Y, om, tr, va, shards)
    try:
        f, g = ctx.eval(theta)
        fell, bound = _last_phi(ctx, shards)
        f2, g2 = ctx.eval(theta)
        route = _route(ctx, shards)
        assert ctx.info == 0
    finally:
        ctx.close()
    assert ("PHI: k_phi_quad" in route) == quad, route
    assert ("streamed" in route) == bool(tile), route
    if quad:
        assert not fell and 0.0 < bound <= TAU, (fell, bound)
    else:
        assert not fell and bound == 0.0, (fell, bound)
    assert f2 == f and np.array_equal(g, g2)                       # the same bits from the same theta
    fo, go, _ = _old_route(tmp_path, model, [theta], X, Y, om, tr, va, shards, env_extra)
    tol = grad_tol(ref.cond)
    e_new, e_old, e_routes = rel(g, ref.grad), rel(go[0], ref.grad), rel(g, go[0])
    print(f"phi_quad {method} d={d} m={m} n={n} k={k} shards={shards} tile={tile}: bound {bound:.2e}, new vs oracle {e_new:.2e}, "
          f"old vs oracle {e_old:.2e}, new vs old g {e_routes:.2e} f {abs(f - fo[0]) / abs(fo[0]):.2e} (gate {tol:.1e})")
    assert abs(f - ref.nlogML) <= FTOL * abs(ref.nlogML) and abs(fo[0] - ref.nlogML) <= FTOL * abs(ref.nlogML)
    assert e_new <= tol and e_old <= tol, (e_new, e_old, tol)
    assert abs(f - fo[0]) <= ROUTE_TOL * abs(fo[0]), (f, fo[0])
    assert e_routes <= ROUTE_TOL, e_routes
    if not quad:
        assert f == fo[0] and np.array_equal(g, go[0])             # nothing changed where the route is not taken


@pytest.mark.parametrize("method", ["VC", "GC"])
@pytest.mark.parametrize("d", [8, 10])
@pytest.mark.parametrize("m", [257, 500, 1001])
def test_quad_route_agrees_with_the_vector_kernel_and_the_oracle(tmp_path, monkeypatch, method, d, m):
    """Columns that end inside a 16-block (257 -> mp 272 with 14 padding columns, 500 -> 512, 1001 -> 1008), rows that are no multiple of
    16, 64 or the workgroup's 128."""
    _compare(tmp_path, monkeypatch, method, d, m, n=2400 + 7 * d + (m % 13))


@pytest.mark.parametrize("case", [
    dict(method="GC", d=8, m=260, n=2777, omega="n1"),                            # omega n x 1
    dict(method="VC", d=10, m=300, n=3001, masks=True),                           # training / validation masks (validation rows stay on k_phi_cov)
    dict(method="VC", d=10, m=300, n=3500, tile=1024),                            # forced row tiles: 4 tiles, the last one short
    dict(method="VC", d=10, m=300, n=3500, masks=True, shards=2),                 # two loopback shards, each about its own column means
    dict(method="VC", d=10, m=300, n=2600, k=2, quad=False),                      # two outputs: not this route, and nothing moves
])
def test_quad_route_weights_masks_row_tiles_shards_and_two_outputs(tmp_path, monkeypatch, case):
    _compare(tmp_path, monkeypatch, seed=23, **case)


def _phi_longdouble(model, theta, X):
    m, d = model.m, model.d
    P = theta[:m * d].reshape((m, d), order="F").astype(np.longdouble)
    G = theta[m * d:m * d + d * d * m].reshape((d, d, m), order="F").astype(np.longdouble)
    Xl = X.astype(np.longdouble)
    out = np.empty((X.shape[0], m), dtype=np.longdouble)
    for j in range(m):
        dl = Xl - P[j]
        y = dl @ G[:, :, j].T                                          # Gamma_j (x - p_j)
        out[:, j] = np.exp(-0.5 * np.sum(y * y, axis=1))
    return out


def test_phi_itself_against_long_double(tmp_path):
    """PHI = exp(-1/2 |Gamma_j (x - p_j)|^2) of ctx.phi() on both routes against NumPy in long double: the new route's largest absolute
    error is at most 10 x the old route's."""
    n, d, m = 1500, 10, 260
    model, theta, X, Y, _, rng = make_problem(n, d, m, 1, "VC", True, seed=4242)
    ref = _phi_longdouble(model, theta, X)
    ctx = gpz_amd.GPzContext(model, X, Y)
    try:
        ctx.eval(theta)
        assert "PHI: k_phi_quad" in ctx.route() and not ctx.last_phi()[0]
        phi = ctx.phi()
    finally:
        ctx.close()
    _, _, phi_old = _old_route(tmp_path, model, [theta], X, Y, want_phi=True)
    e_new = float(np.max(np.abs(phi.astype(np.longdouble) - ref)))
    e_old = float(np.max(np.abs(phi_old.astype(np.longdouble) - ref)))
    print(f"phi_quad PHI vs long double: new {e_new:.2e}, old {e_old:.2e}; max PHI {float(ref.max()):.3f}")
    assert phi.max() <= 1.0 and phi.min() >= 0.0
    assert e_new <= 10.0 * e_old, (e_new, e_old)


def test_quad_route_far_from_the_origin(tmp_path):
    """Inputs and centres 1e4 standard deviations from the origin (un-normalised data), as
    test_ring_route_moment_sums_far_from_the_origin: k_phi_cov's c_j = R_j p_j cancels there, the centred features do not.  The
    gradient error against the oracle is at most the old route's."""
    n, d, m = 2500, 10, 300
    model, theta, X, Y, _, rng = make_problem(n, d, m, 1, "VC", True, seed=516)
    shift = 1.0e4 * (1.0 + rng.random(d))
    Xs = X + shift
    theta_s = theta.copy()
    theta_s[:m * d] = (theta[:m * d].reshape((m, d), order="F") + shift).reshape(-1, order="F")
    ref = O.GPz(theta_s, model, Xs, Y)
    fo, go, _ = _old_route(tmp_path, model, [theta_s], Xs, Y)
    ctx = gpz_amd.GPzContext(model, Xs, Y)
    try:
        f, g = ctx.eval(theta_s)
        assert "PHI: k_phi_quad" in ctx.route()
        fell, bound = ctx.last_phi()
    finally:
        ctx.close()
    e_old, e_new = rel(go[0], ref.grad), rel(g, ref.grad)
    print(f"phi_quad far from the origin: bound {bound:.2e}, old vs oracle {e_old:.2e}, new vs oracle {e_new:.2e}, new vs old {rel(g, go[0]):.2e}")
    assert not fell
    assert abs(f - ref.nlogML) <= FTOL * abs(ref.nlogML)
    assert e_new <= e_old, (e_new, e_old)


def test_fallback_is_the_old_route_bit_for_bit_inside_the_replayed_graph(tmp_path):
    """Gamma x 100 exceeds the bound: that evaluation is k_phi_cov's, bit for bit, and the next one with the normal theta is back on the
    fast route - alternating, so that from the third evaluation on the replayed graph is what runs.  Gamma x 10 stays on the fast route
    and passes the oracle gate."""
    n, d, m = 2500, 10, 300
    model, theta, X, Y, _, rng = make_problem(n, d, m, 1, "VC", True, seed=77)
    t100, t10 = _scale_gamma(model, theta, 100.0), _scale_gamma(model, theta, 10.0)
    seq = [theta, t100, theta, t100, theta, t100, t10]
    fo, go, _ = _old_route(tmp_path, model, seq, X, Y)
    ref10 = O.GPz(t10, model, X, Y)
    ctx = gpz_amd.GPzContext(model, X, Y)
    try:
        res, lp = [], []
        for t in seq:
            res.append(ctx.eval(t))
            lp.append(ctx.last_phi())
        route = ctx.route()
    finally:
        ctx.close()
    assert "PHI: k_phi_quad" in route and "replayed" in route, route
    print("phi_quad fallback: bounds " + ", ".join(f"{b:.2e}" for _, b in lp))
    for i, t in enumerate(seq):
        f, g = res[i]
        if t is t100:
            assert lp[i][0] and lp[i][1] > TAU, lp[i]
            assert np.array_equal(np.float64(f), fo[i], equal_nan=True) and np.array_equal(g, go[i], equal_nan=True)
        else:
            assert not lp[i][0] and 0.0 < lp[i][1] <= TAU, lp[i]
    for i in (2, 4):                                                   # back on the fast route: the first evaluation's bits
        assert res[i][0] == res[0][0] and np.array_equal(res[i][1], res[0][1])
    f10, g10 = res[-1]
    assert abs(f10 - ref10.nlogML) <= FTOL * abs(ref10.nlogML)
    assert rel(g10, ref10.grad) <= grad_tol(ref10.cond), (rel(g10, ref10.grad), grad_tol(ref10.cond))
    assert abs(f10 - fo[-1]) <= ROUTE_TOL * abs(fo[-1]) and rel(g10, go[-1]) <= ROUTE_TOL


@pytest.mark.parametrize("shards", [1, 2])
def test_quad_route_graph_replay_is_bitwise_the_eager_evaluation(shards, monkeypatch):
    model, theta, X, Y, _, rng = make_problem(2600, 10, 300, 1, "VC", True, seed=74)
    thetas = [theta + 0.01 * rng.standard_normal(theta.size) for _ in range(3)]
    thetas.insert(2, _scale_gamma(model, theta, 100.0))                # one evaluation that falls back
    res, fell = {}, {}
    for mode in ("graph", "eager"):
        if mode == "eager":
            monkeypatch.setenv("GPZ_NO_GRAPH", "1")
        else:
            monkeypatch.delenv("GPZ_NO_GRAPH", raising=False)
        ctx = _mk(model, X, Y, None, None, None, shards)
        try:
            res[mode], fell[mode] = [], []
            for t in thetas + [thetas[0]]:
                res[mode].append(ctx.eval(t))
                fell[mode].append(_last_phi(ctx, shards)[0])
            route = _route(ctx, shards)
        finally:
            ctx.close()
        assert "PHI: k_phi_quad" in route and ("replayed" in route) == (mode == "graph"), route
        assert fell[mode] == [False, False, True, False, False], fell[mode]
    for (f0, g0), (f1, g1) in zip(res["graph"], res["eager"]):
        assert np.array_equal(np.float64(f0), np.float64(f1), equal_nan=True) and np.array_equal(g0, g1, equal_nan=True)
    assert res["graph"][0][0] == res["graph"][-1][0] and np.array_equal(res["graph"][0][1], res["graph"][-1][1])
