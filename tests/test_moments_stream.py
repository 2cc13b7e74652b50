"""The streaming moment kernel of the covariance kinds with many basis functions (k_moments_ring.hip: PHI and T through an LDS ring,
raw sums about the rows' column means) against the kernel it replaces on those shapes (k_moments_fused: developer build,
GPZ_MOMENTS_RING_OFF) and against the oracle.

Bounds.  The two routes differ in the moment stage only: the objective and the four statistics do not depend on it and must carry the
same bits; the gradients must agree to 1e-10 of max|g| - one hundredth of the 1e-8 gate against the oracle, so
that no parity figure of the route moves visibly.  Against the oracle both routes pass the gate of tests/helpers.py (grad_tol).
Measured figures: DESIGN.md section 8."""
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


def _mk(model, X, Y, om, tr, va, shards):
    if shards > 1:
        return gpz_amd.GPzMulti(model, X, Y, None, om, tr, va, n_gpus=shards, reducer="loopback")
    return gpz_amd.GPzContext(model, X, Y, None, om, tr, va)


def _route(ctx, shards):
    return ctx.route(0) if shards > 1 else ctx.route()


def _old_route(tmp_path, model, thetas, X, Y, om, tr, va, shards, env_extra):
    """The same evaluations in a FRESH process on the developer build with GPZ_MOMENTS_RING_OFF -> (f[], g[], stats[], route)"""
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
            "out = []\n"
            "for t in z['thetas']:\n"
            "    f, g = ctx.eval(t); out.append((f, g, [ctx.stats.get(k, 0.0) for k in ('trainRMSE', 'trainLL', 'validRMSE', 'validLL')], ctx.info))\n"
            "route = ctx.route(0) if S > 1 else ctx.route()\n"
            "ctx.close()\n"
            "np.savez(%r, f=np.array([o[0] for o in out]), g=np.stack([o[1] for o in out]), st=np.array([o[2] for o in out]),\n"
            "         info=np.array([o[3] for o in out]), route=route)\n"
            ) % (ROOT, str(tmp_path / "in.npz"), model.m, model.d, model.k, model.method, shards, str(tmp_path / "out.npz"))
    env = dict(os.environ, GPZ_HIP_LIB=DEV_LIB, GPZ_MOMENTS_RING_OFF="1", **env_extra)
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=900)
    o = np.load(tmp_path / "out.npz")
    assert "k_moments_ring" not in str(o["route"]), str(o["route"])
    assert (o["info"] == 0).all()
    return o["f"], o["g"], o["st"]


def _stats(ctx):
    return [ctx.stats.get(k, 0.0) for k in ("trainRMSE", "trainLL", "validRMSE", "validLL")]


def _compare(tmp_path, monkeypatch, method, d, m, n, k=1, omega=None, masks=False, shards=1, tile=0, seed=0):
    model, theta, X, Y, _, rng = make_problem(n, d, m, k, method, True, seed=8800 + seed + m + d)
    om = None
    if omega == "n1":
        om = rng.random((n, 1)) + 0.5
    elif omega == "nk":
        om = rng.random((n, k)) + 0.5
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
        st = _stats(ctx)
        f2, g2 = ctx.eval(theta)
        route = _route(ctx, shards)
        assert ctx.info == 0
    finally:
        ctx.close()
    assert "moments: k_moments_ring" in route, route
    assert ("streamed" in route) == bool(tile), route
    assert f2 == f and np.array_equal(g, g2)                       # the same bits from the same theta
    fo, go, sto = _old_route(tmp_path, model, [theta], X, Y, om, tr, va, shards, env_extra)
    tol = grad_tol(ref.cond)
    e_new, e_old, e_routes = rel(g, ref.grad), rel(go[0], ref.grad), rel(g, go[0])
    print(f"moments_stream {method} d={d} m={m} n={n} k={k} shards={shards} tile={tile}: new vs oracle {e_new:.2e}, old vs oracle {e_old:.2e}, "
          f"new vs old {e_routes:.2e} (gate {tol:.1e})")
    assert abs(f - ref.nlogML) <= FTOL * abs(ref.nlogML)
    assert e_new <= tol and e_old <= tol, (e_new, e_old, tol)
    assert e_routes <= ROUTE_TOL, e_routes
    assert fo[0] == f, (fo[0], f)                                  # f and the statistics do not depend on the moment stage
    assert list(sto[0]) == st, (list(sto[0]), st)


@pytest.mark.parametrize("method", ["VC", "GC"])
@pytest.mark.parametrize("d", [8, 10])
@pytest.mark.parametrize("m", [257, 500, 1000, 1001])
def test_ring_route_agrees_with_the_register_prefetch_kernel_and_the_oracle(tmp_path, monkeypatch, method, d, m):
    """Column counts that end inside a wave's 32 columns (257, 1001), inside a 16-block (500, 1000: mp = 512, 1008), row counts that are
    no multiple of the chunk or of the ring's 8-row slots."""
    _compare(tmp_path, monkeypatch, method, d, m, n=2400 + 7 * d + (m % 13))


@pytest.mark.parametrize("case", [
    dict(method="VC", d=10, m=300, n=3001, k=2, omega="nk", masks=True),          # sums over outputs, omega n x k, validation rows
    dict(method="GC", d=8, m=260, n=2777, k=2, omega="n1"),                       # omega n x 1
    dict(method="VC", d=10, m=300, n=3500, masks=True, shards=2),                 # two loopback shards, each about its own column means
    dict(method="VC", d=10, m=300, n=3500, tile=1024),                            # forced row tiles: 4 tiles, the last one short
    dict(method="GC", d=8, m=400, n=2100, k=2, omega="nk", tile=1024),
])
def test_ring_route_outputs_weights_masks_shards_and_row_tiles(tmp_path, monkeypatch, case):
    _compare(tmp_path, monkeypatch, seed=17, **case)


def test_ring_route_moment_sums_far_from_the_origin(tmp_path, monkeypatch):
    """Inputs 1e4 standard deviations from the origin (un-normalised data), as test_small_tail_moment_sums_far_from_the_origin: the
    conversion of the raw sums about the column means (R2 - q_a R1_b - q_b R1_a + q_a q_b R0, q = p - mu) is where cancellation
    would show.  The old route (sums about the basis centres themselves) is measured against the oracle on the same input first; the
    new route may be at most 10 x worse and stays under that test's bound.  Measured figures: DESIGN.md section 8."""
    n, d, m = 2500, 10, 300
    model, theta, X, Y, _, rng = make_problem(n, d, m, 1, "VC", True, seed=516)
    shift = 1.0e4 * (1.0 + rng.random(d))
    Xs = X + shift
    theta_s = theta.copy()
    theta_s[:m * d] = (theta[:m * d].reshape((m, d), order="F") + shift).reshape(-1, order="F")
    ref = O.GPz(theta_s, model, Xs, Y)
    fo, go, _ = _old_route(tmp_path, model, [theta_s], Xs, Y, None, None, None, 1, {})
    ctx = gpz_amd.GPzContext(model, Xs, Y)
    try:
        f, g = ctx.eval(theta_s)
        assert "moments: k_moments_ring" in ctx.route()
    finally:
        ctx.close()
    e_old, e_new = rel(go[0], ref.grad), rel(g, ref.grad)
    print(f"moments_stream far from the origin: old vs oracle {e_old:.2e}, new vs oracle {e_new:.2e}, new vs old {rel(g, go[0]):.2e}")
    assert abs(f - ref.nlogML) <= FTOL * abs(ref.nlogML)
    assert e_new <= max(grad_tol(ref.cond), 1e-7)
    assert e_new <= 10.0 * e_old, (e_new, e_old)


@pytest.mark.parametrize("shards", [1, 2])
def test_ring_route_graph_replay_is_bitwise_the_eager_evaluation(shards, monkeypatch):
    model, theta, X, Y, _, rng = make_problem(2600, 10, 300, 1, "VC", True, seed=74)
    thetas = [theta + 0.01 * rng.standard_normal(theta.size) for _ in range(4)]
    res = {}
    for mode in ("graph", "eager"):
        if mode == "eager":
            monkeypatch.setenv("GPZ_NO_GRAPH", "1")
        else:
            monkeypatch.delenv("GPZ_NO_GRAPH", raising=False)
        ctx = _mk(model, X, Y, None, None, None, shards)
        try:
            res[mode] = [ctx.eval(t) for t in thetas] + [ctx.eval(thetas[0])]
            route = _route(ctx, shards)
        finally:
            ctx.close()
        assert "moments: k_moments_ring" in route and ("replayed" in route) == (mode == "graph"), route
    for (f0, g0), (f1, g1) in zip(res["graph"], res["eager"]):
        assert f0 == f1 and np.array_equal(g0, g1)
    assert res["graph"][0][0] == res["graph"][-1][0] and np.array_equal(res["graph"][0][1], res["graph"][-1][1])
