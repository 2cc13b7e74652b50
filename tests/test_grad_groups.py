"""The gradient of the HIP evaluation path, gated per parameter block and per group of 32 basis functions (helpers.grad_groups,
helpers.assert_grad_groups), on the smallest shapes that reach each route of the evaluation: the one-workgroup
kernels for m + k <= 256 and the first shapes beyond them, k_moments_ring with and without k_phi_quad, input noise on diagonal and
covariance kinds, missing values, several outputs, per-output weights with training / validation masks, the homoscedastic model,
rows streamed in tiles and rows sharded.  Every case asserts on gpz_ctx_route that the intended route ran, so a moved threshold
cannot silently take a case onto another kernel.  tests/test_grad_groups_cpu.py proves without a GPU that every case here can be
judged (its two CPU references agree to 1e-8 on every group)."""
import numpy as np
import pytest

import gpz_amd
from oracle import gpz_oracle as O
from helpers import GRAD_GROUP_CASES, assert_grad_groups, grad_group_problem

pytestmark = pytest.mark.gpu
FTOL = 1e-8


@pytest.mark.parametrize("case", GRAD_GROUP_CASES, ids=[c["id"] for c in GRAD_GROUP_CASES])
def test_gradient_groups(case, monkeypatch):
    model, theta, X, Y, Psi, omega, training, validation = grad_group_problem(case)
    ref = O.GPz(theta, model, X, Y, Psi, omega, training, validation)
    if case["row_tile"]:
        monkeypatch.setenv("GPZ_ROW_TILE", str(case["row_tile"]))
    else:
        monkeypatch.delenv("GPZ_ROW_TILE", raising=False)
    if case["shards"] > 1:
        ctx = gpz_amd.GPzMulti(model, X, Y, Psi, omega, training, validation, n_gpus=case["shards"], reducer="loopback")
    else:
        ctx = gpz_amd.GPzContext(model, X, Y, Psi, omega, training, validation)
    try:
        f, g = ctx.eval(theta)
        assert ctx.info == 0
        routes = [ctx.route(r) for r in range(case["shards"])] if case["shards"] > 1 else [ctx.route()]
    finally:
        ctx.close()
    for route in routes:
        for s in case["has"]:
            assert s in route, (s, route)
        for s in case["has_not"]:
            assert s not in route, (s, route)
    assert abs(f - ref.nlogML) <= FTOL * abs(ref.nlogML)
    rep = assert_grad_groups(g, model, theta, X, Y, Psi, omega, training, ref.cond, ref.grad)
    print("grad-groups %s | cond %.1e | worst e_B %.1e (%s) | worst error/tolerance %.3f (%s) | %s"
          % (case["id"], ref.cond, rep["worst_e"][0], rep["worst_e"][1], rep["worst_ratio"][0], rep["worst_ratio"][1], routes[0]))
