"""The per-group gradient gate of tests/helpers.py, without a GPU: the partition of theta, that the gate catches errors the
whole-vector gate misses, and that every case of the GPU table (tests/test_grad_groups.py) can be judged: its two fp64
references (the NumPy oracle and torch autograd of tests/mp_reference.py's objective) agree to 1e-8 on every group."""
import numpy as np
import pytest

from oracle import gpz_oracle as O
from helpers import (GRAD_GROUP_CASES, GROUP_FITNESS, assert_grad_groups, grad_group_problem, grad_group_problem_key, grad_groups,
                     grad_tol, group_reference_errors, make_problem, rel, torch_gradient)

METHODS = ["GL", "VL", "GD", "VD", "GC", "VC"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("hetero", [True, False])
@pytest.mark.parametrize("m", [1, 31, 32, 33, 257])
def test_partition(method, k, hetero, m):
    d = 3
    model = O.Model(m=m, d=d, k=k, method=method, heteroscedastic=hetero)
    p = O.theta_len(model)
    groups = grad_groups(model)
    allidx = np.concatenate(list(groups.values()))
    assert np.array_equal(np.sort(allidx), np.arange(p))                  # disjoint, and they cover theta
    assert all(np.array_equal(v, np.unique(v)) for v in groups.values())
    blocks = {name.split("[")[0] for name in groups}
    assert blocks == {"dP", "dG", "dlnA", "db"} | ({"dv", "dlnT"} if hetero else set())
    if method in ("GL", "GD", "GC"):
        assert "dG" in groups and groups["dG"].size == model.g_dim
    assert groups["db"].size == k
    if m == 257:
        assert groups["dlnA[256:257]"].size == k and groups["dP[256:257]"].size == d

    def where(e):                                                          # the group that holds index e
        hit = [name for name, idx in groups.items() if e in idx]
        assert len(hit) == 1
        return hit[0]

    def moved(which, pos, value=7.25):
        """The index of theta that O.unpack_theta reads parameter `which`[pos] from."""
        hits = []
        for e in range(p) if p <= 400 else cand[which]:
            th = np.zeros(p); th[e] = value
            arr = O.unpack_theta(th, model)[which]
            if which == 1:
                arr = O.expand_gamma(arr, model)
            if arr[pos] == value:
                hits.append(e)
        return hits

    # candidate indices for the large shapes (a full scan of theta costs p unpackings): the block of the named parameter
    md, gd, mk = m * d, model.g_dim, m * k
    cand = {0: range(0, md), 1: range(md, md + gd), 2: range(md + gd, md + gd + mk), 4: range(md + gd + mk + k, md + gd + 2 * mk + k),
            5: range(md + gd + 2 * mk + k, p)}
    for j in sorted({0, m // 2, m - 1}):
        grp = "[%d:%d]" % (j // 32 * 32, min(j // 32 * 32 + 32, m))
        q, c = k - 1, d - 1
        (e,) = moved(0, (j, c)); assert where(e) == "dP" + grp
        (e,) = moved(2, (j, q)); assert where(e) == "dlnA" + grp
        if hetero:
            (e,) = moved(4, (j, q)); assert where(e) == "dv" + grp
            (e,) = moved(5, (j, q)); assert where(e) == "dlnT" + grp
        # Gamma through expand_gamma: VD m x d, VC d x d x m; the shared kinds repeat one parameter over j
        pos = (1, c, j) if method[1] == "C" else (j, c)
        es = moved(1, pos)
        assert len(es) == 1
        assert where(es[0]) == ("dG" + grp if method[0] == "V" else "dG")
    assert where(md + gd + mk) == "db"


@pytest.fixture(scope="module")
def vd257():
    model, theta, X, Y, Psi, rng = make_problem(600, 3, 257, 1, "VD", True, seed=11)
    ref = O.GPz(theta, model, X, Y)
    return model, theta, X, Y, ref, torch_gradient(model, theta, X, Y)


def test_the_unperturbed_oracle_gradient_passes(vd257):
    model, theta, X, Y, ref, g2 = vd257
    rep = assert_grad_groups(ref.grad.copy(), model, theta, X, Y, None, None, None, ref.cond, ref.grad, g_second=g2)
    assert rep["worst_ratio"][0] == 0.0 and rep["worst_e"][0] <= GROUP_FITNESS


@pytest.mark.parametrize("group", ["dlnA[256:257]", "dP[256:257]", "dG[128:160]"])
def test_the_gate_catches_what_the_whole_vector_gate_misses(vd257, group):
    """A relative error in the entries of one group, as large as max|g - g_ref| / max|g_ref| <= grad_tol lets through (0.9 of
    that, and 1e-5 at the most): 1e-5 for dlnA of j = 256, 7e-7 for dP of j >= 256, 9e-8 for a middle group of dG, whose
    largest entries are 7e-4, 1.2e-2 and 0.1 of max|g|.  The gate per group names each."""
    model, theta, X, Y, ref, g2 = vd257
    g = ref.grad.copy()
    idx = grad_groups(model)[group]
    size = min(1e-5, 0.9 * grad_tol(ref.cond) * np.max(np.abs(ref.grad)) / np.max(np.abs(ref.grad[idx])))
    assert size >= 8e-8                                                     # (eight times the gate per group, at the least)
    g[idx] *= 1.0 + size
    assert rel(g, ref.grad) <= grad_tol(ref.cond)
    with pytest.raises(AssertionError) as ei:
        assert_grad_groups(g, model, theta, X, Y, None, None, None, ref.cond, ref.grad, g_second=g2)
    msg = str(ei.value)
    assert group in msg and "tolerance" in msg and "e_B" in msg
    assert msg.count("error") == 1                                         # that group and no other


def test_a_case_that_cannot_be_judged_is_refused(vd257):
    model, theta, X, Y, ref, g2 = vd257
    bad = g2.copy()
    bad[grad_groups(model)["dv[32:64]"]] *= 1.0 + 1e-6                       # the references disagree: not the kernel's fault
    with pytest.raises(AssertionError, match="cannot be judged"):
        assert_grad_groups(ref.grad, model, theta, X, Y, None, None, None, ref.cond, ref.grad, g_second=bad)


_PROBLEMS = {}
for _c in GRAD_GROUP_CASES:
    _PROBLEMS.setdefault(grad_group_problem_key(_c), _c)


@pytest.mark.parametrize("case", list(_PROBLEMS.values()), ids=[c["id"] for c in _PROBLEMS.values()])
def test_every_case_of_the_gpu_table_can_be_judged(case):
    model, theta, X, Y, Psi, omega, training, validation = grad_group_problem(case)
    ref = O.GPz(theta, model, X, Y, Psi, omega, training, validation)
    g2 = torch_gradient(model, theta, X, Y, Psi, omega, training)
    errs = group_reference_errors(model, ref.grad, g2)
    worst = max((e, name) for name, (s, e) in errs.items())
    print("fitness %s cond %.2e worst e_B %.2e (%s)" % (case["id"], ref.cond, worst[0], worst[1]))
    assert worst[0] <= GROUP_FITNESS, worst
