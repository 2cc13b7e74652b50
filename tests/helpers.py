"""Shared helpers for the test-suite."""
import glob
import os

import numpy as np

from oracle import gpz_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_names(prefix="g_"):
    """g_: GPz / getPHI / predictFull cases (make_golden.py); p_: predict with every branch; s_: truncating inv_logdet
    (make_golden_predict.py)."""
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def load_predict_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    model = O.Model(m=int(g["m"]), d=int(g["d"]), k=int(g["k"]), method=str(g["method"]), heteroscedastic=True)
    model.muX, model.sdX, model.muY = g["muX"], g["sdX"], g["muY"]
    model.sets["best"] = {"theta": g["theta"], "w": g["w"], "iSigma_w": g["iSigma_w"], "priors": g["priors"]}
    return g, model, (g["Psi"] if int(g["has_psi"]) else None)


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    model = O.Model(m=int(g["m"]), d=int(g["d"]), k=int(g["k"]), method=str(g["method"]),
                    heteroscedastic=bool(int(g["heteroscedastic"])))
    Psi = g["Psi"] if int(g["has_psi"]) else None
    if int(g["has_masks"]):
        omega, training, validation = g["omega"], g["training"], g["validation"]
    else:
        omega = training = validation = None
    return g, model, Psi, omega, training, validation


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def make_problem(n, d, m, k, method, hetero, seed, psi=False, nanfrac=0.0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    A = rng.standard_normal((d, k)) / np.sqrt(d)
    Y = np.sin(X @ A) + 0.1 * rng.standard_normal((n, k))
    Y -= Y.mean(0)
    model, theta = O.init_theta(X, Y, method, m, hetero, rng)
    theta = theta + 0.05 * rng.standard_normal(theta.size)
    if hetero:
        o = theta.size - 2 * m * k
        theta[o:o + m * k] = 0.05 * rng.standard_normal(m * k)
    Psi = None
    if psi:
        if model.method[1] == "C":
            Psi = np.zeros((d, d, n))
            for i in range(n):
                B = 0.3 * rng.standard_normal((d, d))
                Psi[:, :, i] = B @ B.T
        else:
            Psi = rng.gamma(1.0, 0.2, (n, d))
    if nanfrac > 0 and d > 1:
        rows = rng.random(n) < nanfrac
        X[rows, rng.integers(0, d, n)[rows]] = np.nan
    return model, theta, X, Y, Psi, rng


def recondition_gamma(model, theta, rng, amp=0.3):
    """Redraw the Gamma blocks of a GC/VC theta as gamma_j (I + amp G / sqrt(d)).  make_problem's 0.05 N(0,1) perturbation of
    gamma_j I is larger than gamma_j itself once d ~ 20 (cond(Gamma'Gamma) ~ 1e8 ... 1e9): with input noise the reference's own
    dGamma chain loses cond^1.5 eps there and both sides of a comparison are rounding noise."""
    if model.method[1] != "C":
        return theta
    m, d = model.m, model.d
    md = m * d
    for q in range(1 if model.method == "GC" else m):
        blk = theta[md + q * d * d: md + (q + 1) * d * d].reshape((d, d), order="F")
        gam = float(np.mean(np.diag(blk)))
        theta[md + q * d * d: md + (q + 1) * d * d] = (gam * (np.eye(d) + amp * rng.standard_normal((d, d)) / np.sqrt(d))).reshape(-1, order="F")
    return theta


def grad_tol(cond):
    """Parity gate of BASELINE.md §6."""
    return max(1e-8, 50.0 * cond * 2.2e-16)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "gpz_amd", "lib", "libgpz_hip_dev.so")


def eval_with_dev_switches(tmp_path, method, m, d, k, hetero, theta, X, Y, Psi, switches):
    """One evaluation in a FRESH process on the developer build of the library (./build.sh --dev: -DGPZ_DEV_SWITCHES, the only build
    in which the A/B switches of gpz_amd/csrc/gpz_options.h exist), with `switches` in its environment.  -> (f, g, info)"""
    import subprocess
    import sys
    if not os.path.exists(DEV_LIB):      # (normally built by __graft_entry__.build() and shipped in-tree; a bare checkout builds it here)
        subprocess.run(["bash", os.path.join(ROOT, "build.sh"), "--dev"], cwd=ROOT, check=True, capture_output=True, timeout=1800)
    assert os.path.exists(DEV_LIB), "developer build missing: ./build.sh --dev failed"
    np.savez(tmp_path / "in.npz", theta=theta, X=X, Y=Y, Psi=(Psi if Psi is not None else np.zeros(0)), has_psi=int(Psi is not None))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import gpz_amd\n"
            "z = np.load(%r)\n"
            "model = gpz_amd.Model(m=%d, d=%d, k=%d, method=%r, heteroscedastic=%r)\n"
            "ctx = gpz_amd.GPzContext(model, z['X'], z['Y'], z['Psi'] if int(z['has_psi']) else None)\n"
            "f, g = ctx.eval(z['theta']); info = ctx.info; ctx.close()\n"
            "np.savez(%r, f=f, g=g, info=info)\n") % (ROOT, str(tmp_path / "in.npz"), m, d, k, method, bool(hetero), str(tmp_path / "out.npz"))
    env = dict(os.environ, GPZ_HIP_LIB=DEV_LIB, **{k_: str(v) for k_, v in switches.items()})
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=600)
    o = np.load(tmp_path / "out.npz")
    return float(o["f"]), o["g"], int(o["info"])


# ---- the gradient gate per parameter block and basis-function group ---------------------------------
def grad_groups(model, width=32):
    """Partition of the indices of theta into named groups.  Blocks with one entry per basis function (dP, dG of VL / VD / VC,
    dlnA, dv, dlnT) are cut by basis-function index j into groups of `width`, in the column-major layout of O.unpack_theta and
    tests/mp_reference.py; dG of GL / GD / GC and db are one group each.  32 divides every tile edge of the kernels (the
    16-column blocks of k_small, the Cholesky panels of 32, the 64- and 128-column tiles), and m = 257 leaves a group that holds
    j = 256 alone.  -> {"dP[0:32]": index array, ..., "db": ...}; every index of theta is in exactly one group."""
    m, d, k, method = model.m, model.d, model.k, model.method
    j = np.arange(m)
    per_j = {"dP": j[:, None] + m * np.arange(d)[None, :]}                     # [j, entries of j] -> offset inside the block
    blocks = [("dP", m * d, "dP")]
    if method == "VL":
        per_j["dG"] = j[:, None]
    elif method == "VD":
        per_j["dG"] = per_j["dP"]
    elif method == "VC":
        per_j["dG"] = d * d * j[:, None] + np.arange(d * d)[None, :]
    blocks.append(("dG", model.g_dim, "dG" if "dG" in per_j else None))
    per_j["mk"] = j[:, None] + m * np.arange(k)[None, :]
    blocks += [("dlnA", m * k, "mk"), ("db", k, None)]
    if model.heteroscedastic:
        blocks += [("dv", m * k, "mk"), ("dlnT", m * k, "mk")]
    groups, o = {}, 0
    for name, size, layout in blocks:
        if layout is None:
            groups[name] = o + np.arange(size)
        else:
            for a in range(0, m, width):
                groups["%s[%d:%d]" % (name, a, min(a + width, m))] = np.sort(o + per_j[layout][a:a + width].ravel())
        o += size
    assert o == O.theta_len(model)
    return groups


def torch_gradient(model, theta, X, Y, Psi=None, omega=None, training=None):
    """The second, independent fp64 gradient: torch.autograd of mp_reference.torch_nlogml on the CPU, on the training rows
    (validation rows do not enter the gradient; GPz.m:24 normalises by the number of training rows)."""
    import torch
    import mp_reference as R
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64).reshape(X.shape[0], -1)
    if omega is not None:
        omega = np.asarray(omega, dtype=np.float64).reshape(X.shape[0], -1)
    if training is not None:
        tr = np.asarray(training, dtype=bool)
        X, Y = X[tr], Y[tr]
        omega = None if omega is None else omega[tr]
        if Psi is not None:
            Psi = Psi[:, :, tr] if Psi.ndim == 3 else Psi[tr]
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    f = R.torch_nlogml(th, model.method, model.m, model.d, model.k, model.heteroscedastic, X, Y, Psi, omega)
    f.backward()
    return th.grad.numpy().copy()


GROUP_FITNESS = 1e-8          # the two fp64 references must agree to this on every group, or the case cannot be judged


def group_reference_errors(model, g_ref, g_second, width=32):
    """-> {group: (s_B, e_B)}: s_B = max|g_ref[B]|, e_B = max|g_ref[B] - g_second[B]| / s_B."""
    out = {}
    for name, idx in grad_groups(model, width).items():
        s = max(float(np.max(np.abs(g_ref[idx]))), 1e-300)
        out[name] = (s, float(np.max(np.abs(g_ref[idx] - g_second[idx]))) / s)
    return out


def assert_grad_groups(g, model, theta, X, Y, Psi, omega, training, cond, g_oracle, floor=1e-8, g_second=None, width=32):
    """The gradient gate per group.  For every group B of grad_groups, with s_B = max|g_oracle[B]| and e_B the disagreement of the
    two CPU references on B (g_oracle against torch autograd of the objective, relative to s_B):

        fitness   e_B <= 1e-8                    (otherwise the INPUTS cannot be judged: change the case, never the rule)
        gate      max|g[B] - g_oracle[B]| / s_B <= max(floor, 50 cond eps, 10 e_B)

    max(floor, 50 cond eps) is grad_tol(cond), the gate the whole gradient always had, now per group.  10 e_B: some groups are
    small through cancellation (dlnA_j = alpha_j (w_j^2 + inv(SIGMA)_jj) minus a constant), two fp64 evaluations of them differ by
    cond eps times the size of the TERMS, and e_B measures exactly that; one decimal order of margin because e_B is a single
    sample of a rounding error and the kernels sum in yet another order.  g_second: the second gradient when the caller has it
    already.  -> {"worst_e": (e_B, group), "worst_ratio": (error / tolerance, group)}."""
    g = np.asarray(g, dtype=np.float64)
    g_oracle = np.asarray(g_oracle, dtype=np.float64)
    if g_second is None:
        g_second = torch_gradient(model, theta, X, Y, Psi, omega, training)
    assert g.shape == g_oracle.shape == g_second.shape
    base = max(floor, 50.0 * cond * 2.2e-16)
    errs = group_reference_errors(model, g_oracle, g_second, width)
    worst_e = max((e, name) for name, (s, e) in errs.items())
    unfit = ["%s: e_B = %.2e" % (name, e) for name, (s, e) in errs.items() if not e <= GROUP_FITNESS]
    assert not unfit, "the references disagree beyond %.0e, the case cannot be judged: %s" % (GROUP_FITNESS, "; ".join(unfit))
    worst_r, failed = (0.0, ""), []
    for name, idx in grad_groups(model, width).items():
        s, e = errs[name]
        tol = max(base, 10.0 * e)
        err = float(np.max(np.abs(g[idx] - g_oracle[idx]))) / s
        if not err <= tol:                                   # (also catches NaN)
            failed.append("%s: error %.2e > tolerance %.2e (e_B = %.2e)" % (name, err, tol, e))
        worst_r = max(worst_r, (err / tol if err == err else float("inf"), name))
    assert not failed, "gradient groups outside the gate: " + "; ".join(failed)
    return {"worst_e": worst_e, "worst_ratio": worst_r}


# ---- the case table of tests/test_grad_groups.py (GPU) and tests/test_grad_groups_cpu.py (fitness of the same inputs) ----------
SMALL = ("k_syrk_small", "k_small_tail: T stays in registers")          # substrings of gpz_ctx_route (gpz_ctx.hip)
NOT_SMALL = ("k_syrk_small", "k_small_tail", "k_moments_ring", "k_phi_quad", "streamed")
RING, QUAD = "moments: k_moments_ring", "PHI: k_phi_quad"


def _case(id, method, n, d, m, k=1, hetero=True, psi=False, nanfrac=0.0, seed=11, omega_k=False, train_frac=None, row_tile=0, shards=1,
          recondition=False, has=(), has_not=()):
    return dict(id=id, method=method, n=n, d=d, m=m, k=k, hetero=hetero, psi=psi, nanfrac=nanfrac, seed=seed, omega_k=omega_k,
                train_frac=train_frac, row_tile=row_tile, shards=shards, recondition=recondition, has=tuple(has), has_not=tuple(has_not))


GRAD_GROUP_CASES = [
    # 1: PHI'W PHI in one workgroup + the one-kernel tail (m + k <= 256)
    _case("small-VL-k2", "VL", 500, 4, 40, k=2, has=SMALL),
    _case("small-VD-255", "VD", 521, 5, 255, has=SMALL),                       # m + k = 256: the last shape inside
    _case("small-VC-90", "VC", 403, 5, 90, has=SMALL),
    _case("small-GL-129-nan", "GL", 513, 3, 129, nanfrac=0.3, has=SMALL),
    # 2: the first shapes beyond: k_syrk, k_tgemm, k_moments_fused, the Cholesky chain with mq > 256
    _case("large-VD-256", "VD", 601, 3, 256, has_not=NOT_SMALL),              # m + k = 257
    _case("large-VD-257", "VD", 600, 3, 257, has_not=NOT_SMALL),
    _case("large-VL-385", "VL", 450, 2, 385, has_not=NOT_SMALL),              # four column tiles, the last of one column
    # 3: k_moments_ring with and without k_phi_quad (moments_ring_fits / phi_quad_fits: GC / VC, padded d of 8 or 10, m + k > 256)
    _case("ring-VC-d8", "VC", 700, 8, 257, has=(RING, QUAD), has_not=SMALL),
    _case("ring-GC-d10", "GC", 900, 10, 300, has=(RING, QUAD), has_not=SMALL),
    _case("ring-VC-d8-k2", "VC", 500, 8, 257, k=2, has=(RING,), has_not=SMALL + (QUAD,)),   # k = 2: the ring without the MFMA PHI build
    _case("noring-VC-d6", "VC", 450, 6, 270, has_not=NOT_SMALL),              # d not in {8, 10}: neither
    # 4: diagonal kinds with input noise
    _case("psi-VD-100", "VD", 600, 4, 100, psi=True, has=("k_syrk_small", "k_small_tail; moment sums with input noise by k_moments_diag")),
    _case("psi-VD-270", "VD", 600, 4, 270, psi=True, has_not=NOT_SMALL),
    # 5: covariance kinds with input noise, fp64 pair kernels
    _case("pair-VC-d4", "VC", 300, 4, 64, psi=True, has=("(k_psi)",)),
    _case("pair-GC-d12", "GC", 250, 12, 40, psi=True, has=("(k_cpsi4)",)),
    # (Gamma redrawn: as make_problem draws it at d = 36, the two references disagree on dG by 1e-5)
    _case("pair-VC-d36", "VC", 150, 36, 40, psi=True, recondition=True, has=("(k_cpsi4w / k_cpsi)",)),
    # 6: missing values on covariance kinds: pair kernels over the patterns, and the per-pattern tuned kernels (the workspace form
    # of k_gen is not reached: with input noise every d <= 64 has a tuned pair kernel)
    _case("pair-VC-d4-nan", "VC", 300, 4, 20, psi=True, nanfrac=0.3, has=("(k_psi)",)),
    _case("pattern-GC-k2-nan", "GC", 500, 5, 40, k=2, nanfrac=0.3, has=("tuned kernels per NaN pattern",)),
    # 7: missing values on a diagonal kind, two outputs, m > 256
    _case("large-GD-k2-nan", "GD", 640, 6, 300, k=2, nanfrac=0.3, has_not=NOT_SMALL),
    # 8: per-output weights, training and validation rows
    _case("masks-VD-257", "VD", 600, 3, 257, k=2, omega_k=True, train_frac=0.8, has_not=NOT_SMALL),
    _case("masks-VD-100", "VD", 600, 3, 100, k=2, omega_k=True, train_frac=0.8, has=SMALL),
    # 9: homoscedastic (no dv / dlnT groups)
    _case("homo-VD-257", "VD", 600, 3, 257, hetero=False, has_not=NOT_SMALL),
    _case("homo-VC-90", "VC", 403, 5, 90, hetero=False, has=SMALL),
    # 10: rows streamed in tiles
    _case("streamed-VD-270", "VD", 2500, 3, 270, row_tile=1024, has=("rows: streamed",), has_not=("k_syrk_small", "k_small_tail")),
    # 11: row shards
    _case("shards-VD-257", "VD", 600, 3, 257, shards=2, has_not=NOT_SMALL),
    _case("shards-GD-k2-nan", "GD", 640, 6, 300, k=2, nanfrac=0.3, shards=2, has_not=NOT_SMALL),
]


def grad_group_problem(case):
    """-> (model, theta, X, Y, Psi, omega, training, validation) of one row of the table; cases that differ only in how the
    rows are walked (row tiles, shards) are the same problem."""
    model, theta, X, Y, Psi, rng = make_problem(case["n"], case["d"], case["m"], case["k"], case["method"], case["hetero"], case["seed"],
                                                psi=case["psi"], nanfrac=case["nanfrac"])
    if case["recondition"]:
        theta = recondition_gamma(model, theta, rng)
    omega = training = validation = None
    if case["omega_k"]:
        omega = rng.random((case["n"], case["k"])) + 0.5
    if case["train_frac"]:
        training = rng.random(case["n"]) < case["train_frac"]
        validation = ~training
    return model, theta, X, Y, Psi, omega, training, validation


def grad_group_problem_key(case):
    return tuple(case[f] for f in ("method", "n", "d", "m", "k", "hetero", "psi", "nanfrac", "seed", "omega_k", "train_frac", "recondition"))
