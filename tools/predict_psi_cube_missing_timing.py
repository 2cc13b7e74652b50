"""Timings of rows with a full input-noise covariance and missing inputs on the predictor handle
(gpz_amd.Predictor.predict_psi_cube_missing_dev / draws_psi_cube_missing_dev / stack_psi_cube_missing_dev; DESIGN.md section 34,
profiles/r26_predict_psi_cube_missing.txt).

    python tools/predict_psi_cube_missing_timing.py e2e [--method VC] [--rows N] [--rounds R]   # the new methods against what there was
    python tools/predict_psi_cube_missing_timing.py kernel --route new|old|twin|gamma|gamma_twin [--method VC] [--d D] [--rows N]
                                                                            # one call, for rocprofv3 --kernel-trace --stats
    python tools/predict_psi_cube_missing_timing.py tiles --new T --old T [--twin T] [--gamma T] [--gamma-twin T]   # those runs' traces

The shape: VC or GC, d = 5, m = 100, k = 1, non-uniform priors; a cube u u' + diag(g) on every row; 20 % of the rows with missing values
in four patterns (dimension 1, dimension 4, both, dimensions 0 and 2: 5 % of the rows each); 64 draws, 300 bins, 8 groups.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: predict(X, Psi=cube) of the same handle with X and the cube moved to the host
inside the clock (the only route such a catalogue had) and on host arrays that are there already, predict_psi_cube_missing_dev,
draws_psi_cube_missing_dev with 64 draws, stack_psi_cube_missing_dev.
kernel: one group of --rows rows (one tile of 16 384 by default) with dimension 1 missing through ONE route per process, no warm-up, so
every launch of a trace belongs to that route, table kernels and staging included: new is predict_psi_cube_missing_dev, old is
predict(X, Psi=cube) on host arrays, twin is predict_noisy_missing_cov_dev with the cube's diagonal as variances, gamma and gamma_twin
are the two draws methods with return_gamma=True.  With twin routes the cube holds the variances on its diagonal and zeros elsewhere, so
both routes do the same arithmetic.
tiles: per kernel the launches and the total of each trace; every kernel of the new trace against every kernel of the old one (condition
2: at most that plus 5 %); each new kernel over its per-dimension twin; the gamma kernel over the new pair kernel (condition 3: at most
1.10)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpz_amd  # noqa: E402
from predict_dev_timing import timed  # noqa: E402
from predict_draws_timing import model_of  # noqa: E402
from predict_missing_timing import PATTERNS  # noqa: E402
from predict_noisy_missing_cov_timing import durations  # noqa: E402
from predict_stack_timing import BINS, D, DRAWS, GROUPS, K, M  # noqa: E402

TWINS = (("k_pcm_ex", "k_pnmc_ex"), ("k_pcm_phi", "k_pnmc_phi"),
         ("k_predict_psi_cube_missing_pairs", "k_predict_noisy_missing_cov_pairs"),
         ("k_predict_psi_cube_missing_gamma", "k_predict_noisy_missing_cov_gamma"))


def model(method, d=D):
    mdl = model_of(method, M, d, K, seed=1)
    mdl.sets["best"]["priors"] = np.random.default_rng(3).dirichlet(np.full(M, 2.0))
    return mdl


def catalogue(rows, d, dev, full=True, one_group=False):
    """X, the variances, the cube (d, d, rows) and the stack's labels on the device; full: u u' + diag(g), else diag(g).  one_group:
    dimension 1 missing on every row, else the four patterns on 5 % of the rows each."""
    import torch
    gen = torch.Generator(device=dev).manual_seed(2)
    X = torch.randn((rows, d), dtype=torch.float64, device=dev, generator=gen)
    g = torch.from_numpy(np.random.default_rng(2).gamma(1.0, 0.05, (rows, d))).to(dev)
    u = 0.3 * torch.randn((rows, d), dtype=torch.float64, device=dev, generator=gen)
    cube = (u.T[:, None, :] * u.T[None, :, :]) if full else torch.zeros((d, d, rows), dtype=torch.float64, device=dev)
    idx = torch.arange(d, device=dev)
    cube[idx, idx, :] += g.T
    groups = torch.clamp(torch.floor((X[:, 0] + 2.0) * (GROUPS / 4.0)), 0, GROUPS - 1).to(torch.int32)
    if one_group:
        X[:, 1] = float("nan")
    else:
        pick = torch.from_numpy(np.random.default_rng(2).random(rows)).to(dev)
        for i, cols in enumerate(PATTERNS):
            sel = (pick >= 0.05 * i) & (pick < 0.05 * (i + 1))
            for c in cols:
                X[sel, c] = float("nan")
    return X, g, cube, groups


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    X, _, cube, groups = catalogue(a.rows, D, dev)
    Xh, Ch = X.cpu().numpy(), np.asfortranarray(cube.cpu().numpy())
    missing = int(torch.isnan(X).any(dim=1).sum())
    names = ("predict(X, Psi=cube), moved to the host", "predict(X, Psi=cube), host arrays", "predict_psi_cube_missing_dev",
             "draws_psi_cube_missing_dev", "stack_psi_cube_missing_dev")
    with gpz_amd.Predictor(model(a.method)) as p:
        w = 4096
        mu = p.predict_psi_cube_missing_dev(X[:100_000], cube[:, :, :100_000])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), BINS + 1)
        kw = dict(n_draws=DRAWS, seed=1, n_groups=GROUPS)
        calls = (lambda: p.predict(X.cpu().numpy(), Psi=np.asfortranarray(cube.cpu().numpy())), lambda: p.predict(Xh, Psi=Ch),
                 lambda: p.predict_psi_cube_missing_dev(X, cube), lambda: p.draws_psi_cube_missing_dev(X, cube, DRAWS, seed=1),
                 lambda: p.stack_psi_cube_missing_dev(X, cube, edges, groups=groups, **kw))
        p.predict(Xh[:w], Psi=np.asfortranarray(Ch[:, :, :w])); p.predict_psi_cube_missing_dev(X[:w], cube[:, :, :w])
        p.draws_psi_cube_missing_dev(X[:w], cube[:, :, :w], DRAWS, seed=1)
        p.stack_psi_cube_missing_dev(X[:w], cube[:, :, :w], edges, groups=groups[:w], **kw)
        ts = {n: [] for n in names}
        for r in range(a.rounds):
            for n, c in zip(names, calls):
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n == names[1]:
                    ref = res
                if r == 0 and n == names[2]:
                    err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(res, ref)]
                    print(f"{names[2]} against {names[1]} on {a.rows} rows, norm ratios: " + ", ".join(f"{e:.1e}" for e in err), flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in names), flush=True)
        med = {n: float(np.median(v)) for n, v in ts.items()}
        print(f"e2e {a.method}, {a.rows} rows ({missing} with missing values in 4 patterns), d = {D}, m = {M}, k = {K}, {DRAWS} draws, "
              f"B = {BINS}, G = {GROUPS}, medians of {a.rounds} rounds:")
        for n in names:
            print(f"  {n:42s} {med[n]:8.4f} s   {a.rows / med[n]:.3g} rows/s   ({min(ts[n]):.4f} .. {max(ts[n]):.4f})")
        print(f"  condition 1: {names[2]} = {med[names[0]] / med[names[2]]:.1f} x {names[0]} "
              f"({med[names[1]] / med[names[2]]:.1f} x with the arrays on the host already); not slower is the condition")
        print(f"  condition 3: the stack takes {med[names[4]] / med[names[2]]:.2f} x the moments call (at most 3)")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    X, g, cube, _ = catalogue(a.rows, a.d, dev, full=a.route in ("new", "old", "gamma") and not a.diagonal, one_group=True)
    with gpz_amd.Predictor(model(a.method, a.d), tile_rows=a.rows) as p:
        if a.route == "old":
            Xh, Ch = X.cpu().numpy(), np.asfortranarray(cube.cpu().numpy())
        call = {"new": lambda: p.predict_psi_cube_missing_dev(X, cube), "old": lambda: p.predict(Xh, Psi=Ch),
                "twin": lambda: p.predict_noisy_missing_cov_dev(X, g),
                "gamma": lambda: p.draws_psi_cube_missing_dev(X, cube, DRAWS, seed=1, return_gamma=True),
                "gamma_twin": lambda: p.draws_noisy_missing_cov_dev(X, g, DRAWS, seed=1, return_gamma=True)}[a.route]
        t, res = timed(call, sync)
        print(f"{a.method} d = {a.d}, {a.rows} rows in one group, route {a.route}: {1e3 * t:.2f} ms end to end ({p.route})", flush=True)
        print("sums of the outputs: " + ", ".join(f"{float(np.asarray(u.cpu() if hasattr(u, 'cpu') else u).sum()):.12e}" for u in res[:5]))


def tiles(a):
    tot = {}
    for what in ("new", "old", "twin", "gamma", "gamma_twin"):
        path = getattr(a, what)
        if not path:
            continue
        tot[what] = durations(path)
        print(f"---- {what}: {path}")
        for name, d in sorted(tot[what].items(), key=lambda q: -sum(q[1])):
            print(f"{name}: {len(d)} launches, {sum(d) / 1e6:.3f} ms in all")
    if "new" in tot and "old" in tot:
        sn, so = sum(sum(d) for d in tot["new"].values()), sum(sum(d) for d in tot["old"].values())
        print(f"condition 2: every kernel of the handle's route {sn / 1e6:.3f} ms, of the one-shot route {so / 1e6:.3f} ms: "
              f"new / old = {sn / so:.4f} (at most 1.05)")
    every = {}
    for d in tot.values():
        for name, v in d.items():
            every[name] = max(every.get(name, 0.0), sum(v))
    for new, old in TWINS:
        if new in every and old in every:
            print(f"{new}: {every[new] / 1e6:.3f} ms, {old}: {every[old] / 1e6:.3f} ms, new / twin = {every[new] / every[old]:.3f}")
    pair, gam = every.get("k_predict_psi_cube_missing_pairs"), every.get("k_predict_psi_cube_missing_gamma")
    if pair and gam:
        print(f"condition 3: k_predict_psi_cube_missing_gamma / k_predict_psi_cube_missing_pairs = {gam / pair:.3f} (at most 1.10)")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=1_000_000)
    q.add_argument("--rounds", type=int, default=3)
    q = sub.add_parser("kernel")
    q.add_argument("--route", choices=("new", "old", "twin", "gamma", "gamma_twin"), required=True)
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--d", type=int, default=D)
    q.add_argument("--rows", type=int, default=16_384)
    q.add_argument("--diagonal", action="store_true", help="the cube holds the twin's variances on its diagonal and zeros elsewhere")
    q = sub.add_parser("tiles")
    for what in ("new", "old", "twin", "gamma", "gamma-twin"):
        q.add_argument("--" + what, help=f"kernel_trace.csv of the rocprofv3 run of kernel --route {what.replace('-', '_')}")
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
