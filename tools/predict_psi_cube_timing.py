"""Timings of rows with a full input-noise covariance on the predictor handle (gpz_amd.Predictor.predict_psi_cube_dev /
draws_psi_cube_dev / stack_psi_cube_dev; DESIGN.md section 33, profiles/r24_predict_psi_cube.txt).

    python tools/predict_psi_cube_timing.py e2e [--method VC] [--rows N] [--rounds R]     # predict_psi_cube_dev against Predictor.predict
    python tools/predict_psi_cube_timing.py stack [--method VC] [--rows N] [--alt-rows N]  # the stack against draws + predict + torch
    python tools/predict_psi_cube_timing.py kernel [--method VC] [--d D] [--rows N]        # one tile of each kernel and of its twin, for
                                                                                          # rocprofv3 --kernel-trace
    python tools/predict_psi_cube_timing.py tiles TRACE [TRACE ...]                        # those runs' kernel_trace.csv: new / twin

The shape of e2e and stack: VC or GC, d = 5, m = 100, k = 1, Psi_i = u_i u_i' + diag(g_i) with g ~ Gamma(1, 0.05) and u = 0.3 N(0, 1);
64 draws, 300 bins, 8 groups.  e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed
from entry to return with the current stream synchronised before the clock starts; Predictor.predict(X, Psi=cube) on the host arrays is
the only route such rows had.  kernel: one tile of --rows rows (the default tile of 131 072) at width --d, the cube holding the twin's
variances on its diagonal and zeros off it, so that each new kernel and its per-dimension twin do the same work on the same handle and
rows.  tiles: per kernel the longest launch (the full tile), and the three ratios."""
import argparse
import csv
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpz_amd  # noqa: E402
from predict_dev_timing import timed  # noqa: E402
from predict_draws_timing import model_of  # noqa: E402
from predict_stack_timing import BINS, D, DRAWS, GROUPS, K, M  # noqa: E402

PAIRS = (("k_predict_psi_cube_small", "k_predict_noisy_cov_small"), ("k_predict_psi_cube_phi", "k_predict_noisy_cov_phi"),
         ("k_predict_psi_cube_gamma", "k_predict_noisy_cov_gamma"))


def catalogue(rows, d, dev, full=True):
    """X, the variances and the cube (d, d, rows) on the device; full: u u' + diag(g), else diag(g)."""
    import torch
    gen = torch.Generator(device=dev).manual_seed(2)
    X = torch.randn((rows, d), dtype=torch.float64, device=dev, generator=gen)
    g = torch.from_numpy(np.random.default_rng(2).gamma(1.0, 0.05, (rows, d))).to(dev)
    u = 0.3 * torch.randn((rows, d), dtype=torch.float64, device=dev, generator=gen)
    cube = (u.T[:, None, :] * u.T[None, :, :]) if full else torch.zeros((d, d, rows), dtype=torch.float64, device=dev)
    idx = torch.arange(d, device=dev)
    cube[idx, idx, :] += g.T
    groups = torch.clamp(torch.floor((X[:, 0] + 2.0) * (GROUPS / 4.0)), 0, GROUPS - 1).to(torch.int32)
    return X, g, cube, groups


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of(a.method, M, D, K, seed=1)
    X, g, cube, _ = catalogue(a.rows, D, dev)
    Xh, Ch = X.cpu().numpy(), np.asfortranarray(cube.cpu().numpy())
    names = ("predict(X, Psi=cube)", "predict_psi_cube_dev(X, cube)", "predict_noisy_cov_dev(X, diag)", "predict_dev(X)")
    with gpz_amd.Predictor(model) as p:
        calls = (lambda: p.predict(Xh, Psi=Ch), lambda: p.predict_psi_cube_dev(X, cube), lambda: p.predict_noisy_cov_dev(X, g),
                 lambda: p.predict_dev(X))
        w = 4096
        p.predict(Xh[:w], Psi=np.asfortranarray(Ch[:, :, :w])); p.predict_psi_cube_dev(X[:w], cube[:, :, :w])
        p.predict_noisy_cov_dev(X[:w], g[:w]); p.predict_dev(X[:w])
        ts = {n: [] for n in names}
        for r in range(a.rounds):
            for n, c in zip(names, calls):
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n == names[0]:
                    ref = res
                if r == 0 and n == names[1]:
                    err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(res, ref)]
                    print(f"predict_psi_cube_dev against predict(X, Psi=cube) on {a.rows} rows, norm ratios: " +
                          ", ".join(f"{e:.1e}" for e in err), flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in names), flush=True)
        med = {n: float(np.median(v)) for n, v in ts.items()}
        print(f"e2e {a.method}, {a.rows} rows, d = {D}, m = {M}, k = {K}, medians of {a.rounds} rounds:")
        for n in names:
            print(f"  {n:32s} {med[n]:8.4f} s   {a.rows / med[n]:.3g} rows/s")
        print(f"  predict_psi_cube_dev = {med[names[0]] / med[names[1]]:.1f} x predict(X, Psi=cube), "
              f"{med[names[1]] / med[names[2]]:.2f} x the time of predict_noisy_cov_dev")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def torch_stack(p, X, cube, g, edges):
    """The same stack as a torch reduction over the per-row results on the device: hist (1 + DRAWS, G, B) for k = 1."""
    import torch
    mu, sigma, _, beta, _ = p.predict_psi_cube_dev(X, cube)
    F, Gam = p.draws_psi_cube_dev(X, cube, DRAWS, seed=1, return_gamma=True)
    m = torch.cat([mu.T[None], F.permute(0, 2, 1)])[:, 0]                # (1 + DRAWS, n)
    s = torch.sqrt(torch.cat([sigma.T[None], (beta.T[None] + Gam.permute(0, 2, 1).clamp_min(0.0))])[:, 0])
    e = torch.from_numpy(edges).to(X.device)
    hist = torch.zeros((1 + DRAWS, GROUPS, BINS), dtype=torch.float64, device=X.device)
    step = 1 << 14
    for i in range(0, X.shape[0], step):
        cdf = torch.special.ndtr((e[None, None, :] - m[:, i:i + step, None]) / s[:, i:i + step, None])
        hist.index_add_(1, g[i:i + step].long(), cdf[:, :, 1:] - cdf[:, :, :-1])
    return hist


def stack(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of(a.method, M, D, K, seed=1)
    X, v, cube, g = catalogue(a.rows, D, dev)
    with gpz_amd.Predictor(model) as p:
        mu = p.predict_psi_cube_dev(X[:100_000], cube[:, :, :100_000])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), BINS + 1)
        Xa, Ca, ga = X[:a.alt_rows], cube[:, :, :a.alt_rows], g[:a.alt_rows]
        kw = dict(n_draws=DRAWS, seed=1, n_groups=GROUPS)
        calls = {"stack_psi_cube_dev": lambda: p.stack_psi_cube_dev(X, cube, edges, groups=g, **kw),
                 "predict_psi_cube_dev": lambda: p.predict_psi_cube_dev(X, cube),
                 f"stack_psi_cube_dev, {a.alt_rows} rows": lambda: p.stack_psi_cube_dev(Xa, Ca, edges, groups=ga, **kw),
                 f"draws + predict + torch, {a.alt_rows} rows": lambda: torch_stack(p, Xa, Ca, ga, edges)}
        w = 4096
        p.stack_psi_cube_dev(X[:w], cube[:, :, :w], edges, groups=g[:w], **kw)
        torch_stack(p, X[:w], cube[:, :, :w], g[:w], edges)
        ts = {n: [] for n in calls}
        for r in range(a.rounds):
            for n, c in calls.items():
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n.startswith("stack_psi_cube_dev,"):
                    mine = res.hist[:, :, 0, :]
                if r == 0 and n.startswith("draws"):
                    alt = res.cpu().numpy()
                    print(f"stack_psi_cube_dev against the torch reduction on {a.alt_rows} rows: max abs. difference / largest entry "
                          f"{np.abs(mine - alt).max() / alt.max():.1e}", flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in calls), flush=True)
        print(f"stack {a.method}, {a.rows} rows, d = {D}, m = {M}, k = {K}, {DRAWS} draws, B = {BINS}, G = {GROUPS}, medians of "
              f"{a.rounds} rounds:")
        for n, t in ts.items():
            print(f"  {n:52s} {float(np.median(t)):8.4f} s")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of(a.method, M, a.d, K, seed=1)
    X, g, cube, _ = catalogue(a.rows, a.d, dev, full=False)
    with gpz_amd.Predictor(model, tile_rows=a.rows) as p:
        w = 4096
        for fn in (lambda x, v, c: p.predict_psi_cube_dev(x, c), lambda x, v, c: p.predict_noisy_cov_dev(x, v),
                   lambda x, v, c: p.draws_psi_cube_dev(x, c, DRAWS, seed=1, return_gamma=True),
                   lambda x, v, c: p.draws_noisy_cov_dev(x, v, DRAWS, seed=1, return_gamma=True)):
            fn(X[:w], g[:w], cube[:, :, :w])
            t, _ = timed(lambda: fn(X, g, cube), sync)
            print(f"{a.method} d = {a.d}, {a.rows} rows: {1e3 * t:.2f} ms end to end", flush=True)
        print(f"route: {p.route}")


def tiles(a):
    longest = {}
    for trace in a.trace:
        rows = list(csv.DictReader(open(trace)))
        if not rows:
            sys.exit("no launches in " + trace)
        key = lambda names: next(c for c in rows[0] if c.lower().replace("_", "") in names)
        kn, ks, ke = key(("kernelname", "name")), key(("starttimestamp", "start")), key(("endtimestamp", "end"))
        for r in rows:
            name = re.sub(r"^void ", "", r[kn].split("(")[0])
            longest[name] = max(longest.get(name, 0.0), float(r[ke]) - float(r[ks]))
    for new, old in PAIRS:
        for name in sorted(n for n in longest if n.startswith(new + "<")):
            twin = name.replace(new, old)
            if twin in longest:
                print(f"{name}: {longest[name] / 1e3:.1f} us, {twin}: {longest[twin] / 1e3:.1f} us, ratio {longest[name] / longest[twin]:.3f}")
            else:
                print(f"{name}: {longest[name] / 1e3:.1f} us (no launch of {twin} in the traces)")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for cmd in ("e2e", "stack"):
        q = sub.add_parser(cmd)
        q.add_argument("--method", choices=("VC", "GC"), default="VC")
        q.add_argument("--rows", type=int, default=1_000_000)
        q.add_argument("--rounds", type=int, default=3)
        if cmd == "stack":
            q.add_argument("--alt-rows", type=int, default=131_072)
    q = sub.add_parser("kernel")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--d", type=int, default=D)
    q.add_argument("--rows", type=int, default=131_072)
    q = sub.add_parser("tiles")
    q.add_argument("trace", nargs="+", help="kernel_trace.csv of the rocprofv3 runs")
    a = ap.parse_args()
    {"e2e": e2e, "stack": stack, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
