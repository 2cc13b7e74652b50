"""Timings of the stacks of rows with input noise on a covariance kind (gpz_amd.Predictor.stack_noisy_cov_dev,
draws_noisy_cov_dev(..., return_gamma=True); DESIGN.md section 27, profiles/r19_predict_stack_noisy_cov.txt).

    python tools/predict_stack_noisy_cov_timing.py e2e [--method VC] [--rows N] [--alt-rows N] [--rounds R]   # against the alternatives
    python tools/predict_stack_noisy_cov_timing.py kernel [--method VC] [--rows N]   # one call, for rocprofv3 --kernel-trace --stats
    python tools/predict_stack_noisy_cov_timing.py tiles TRACE [--csv OUT]           # that run's kernel_trace.csv: the kernels per full tile

The shape: VC or GC, d = 5, m = 100, k = 1, Psi ~ Gamma(1, 0.05) per dimension, 64 draws, B = 300 bins over the 1st to 99th percentile of
mu, G = 8 groups (the shape of sections 18 and 26).
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: stack_noisy_cov_dev; the noise-free stack_dev on the same handle and rows;
and, on --alt-rows rows (its draws and widths are two arrays of 8 * 64 bytes per row), draws_noisy_cov_dev(return_gamma=True) +
predict_noisy_cov_dev + a torch reduction of the same stack on the device, with the largest difference of the two results.
tiles: per kernel the launches, the total, and the median of the launches that take more than half of the longest one (the full
tiles); then k_predict_noisy_cov_gamma against k_predict_noisy_cov_small on the same tiles of the same run (the count-based
expectation for VC: 1.0 to 1.3), and k_stack_tile_w.  It ends with an error when the trace is empty or does not hold both kernels."""
import argparse
import csv
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpz_amd  # noqa: E402
from predict_dev_timing import timed  # noqa: E402
from predict_draws_timing import model_of  # noqa: E402
from predict_stack_noisy_timing import B, G, catalogue  # noqa: E402
from predict_stack_timing import D, DRAWS, K, M  # noqa: E402


def torch_stack(p, X, Psi, g, edges):
    """The same stack as a torch reduction over the per-row results on the device: hist (1 + DRAWS, G, B) for k = 1."""
    import torch
    mu, sigma, _, beta, _ = p.predict_noisy_cov_dev(X, Psi)
    F, Gam = p.draws_noisy_cov_dev(X, Psi, DRAWS, seed=1, return_gamma=True)
    m = torch.cat([mu.T[None], F.permute(0, 2, 1)])[:, 0]                # (1 + DRAWS, n)
    s = torch.sqrt(torch.cat([sigma.T[None], (beta.T[None] + Gam.permute(0, 2, 1).clamp_min(0.0))])[:, 0])
    e = torch.from_numpy(edges).to(X.device)
    hist = torch.zeros((1 + DRAWS, G, B), dtype=torch.float64, device=X.device)
    step = 1 << 14
    for i in range(0, X.shape[0], step):
        cdf = torch.special.ndtr((e[None, None, :] - m[:, i:i + step, None]) / s[:, i:i + step, None])
        hist.index_add_(1, g[i:i + step], cdf[:, :, 1:] - cdf[:, :, :-1])
    return hist


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of(a.method, M, D, K, seed=1)
    X, Psi, g = catalogue(a.rows)
    with gpz_amd.Predictor(model) as p:
        mu = p.predict_noisy_cov_dev(X[:100_000], Psi[:100_000])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), B + 1)
        Xa, Pa, ga = X[:a.alt_rows], Psi[:a.alt_rows], g[:a.alt_rows]
        kw = dict(n_draws=DRAWS, seed=1, n_groups=G)
        calls = {"stack_noisy_cov_dev": lambda: p.stack_noisy_cov_dev(X, Psi, edges, groups=g, **kw),
                 "stack_dev (noise-free)": lambda: p.stack_dev(X, edges, groups=g, **kw),
                 f"stack_noisy_cov_dev, {a.alt_rows} rows": lambda: p.stack_noisy_cov_dev(Xa, Pa, edges, groups=ga, **kw),
                 f"draws + predict + torch, {a.alt_rows} rows": lambda: torch_stack(p, Xa, Pa, ga, edges)}
        w = 4096
        p.stack_noisy_cov_dev(X[:w], Psi[:w], edges, groups=g[:w], **kw)
        p.stack_dev(X[:w], edges, groups=g[:w], **kw)
        torch_stack(p, X[:w], Psi[:w], g[:w], edges)
        ts = {n: [] for n in calls}
        for r in range(a.rounds):
            for n, c in calls.items():
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n.startswith("stack_noisy_cov_dev,"):
                    mine = res.hist[:, :, 0, :]
                if r == 0 and n.startswith("draws"):
                    alt = res.cpu().numpy()
                    print(f"stack_noisy_cov_dev against the torch reduction on {a.alt_rows} rows: max abs. difference / largest entry "
                          f"{np.abs(mine - alt).max() / alt.max():.1e}", flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in calls), flush=True)
        print(f"e2e {a.method}, {a.rows} rows, d = {D}, m = {M}, k = {K}, {DRAWS} draws, B = {B}, G = {G}, medians of {a.rounds} rounds:")
        for n, v in ts.items():
            print(f"  {n:52s} {float(np.median(v)):8.4f} s")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of(a.method, M, D, K, seed=1)
    X, Psi, g = catalogue(a.rows)
    with gpz_amd.Predictor(model) as p:
        mu = p.predict_noisy_cov_dev(X[:4096], Psi[:4096])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), B + 1)
        t, _ = timed(lambda: p.stack_noisy_cov_dev(X, Psi, edges, n_draws=DRAWS, seed=1, groups=g, n_groups=G), sync)
        print(f"{a.method} {a.rows} rows, stack_noisy_cov_dev: {1e3 * t:.2f} ms end to end ({p.route})", flush=True)


def tiles(a):
    rows = list(csv.DictReader(open(a.trace)))
    if not rows:
        sys.exit("no launches in " + a.trace)
    key = lambda names: next(c for c in rows[0] if c.lower().replace("_", "") in names)
    kn, ks, ke = key(("kernelname", "name")), key(("starttimestamp", "start")), key(("endtimestamp", "end"))
    dur = {}
    for r in rows:
        dur.setdefault(r[kn].split("(")[0], []).append(float(r[ke]) - float(r[ks]))
    out = []
    for name, d in sorted(dur.items(), key=lambda q: -sum(q[1])):
        d = np.array(d)
        out.append({"Name": name, "Calls": d.size, "TotalDurationNs": f"{d.sum():.0f}", "AverageNs": f"{d.mean():.0f}",
                    "FullTileMedianNs": f"{np.median(d[d > 0.5 * d.max()]):.0f}"})
        print(f"{name}: {d.size} launches, {d.sum() / 1e6:.3f} ms in all, full tiles: median {float(out[-1]['FullTileMedianNs']) / 1e3:.1f} us")
    if a.csv:
        with open(a.csv, "w", newline="") as fh:
            w = csv.DictWriter(fh, fieldnames=list(out[0]))
            w.writeheader()
            w.writerows(out)

    def full(kernel_name):   # the name itself, not a longer one that begins with it
        v = [float(r["FullTileMedianNs"]) for r in out if re.search(r"\b" + kernel_name + r"(?![A-Za-z0-9_])", r["Name"])]
        return max(v) if v else 0.0
    gam, small, tw = full("k_predict_noisy_cov_gamma"), full("k_predict_noisy_cov_small"), full("k_stack_tile_w")
    if not gam or not small:
        sys.exit("the trace does not hold both k_predict_noisy_cov_gamma and k_predict_noisy_cov_small")
    print(f"per full tile: k_predict_noisy_cov_gamma {gam / 1e3:.1f} us / k_predict_noisy_cov_small {small / 1e3:.1f} us = {gam / small:.2f} "
          f"(expected from the counts for VC: 1.0 to 1.3)")
    if tw:
        print(f"per full tile: k_stack_tile_w {tw / 1e3:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=1_000_000)
    q.add_argument("--alt-rows", type=int, default=200_000)
    q.add_argument("--rounds", type=int, default=3)
    q = sub.add_parser("kernel")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=1_048_576)
    q = sub.add_parser("tiles")
    q.add_argument("trace", help="kernel_trace.csv of the rocprofv3 run")
    q.add_argument("--csv", help="write the per-kernel statistics to this file")
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
