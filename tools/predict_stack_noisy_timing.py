"""Timings of the stacks of rows with input noise (gpz_amd.Predictor.stack_noisy_dev, draws_dev(..., Psi=, return_gamma=True); DESIGN.md
section 18, profiles/r12_predict_stack_noisy.txt).

    python tools/predict_stack_noisy_timing.py e2e [--rows N] [--alt-rows N] [--rounds R]   # stack_noisy_dev against the alternatives
    python tools/predict_stack_noisy_timing.py kernel [--rows N]        # one call of each route, for rocprofv3 --kernel-trace --stats
    python tools/predict_stack_noisy_timing.py tiles TRACE [--csv OUT]  # that run's kernel_trace.csv: the kernels per full tile

The shape: VD, d = 5, m = 100, k = 1, Psi ~ Gamma(1, 0.05) per dimension, 64 draws, B = 300 bins over the 1st to 99th percentile of mu,
G = 8 groups (the shape of sections 14 and 16).
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: stack_noisy_dev; noise-free stack_dev on the same rows; and, on --alt-rows
rows (its draws and widths are two arrays of 8 * 64 bytes per row), draws_dev(Psi, return_gamma) + predict_dev(Psi) + a torch reduction
of the same stack on the device.  Also the edges within 9 widths per (row, column), counted in that reduction.
tiles: per kernel the launches, the total, and the median of the launches that take more than half of the longest one (the full
tiles); then k_predict_noisy_gamma against k_predict_noisy_small (the target: at most 1.5 x) and k_stack_tile_w against k_stack_tile.
It ends with an error when the trace is empty or does not hold both kernels of the first ratio."""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpz_amd  # noqa: E402
from predict_dev_timing import timed  # noqa: E402
from predict_draws_timing import model_of  # noqa: E402
from predict_stack_timing import D, DRAWS, K, M, chunk_of  # noqa: E402

B, G = 300, 8


def catalogue(rows):
    import torch
    dev = torch.device("cuda", 0)
    X = np.ascontiguousarray(chunk_of(rows, 1)[0])
    Psi = np.random.default_rng(2).gamma(1.0, 0.05, (rows, D))
    g = np.random.default_rng(3).integers(0, G, rows)
    return torch.from_numpy(X).to(dev), torch.from_numpy(Psi).to(dev), torch.from_numpy(g).to(dev)


def torch_stack(p, X, Psi, g, edges):
    """The same stack as a torch reduction over the per-row results on the device: hist (1 + DRAWS, G, B) for k = 1."""
    import torch
    mu, sigma, _, beta, _ = p.predict_dev(X, Psi=Psi)
    F, Gam = p.draws_dev(X, DRAWS, seed=1, Psi=Psi, return_gamma=True)
    m = torch.cat([mu.T[None], F.permute(0, 2, 1)])[:, 0]                # (1 + DRAWS, n)
    s = torch.sqrt(torch.cat([sigma.T[None], (beta.T[None] + Gam.permute(0, 2, 1).clamp_min(0.0))])[:, 0])
    e = torch.from_numpy(edges).to(X.device)
    hist = torch.zeros((1 + DRAWS, G, B), dtype=torch.float64, device=X.device)
    step = 1 << 14
    nedge = 0
    for i in range(0, X.shape[0], step):
        t = (e[None, None, :] - m[:, i:i + step, None]) / s[:, i:i + step, None]
        cdf = torch.special.ndtr(t)
        hist.index_add_(1, g[i:i + step], cdf[:, :, 1:] - cdf[:, :, :-1])
        nedge += int((t.abs() <= 9.0).sum())
    return hist, nedge / (X.shape[0] * (1 + DRAWS))


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of("VD", M, D, K, seed=1)
    X, Psi, g = catalogue(a.rows)
    with gpz_amd.Predictor(model) as p:
        mu = p.predict_dev(X[:100_000], Psi=Psi[:100_000])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), B + 1)
        Xa, Pa, ga = X[:a.alt_rows], Psi[:a.alt_rows], g[:a.alt_rows]
        calls = {"stack_noisy_dev": lambda: p.stack_noisy_dev(X, Psi, edges, n_draws=DRAWS, seed=1, groups=g, n_groups=G),
                 "stack_dev (noise-free)": lambda: p.stack_dev(X, edges, n_draws=DRAWS, seed=1, groups=g, n_groups=G),
                 f"stack_noisy_dev, {a.alt_rows} rows": lambda: p.stack_noisy_dev(Xa, Pa, edges, n_draws=DRAWS, seed=1, groups=ga, n_groups=G),
                 f"draws_dev + predict_dev + torch, {a.alt_rows} rows": lambda: torch_stack(p, Xa, Pa, ga, edges)}
        w = 4096
        p.stack_noisy_dev(X[:w], Psi[:w], edges, n_draws=DRAWS, seed=1, groups=g[:w], n_groups=G)
        p.stack_dev(X[:w], edges, n_draws=DRAWS, seed=1, groups=g[:w], n_groups=G)
        torch_stack(p, X[:w], Psi[:w], g[:w], edges)
        ts = {n: [] for n in calls}
        for r in range(a.rounds):
            for n, c in calls.items():
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n.startswith("stack_noisy_dev,"):
                    mine = res.hist[:, :, 0, :]
                if r == 0 and n.startswith("draws_dev"):
                    alt, per = res[0].cpu().numpy(), res[1]
                    print(f"stack_noisy_dev against the torch reduction on {a.alt_rows} rows: max abs. difference / largest entry "
                          f"{np.abs(mine - alt).max() / alt.max():.1e}; edges within 9 widths per (row, column): {per:.0f}", flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in calls), flush=True)
        print(f"e2e {a.rows} rows, d = {D}, m = {M}, k = {K}, {DRAWS} draws, B = {B}, G = {G}, medians of {a.rounds} rounds:")
        for n, v in ts.items():
            print(f"  {n:52s} {float(np.median(v)):8.4f} s")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of("VD", M, D, K, seed=1)
    X, Psi, g = catalogue(a.rows)
    with gpz_amd.Predictor(model) as p:
        mu = p.predict_dev(X[:4096], Psi=Psi[:4096])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), B + 1)
        t, _ = timed(lambda: p.stack_noisy_dev(X, Psi, edges, n_draws=DRAWS, seed=1, groups=g, n_groups=G), sync)
        print(f"{a.rows} rows, stack_noisy_dev: {1e3 * t:.2f} ms end to end", flush=True)
        t, _ = timed(lambda: p.stack_dev(X, edges, n_draws=DRAWS, seed=1, groups=g, n_groups=G), sync)
        print(f"{a.rows} rows, stack_dev: {1e3 * t:.2f} ms end to end ({p.route})", flush=True)


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

    def full(part):
        v = [float(r["FullTileMedianNs"]) for r in out if part in r["Name"]]
        return max(v) if v else 0.0
    gam, small = full("k_predict_noisy_gamma"), full("k_predict_noisy_small")
    if not gam or not small:
        sys.exit("the trace does not hold both k_predict_noisy_gamma and k_predict_noisy_small")
    ratio = gam / small
    print(f"per full tile: k_predict_noisy_gamma {gam / 1e3:.1f} us / k_predict_noisy_small {small / 1e3:.1f} us = {ratio:.2f} "
          f"(target: at most 1.5; {'met' if ratio <= 1.5 else 'missed'})")
    tw, t0 = full("k_stack_tile_w"), max([float(r["FullTileMedianNs"]) for r in out if r["Name"].strip() == "k_stack_tile"] or [0.0])
    if tw and t0:
        print(f"per full tile: k_stack_tile_w {tw / 1e3:.1f} us / k_stack_tile {t0 / 1e3:.1f} us = {tw / t0:.2f}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--rows", type=int, default=1_000_000)
    q.add_argument("--alt-rows", type=int, default=200_000)
    q.add_argument("--rounds", type=int, default=3)
    q = sub.add_parser("kernel")
    q.add_argument("--rows", type=int, default=1_048_576)
    q = sub.add_parser("tiles")
    q.add_argument("trace", help="kernel_trace.csv of the rocprofv3 run")
    q.add_argument("--csv", help="write the per-kernel statistics to this file")
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
