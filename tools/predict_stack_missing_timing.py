"""Timings of the stacks of rows with missing inputs (gpz_amd.Predictor.stack_missing_dev, draws_dev(..., missing=True,
return_gamma=True); DESIGN.md section 19, profiles/r13_predict_stack_missing.txt).

    python tools/predict_stack_missing_timing.py e2e [--rows N] [--alt-rows N] [--rounds R]   # stack_missing_dev against the alternatives
    python tools/predict_stack_missing_timing.py kernel [--rows N]        # one group of N rows, for rocprofv3 --kernel-trace --stats
    python tools/predict_stack_missing_timing.py tiles TRACE [--csv OUT]  # that run's kernel_trace.csv: the kernels per full tile

The shape: VD, d = 5, m = 100, k = 1, non-uniform priors, 20 % of the rows with missing values in four patterns (section 17's
catalogue, tools/predict_missing_timing.py), 64 draws, B = 300 bins over the 1st to 99th percentile of mu, G = 8 groups.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: stack_missing_dev; stack_dev on the complete rows alone; and, on
--alt-rows rows (its draws and widths are two arrays of 8 * 64 bytes per row), draws_dev(missing, return_gamma) + predict_dev(missing)
+ a torch reduction of the same stack on the device, with the largest difference between the two results over the largest entry.
kernel: stack_missing_dev and predict_dev(missing=True) for a single group of --rows rows with dimension 1 missing (tiles of 16 384 rows).
tiles: per kernel the launches, the total, and the median of the launches that take more than half of the longest one (the full
tiles); then k_predict_missing_gamma against k_predict_missing_pairs<1> of the same run, the expectation from the MFMA counts (56 for
the U product per 16-pair block and 32 rows at m = 100, plus 8 per 16-column block: 88 / 56 = 1.57 at 64 columns) and the share of the
bound 2 (112 + 64) 5050 flop per row at 78.6 Tflop/s.  It ends with an error when the trace does not hold both kernels."""
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
from predict_missing_timing import catalogue, model  # noqa: E402
from predict_stack_timing import D, DRAWS, K, M  # noqa: E402

B, G = 300, 8
TILE = 16_384   # GPZ_PREDICTOR_TILE_MISSING


def torch_stack(p, X, g, edges):
    """The same stack as a torch reduction over the per-row results on the device: hist (1 + DRAWS, G, B) for k = 1."""
    import torch
    mu, sigma, _, beta, _ = p.predict_dev(X, missing=True)
    F, Gam = p.draws_dev(X, DRAWS, seed=1, missing=True, return_gamma=True)
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
    X = torch.from_numpy(catalogue(a.rows)).to(dev)
    g = torch.from_numpy(np.random.default_rng(3).integers(0, G, a.rows)).to(dev)
    full = ~torch.isnan(X).any(dim=1)
    Xc, gc = X[full].contiguous(), g[full].contiguous()
    with gpz_amd.Predictor(model()) as p:
        mu = p.predict_dev(X[:100_000], missing=True)[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), B + 1)
        Xa, ga = X[:a.alt_rows], g[:a.alt_rows]
        calls = {"stack_missing_dev": lambda: p.stack_missing_dev(X, edges, n_draws=DRAWS, seed=1, groups=g, n_groups=G),
                 f"stack_dev, the {Xc.shape[0]} complete rows": lambda: p.stack_dev(Xc, edges, n_draws=DRAWS, seed=1, groups=gc, n_groups=G),
                 f"stack_missing_dev, {a.alt_rows} rows": lambda: p.stack_missing_dev(Xa, edges, n_draws=DRAWS, seed=1, groups=ga, n_groups=G),
                 f"draws_dev + predict_dev + torch, {a.alt_rows} rows": lambda: torch_stack(p, Xa, ga, edges)}
        w = 4096
        p.stack_missing_dev(X[:w], edges, n_draws=DRAWS, seed=1, groups=g[:w], n_groups=G)
        p.stack_dev(Xc[:w], edges, n_draws=DRAWS, seed=1, groups=gc[:w], n_groups=G)
        torch_stack(p, X[:w], g[:w], edges)
        ts = {n: [] for n in calls}
        for r in range(a.rounds):
            for n, c in calls.items():
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n.startswith("stack_missing_dev,"):
                    mine = res.hist[:, :, 0, :]
                if r == 0 and n.startswith("draws_dev"):
                    alt = res.cpu().numpy()
                    print(f"stack_missing_dev against the torch reduction on {a.alt_rows} rows: max abs. difference / largest entry "
                          f"{np.abs(mine - alt).max() / alt.max():.1e}", flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in calls), flush=True)
        print(f"e2e {a.rows} rows ({a.rows - Xc.shape[0]} with missing values), d = {D}, m = {M}, k = {K}, {DRAWS} draws, B = {B}, G = {G}, "
              f"medians of {a.rounds} rounds:")
        for n, v in ts.items():
            print(f"  {n:52s} {float(np.median(v)):8.4f} s")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh = catalogue(a.rows)
    Xh[:, :] = np.where(np.isnan(Xh), 0.1, Xh)
    Xh[:, 1] = np.nan                                                    # one group
    X = torch.from_numpy(Xh).to(dev)
    g = torch.from_numpy(np.random.default_rng(3).integers(0, G, a.rows)).to(dev)
    with gpz_amd.Predictor(model()) as p:
        mu = p.predict_dev(X[:4096], missing=True)[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), B + 1)
        p.stack_missing_dev(X[:4096], edges, n_draws=DRAWS, seed=1, groups=g[:4096], n_groups=G)
        t, _ = timed(lambda: p.stack_missing_dev(X, edges, n_draws=DRAWS, seed=1, groups=g, n_groups=G), sync)
        print(f"{a.rows} rows in one group, stack_missing_dev: {1e3 * t:.2f} ms end to end", flush=True)
        t, _ = timed(lambda: p.predict_dev(X, missing=True), sync)
        print(f"{a.rows} rows in one group, predict_dev(missing=True): {1e3 * t:.2f} ms end to end ({p.route})", flush=True)


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
    gam, pairs = full("k_predict_missing_gamma"), full("k_predict_missing_pairs")
    if not gam or not pairs:
        sys.exit("the trace does not hold both k_predict_missing_gamma and k_predict_missing_pairs")
    npair, nk, ncol = M * (M + 1) // 2, (M + 15) // 16 * 16, (DRAWS * K + 15) // 16 * 16
    bound = 2.0 * (nk + ncol) * npair * TILE / 78.6e12 * 1e9             # ns per full tile
    print(f"per {TILE}-row tile: k_predict_missing_gamma {gam / 1e3:.1f} us / k_predict_missing_pairs {pairs / 1e3:.1f} us = {gam / pairs:.2f} "
          f"(the MFMA counts give {(nk // 2 + ncol // 2) / (nk // 2):.2f}); per 131 072 rows {8 * gam / 1e6:.2f} ms and {8 * pairs / 1e6:.2f} ms")
    print(f"the bound 2 ({nk} + {ncol}) {npair} flop per row at 78.6 Tflop/s: {bound / 1e3:.1f} us per tile, {100 * bound / gam:.0f} % reached")
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
    q.add_argument("--rows", type=int, default=131_072)
    q = sub.add_parser("tiles")
    q.add_argument("trace", help="kernel_trace.csv of the rocprofv3 run")
    q.add_argument("--csv", help="write the per-kernel statistics to this file")
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
