"""Timings of the stacks of rows with input noise and missing inputs on a covariance kind (gpz_amd.Predictor.stack_noisy_missing_cov_dev,
draws_noisy_missing_cov_dev(..., return_gamma=True); DESIGN.md section 32, profiles/r23_predict_stack_noisy_missing_cov.txt).

    python tools/predict_stack_noisy_missing_cov_timing.py e2e [--method VC] [--rows N] [--rounds R]   # the stack against what there was
    python tools/predict_stack_noisy_missing_cov_timing.py kernel [--method VC] [--rows N]   # one group of N rows, for rocprofv3 --kernel-trace --stats
    python tools/predict_stack_noisy_missing_cov_timing.py tiles TRACE                       # that run's kernel_trace.csv: the kernels per full tile

The shape is section 31's (tools/predict_noisy_missing_cov_timing.py): VC or GC, d = 5, m = 100, k = 1, non-uniform priors, Psi on every
row, 20 % of the rows with missing values in four patterns, 64 draws; B = 300 bins over the 1st to 99th percentile of mu, G = 8 groups.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: stack_noisy_missing_cov_dev on all rows; stack_noisy_cov_dev on the
complete rows alone; the parent's predict_noisy_missing_cov_dev on the same rows (the yardstick: the stack may take 3 x that);
draws_noisy_missing_cov_dev with gamma.  The rows with missing values form every density twice (once per kernel), plus the draws and
the stack kernel.  Reported beside it: 64 x the moments call, which is what 64 handles with w := w_s cost before their set-up.
kernel: stack_noisy_missing_cov_dev for a single group of --rows rows with dimension 1 missing (tiles of 16 384 rows), after a warm-up
call on 4096 rows.
tiles: per kernel the launches, the total, and the median of the launches that take more than half of the longest one (the full
tiles, one launch per slab of the pair table); then k_predict_noisy_missing_cov_gamma against k_predict_noisy_missing_cov_pairs of the
same run: the two form the same densities, so the count gives a ratio of about 1.0 (condition: at most 1.10).  It ends with an error when the trace does not hold both
kernels."""
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
from predict_missing_cov_timing import model  # noqa: E402
from predict_missing_timing import catalogue  # noqa: E402
from predict_noisy_missing_timing import noise  # noqa: E402
from predict_stack_timing import D, DRAWS, K, M, chunk_of  # noqa: E402

B, G = 300, 8
TILE = 16_384   # GPZ_PREDICTOR_TILE_MISSING


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    X, P = torch.from_numpy(catalogue(a.rows)).to(dev), torch.from_numpy(noise(a.rows)).to(dev)
    g = torch.from_numpy(np.random.default_rng(3).integers(0, G, a.rows)).to(dev)
    full = ~torch.isnan(X).any(dim=1)
    Xc, Pc, gc = X[full].contiguous(), P[full].contiguous(), g[full].contiguous()
    stack, moments = "stack_noisy_missing_cov_dev(X, Psi)", "predict_noisy_missing_cov_dev(X, Psi)"
    with gpz_amd.Predictor(model(a.method)) as p:
        mu = p.predict_noisy_missing_cov_dev(X[:100_000], P[:100_000])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), B + 1)
        calls = {stack: lambda: p.stack_noisy_missing_cov_dev(X, P, edges, n_draws=DRAWS, seed=1, groups=g, n_groups=G),
                 "stack_noisy_cov_dev(complete rows)": lambda: p.stack_noisy_cov_dev(Xc, Pc, edges, n_draws=DRAWS, seed=1, groups=gc,
                                                                                     n_groups=G),
                 moments: lambda: p.predict_noisy_missing_cov_dev(X, P),
                 "draws_noisy_missing_cov_dev(X, Psi, gamma)": lambda: p.draws_noisy_missing_cov_dev(X, P, DRAWS, seed=1, return_gamma=True)}
        w = 4096
        p.stack_noisy_missing_cov_dev(X[:w], P[:w], edges, n_draws=DRAWS, seed=1, groups=g[:w], n_groups=G)
        p.stack_noisy_cov_dev(Xc[:w], Pc[:w], edges, n_draws=DRAWS, seed=1, groups=gc[:w], n_groups=G)
        p.draws_noisy_missing_cov_dev(X[:w], P[:w], DRAWS, seed=1, return_gamma=True)
        ts = {n: [] for n in calls}
        for r in range(a.rounds):
            for n, c in calls.items():
                t, res = timed(c, sync)
                ts[n].append(t)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in calls), flush=True)
        med = {n: float(np.median(v)) for n, v in ts.items()}
        print(f"e2e {a.method}, {a.rows} rows ({a.rows - Xc.shape[0]} with missing values in 4 patterns), d = {D}, m = {M}, k = {K}, "
              f"{DRAWS} draws, B = {B}, G = {G}, medians of {a.rounds} rounds:")
        for n in calls:
            print(f"  {n:44s} {med[n]:8.4f} s   {a.rows / med[n]:.3g} rows/s   ({min(ts[n]):.4f} .. {max(ts[n]):.4f})")
        print(f"  {stack} = {med[stack] / med[moments]:.2f} x {moments} (condition: at most 3)")
        print(f"  {DRAWS} x {moments} = {DRAWS * med[moments]:.2f} s, what {DRAWS} handles with w := w_s take before their set-up: "
              f"{DRAWS * med[moments] / med[stack]:.1f} x {stack}")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh = np.ascontiguousarray(chunk_of(a.rows, 1)[0])
    Xh[:, 1] = np.nan                                                    # one group
    X, P = torch.from_numpy(Xh).to(dev), torch.from_numpy(noise(a.rows)).to(dev)
    g = torch.from_numpy(np.random.default_rng(3).integers(0, G, a.rows)).to(dev)
    with gpz_amd.Predictor(model(a.method)) as p:
        mu = p.predict_noisy_missing_cov_dev(X[:4096], P[:4096])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), B + 1)
        p.stack_noisy_missing_cov_dev(X[:4096], P[:4096], edges, n_draws=DRAWS, seed=1, groups=g[:4096], n_groups=G)
        t, _ = timed(lambda: p.stack_noisy_missing_cov_dev(X, P, edges, n_draws=DRAWS, seed=1, groups=g, n_groups=G), sync)
        print(f"{a.method} {a.rows} rows in one group, stack_noisy_missing_cov_dev: {1e3 * t:.2f} ms end to end ({p.route})", flush=True)


def tiles(a):
    rows = list(csv.DictReader(open(a.trace)))
    if not rows:
        sys.exit("no launches in " + a.trace)
    key = lambda names: next(c for c in rows[0] if c.lower().replace("_", "") in names)
    kn, ks, ke = key(("kernelname", "name")), key(("starttimestamp", "start")), key(("endtimestamp", "end"))
    dur = {}
    for r in rows:
        name = r[kn].split("(")[0].split("<")[0].replace("void ", "").strip()
        dur.setdefault(name, []).append(float(r[ke]) - float(r[ks]))
    full = {}
    for name, d in sorted(dur.items(), key=lambda q: -sum(q[1])):
        d = np.array(d)
        full[name] = float(np.median(d[d > 0.5 * d.max()]))
        print(f"{name}: {d.size} launches, {d.sum() / 1e6:.3f} ms in all, full tiles: median {full[name] / 1e3:.1f} us")
    gam, pairs = full.get("k_predict_noisy_missing_cov_gamma", 0.0), full.get("k_predict_noisy_missing_cov_pairs", 0.0)
    if not gam or not pairs:
        sys.exit("the trace does not hold both k_predict_noisy_missing_cov_gamma and k_predict_noisy_missing_cov_pairs")
    dens = TILE * (M * (M + 1) // 2) * M
    nt = len(dur.get("k_stack_tile_w", [])) or 1                        # the tiles of the call; a tile passes its slabs one launch each
    slabs = max(1, round(len(dur["k_predict_noisy_missing_cov_gamma"]) / nt))
    print(f"per launch of a full {TILE}-row tile ({slabs} slabs per tile, {dens:.3e} densities per tile): k_predict_noisy_missing_cov_gamma "
          f"{gam / 1e6:.3f} ms / k_predict_noisy_missing_cov_pairs {pairs / 1e6:.3f} ms = {gam / pairs:.3f} (the density count gives about "
          f"1.0; condition: at most 1.10); per tile {slabs * gam / 1e6:.1f} ms / {slabs * pairs / 1e6:.1f} ms")
    tw = full.get("k_stack_tile_w", 0.0)
    if tw:
        print(f"per full tile: k_stack_tile_w {tw / 1e3:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=1_000_000)
    q.add_argument("--rounds", type=int, default=3)
    q = sub.add_parser("kernel")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=65_536)
    q = sub.add_parser("tiles")
    q.add_argument("trace", help="kernel_trace.csv of the rocprofv3 run")
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
