"""Timings of the stacks of rows with input noise and missing inputs (gpz_amd.Predictor.stack_noisy_missing_dev,
draws_noisy_missing_dev(..., return_gamma=True); DESIGN.md section 23, profiles/r17_predict_stack_noisy_missing.txt).

    python tools/predict_stack_noisy_missing_timing.py e2e [--rows N] [--rounds R]   # stack_noisy_missing_dev against the alternatives
    python tools/predict_stack_noisy_missing_timing.py kernel [--rows N]        # one group of N rows, for rocprofv3 --kernel-trace --stats
    python tools/predict_stack_noisy_missing_timing.py tiles TRACE [--csv OUT]  # that run's kernel_trace.csv: the kernels per full tile

The shape: VD, d = 5, m = 100, k = 1, non-uniform priors, 20 % of the rows with missing values in four patterns (section 22's
catalogue, tools/predict_noisy_missing_timing.py), Psi everywhere, 64 draws, B = 300 bins over the 1st to 99th percentile of mu, G = 8
groups.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: stack_noisy_missing_dev on all rows; stack_noisy_dev on the complete rows
alone; stack_noisy_missing_dev and stack_noisy_dev on a catalogue without NaN (the same rows with the NaN filled); and, on the rows with
missing values alone, stack_noisy_missing_dev against the route it replaces, draws_noisy_missing_dev(return_gamma) +
predict_noisy_missing_dev + a torch reduction of the same stack on the device, with the largest difference between the two results
over the largest entry.
kernel: stack_noisy_missing_dev, predict_noisy_missing_dev and the noise-free stack_missing_dev for a single group of --rows rows with
dimension 1 missing (tiles of 16 384 rows).
tiles: per kernel the launches, the total, and the median of the launches that take more than half of the longest one (the full
tiles); then k_predict_noisy_missing_gamma against k_predict_noisy_missing_pairs<1> and k_predict_missing_gamma of the same run, and the
expectation from the MFMA counts (56 for the U product per 16-pair block and 32 rows at m = 100, plus 8 per 16-column block: 88 / 56 =
1.57 at 64 columns).  It ends with an error when the trace does not hold the three kernels."""
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
from predict_noisy_missing_timing import noise  # noqa: E402
from predict_stack_timing import D, DRAWS, K, M  # noqa: E402

B, G = 300, 8
TILE = 16_384   # GPZ_PREDICTOR_TILE_MISSING


def torch_stack(p, X, Psi, g, edges):
    """The same stack as a torch reduction over the per-row results on the device: hist (1 + DRAWS, G, B) for k = 1."""
    import torch
    mu, sigma, _, beta, _ = p.predict_noisy_missing_dev(X, Psi)
    F, Gam = p.draws_noisy_missing_dev(X, Psi, DRAWS, seed=1, return_gamma=True)
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
    Xh = catalogue(a.rows)
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(noise(a.rows)).to(dev)
    g = torch.from_numpy(np.random.default_rng(3).integers(0, G, a.rows)).to(dev)
    full = ~torch.isnan(X).any(dim=1)
    Xc, Pc, gc = X[full].contiguous(), Psi[full].contiguous(), g[full].contiguous()
    Xm, Pm, gm = X[~full].contiguous(), Psi[~full].contiguous(), g[~full].contiguous()
    Xf = torch.from_numpy(np.where(np.isnan(Xh), 0.1, Xh)).to(dev)       # the catalogue without NaN
    nm = Xm.shape[0]
    kw = dict(n_draws=DRAWS, seed=1, n_groups=G)
    with gpz_amd.Predictor(model()) as p:
        mu = p.predict_noisy_missing_dev(X[:100_000], Psi[:100_000])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), B + 1)
        calls = {"stack_noisy_missing_dev": lambda: p.stack_noisy_missing_dev(X, Psi, edges, groups=g, **kw),
                 f"stack_noisy_dev, the {Xc.shape[0]} complete rows": lambda: p.stack_noisy_dev(Xc, Pc, edges, groups=gc, **kw),
                 "stack_noisy_missing_dev, no NaN": lambda: p.stack_noisy_missing_dev(Xf, Psi, edges, groups=g, **kw),
                 "stack_noisy_dev, no NaN": lambda: p.stack_noisy_dev(Xf, Psi, edges, groups=g, **kw),
                 f"stack_noisy_missing_dev, the {nm} rows with NaN": lambda: p.stack_noisy_missing_dev(Xm, Pm, edges, groups=gm, **kw),
                 f"draws + predict + torch, the {nm} rows with NaN": lambda: torch_stack(p, Xm, Pm, gm, edges)}
        w = 4096
        p.stack_noisy_missing_dev(X[:w], Psi[:w], edges, groups=g[:w], **kw)
        p.stack_noisy_dev(Xc[:w], Pc[:w], edges, groups=gc[:w], **kw)
        torch_stack(p, X[:w], Psi[:w], g[:w], edges)
        ts = {n: [] for n in calls}
        for r in range(a.rounds):
            for n, c in calls.items():
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n.startswith("stack_noisy_missing_dev, the"):
                    mine = res.hist[:, :, 0, :]
                if r == 0 and n.startswith("draws"):
                    alt = res.cpu().numpy()
                    print(f"stack_noisy_missing_dev against the torch reduction on {nm} rows: max abs. difference / largest entry "
                          f"{np.abs(mine - alt).max() / alt.max():.1e}", flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in calls), flush=True)
        print(f"e2e {a.rows} rows ({nm} with missing values), d = {D}, m = {M}, k = {K}, {DRAWS} draws, B = {B}, G = {G}, "
              f"medians of {a.rounds} rounds (min .. max):")
        for n, v in ts.items():
            print(f"  {n:56s} {float(np.median(v)):8.4f} s  ({min(v):.4f} .. {max(v):.4f})")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh = catalogue(a.rows)
    Xh[:, :] = np.where(np.isnan(Xh), 0.1, Xh)
    Xh[:, 1] = np.nan                                                    # one group
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(noise(a.rows)).to(dev)
    g = torch.from_numpy(np.random.default_rng(3).integers(0, G, a.rows)).to(dev)
    kw = dict(n_draws=DRAWS, seed=1, n_groups=G)
    with gpz_amd.Predictor(model()) as p:
        mu = p.predict_noisy_missing_dev(X[:4096], Psi[:4096])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), B + 1)
        p.stack_noisy_missing_dev(X[:4096], Psi[:4096], edges, groups=g[:4096], **kw)
        p.stack_missing_dev(X[:4096], edges, groups=g[:4096], **kw)
        t, _ = timed(lambda: p.stack_noisy_missing_dev(X, Psi, edges, groups=g, **kw), sync)
        print(f"{a.rows} rows in one group, stack_noisy_missing_dev: {1e3 * t:.2f} ms end to end", flush=True)
        t, _ = timed(lambda: p.predict_noisy_missing_dev(X, Psi), sync)
        print(f"{a.rows} rows in one group, predict_noisy_missing_dev: {1e3 * t:.2f} ms end to end", flush=True)
        t, _ = timed(lambda: p.stack_missing_dev(X, edges, groups=g, **kw), sync)
        print(f"{a.rows} rows in one group, stack_missing_dev (no noise): {1e3 * t:.2f} ms end to end ({p.route})", flush=True)


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
    gam, pairs, mgam = full("k_predict_noisy_missing_gamma"), full("k_predict_noisy_missing_pairs"), full("k_predict_missing_gamma")
    if not gam or not pairs or not mgam:
        sys.exit("the trace does not hold k_predict_noisy_missing_gamma, k_predict_noisy_missing_pairs and k_predict_missing_gamma")
    nk, ncol = (M + 15) // 16 * 16, (DRAWS * K + 15) // 16 * 16
    print(f"per {TILE}-row tile: k_predict_noisy_missing_gamma {gam / 1e3:.1f} us / k_predict_noisy_missing_pairs {pairs / 1e3:.1f} us = "
          f"{gam / pairs:.2f} (the MFMA counts give {(nk // 2 + ncol // 2) / (nk // 2):.2f})")
    print(f"per {TILE}-row tile: k_predict_noisy_missing_gamma {gam / 1e3:.1f} us / k_predict_missing_gamma {mgam / 1e3:.1f} us = "
          f"{gam / mgam:.2f} (the same MFMAs: the excess is the rsqrt chains of the epilogue)")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--rows", type=int, default=1_000_000)
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
