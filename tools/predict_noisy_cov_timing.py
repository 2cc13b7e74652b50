"""Timings of input noise for the covariance kinds on the predictor handle (gpz_amd.Predictor.predict_noisy_cov_dev /
draws_noisy_cov_dev; DESIGN.md section 26, profiles/r18_predict_noisy_cov.txt).

    python tools/predict_noisy_cov_timing.py e2e [--method VC] [--rows N] [--rounds R]   # the new methods against what there was
    python tools/predict_noisy_cov_timing.py kernel [--method VC] [--rows N]             # one call of each route, for rocprofv3 --kernel-trace --stats
    python tools/predict_noisy_cov_timing.py tiles TRACE [--csv OUT]                     # that run's kernel_trace.csv: both routes per full tile

The shape: VC or GC, d = 5, m = 100, k = 1, Psi ~ Gamma(1, 0.05) per dimension; 64 draws.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: predict(X, Psi) of the same handle on the host arrays (the one-shot
predictNoisy per tile, the only route such a catalogue had), predict_noisy_cov_dev(X, Psi), predict_dev(X);
draws_noisy_cov_dev(X, Psi, 64) and draws_dev(X, 64).
tiles: per kernel the launches, the total, and the median of the launches that take more than half of the longest one (the full
tiles); then k_predict_noisy_cov_small + k_predict_noisy_finish per full tile against the one-shot route's k_predict_noisy_cov +
k_pair_table + k_psi_phi + k_gen_rowdot per tile (the condition: at most that plus 5 %)."""
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
from predict_noisy_timing import catalogue, shape  # noqa: E402
from predict_stack_timing import D, DRAWS, K, M  # noqa: E402


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of(a.method, M, D, K, seed=1)
    Xh, Ph = catalogue(a.rows)
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(Ph).to(dev)
    names = ("predict(X, Psi)", "predict_noisy_cov_dev(X, Psi)", "predict_dev(X)", "draws_noisy_cov_dev(X, Psi)", "draws_dev(X)")
    with gpz_amd.Predictor(model) as p:
        calls = (lambda: p.predict(Xh, Psi=Ph), lambda: p.predict_noisy_cov_dev(X, Psi), lambda: p.predict_dev(X),
                 lambda: p.draws_noisy_cov_dev(X, Psi, DRAWS, seed=1), lambda: p.draws_dev(X, DRAWS, seed=1))
        w = 4096
        p.predict(Xh[:w], Psi=Ph[:w]); p.predict_noisy_cov_dev(X[:w], Psi[:w]); p.predict_dev(X[:w])
        p.draws_noisy_cov_dev(X[:w], Psi[:w], DRAWS, seed=1); p.draws_dev(X[:w], DRAWS, seed=1)
        ts = {n: [] for n in names}
        for r in range(a.rounds):
            for n, c in zip(names, calls):
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n == "predict(X, Psi)":
                    ref = res
                if r == 0 and n == "predict_noisy_cov_dev(X, Psi)":
                    err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(res, ref)]
                    print(f"predict_noisy_cov_dev(X, Psi) against predict(X, Psi) on {a.rows} rows, norm ratios: " +
                          ", ".join(f"{e:.1e}" for e in err), flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in names), flush=True)
        med = {n: float(np.median(v)) for n, v in ts.items()}
        print(f"e2e {a.method}, {a.rows} rows, d = {D}, m = {M}, k = {K}, {DRAWS} draws, medians of {a.rounds} rounds:")
        for n in names:
            print(f"  {n:30s} {med[n]:8.4f} s   {a.rows / med[n]:.3g} rows/s")
        print(f"  predict_noisy_cov_dev(X, Psi) = {med['predict(X, Psi)'] / med['predict_noisy_cov_dev(X, Psi)']:.1f} x predict(X, Psi), "
              f"{med['predict_noisy_cov_dev(X, Psi)'] / med['predict_dev(X)']:.1f} x the time of predict_dev(X); "
              f"draws_noisy_cov_dev(X, Psi) {med['draws_noisy_cov_dev(X, Psi)'] / med['draws_dev(X)']:.2f} x the time of draws_dev(X)")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of(a.method, M, D, K, seed=1)
    Xh, Ph = catalogue(a.rows)
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(Ph).to(dev)
    with gpz_amd.Predictor(model) as p:
        p.predict_noisy_cov_dev(X[:4096], Psi[:4096])
        p.draws_noisy_cov_dev(X[:4096], Psi[:4096], DRAWS, seed=1)
        t, _ = timed(lambda: p.predict_noisy_cov_dev(X, Psi), sync)
        print(f"{a.method} {a.rows} rows, predict_noisy_cov_dev(X, Psi): {1e3 * t:.2f} ms end to end", flush=True)
        t, _ = timed(lambda: p.draws_noisy_cov_dev(X, Psi, DRAWS, seed=1), sync)
        print(f"{a.method} {a.rows} rows, draws_noisy_cov_dev(X, Psi, {DRAWS}): {1e3 * t:.2f} ms end to end", flush=True)
        t, _ = timed(lambda: p.predict(Xh, Psi=Ph), sync)
        print(f"{a.method} {a.rows} rows, predict(X, Psi): {1e3 * t:.2f} ms end to end ({p.route})", flush=True)


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

    def full(kernel_name):   # the name itself, not a longer one that begins with it (k_predict_noisy_cov / k_predict_noisy_cov_small)
        v = [float(r["FullTileMedianNs"]) for r in out if re.search(r"\b" + kernel_name + r"(?![A-Za-z0-9_])", r["Name"])]
        return max(v) if v else 0.0
    new = {n: full(n) for n in ("k_predict_noisy_cov_small", "k_predict_noisy_finish")}
    old = {n: full(n) for n in ("k_predict_noisy_cov", "k_pair_table", "k_psi_phi", "k_gen_rowdot")}
    drw = {n: full(n) for n in ("k_predict_noisy_cov_phi", "k_tgemm", "k_transpose_out")}
    if not new["k_predict_noisy_cov_small"] or not old["k_predict_noisy_cov"]:
        sys.exit("the trace does not hold both routes")
    sn, so = sum(new.values()), sum(old.values())
    print("per full tile, the handle's route: " + " + ".join(f"{n} {v / 1e3:.1f} us" for n, v in new.items()) + f" = {sn / 1e3:.1f} us")
    print("per full tile, the one-shot route: " + " + ".join(f"{n} {v / 1e3:.1f} us" for n, v in old.items()) + f" = {so / 1e3:.1f} us")
    print(f"new / old = {sn / so:.3f} (condition: at most 1.05)")
    print("per full tile, the draws: " + " + ".join(f"{n} {v / 1e3:.1f} us" for n, v in drw.items()))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=1_000_000)
    q.add_argument("--rounds", type=int, default=3)
    q = sub.add_parser("kernel")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=1_048_576)
    q = sub.add_parser("tiles")
    q.add_argument("trace", help="kernel_trace.csv of the rocprofv3 run")
    q.add_argument("--csv", help="write the per-kernel statistics to this file")
    a = ap.parse_args()
    shape()   # (predict_noisy_timing.catalogue reads its shape from there)
    {"e2e": e2e, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
