"""Timings of rows with input noise on a predictor handle made with large_m=True (GPZ_PREDICT_LARGE_M; DESIGN.md section 36,
profiles/r28_predict_noisy_large.txt).

    python tools/predict_noisy_large_timing.py e2e --config vc500|vd1000 [--rows N]   # the handle against the one-shot route per tile
    python tools/predict_noisy_large_timing.py kernel --method VD|VC [--rows N]       # m = 256, 512, 1024 in turn, for rocprofv3 --kernel-trace --stats
    python tools/predict_noisy_large_timing.py pairs TRACE --method VD|VC [--rows N]  # that run's kernel_trace.csv: time per pair density

e2e, one call each after a warm-up on 4096 rows (which also builds the pair table), timed from entry to return with the stream
synchronised before the clock starts: vc500 is VC, d = 10, m = 500, k = 1 (the photo-z configuration of BASELINE.json), vd1000 is
VD, d = 10, m = 1000, k = 1; Psi ~ Gamma(1, 0.05) per dimension.  predict_*_dev(X, Psi) against p.predict(X, Psi=Psi) of the same
handle, and the stack with 64 draws and 300 bins against the moments plus draws_*_dev(..., return_gamma=True).
kernel: at each m two calls of the moments and of the draws with gamma on --rows rows (16 384: one tile), so that the trace holds
two launches of every pair kernel per m, in the order of m.  pairs: the second launch of each, divided by rows x m (m + 1) / 2 pair
densities, and its ratio to the same kernel's figure at m = 256 (the expectation under test: within 15 %).

Every step is one process under a time limit of its own, chained with && so that a step that fails or runs out of time ends the
job (no step is tried twice):

    timeout -k 10 240 python tools/predict_noisy_large_timing.py e2e --config vc500 &&
    timeout -k 10 240 python tools/predict_noisy_large_timing.py e2e --config vd1000 &&
    timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/vd -o vd -- python tools/predict_noisy_large_timing.py kernel --method VD &&
    timeout -k 10 60 python tools/predict_noisy_large_timing.py pairs OUT/vd/vd_kernel_trace.csv --method VD
    (and the same two for --method VC)"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpz_amd  # noqa: E402
from predict_dev_timing import timed  # noqa: E402
from predict_draws_timing import model_of  # noqa: E402

CONFIGS = {"vc500": ("VC", 10, 500), "vd1000": ("VD", 10, 1000)}
MS = (256, 512, 1024)
DRAWS, BINS, D = 64, 300, 10
PAIR_KERNELS = {"VD": ("k_predict_noisy_small", "k_predict_noisy_gamma"), "VC": ("k_predict_noisy_cov_small", "k_predict_noisy_cov_gamma")}


def rows_of(n, d, seed=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)), rng.gamma(1.0, 0.05, (n, d))


def methods_of(p, method):
    if method[1] == "C":
        return p.predict_noisy_cov_dev, p.draws_noisy_cov_dev, p.stack_noisy_cov_dev
    return (lambda X, Psi: p.predict_dev(X, Psi=Psi)), (lambda X, Psi, nd, **kw: p.draws_dev(X, nd, Psi=Psi, **kw)), p.stack_noisy_dev


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    method, d, m = CONFIGS[a.config]
    model = model_of(method, m, d, 1, seed=1)
    Xh, Ph = rows_of(a.rows, d)
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(Ph).to(dev)
    with gpz_amd.Predictor(model, large_m=True) as p:
        moments, draws, stack = methods_of(p, method)
        w = 4096
        t, _ = timed(lambda: moments(X[:w], Psi[:w]), sync)
        print(f"{a.config}: first call on {w} rows (builds the pair table): {t:.3f} s", flush=True)
        mu = moments(X[:w], Psi[:w])[0].cpu().numpy()
        edges = np.linspace(*np.percentile(mu, [1, 99]), BINS + 1)
        draws(X[:w], Psi[:w], DRAWS, seed=1, return_gamma=True)
        stack(X[:w], Psi[:w], edges, n_draws=DRAWS, seed=1)
        p.predict(Xh[:w], Psi=Ph[:w])
        t_dev, out = timed(lambda: moments(X, Psi), sync)
        print(f"{a.config}: moments on the handle, {a.rows} rows: {t_dev:.3f} s", flush=True)
        t_one, ref = timed(lambda: p.predict(Xh, Psi=Ph), sync)
        print(f"{a.config}: p.predict(X, Psi=Psi), {a.rows} rows: {t_one:.3f} s", flush=True)
        err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(out, ref)]
        print("  norm ratios of the five outputs: " + ", ".join(f"{e:.1e}" for e in err))
        del out, ref
        t_draws, _ = timed(lambda: draws(X, Psi, DRAWS, seed=1, return_gamma=True), sync)
        t_stack, _ = timed(lambda: stack(X, Psi, edges, n_draws=DRAWS, seed=1), sync)
        print(f"{a.config}: {method}, d = {d}, m = {m}, k = 1, {a.rows} rows")
        print(f"  moments on the handle            {t_dev:8.3f} s   {a.rows / t_dev:.3g} rows/s")
        print(f"  p.predict(X, Psi=Psi)            {t_one:8.3f} s   {a.rows / t_one:.3g} rows/s   ({t_one / t_dev:.1f} x the handle)")
        print(f"  {DRAWS} draws with gamma per draw     {t_draws:8.3f} s")
        print(f"  stack, {DRAWS} draws, {BINS} bins        {t_stack:8.3f} s   ({t_stack / (t_dev + t_draws):.2f} x moments + draws)")
        print(f"  route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh, Ph = rows_of(a.rows, D)
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(Ph).to(dev)
    for m in MS:
        model = model_of(a.method, m, D, 1, seed=1)
        with gpz_amd.Predictor(model, large_m=True) as p:
            moments, draws, _ = methods_of(p, a.method)
            for r in range(2):
                t0, _ = timed(lambda: moments(X, Psi), sync)
                t1, _ = timed(lambda: draws(X, Psi, DRAWS, seed=1, return_gamma=True), sync)
                print(f"{a.method} m = {m} call {r}: moments {1e3 * t0:.2f} ms, {DRAWS} draws with gamma {1e3 * t1:.2f} ms", flush=True)
            print(f"  {p.route}; device bytes {p.info[1]}", flush=True)


def pairs(a):
    rows = list(csv.DictReader(open(a.trace)))
    if not rows:
        sys.exit("no launches in " + a.trace)
    key = lambda names: next(c for c in rows[0] if c.lower().replace("_", "") in names)
    kn, ks, ke = key(("kernelname", "name")), key(("starttimestamp", "start")), key(("endtimestamp", "end"))
    rows.sort(key=lambda r: float(r[ks]))
    for name in PAIR_KERNELS[a.method]:
        d = [float(r[ke]) - float(r[ks]) for r in rows if r[kn].split("(")[0].split("<")[0].endswith(name)]
        if len(d) != 2 * len(MS):
            sys.exit(f"{name}: {len(d)} launches, expected two per m")
        per = {m: d[2 * i + 1] / (a.rows * (m * (m + 1) // 2)) for i, m in enumerate(MS)}   # ns per pair density, all chunks of a launch
        for m in MS:
            print(f"{name} m = {m}: {d[2 * MS.index(m) + 1] / 1e6:.3f} ms, {1e3 * per[m]:.3f} ps per pair density, "
                  f"{per[m] / per[MS[0]]:.3f} x m = {MS[0]}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--config", choices=sorted(CONFIGS), required=True)
    q.add_argument("--rows", type=int, default=100_000)
    q = sub.add_parser("kernel")
    q.add_argument("--method", choices=("VD", "VC"), required=True)
    q.add_argument("--rows", type=int, default=16384)
    q = sub.add_parser("pairs")
    q.add_argument("trace", help="kernel_trace.csv of the rocprofv3 run")
    q.add_argument("--method", choices=("VD", "VC"), required=True)
    q.add_argument("--rows", type=int, default=16384)
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel, "pairs": pairs}[a.cmd](a)


if __name__ == "__main__":
    main()
