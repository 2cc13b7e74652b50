"""Timings of rows with missing inputs on a predictor handle made with large_m_missing=True (GPZ_PREDICT_LARGE_M_MISSING; DESIGN.md
section 37, profiles/r29_predict_missing_large.txt).

    python tools/predict_missing_large_timing.py e2e --m 500|1000 [--rows N] [--psi]   # the handle against the one-shot route
    python tools/predict_missing_large_timing.py kernel [--rows N]      # m = 256, 512, 1024 in turn, for rocprofv3 --kernel-trace --stats
    python tools/predict_missing_large_timing.py pairs TRACE [--rows N] # that run's kernel_trace.csv: time per MFMA product
    python tools/predict_missing_large_timing.py yardstick              # m = 1024: the one-shot route against the oracle on 2 rows

e2e: VD, d = 10, k = 1 on --rows rows (100 000) of which 20 % have missing values in four patterns (dimension 9; 8 and 9; 0; 3, 5 and
7 missing; 5 % of the rows each).  After a warm-up on 4096 rows (which builds every buffer), predict_dev(X, missing=True) against
p.predict(X) of the same handle in three interleaved rounds, then 64 draws with gamma per draw and the stack with 64 draws and 300
bins, each timed from entry to return with the stream synchronised before the clock starts.  --psi: the same through
predict_noisy_missing_dev and its twins with Psi ~ Gamma(1, 0.05) per dimension.
kernel: at each m two calls of the moments on --rows rows (16 384: one tile) of ONE pattern (dimension 9 missing), so that the trace
holds two launches of the pair kernel per m, in the order of m: k_predict_missing_pairs<1> at 256, k_pml_pairs<1> at 512 and 1024.
pairs: the second launch of each divided by rows x pairs x ceil16(m) multiply-adds of the first product, and its ratio to m = 256.
yardstick: test_the_top_of_the_range's model and its first 2 rows; nrel of the five outputs of p.predict(X) against oracle.predict_any.

Every step is one process under a time limit of its own, chained with && so that a step that fails or runs out of time ends the job
(no step is tried twice):

    timeout -k 10 300 python tools/predict_missing_large_timing.py e2e --m 500 &&
    timeout -k 10 420 python tools/predict_missing_large_timing.py e2e --m 1000 &&
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/k -o k -- python tools/predict_missing_large_timing.py kernel &&
    timeout -k 10 60 python tools/predict_missing_large_timing.py pairs OUT/k/k_kernel_trace.csv"""
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

MS = (256, 512, 1024)
DRAWS, BINS, D = 64, 300, 10
PATTERNS = ((9,), (8, 9), (0,), (3, 5, 7))
PAIR_KERNELS = {256: "k_predict_missing_pairs", 512: "k_pml_pairs", 1024: "k_pml_pairs"}


def rows_of(n, d, seed=2):
    """20 % of the rows with missing values: row i with i % 20 == j < 4 has pattern j."""
    rng = np.random.default_rng(seed)
    X, Psi = rng.standard_normal((n, d)), rng.gamma(1.0, 0.05, (n, d))
    r = np.arange(n) % 20
    for j, cols in enumerate(PATTERNS):
        for c in cols:
            X[r == j, c] = np.nan
    return X, Psi


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of("VD", a.m, D, 1, seed=1)
    Xh, Ph = rows_of(a.rows, D)
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(Ph).to(dev)
    what = "with Psi" if a.psi else "clean"
    with gpz_amd.Predictor(model, large_m_missing=True) as p:
        if a.psi:
            moments, one = (lambda n: p.predict_noisy_missing_dev(X[:n], Psi[:n])), (lambda n: p.predict(Xh[:n], Psi=Ph[:n]))
            draws = lambda n: p.draws_noisy_missing_dev(X[:n], Psi[:n], DRAWS, seed=1, return_gamma=True)
            stack = lambda n, e: p.stack_noisy_missing_dev(X[:n], Psi[:n], e, n_draws=DRAWS, seed=1)
        else:
            moments, one = (lambda n: p.predict_dev(X[:n], missing=True)), (lambda n: p.predict(Xh[:n]))
            draws = lambda n: p.draws_dev(X[:n], DRAWS, seed=1, missing=True, return_gamma=True)
            stack = lambda n, e: p.stack_missing_dev(X[:n], e, n_draws=DRAWS, seed=1)
        w = 4096
        t, out = timed(lambda: moments(w), sync)
        print(f"m = {a.m} {what}: first call on {w} rows (builds the buffers and four patterns' tables): {t:.3f} s", flush=True)
        edges = np.linspace(*np.percentile(out[0].cpu().numpy(), [1, 99]), BINS + 1)
        draws(w)
        stack(w, edges)
        one(w)
        t_dev, t_one = [], []
        for r in range(3):                                               # interleaved rounds
            td, out = timed(lambda: moments(a.rows), sync)
            to, ref = timed(lambda: one(a.rows), sync)
            t_dev.append(td)
            t_one.append(to)
            print(f"m = {a.m} {what} round {r}: handle {td:.3f} s, p.predict {to:.3f} s", flush=True)
        err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(out, ref)]
        print("  nrel of the five outputs, handle against p.predict: " + ", ".join(f"{e:.1e}" for e in err))
        del out, ref
        t_draws, _ = timed(lambda: draws(a.rows), sync)
        t_stack, _ = timed(lambda: stack(a.rows, edges), sync)
        td, to = float(np.median(t_dev)), float(np.median(t_one))
        print(f"VD, d = {D}, m = {a.m}, k = 1, {a.rows} rows, 20 % with missing values in four patterns, {what}")
        print(f"  moments on the handle (median of 3)  {td:8.3f} s   {a.rows / td:.3g} rows/s")
        print(f"  p.predict (median of 3)              {to:8.3f} s   {a.rows / to:.3g} rows/s   ({to / td:.2f} x the handle)")
        print(f"  {DRAWS} draws with gamma per draw         {t_draws:8.3f} s")
        print(f"  stack, {DRAWS} draws, {BINS} bins            {t_stack:8.3f} s")
        print(f"  route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh = np.random.default_rng(2).standard_normal((a.rows, D))
    Xh[:, 9] = np.nan
    X = torch.from_numpy(Xh).to(dev)
    for m in MS:
        with gpz_amd.Predictor(model_of("VD", m, D, 1, seed=1), large_m_missing=True) as p:
            for r in range(2):
                t0, _ = timed(lambda: p.predict_dev(X, missing=True), sync)
                print(f"m = {m} call {r}: moments {1e3 * t0:.2f} ms", flush=True)
            print(f"  {p.route}; device bytes {p.info[1]}", flush=True)


def pairs(a):
    rows = list(csv.DictReader(open(a.trace)))
    if not rows:
        sys.exit("no launches in " + a.trace)
    key = lambda names: next(c for c in rows[0] if c.lower().replace("_", "") in names)
    kn, ks, ke = key(("kernelname", "name")), key(("starttimestamp", "start")), key(("endtimestamp", "end"))
    rows.sort(key=lambda r: float(r[ks]))
    per = {}
    for m in MS:
        name = PAIR_KERNELS[m]
        d = [float(r[ke]) - float(r[ks]) for r in rows if r[kn].split("(")[0].split("<")[0].endswith(name)]
        i = 2 * [q for q in MS if PAIR_KERNELS[q] == name].index(m) + 1   # the second launch at this m
        if len(d) != 2 * sum(PAIR_KERNELS[q] == name for q in MS):
            sys.exit(f"{name}: {len(d)} launches, expected two per m")
        nk = (m + 15) // 16 * 16
        per[m] = d[i] / (a.rows * (m * (m + 1) // 2) * nk)               # ns per multiply-add of the first product, all chunks
        print(f"{name} m = {m}: {d[i] / 1e6:.3f} ms, {1e6 * per[m]:.4f} fs per multiply-add, {per[m] / per[MS[0]]:.3f} x m = {MS[0]}, "
              f"{2e-3 * a.rows * (m * (m + 1) // 2) * nk / d[i]:.1f} Tflop/s")


def yardstick(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import gpz_oracle as O
    from test_predictor import nrel
    from test_predictor_large_m_missing import top_inputs
    from test_predictor_missing import NAMES
    model, X = top_inputs()
    X = X[:2]
    with gpz_amd.Predictor(model, large_m_missing=True) as p:
        t, one = timed(lambda: p.predict(X))
    print(f"m = 1024, 2 rows with dimension 1 missing: p.predict {t:.2f} s", flush=True)
    t, orc = timed(lambda: O.predict_any(X, model))
    print(f"oracle.predict_any {t:.1f} s", flush=True)
    for name, u, v in zip(NAMES, one, orc):
        print(f"yardstick {name} {nrel(np.asarray(u), np.asarray(v)):.3e}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--m", type=int, choices=(500, 1000), required=True)
    q.add_argument("--rows", type=int, default=100_000)
    q.add_argument("--psi", action="store_true")
    q = sub.add_parser("kernel")
    q.add_argument("--rows", type=int, default=16384)
    q = sub.add_parser("pairs")
    q.add_argument("trace", help="kernel_trace.csv of the rocprofv3 run")
    q.add_argument("--rows", type=int, default=16384)
    sub.add_parser("yardstick")
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel, "pairs": pairs, "yardstick": yardstick}[a.cmd](a)


if __name__ == "__main__":
    main()
