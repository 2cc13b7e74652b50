"""Timings of rows with missing inputs on the predictor handle (gpz_amd.Predictor.predict_dev / draws_dev with missing=True; DESIGN.md
section 17, profiles/r11_predict_missing.txt).

    python tools/predict_missing_timing.py e2e [--rows N] [--rounds R]   # predict_dev(X, missing=True) against predict(X) of the handle
    python tools/predict_missing_timing.py kernel [--rows N]             # one group of N rows, for rocprofv3 --kernel-trace --stats

The shape: VD, d = 5, m = 100, k = 1, non-uniform priors; 20 % of the rows with missing values in four patterns (dimension 1, dimension
4, both, dimensions 0 and 2: 5 % of the rows each); 64 draws.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: predict(X) of the same handle on the host arrays (complete rows on the
handle, one gpz_predict_missing per pattern: the only route such a catalogue had), predict_dev(X, missing=True), predict_dev on the
complete rows alone, draws_dev(X, 64, missing=True).
kernel: one call for a single group of --rows rows with dimension 1 missing (tiles of 16 384 rows); k_predict_missing_pairs' time per
131 072 rows is 8 x its median launch; its bound is 2 ceil16(m) m (m + 1) / 2 flop per row at 78.6 Tflop/s."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpz_amd  # noqa: E402
from predict_dev_timing import timed  # noqa: E402
from predict_draws_timing import model_of  # noqa: E402
from predict_stack_timing import D, DRAWS, K, M, chunk_of  # noqa: E402

PATTERNS = ((1,), (4,), (1, 4), (0, 2))


def model():
    mdl = model_of("VD", M, D, K, seed=1)
    mdl.sets["best"]["priors"] = np.random.default_rng(3).dirichlet(np.full(M, 2.0))
    return mdl


def catalogue(rows):
    X = np.ascontiguousarray(chunk_of(rows, 1)[0])
    u = np.random.default_rng(2).random(rows)
    for i, cols in enumerate(PATTERNS):
        sel = (u >= 0.05 * i) & (u < 0.05 * (i + 1))
        for c in cols:
            X[sel, c] = np.nan
    return X


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh = catalogue(a.rows)
    X = torch.from_numpy(Xh).to(dev)
    Xc = X[~torch.isnan(X).any(dim=1)].contiguous()
    names = ("predict(X)", "predict_dev(X, missing)", "predict_dev(complete rows)", "draws_dev(X, missing)")
    with gpz_amd.Predictor(model()) as p:
        calls = (lambda: p.predict(Xh), lambda: p.predict_dev(X, missing=True), lambda: p.predict_dev(Xc),
                 lambda: p.draws_dev(X, DRAWS, seed=1, missing=True))
        w = 4096
        p.predict(Xh[:w]); p.predict_dev(X[:w], missing=True); p.predict_dev(Xc[:w]); p.draws_dev(X[:w], DRAWS, seed=1, missing=True)
        ts = {n: [] for n in names}
        for r in range(a.rounds):
            for n, c in zip(names, calls):
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n == "predict(X)":
                    ref = res
                if r == 0 and n == "predict_dev(X, missing)":
                    err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(res, ref)]
                    print(f"predict_dev(X, missing=True) against predict(X) on {a.rows} rows, norm ratios: " +
                          ", ".join(f"{e:.1e}" for e in err), flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in names), flush=True)
        med = {n: float(np.median(v)) for n, v in ts.items()}
        print(f"e2e {a.rows} rows ({a.rows - Xc.shape[0]} with missing values in {len(PATTERNS)} patterns), d = {D}, m = {M}, k = {K}, "
              f"{DRAWS} draws, medians of {a.rounds} rounds:")
        for n in names:
            print(f"  {n:28s} {med[n]:8.4f} s   {a.rows / med[n]:.3g} rows/s")
        print(f"  predict_dev(X, missing=True) = {med['predict(X)'] / med['predict_dev(X, missing)']:.1f} x predict(X) "
              "(condition: not slower)")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh = np.ascontiguousarray(chunk_of(a.rows, 1)[0])
    Xh[:, 1] = np.nan
    X = torch.from_numpy(Xh).to(dev)
    with gpz_amd.Predictor(model()) as p:
        p.predict_dev(X[:4096], missing=True)
        t, _ = timed(lambda: p.predict_dev(X, missing=True), sync)
        nk = (M + 15) // 16 * 16
        bound = 2.0 * nk * (M * (M + 1) // 2) * 131072 / 78.6e12
        print(f"{a.rows} rows in one group, predict_dev(X, missing=True): {1e3 * t:.2f} ms end to end = {1e3 * t * 131072 / a.rows:.2f} ms "
              f"per 131 072 rows; the f64 MFMA bound of the pair product is {1e3 * bound:.2f} ms per 131 072 rows ({p.route})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--rows", type=int, default=1_000_000)
    q.add_argument("--rounds", type=int, default=3)
    q = sub.add_parser("kernel")
    q.add_argument("--rows", type=int, default=131_072)
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel}[a.cmd](a)


if __name__ == "__main__":
    main()
