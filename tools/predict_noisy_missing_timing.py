"""Timings of rows with both input noise and missing inputs on the predictor handle (gpz_amd.Predictor.predict_noisy_missing_dev /
draws_noisy_missing_dev; DESIGN.md section 22, profiles/r16_predict_noisy_missing.txt).

    python tools/predict_noisy_missing_timing.py e2e [--rows N] [--rounds R]   # predict_noisy_missing_dev(X, Psi) against predict(X, Psi=Psi)
    python tools/predict_noisy_missing_timing.py kernel [--rows N]             # one group of N rows, for rocprofv3 --kernel-trace --stats

The shape and the catalogue are those of tools/predict_missing_timing.py (VD, d = 5, m = 100, k = 1, non-uniform priors; 20 % of the
rows with missing values in four patterns), with Psi on every row; 64 draws.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: predict(X, Psi=Psi) of the same handle on the host arrays (the one-shot
predictNoisy per tile for the complete rows, one gpz_predict_missing per pattern: the only route such a catalogue had),
predict_noisy_missing_dev(X, Psi), predict_dev(complete rows, Psi=) alone, draws_noisy_missing_dev(X, Psi, 64).
kernel: one call for a single group of --rows rows with dimension 1 missing (tiles of 16 384 rows); under rocprofv3 the median launch of
k_predict_noisy_missing_pairs is its time per 16 384-row tile."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpz_amd  # noqa: E402
from predict_dev_timing import timed  # noqa: E402
from predict_missing_timing import PATTERNS, catalogue, model  # noqa: E402
from predict_stack_timing import D, DRAWS, K, M, chunk_of  # noqa: E402


def noise(rows):
    return np.random.default_rng(4).gamma(1.0, 0.05, (rows, D))


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh, Ph = catalogue(a.rows), noise(a.rows)
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(Ph).to(dev)
    full = ~torch.isnan(X).any(dim=1)
    Xc, Pc = X[full].contiguous(), Psi[full].contiguous()
    names = ("predict(X, Psi)", "predict_noisy_missing_dev", "predict_dev(complete, Psi)", "draws_noisy_missing_dev")
    with gpz_amd.Predictor(model()) as p:
        calls = (lambda: p.predict(Xh, Psi=Ph), lambda: p.predict_noisy_missing_dev(X, Psi), lambda: p.predict_dev(Xc, Psi=Pc),
                 lambda: p.draws_noisy_missing_dev(X, Psi, DRAWS, seed=1))
        w = 4096
        p.predict(Xh[:w], Psi=Ph[:w]); p.predict_noisy_missing_dev(X[:w], Psi[:w]); p.predict_dev(Xc[:w], Psi=Pc[:w])
        p.draws_noisy_missing_dev(X[:w], Psi[:w], DRAWS, seed=1)
        ts = {n: [] for n in names}
        for r in range(a.rounds):
            for n, c in zip(names, calls):
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n == names[0]:
                    ref = res
                if r == 0 and n == names[1]:
                    err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(res, ref)]
                    print(f"predict_noisy_missing_dev(X, Psi) against predict(X, Psi=Psi) on {a.rows} rows, norm ratios: " +
                          ", ".join(f"{e:.1e}" for e in err), flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in names), flush=True)
        med = {n: float(np.median(v)) for n, v in ts.items()}
        print(f"e2e {a.rows} rows ({a.rows - Xc.shape[0]} with missing values in {len(PATTERNS)} patterns), Psi on every row, d = {D}, "
              f"m = {M}, k = {K}, {DRAWS} draws, medians of {a.rounds} rounds:")
        for n in names:
            print(f"  {n:28s} {med[n]:8.4f} s   {a.rows / med[n]:.3g} rows/s")
        print(f"  predict_noisy_missing_dev(X, Psi) = {med[names[0]] / med[names[1]]:.1f} x predict(X, Psi=Psi) (condition: not slower)")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh = np.ascontiguousarray(chunk_of(a.rows, 1)[0])
    Xh[:, 1] = np.nan
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(noise(a.rows)).to(dev)
    with gpz_amd.Predictor(model()) as p:
        p.predict_noisy_missing_dev(X[:4096], Psi[:4096])
        t, _ = timed(lambda: p.predict_noisy_missing_dev(X, Psi), sync)
        print(f"{a.rows} rows in one group, predict_noisy_missing_dev(X, Psi): {1e3 * t:.2f} ms end to end = "
              f"{1e3 * t * 16384 / a.rows:.3f} ms per 16 384-row tile ({p.route})", flush=True)


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
