"""Timings of rows with input noise and missing inputs for the covariance kinds on the predictor handle
(gpz_amd.Predictor.predict_noisy_missing_cov_dev / draws_noisy_missing_cov_dev; DESIGN.md section 31,
profiles/r22_predict_noisy_missing_cov.txt).

    python tools/predict_noisy_missing_cov_timing.py e2e [--method VC] [--rows N] [--rounds R]   # the new methods against what there was
    python tools/predict_noisy_missing_cov_timing.py kernel --route new|old|plain [--method VC] [--rows N]   # one call, for rocprofv3 --kernel-trace --stats
    python tools/predict_noisy_missing_cov_timing.py tiles NEW_TRACE OLD_TRACE [PLAIN_TRACE] [--rows N]    # those runs' kernel_trace.csv

The shape: VC or GC, d = 5, m = 100, k = 1, non-uniform priors; Psi on every row; 20 % of the rows with missing values in four patterns
(dimension 1, dimension 4, both, dimensions 0 and 2: 5 % of the rows each); 64 draws.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: predict(X, Psi=Psi) of the same handle on the host arrays (one
gpz_predict_missing with Psi per pattern: the only route such a catalogue had), predict_noisy_missing_cov_dev(X, Psi),
predict_noisy_cov_dev on the complete rows alone, draws_noisy_missing_cov_dev(X, Psi, 64).
kernel: one group of --rows rows (one tile of 16 384 by default) with dimension 1 missing through ONE route per process, no warm-up, so
every launch of a trace belongs to that route, table kernels and staging included: new is predict_noisy_missing_cov_dev, old is
predict(X, Psi=Psi), plain is predict_missing_cov_dev on the same rows without Psi (for the pair kernels side by side).
tiles: per kernel the launches and the total of each trace; every kernel of the new trace against every kernel of the old one (the
condition: at most that plus 5 %); k_predict_noisy_missing_cov_pairs against k_predict_missing_cov_pairs of the plain trace and against
its f64 vector bound, densities x VEC_INSTR instructions at the sheet rate of 39.3e12 f64 vector instructions per second."""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpz_amd  # noqa: E402
from predict_dev_timing import timed  # noqa: E402
from predict_missing_cov_timing import model  # noqa: E402
from predict_missing_timing import catalogue  # noqa: E402
from predict_noisy_missing_timing import noise  # noqa: E402
from predict_stack_timing import D, DRAWS, K, M, chunk_of  # noqa: E402

# f64 vector instructions of one density at NO = 4, nu = 1, as the operations stand in the source (the compiled loop is counted in
# DESIGN.md section 31): J x 16, A2 x + b2 and its square 5, M + psi 4, the packed Cholesky 20 multiply-adds + 4 rsqrt_nr2 of about 8 + 8
# scalings, the substitution 6 + 4 + 4 + 4, the argument 2, exp 22, the product with prd and with Pio 2
VEC_INSTR = 16 + 5 + 4 + 20 + 32 + 8 + 18 + 2 + 22 + 2


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh, Ph = catalogue(a.rows), noise(a.rows)
    X, P = torch.from_numpy(Xh).to(dev), torch.from_numpy(Ph).to(dev)
    full = ~torch.isnan(X).any(dim=1)
    Xc, Pc = X[full].contiguous(), P[full].contiguous()
    names = ("predict(X, Psi)", "predict_noisy_missing_cov_dev(X, Psi)", "predict_noisy_cov_dev(complete rows)",
             "draws_noisy_missing_cov_dev(X, Psi)")
    with gpz_amd.Predictor(model(a.method)) as p:
        calls = (lambda: p.predict(Xh, Psi=Ph), lambda: p.predict_noisy_missing_cov_dev(X, P), lambda: p.predict_noisy_cov_dev(Xc, Pc),
                 lambda: p.draws_noisy_missing_cov_dev(X, P, DRAWS, seed=1))
        w = 4096
        p.predict(Xh[:w], Psi=Ph[:w]); p.predict_noisy_missing_cov_dev(X[:w], P[:w]); p.predict_noisy_cov_dev(Xc[:w], Pc[:w])
        p.draws_noisy_missing_cov_dev(X[:w], P[:w], DRAWS, seed=1)
        ts = {n: [] for n in names}
        for r in range(a.rounds):
            for n, c in zip(names, calls):
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n == names[0]:
                    ref = res
                if r == 0 and n == names[1]:
                    err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(res, ref)]
                    print(f"{names[1]} against {names[0]} on {a.rows} rows, norm ratios: " + ", ".join(f"{e:.1e}" for e in err), flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in names), flush=True)
        med = {n: float(np.median(v)) for n, v in ts.items()}
        print(f"e2e {a.method}, {a.rows} rows ({a.rows - Xc.shape[0]} with missing values in 4 patterns), d = {D}, m = {M}, k = {K}, "
              f"{DRAWS} draws, medians of {a.rounds} rounds:")
        for n in names:
            print(f"  {n:40s} {med[n]:8.4f} s   {a.rows / med[n]:.3g} rows/s   ({min(ts[n]):.4f} .. {max(ts[n]):.4f})")
        print(f"  {names[1]} = {med[names[0]] / med[names[1]]:.1f} x {names[0]} (condition: not slower)")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh = np.ascontiguousarray(chunk_of(a.rows, 1)[0])
    Xh[:, 1] = np.nan
    Ph = noise(a.rows)
    X, P = torch.from_numpy(Xh).to(dev), torch.from_numpy(Ph).to(dev)
    with gpz_amd.Predictor(model(a.method)) as p:
        call = {"new": lambda: p.predict_noisy_missing_cov_dev(X, P), "old": lambda: p.predict(Xh, Psi=Ph),
                "plain": lambda: p.predict_missing_cov_dev(X)}[a.route]
        t, res = timed(call, sync)
        print(f"{a.method} {a.rows} rows in one group, route {a.route}: {1e3 * t:.2f} ms end to end ({p.route})", flush=True)
        print("sums of the outputs: " + ", ".join(f"{float(np.asarray(u.cpu() if hasattr(u, 'cpu') else u).sum()):.12e}" for u in res[:5]))


def durations(path):
    rows = list(csv.DictReader(open(path)))
    if not rows:
        sys.exit("no launches in " + path)
    key = lambda names: next(c for c in rows[0] if c.lower().replace("_", "") in names)
    kn, ks, ke = key(("kernelname", "name")), key(("starttimestamp", "start")), key(("endtimestamp", "end"))
    dur = {}
    for r in rows:
        name = r[kn].split("(")[0].split("<")[0].replace("void ", "").strip()
        dur.setdefault(name, []).append(float(r[ke]) - float(r[ks]))
    return dur


def tiles(a):
    tot = {}
    for what, path in (("new", a.new), ("old", a.old), ("plain", a.plain)):
        if not path:
            continue
        dur = durations(path)
        tot[what] = dur
        print(f"---- {what}: {path}")
        for name, d in sorted(dur.items(), key=lambda q: -sum(q[1])):
            print(f"{name}: {len(d)} launches, {sum(d) / 1e6:.3f} ms in all")
    sn, so = sum(sum(d) for d in tot["new"].values()), sum(sum(d) for d in tot["old"].values())
    print(f"{a.rows} rows of one group, every kernel of the handle's route {sn / 1e6:.3f} ms, of the one-shot route {so / 1e6:.3f} ms: "
          f"new / old = {sn / so:.4f} (condition: at most 1.05)")
    pair = sum(tot["new"].get("k_predict_noisy_missing_cov_pairs", []))
    if not pair:
        sys.exit("the new trace does not hold k_predict_noisy_missing_cov_pairs")
    dens = a.rows * (M * (M + 1) // 2) * M
    bound = dens * VEC_INSTR / 39.3e12
    print(f"k_predict_noisy_missing_cov_pairs: {pair / 1e6:.3f} ms for {dens:.3e} densities at no = {D - 1}, {1e3 * pair / dens:.2f} ps "
          f"each; its f64 vector bound at {VEC_INSTR} instructions per density is {1e3 * bound:.3f} ms ({1e3 * bound / (pair / 1e6):.2f} of the time)")
    if "plain" in tot:
        old_pair = sum(tot["plain"].get("k_predict_missing_cov_pairs", []))
        print(f"k_predict_missing_cov_pairs on the same rows without Psi: {old_pair / 1e6:.3f} ms; with Psi / without = {pair / old_pair:.2f}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=1_000_000)
    q.add_argument("--rounds", type=int, default=3)
    q = sub.add_parser("kernel")
    q.add_argument("--route", choices=("new", "old", "plain"), required=True)
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=16_384)
    q = sub.add_parser("tiles")
    q.add_argument("new", help="kernel_trace.csv of the rocprofv3 run of kernel --route new")
    q.add_argument("old", help="... of kernel --route old")
    q.add_argument("plain", nargs="?", help="... of kernel --route plain")
    q.add_argument("--rows", type=int, default=16_384)
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
