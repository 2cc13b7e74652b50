"""Timings of rows with missing inputs for the covariance kinds on the predictor handle (gpz_amd.Predictor.predict_missing_cov_dev /
draws_missing_cov_dev; DESIGN.md section 28, profiles/r19_predict_missing_cov.txt).

    python tools/predict_missing_cov_timing.py e2e [--method VC] [--rows N] [--rounds R]   # the new methods against what there was
    python tools/predict_missing_cov_timing.py kernel [--method VC] [--rows N]             # one call of each route, for rocprofv3 --kernel-trace --stats
    python tools/predict_missing_cov_timing.py tiles TRACE [--rows N]                      # that run's kernel_trace.csv: both routes on the same rows

The shape: VC or GC, d = 5, m = 100, k = 1, non-uniform priors; 20 % of the rows with missing values in four patterns (dimension 1,
dimension 4, both, dimensions 0 and 2: 5 % of the rows each); 64 draws.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: predict(X) of the same handle on the host arrays (complete rows on the
handle, one gpz_predict_missing per pattern: the only route such a catalogue had), predict_missing_cov_dev(X), predict_dev on the
complete rows alone, draws_missing_cov_dev(X, 64).
kernel: one group of --rows rows (one tile of 16 384 by default) with dimension 1 missing, through predict_missing_cov_dev and then
through predict(X); no warm-up, so every launch of the trace belongs to one of the two calls, table kernels included.
tiles: per kernel the launches and the total; the new kernels' sum against the one-shot route's (the condition: at most that plus
5 %); and k_predict_missing_cov_pairs against its f64 vector bound, densities x (no (no + 3) / 2 + EXP_INSTR) instructions at the sheet
rate of 39.3e12 f64 vector instructions per second (78.6 Tflop/s of multiply-adds)."""
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
from predict_missing_timing import catalogue  # noqa: E402
from predict_stack_timing import D, DRAWS, K, M, chunk_of  # noqa: E402

EXP_INSTR = 22   # vector instructions of the library's f64 exp in the pair kernel's inner loop (counted in the gfx950 assembly at NO = 4:
                 # 42 vector instructions per density, of which 14 are the quadratic, 4 x - a, 1 the argument and 1 the product with Pio)
NEW = ("k_pmcv_ex", "k_pmcv_phi", "k_pmcv_hd", "k_pmc_triples", "k_predict_missing_cov_pairs", "k_pmd_finish", "k_pmcv_basis",
       "k_pmcv_phirec", "k_pmcv_coef")
OLD = ("k_pmc_sum_s", "k_pmc_rows", "k_pmc_pairs", "k_pmc_prep_t", "k_pmc_prep", "k_pmc_cut", "k_pmc_phitab", "k_pm_pio", "k_slab_sum",
       "k_gen_rowdot", "k_predict_noisy_final")


def model(method):
    mdl = model_of(method, M, D, K, seed=1)
    mdl.sets["best"]["priors"] = np.random.default_rng(3).dirichlet(np.full(M, 2.0))
    return mdl


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh = catalogue(a.rows)
    X = torch.from_numpy(Xh).to(dev)
    Xc = X[~torch.isnan(X).any(dim=1)].contiguous()
    names = ("predict(X)", "predict_missing_cov_dev(X)", "predict_dev(complete rows)", "draws_missing_cov_dev(X)")
    with gpz_amd.Predictor(model(a.method)) as p:
        calls = (lambda: p.predict(Xh), lambda: p.predict_missing_cov_dev(X), lambda: p.predict_dev(Xc),
                 lambda: p.draws_missing_cov_dev(X, DRAWS, seed=1))
        w = 4096
        p.predict(Xh[:w]); p.predict_missing_cov_dev(X[:w]); p.predict_dev(Xc[:w]); p.draws_missing_cov_dev(X[:w], DRAWS, seed=1)
        ts = {n: [] for n in names}
        for r in range(a.rounds):
            for n, c in zip(names, calls):
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n == "predict(X)":
                    ref = res
                if r == 0 and n == "predict_missing_cov_dev(X)":
                    err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(res, ref)]
                    print(f"predict_missing_cov_dev(X) against predict(X) on {a.rows} rows, norm ratios: " +
                          ", ".join(f"{e:.1e}" for e in err), flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in names), flush=True)
        med = {n: float(np.median(v)) for n, v in ts.items()}
        print(f"e2e {a.method}, {a.rows} rows ({a.rows - Xc.shape[0]} with missing values in 4 patterns), d = {D}, m = {M}, k = {K}, "
              f"{DRAWS} draws, medians of {a.rounds} rounds:")
        for n in names:
            print(f"  {n:28s} {med[n]:8.4f} s   {a.rows / med[n]:.3g} rows/s")
        print(f"  predict_missing_cov_dev(X) = {med['predict(X)'] / med['predict_missing_cov_dev(X)']:.1f} x predict(X) "
              "(condition: not slower)")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    Xh = np.ascontiguousarray(chunk_of(a.rows, 1)[0])
    Xh[:, 1] = np.nan
    X = torch.from_numpy(Xh).to(dev)
    with gpz_amd.Predictor(model(a.method)) as p:
        t, new = timed(lambda: p.predict_missing_cov_dev(X), sync)
        print(f"{a.method} {a.rows} rows in one group, predict_missing_cov_dev(X): {1e3 * t:.2f} ms end to end", flush=True)
        t, old = timed(lambda: p.predict(Xh), sync)
        print(f"{a.method} {a.rows} rows in one group, predict(X): {1e3 * t:.2f} ms end to end ({p.route})", flush=True)
        err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(new, old)]
        print("norm ratios: " + ", ".join(f"{e:.1e}" for e in err), flush=True)


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
    for name, d in sorted(dur.items(), key=lambda q: -sum(q[1])):
        print(f"{name}: {len(d)} launches, {sum(d) / 1e6:.3f} ms in all")
    new = {n: sum(dur.get(n, [])) for n in NEW}
    old = {n: sum(dur.get(n, [])) for n in OLD}
    if not new["k_predict_missing_cov_pairs"] or not old["k_pmc_sum_s"]:
        sys.exit("the trace does not hold both routes")
    sn, so = sum(new.values()), sum(old.values())
    print(f"{a.rows} rows of one group, the handle's route: " + " + ".join(f"{n} {v / 1e6:.3f}" for n, v in new.items() if v) + f" = {sn / 1e6:.3f} ms")
    print(f"{a.rows} rows of one group, the one-shot route: " + " + ".join(f"{n} {v / 1e6:.3f}" for n, v in old.items() if v) + f" = {so / 1e6:.3f} ms")
    print(f"new / old = {sn / so:.4f} (condition: at most 1.05)")
    no = D - 1
    dens = a.rows * (M * (M + 1) // 2) * M
    bound = dens * (no * (no + 3) // 2 + EXP_INSTR) / 39.3e12
    print(f"k_predict_missing_cov_pairs: {new['k_predict_missing_cov_pairs'] / 1e6:.3f} ms for {dens:.3e} densities at no = {no}; its f64 "
          f"vector bound is {1e3 * bound:.3f} ms ({1e3 * bound / (new['k_predict_missing_cov_pairs'] / 1e6):.2f} of the time)")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=1_000_000)
    q.add_argument("--rounds", type=int, default=3)
    q = sub.add_parser("kernel")
    q.add_argument("--method", choices=("VC", "GC"), default="VC")
    q.add_argument("--rows", type=int, default=16_384)
    q = sub.add_parser("tiles")
    q.add_argument("trace", help="kernel_trace.csv of the rocprofv3 run")
    q.add_argument("--rows", type=int, default=16_384)
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
