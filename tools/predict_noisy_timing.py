"""Timings of input noise on the predictor handle (gpz_amd.Predictor.predict_dev / draws_dev with Psi=; DESIGN.md section 16,
profiles/r10_predict_noisy.txt).

    python tools/predict_noisy_timing.py e2e [--rows N] [--rounds R]   # predict_dev(X, Psi) against predict(X, Psi) and predict_dev(X)
    python tools/predict_noisy_timing.py kernel [--rows N]             # one call of each route, for rocprofv3 --kernel-trace --stats
    python tools/predict_noisy_timing.py tiles TRACE [--csv OUT]       # that run's kernel_trace.csv: both routes per full tile
    python tools/predict_noisy_timing.py [ns] [m] [d] [method]         # wall time of the one-shot predict() with and without Psi

The shape: VD, d = 5, m = 100, k = 1, Psi ~ Gamma(1, 0.05) per dimension; 64 draws.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return with the
current stream synchronised before the clock starts.  Rows: predict(X, Psi) of the same handle on the host arrays (the one-shot
predictNoisy per tile), predict_dev(X, Psi), predict_dev(X); draws_dev(X, 64, Psi) and draws_dev(X, 64).
tiles: per kernel the launches, the total, and the median of the launches that take more than half of the longest one (the full
tiles); then k_predict_noisy_small + k_predict_noisy_finish per full tile against the one-shot route's k_predict_noisy_diag +
k_pair_table + k_phi_diag + k_gen_rowdot per tile (the condition: at most that plus 5 %).
Without a sub-command (tools/measure_extras.sh): predict() of a solved model with input noise and no missing values, any method."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpz_amd  # noqa: E402


def shape():
    """The sub-commands' shape and helpers (the positional mode needs none of these modules)."""
    global timed, model_of, D, DRAWS, K, M, chunk_of
    from predict_dev_timing import timed
    from predict_draws_timing import model_of
    from predict_stack_timing import D, DRAWS, K, M, chunk_of


def catalogue(rows):
    X = np.ascontiguousarray(chunk_of(rows, 1)[0])
    Psi = np.random.default_rng(2).gamma(1.0, 0.05, (rows, D))
    return X, Psi


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of("VD", M, D, K, seed=1)
    Xh, Ph = catalogue(a.rows)
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(Ph).to(dev)
    names = ("predict(X, Psi)", "predict_dev(X, Psi)", "predict_dev(X)", "draws_dev(X, Psi)", "draws_dev(X)")
    with gpz_amd.Predictor(model) as p:
        calls = (lambda: p.predict(Xh, Psi=Ph), lambda: p.predict_dev(X, Psi=Psi), lambda: p.predict_dev(X),
                 lambda: p.draws_dev(X, DRAWS, seed=1, Psi=Psi), lambda: p.draws_dev(X, DRAWS, seed=1))
        w = 4096
        p.predict(Xh[:w], Psi=Ph[:w]); p.predict_dev(X[:w], Psi=Psi[:w]); p.predict_dev(X[:w])
        p.draws_dev(X[:w], DRAWS, seed=1, Psi=Psi[:w]); p.draws_dev(X[:w], DRAWS, seed=1)
        ts = {n: [] for n in names}
        for r in range(a.rounds):
            for n, c in zip(names, calls):
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n == "predict(X, Psi)":
                    ref = res
                if r == 0 and n == "predict_dev(X, Psi)":
                    err = [float(np.linalg.norm(u.cpu().numpy() - v) / np.linalg.norm(v)) for u, v in zip(res, ref)]
                    print(f"predict_dev(X, Psi) against predict(X, Psi) on {a.rows} rows, norm ratios: " +
                          ", ".join(f"{e:.1e}" for e in err), flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in names), flush=True)
        med = {n: float(np.median(v)) for n, v in ts.items()}
        print(f"e2e {a.rows} rows, d = {D}, m = {M}, k = {K}, {DRAWS} draws, medians of {a.rounds} rounds:")
        for n in names:
            print(f"  {n:22s} {med[n]:8.4f} s   {a.rows / med[n]:.3g} rows/s")
        print(f"  predict_dev(X, Psi) = {med['predict(X, Psi)'] / med['predict_dev(X, Psi)']:.1f} x predict(X, Psi), "
              f"{med['predict_dev(X, Psi)'] / med['predict_dev(X)']:.1f} x the time of predict_dev(X); "
              f"draws_dev(X, Psi) {med['draws_dev(X, Psi)'] / med['draws_dev(X)']:.2f} x the time of draws_dev(X)")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of("VD", M, D, K, seed=1)
    Xh, Ph = catalogue(a.rows)
    X, Psi = torch.from_numpy(Xh).to(dev), torch.from_numpy(Ph).to(dev)
    with gpz_amd.Predictor(model) as p:
        p.predict_dev(X[:4096], Psi=Psi[:4096])
        t, _ = timed(lambda: p.predict_dev(X, Psi=Psi), sync)
        print(f"{a.rows} rows, predict_dev(X, Psi): {1e3 * t:.2f} ms end to end", flush=True)
        t, _ = timed(lambda: p.predict(Xh, Psi=Ph), sync)
        print(f"{a.rows} rows, predict(X, Psi): {1e3 * t:.2f} ms end to end ({p.route})", flush=True)


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
    new = {n: full(n) for n in ("k_predict_noisy_small", "k_predict_noisy_finish")}
    old = {n: full(n) for n in ("k_predict_noisy_diag", "k_pair_table", "k_phi_diag", "k_gen_rowdot")}
    if not new["k_predict_noisy_small"] or not old["k_predict_noisy_diag"]:
        sys.exit("the trace does not hold both routes")
    sn, so = sum(new.values()), sum(old.values())
    print("per full tile, the handle's route: " + " + ".join(f"{n} {v / 1e3:.1f} us" for n, v in new.items()) + f" = {sn / 1e3:.1f} us")
    print("per full tile, the one-shot route: " + " + ".join(f"{n} {v / 1e3:.1f} us" for n, v in old.items()) + f" = {so / 1e3:.1f} us")
    print(f"new / old = {sn / so:.3f} (condition: at most 1.05)")


def one_shot(argv):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import make_problem
    ns = int(argv[1]) if len(argv) > 1 else 20000
    m = int(argv[2]) if len(argv) > 2 else 500
    d = int(argv[3]) if len(argv) > 3 else 10
    method = argv[4] if len(argv) > 4 else "GC"
    model, theta, X, Y, _, rng = make_problem(2000, d, m, 1, method, True, seed=7)
    ctx = gpz_amd.GPzContext(model, X, Y)
    w, iS, _ = ctx.solve(theta)
    ctx.close()
    model.sets = {"best": {"theta": theta, "w": w, "iSigma_w": iS}}
    Xs = rng.standard_normal((ns, d))
    diag = rng.gamma(1.0, 0.05, (ns, d))
    if method[1] == "C":
        Psi = np.zeros((d, d, ns)); Psi[np.arange(d), np.arange(d), :] = diag.T
    else:
        Psi = diag
    gpz_amd.predict(Xs[:64], model, Psi=Psi[:, :, :64] if Psi.ndim == 3 else Psi[:64])
    for name, PP in (("plain", None), ("psi", Psi)):
        t0 = time.perf_counter()
        out = gpz_amd.predict(Xs, model, Psi=PP)
        print(f"{method} {name} ns={ns} m={m} d={d}: {(time.perf_counter() - t0) * 1e3:.1f} ms finite={bool(np.isfinite(out[0]).all())}", flush=True)


def main():
    if len(sys.argv) < 2 or sys.argv[1] not in ("e2e", "kernel", "tiles", "-h", "--help"):
        return one_shot(sys.argv)
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--rows", type=int, default=1_000_000)
    q.add_argument("--rounds", type=int, default=3)
    q = sub.add_parser("kernel")
    q.add_argument("--rows", type=int, default=1_048_576)
    q = sub.add_parser("tiles")
    q.add_argument("trace", help="kernel_trace.csv of the rocprofv3 run")
    q.add_argument("--csv", help="write the per-kernel statistics to this file")
    a = ap.parse_args()
    shape()
    {"e2e": e2e, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
