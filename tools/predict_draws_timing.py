"""Timings of the posterior draws (gpz_amd.Predictor.draws; DESIGN.md section 13, profiles/r08_predict_draws*).

    python tools/predict_draws_timing.py kernel [--rows N]             # the k_predict_draws shapes, for rocprofv3 --kernel-trace --stats
    python tools/predict_draws_timing.py bound STATS_CSV [--rows N]    # kernel time from rocprofv3's kernel_stats.csv against the bound
    python tools/predict_draws_timing.py e2e [--quick]                 # end to end: draws vs predict() on the handle vs the host product

kernel: VD, d = 10, m = 200, k = 1, 1e6 rows, n_draws 16, 64, 256 in that order (one call each after a warm-up call of 4096 rows).
bound: the launches of k_predict_draws in kernel_trace.csv, in launch order, are the warm-up call's one and then one group per
n_draws (16, 64, 256), a launch per tile; kernel_stats.csv's row is printed beside them.  The bound per row is the larger of
2 ceil16(m) n_draws k flop at the f64 MFMA peak (78.6 TF) and 8 n_draws k bytes at the HBM peak (8 TB/s).
e2e: 1e7 rows, d = 5, m = 100, n_draws = 64 (rows/s of draws and of predict() on the same handle and rows); the host alternative -
predict(return_phi=True), then PHI (w + R Z) with NumPy - at 1e6 rows; the tile route at m = 1000, 2e6 rows, n_draws = 64.
Each timed call follows a warm-up call; a device synchronise closes every timed region (the calls return host arrays).
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpz_amd  # noqa: E402

F64_PEAK = 78.6e12   # f64 MFMA, MI355X
HBM_PEAK = 8.0e12
KERNEL_DRAWS = (16, 64, 256)


def model_of(method, m, d, k=1, seed=0):
    rng = np.random.default_rng(seed)
    model = gpz_amd.Model(m=m, d=d, k=k, method=method, heteroscedastic=True)
    if method[1] == "C":
        blocks = 1 if method == "GC" else m
        G = np.concatenate([(0.6 * np.eye(d) + 0.05 * rng.standard_normal((d, d))).ravel(order="F") for _ in range(blocks)])
    else:
        G = rng.uniform(0.3, 0.6, model.g_dim)
    theta = np.concatenate([rng.standard_normal(m * d), G, rng.uniform(-1, 1, m * k), rng.uniform(-3, -1, k),
                            0.05 * rng.standard_normal(m * k), rng.uniform(-1, 1, m * k)])
    A = rng.standard_normal((m, m)) / np.sqrt(m)
    iS = np.stack([0.05 * (A @ A.T) + 0.02 * np.eye(m) for _ in range(k)], axis=2)
    model.sets["best"] = {"theta": theta, "w": rng.standard_normal((m, k)), "iSigma_w": iS}
    return model


def catalogue(n, d, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, d)))   # a columnar catalogue


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def kernel(a):
    model = model_of("VD", 200, 10, seed=1)
    X = catalogue(a.rows, 10, seed=2)
    with gpz_amd.Predictor(model) as p:
        p.draws(X[:4096], 256, seed=1)
        for nd in KERNEL_DRAWS:
            t, _ = timed(lambda: p.draws(X, nd, seed=1))
            print(f"n_draws {nd:4d}: {a.rows} rows in {1e3 * t:.1f} ms end to end ({p.route})", flush=True)


def bound(a):
    rows = list(csv.DictReader(open(a.stats)))
    kr = [r for r in rows if "k_predict_draws" in r.get("Name", r.get("KernelName", ""))]
    if not kr:
        sys.exit("no k_predict_draws rows in " + a.stats)
    m16, k = 208, 1
    # the three timed calls launch one kernel per 131 072-row tile (1e6 rows: 8 launches each) after the warm-up call's one
    if a.trace:
        tr = [r for r in csv.DictReader(open(a.trace)) if "k_predict_draws" in r["Kernel_Name"]]
        tr.sort(key=lambda r: int(r["Start_Timestamp"]))
        tr = tr[1:]   # the warm-up call
        per = len(tr) // len(KERNEL_DRAWS)
        groups = [tr[i * per:(i + 1) * per] for i in range(len(KERNEL_DRAWS))]
        for nd, g in zip(KERNEL_DRAWS, groups):
            ns = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in g)
            fl = 2.0 * m16 * nd * k * a.rows / F64_PEAK
            by = 8.0 * nd * k * a.rows / HBM_PEAK
            bnd = max(fl, by)
            print(f"n_draws {nd:4d}: k_predict_draws {1e-6 * ns:8.3f} ms over {len(g)} launches; bound {1e3 * bnd:7.3f} ms "
                  f"({'f64 MFMA' if fl >= by else 'HBM'}); share {bnd / (1e-9 * ns):.2f}")
    for r in kr:
        print({key: r[key] for key in r if key in ("Name", "KernelName", "Calls", "TotalDurationNs", "AverageNs", "Percentage")})


def e2e(a):
    big = 1_000_000 if a.quick else 10_000_000
    host_rows = 1_000_000 if not a.quick else 200_000
    nd = 64
    print(f"{'case':<34} {'rows':>9} {'ms':>9} {'rows/s':>9}", flush=True)
    model = model_of("VD", 100, 5, seed=3)
    X = catalogue(big, 5, seed=4)
    with gpz_amd.Predictor(model) as p:
        p.draws(X[:100_000], nd, seed=1)
        p.predict(X[:100_000])
        t, F = timed(lambda: p.draws(X, nd, seed=1))
        print(f"{'draws, m=100, 64 draws':<34} {big:>9} {1e3 * t:>9.1f} {big / t:>9.3g}   {p.route}", flush=True)
        del F
        t, _ = timed(lambda: p.predict(X))
        print(f"{'Predictor.predict, m=100':<34} {big:>9} {1e3 * t:>9.1f} {big / t:>9.3g}", flush=True)
        Xh = X[:host_rows]
        st = model.sets["best"]
        iS = np.asarray(st["iSigma_w"]).reshape(100, 100, 1)[:, :, 0]
        R = np.linalg.cholesky(0.5 * (iS + iS.T))
        Z = np.random.default_rng(5).standard_normal((100, nd))

        def host():
            mu, _, _, _, _, PHI = p.predict(Xh, return_phi=True)
            W = st["w"][:, :1] + R @ Z
            return PHI @ W + model.muY
        host()
        t, _ = timed(host)
        print(f"{'host: return_phi + NumPy product':<34} {host_rows:>9} {1e3 * t:>9.1f} {host_rows / t:>9.3g}", flush=True)
    n_tile = 2 * big // 10
    model = model_of("VD", 1000, 10, seed=6)
    X = catalogue(n_tile, 10, seed=7)
    with gpz_amd.Predictor(model) as p:
        p.draws(X[:50_000], nd, seed=1)
        t, _ = timed(lambda: p.draws(X, nd, seed=1))
        print(f"{'draws, tile route, m=1000':<34} {n_tile:>9} {1e3 * t:>9.1f} {n_tile / t:>9.3g}   {p.route}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--rows", type=int, default=1_000_000)
    b = sub.add_parser("bound")
    b.add_argument("stats")
    b.add_argument("--trace", help="rocprofv3's kernel_trace.csv of the same run (per-launch times)")
    b.add_argument("--rows", type=int, default=1_000_000)
    e = sub.add_parser("e2e")
    e.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    {"kernel": kernel, "bound": bound, "e2e": e2e}[a.cmd](a)


if __name__ == "__main__":
    main()
