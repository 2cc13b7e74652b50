"""Wall time and rows/s of gpz_amd.Predictor.predict against gpz_amd.predict on the same seeded inputs (profiles/r07_predict_stream.txt).

    python tools/predict_stream_timing.py [--quick] [--api-cap N]

Each measurement: one warm-up call, then the best of --reps timed calls, a device synchronise inside the timed region.  The handle is
created outside the timed region (its creation time is printed separately).  predict() returns PHI (n x m doubles on the host) on every
call, so it is timed on at most --api-cap rows (default 1e6) and reported as rows/s; the speed-up compares rows/s.  The models are
synthetic (random well-conditioned parameters): prediction cost does not depend on the values.  X is column-major (a columnar
catalogue); a row-major X adds one transposing pass on the host to both paths.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpz_amd  # noqa: E402


def sync():
    try:
        import torch
        torch.cuda.synchronize()
    except Exception:
        pass


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


def best_of(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="1e6 instead of 1e7 rows for the catalogue shapes")
    ap.add_argument("--api-cap", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    big = 1_000_000 if a.quick else 10_000_000
    shapes = [(100_000, 10, 100, "VD", False), (100_000, 10, 100, "VC", False), (100_000, 10, 200, "VD", False),
              (100_000, 10, 200, "VC", False), (100_000, 10, 500, "VD", False), (100_000, 10, 500, "VC", False),
              (big, 5, 100, "VD", False), (big, 5, 100, "VD", True), (big, 10, 200, "VD", False),
              (2 * big, 10, 1000, "VD", False)]   # more rows than predict() could hold on the device at m = 1000
    print(f"{'n':>9} {'d':>3} {'m':>4} {'kind':>4} {'Psi':>3} | {'route':>5} {'create ms':>9} {'handle ms':>10} {'rows/s':>9} | "
          f"{'predict rows':>12} {'ms':>9} {'rows/s':>9} | {'speed-up':>8}")
    for n, d, m, method, with_psi in shapes:
        model = model_of(method, m, d, seed=m + d)
        rng = np.random.default_rng(n + m + d)
        X = np.asfortranarray(rng.standard_normal((n, d)))           # a columnar catalogue (one array per band)
        Psi = np.asfortranarray(rng.gamma(1.0, 0.02, (n, d))) if with_psi else None
        t0 = time.perf_counter()
        p = gpz_amd.Predictor(model)
        route = p.info[2]
        t_create = time.perf_counter() - t0
        reps = 1 if n >= 10_000_000 else a.reps
        t_h = best_of(lambda: p.predict(X, Psi=Psi), reps)
        p.close()
        na = min(n, a.api_cap if m < 1000 else a.api_cap // 10)
        Xa, Pa = X[:na], (None if Psi is None else Psi[:na])
        t_a = best_of(lambda: gpz_amd.predict(Xa, model, Psi=Pa), 1 if na >= 1_000_000 else a.reps)
        rh, ra = n / t_h, na / t_a
        print(f"{n:>9} {d:>3} {m:>4} {method:>4} {'yes' if with_psi else 'no':>3} | {('fused', 'tiles')[route]:>5} {1e3 * t_create:>9.1f} "
              f"{1e3 * t_h:>10.1f} {rh:>9.3g} | {na:>12} {1e3 * t_a:>9.1f} {ra:>9.3g} | {rh / ra:>8.1f}", flush=True)


if __name__ == "__main__":
    main()
