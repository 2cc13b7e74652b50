"""Timings of the device-resident predictor entries (gpz_amd.Predictor.predict_dev / draws_dev / stack_dev; DESIGN.md section 15,
profiles/r10_predict_dev.txt).

    python tools/predict_dev_timing.py e2e [--rows N] [--rounds R]   # the *_dev methods against the host methods of the same handle
    python tools/predict_dev_timing.py kernel [--rows N]             # predict_dev calls only, for rocprofv3 --kernel-trace --stats
    python tools/predict_dev_timing.py tiles TRACE [--csv OUT]       # that run's kernel_trace.csv: the new kernels per full tile

The shape: VD, d = 5, m = 100, k = 1; 64 draws, 300 bins, 8 groups for draws and stack, as tools/predict_stack_timing.py.
e2e: medians over interleaved rounds in one process after a warm-up call per method, each call timed from entry to return (the
device methods return when the device is done; the current stream is synchronised before the clock starts).  Rows: predict_dev with X
float64 row-major and float32 on the device; the honest end to end for a host catalogue (torch.from_numpy(X).cuda() + predict_dev +
.cpu() of the five outputs); draws_dev and stack_dev; against predict, draws and stack on the same rows as NumPy arrays.
tiles: per kernel the launches, the total, and the median of the launches that take more than half of the longest one (the full
tiles); then k_pred_stage + k_pred_finish_dev per full tile as a share of k_predict_small's (the acceptance condition is 25 %)."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpz_amd  # noqa: E402
from predict_draws_timing import model_of  # noqa: E402
from predict_stack_timing import BINS, D, DRAWS, GROUPS, K, M, chunk_of, edges_of  # noqa: E402


def timed(fn, sync=None):
    if sync:
        sync()
    t0 = time.perf_counter()
    r = fn()
    if sync:
        sync()
    return time.perf_counter() - t0, r


def e2e(a):
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    model = model_of("VD", M, D, K, seed=1)
    Xf, groups, weights = chunk_of(a.rows, 1)
    X = torch.from_numpy(np.ascontiguousarray(Xf)).to(dev)               # row-major on the device, as torch makes it
    Xh = Xf                                                              # columnar on the host: the host methods' best case
    X32 = X.float()
    gd, wd = torch.from_numpy(groups).to(dev), torch.from_numpy(weights).to(dev)
    names = ("predict", "predict_dev f64", "predict_dev f32", "host catalogue through predict_dev", "draws", "draws_dev", "stack",
             "stack_dev")
    with gpz_amd.Predictor(model) as p:
        edges = edges_of(p)
        kw = dict(n_draws=DRAWS, seed=1, n_groups=GROUPS)

        def through_device():
            return [t.cpu() for t in p.predict_dev(torch.from_numpy(Xh).to(dev))]

        calls = (lambda: p.predict(Xh), lambda: p.predict_dev(X), lambda: p.predict_dev(X32), through_device,
                 lambda: p.draws(Xh, DRAWS, seed=1), lambda: p.draws_dev(X, DRAWS, seed=1),
                 lambda: p.stack(Xh, edges, groups=groups, weights=weights, **kw),
                 lambda: p.stack_dev(X, edges, groups=gd, weights=wd, **kw))
        w = 4096
        p.predict(Xh[:w]); p.predict_dev(X[:w]); p.predict_dev(X32[:w]); p.draws(Xh[:w], DRAWS, seed=1); p.draws_dev(X[:w], DRAWS, seed=1)
        p.stack(Xh[:w], edges, groups=groups[:w], weights=weights[:w], **kw)
        p.stack_dev(X[:w], edges, groups=gd[:w], weights=wd[:w], **kw)
        ts = {n: [] for n in names}
        for r in range(a.rounds):
            for n, c in zip(names, calls):
                t, res = timed(c, sync)
                ts[n].append(t)
                if r == 0 and n == "predict":
                    ref = res
                if r == 0 and n == "predict_dev f64":
                    same = all(np.array_equal(u.cpu().numpy(), v) for u, v in zip(res, ref))
                    print(f"predict_dev against predict on {a.rows} rows: {'the same bits' if same else 'DIFFERENT'}", flush=True)
                del res
            print(f"round {r}: " + ", ".join(f"{n} {ts[n][-1]:.4f} s" for n in names), flush=True)
        med = {n: float(np.median(v)) for n, v in ts.items()}
        print(f"e2e {a.rows} rows, d = {D}, m = {M}, k = {K}, {DRAWS} draws, {BINS} bins, {GROUPS} groups, medians of {a.rounds} rounds:")
        for n in names:
            print(f"  {n:36s} {med[n]:8.4f} s   {a.rows / med[n]:.3g} rows/s")
        print(f"  predict_dev f64 = {med['predict'] / med['predict_dev f64']:.1f} x predict, f32 {med['predict'] / med['predict_dev f32']:.1f} x; "
              f"host catalogue through the device {med['predict'] / med['host catalogue through predict_dev']:.2f} x; "
              f"draws_dev {med['draws'] / med['draws_dev']:.1f} x draws; stack_dev {med['stack'] / med['stack_dev']:.2f} x stack")
        print(f"route: {p.route}; device bytes {p.info[1]}")


def kernel(a):
    import torch
    dev = torch.device("cuda", 0)
    model = model_of("VD", M, D, K, seed=1)
    X = torch.from_numpy(np.ascontiguousarray(chunk_of(a.rows, 1)[0])).to(dev)
    X32 = X.float()
    with gpz_amd.Predictor(model) as p:
        p.predict_dev(X[:4096])
        for x, what in ((X, "float64 row-major"), (X32, "float32 row-major"), (X.T.contiguous().T, "float64 column-major")):
            t, _ = timed(lambda: p.predict_dev(x), lambda: torch.cuda.synchronize(dev))
            print(f"{a.rows} rows, {what}: {1e3 * t:.2f} ms end to end ({p.route})", flush=True)


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

    def full(part):   # all instantiations of a kernel in the trace (k_pred_stage: f64 and f32 rows), the slowest full-tile median
        v = [float(r["FullTileMedianNs"]) for r in out if part in r["Name"]]
        if not v:
            sys.exit(f"no {part} row in {a.trace}")
        return max(v)
    st, fi, sm = full("k_pred_stage"), full("k_pred_finish_dev"), full("k_predict_small")
    print(f"per full tile: k_pred_stage {st / 1e3:.1f} us + k_pred_finish_dev {fi / 1e3:.1f} us = {(st + fi) / 1e3:.1f} us, "
          f"{100 * (st + fi) / sm:.1f} % of k_predict_small's {sm / 1e3:.1f} us (condition: at most 25 %); "
          f"k_pred_check_dev (once per call, all rows): {full('k_pred_check_dev') / 1e3:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--rows", type=int, default=10_000_000)
    q.add_argument("--rounds", type=int, default=3)
    q = sub.add_parser("kernel")
    q.add_argument("--rows", type=int, default=1_048_576)
    q = sub.add_parser("tiles")
    q.add_argument("trace", help="kernel_trace.csv of the rocprofv3 run")
    q.add_argument("--csv", help="write the per-kernel statistics to this file")
    a = ap.parse_args()
    {"e2e": e2e, "kernel": kernel, "tiles": tiles}[a.cmd](a)


if __name__ == "__main__":
    main()
