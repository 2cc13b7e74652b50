"""Timings of the stacked predictive densities (gpz_amd.Predictor.stack; DESIGN.md section 14, profiles/r09_predict_stack.txt).

    python tools/predict_stack_timing.py e2e [--rows N] [--rounds R]   # stack vs draws vs draws + predict + the host reduction
    python tools/predict_stack_timing.py big [--rows N] [--chunk C]    # a catalogue generated and stacked in chunks, summed
    python tools/predict_stack_timing.py kernel [--rows N]             # one stack call, for rocprofv3 --kernel-trace --stats
    python tools/predict_stack_timing.py bound STATS [--rows N]        # that run's kernel_stats.csv or results .db against the bound

The shape: VD, d = 5, m = 100, k = 1, 64 draws, 300 bins over the 1st to 99th percentile of the predictions, 8 groups by a split of
the first input, weights in (0.5, 1.5).
e2e: medians over interleaved rounds in one process, each call timed from entry to return (the calls return host arrays): (s) stack,
(a) draws alone, (b) draws + predict + the NumPy / SciPy reduction of tests/test_predictor_stack_cpu.py; the reduction is timed on
--ref-rows rows and scaled to --rows (it is linear in the rows and would take an hour at 1e7).
big: rows/s of chunked stack calls summed on the host, the handle's device bytes after the first and the last chunk.
bound: evaluations of Phi in the window x columns x rows x 70 f64 vector instructions (the f64 arithmetic of one edge in the compiled
pass of k_stack_tile: stack_tail and the mass; DESIGN.md section 14 uses the same number) at the f64 vector rate (256 CUs x 4 SIMDs x
16 lanes x 2.4 GHz), against the summed time of k_stack_tile; k_predict_draws and k_stack_accum beside it."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpz_amd  # noqa: E402
from predict_draws_timing import model_of  # noqa: E402

D, M, K, DRAWS, BINS, GROUPS = 5, 100, 1, 64, 300, 8
F64_LANES_PER_S = 256 * 4 * 16 * 2.4e9
TAIL_INSTRUCTIONS = 70   # f64 vector arithmetic per edge in the compiled pass (stack_tail + the mass), as in DESIGN.md section 14
TCUT = 9.0   # GPZ_STACK_TCUT


def chunk_of(n, seed):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.standard_normal((n, D)))
    groups = np.clip(np.floor((X[:, 0] + 2.0) * (GROUPS / 4.0)), 0, GROUPS - 1).astype(np.int32)
    return X, groups, rng.uniform(0.5, 1.5, n)


def edges_of(p):
    mu = p.predict(chunk_of(100_000, 99)[0])[0]
    lo, hi = np.percentile(mu, [1, 99])
    return np.linspace(lo, hi, BINS + 1)


def window_of(p, edges, n=20_000):
    """Mean number of edges evaluated per (row, column): the edges within TCUT widths and one beyond on either side."""
    X = chunk_of(n, 98)[0]
    mu, sigma, _, beta = p.predict(X)[:4]
    F = p.draws(X, DRAWS, seed=1)
    tot = 0.0
    for m, s2 in [(mu, sigma)] + [(f, beta) for f in F]:
        s = np.sqrt(s2[:, 0])
        a = np.searchsorted(edges, m[:, 0] - TCUT * s, side="left")
        b = np.searchsorted(edges, m[:, 0] + TCUT * s, side="right")
        ja, jb = np.maximum(a - 1, 0), np.minimum(b, BINS)
        tot += np.mean(np.where(jb > ja, jb - ja + 1, 0))
    return tot / (1 + DRAWS)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def e2e(a):
    from test_predictor_stack_cpu import stack_reference
    model = model_of("VD", M, D, K, seed=1)
    X, groups, weights = chunk_of(a.rows, 1)
    nr = min(a.ref_rows, a.rows)
    with gpz_amd.Predictor(model) as p:
        edges = edges_of(p)
        p.stack(X[:4096], edges, n_draws=DRAWS, seed=1, groups=groups[:4096], n_groups=GROUPS, weights=weights[:4096])
        p.draws(X[:4096], DRAWS, seed=1)
        ts, ta, tp, tr = [], [], [], []
        for r in range(a.rounds):
            t, res = timed(lambda: p.stack(X, edges, n_draws=DRAWS, seed=1, groups=groups, n_groups=GROUPS, weights=weights))
            ts.append(t)
            t, F = timed(lambda: p.draws(X, DRAWS, seed=1))
            ta.append(t)
            t, out = timed(lambda: p.predict(X))
            tp.append(t)
            t, ref = timed(lambda: stack_reference(out[0][:nr], out[1][:nr], F[:, :nr], out[3][:nr], edges, groups[:nr], weights[:nr],
                                                   n_groups=GROUPS))
            tr.append(t * a.rows / nr)
            if r == 0:
                part = p.stack(X[:nr], edges, n_draws=DRAWS, seed=1, groups=groups[:nr], n_groups=GROUPS, weights=weights[:nr])
                err = np.max(np.abs(part.hist - ref[0])) / np.max(ref[0])
                print(f"stack against the host reduction on {nr} rows: max |diff| / max = {err:.2e}", flush=True)
            del F, out
            print(f"round {r}: stack {ts[-1]:.3f} s, draws {ta[-1]:.3f} s, predict {tp[-1]:.3f} s, host reduction (scaled) {tr[-1]:.1f} s",
                  flush=True)
        s, d, pr, hr = (float(np.median(v)) for v in (ts, ta, tp, tr))
        print(f"e2e {a.rows} rows, {DRAWS} draws, {BINS} bins, {GROUPS} groups, medians of {a.rounds} rounds: stack {s:.3f} s "
              f"({a.rows / s:.3g} rows/s); (a) draws alone {d:.3f} s = {d / s:.2f} x stack; (b) draws + predict + host reduction "
              f"{d + pr + hr:.1f} s = {(d + pr + hr) / s:.0f} x stack (the reduction timed on {nr} rows and scaled)")
        print(f"route: {p.route}; device bytes {p.info[1]}; edges evaluated per (row, column): {window_of(p, edges):.1f}")


def big(a):
    model = model_of("VD", M, D, K, seed=1)
    with gpz_amd.Predictor(model) as p:
        edges = edges_of(p)
        X, groups, weights = chunk_of(4096, 0)
        p.stack(X, edges, n_draws=DRAWS, seed=1, groups=groups, n_groups=GROUPS, weights=weights)
        total, t_stack, t_all, first = None, 0.0, time.perf_counter(), None
        for c in range(a.rows // a.chunk):
            X, groups, weights = chunk_of(a.chunk, 1000 + c)
            t, r = timed(lambda: p.stack(X, edges, n_draws=DRAWS, seed=1, groups=groups, n_groups=GROUPS, weights=weights))
            t_stack += t
            total = list(r[:4]) if total is None else [u + v for u, v in zip(total, r[:4])]
            first = p.info[1] if first is None else first
            print(f"chunk {c}: {a.chunk} rows in {t:.3f} s, device bytes {p.info[1]}", flush=True)
        t_all = time.perf_counter() - t_all
        n = a.rows // a.chunk * a.chunk
        print(f"big {n} rows in chunks of {a.chunk}: {t_stack:.2f} s in stack = {n / t_stack:.3g} rows/s ({t_all:.1f} s with the "
              f"generation of the chunks); device bytes after the first chunk {first}, after the last {p.info[1]}; "
              f"sum of the weights {total[1].sum():.6g}, mass in the bins, column 0: {total[0][0].sum():.6g}")


def kernel(a):
    model = model_of("VD", M, D, K, seed=1)
    X, groups, weights = chunk_of(a.rows, 1)
    with gpz_amd.Predictor(model) as p:
        edges = edges_of(p)
        p.stack(X[:4096], edges, n_draws=DRAWS, seed=1, groups=groups[:4096], n_groups=GROUPS, weights=weights[:4096])
        t, _ = timed(lambda: p.stack(X, edges, n_draws=DRAWS, seed=1, groups=groups, n_groups=GROUPS, weights=weights))
        print(f"{a.rows} rows in {1e3 * t:.1f} ms end to end ({p.route})")
        print(f"edges evaluated per (row, column): {window_of(p, edges):.2f}", flush=True)


def stats_rows(path, out_csv=None):
    """Rows (Name, Calls, TotalDurationNs, AverageNs, Percentage) of rocprofv3 --kernel-trace --stats: its kernel_stats.csv (--output-format
    csv) or the top_kernels view of its results database (the default format, microseconds there), and per kernel the median of the
    launches that take more than half of the longest one (the full tiles) where the database gives the launches."""
    if not path.endswith(".db"):
        rows = list(csv.DictReader(open(path)))
        return [dict(r, Name=r.get("Name", r.get("KernelName", ""))) for r in rows], {}
    import sqlite3
    con = sqlite3.connect(path)
    rows = [{"Name": n, "Calls": str(c), "TotalDurationNs": f"{1e3 * t:.0f}", "AverageNs": f"{1e3 * av:.0f}", "Percentage": f"{pc:.4f}"}
            for n, c, t, av, pc in con.execute("select name, total_calls, total_duration, average, percentage from top_kernels")]
    full = {}
    for r in rows:
        d = np.array([v[0] for v in con.execute("select duration from kernels where name = ?", (r["Name"],))], dtype=np.float64)
        if d.size:
            full[r["Name"]] = float(np.median(d[d > 0.5 * d.max()]))
    if out_csv:
        with open(out_csv, "w", newline="") as fh:
            w = csv.DictWriter(fh, fieldnames=list(rows[0]))
            w.writeheader()
            w.writerows(rows)
    return rows, full


def bound(a):
    rows, full = stats_rows(a.stats, a.csv)
    for r in rows:
        if any(s in r["Name"] for s in ("k_stack", "k_predict_draws", "k_predict_small")):
            tile = f", full tiles: median {full[r['Name']] / 1e6:.3f} ms" if r["Name"] in full else ""
            print(f"{r['Name'].split('(')[0]}: {r['Calls']} launches, {float(r['TotalDurationNs']) / 1e6:.3f} ms in all, "
                  f"{float(r['Percentage']):.2f} % of the kernel time{tile}")
    st = [r for r in rows if "k_stack_tile" in r["Name"]]
    if not st:
        sys.exit("no k_stack_tile row in " + a.stats)
    total_ns, calls = float(st[0]["TotalDurationNs"]), int(st[0]["Calls"])
    evals = a.window * (1 + DRAWS) * K * (a.rows + 4096)
    floor = evals * TAIL_INSTRUCTIONS / F64_LANES_PER_S
    print(f"k_stack_tile: {calls} launches, {total_ns / 1e6:.2f} ms in all, {total_ns / 1e6 * 131072 / (a.rows + 4096):.3f} ms per "
          f"131072-row tile; bound {floor * 1e3:.2f} ms ({a.window:.1f} edges x {(1 + DRAWS) * K} columns x {a.rows + 4096} rows x "
          f"{TAIL_INSTRUCTIONS} instructions): {100 * floor / (total_ns / 1e9):.0f} % of the kernel's time")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("e2e")
    q.add_argument("--rows", type=int, default=10_000_000)
    q.add_argument("--rounds", type=int, default=3)
    q.add_argument("--ref-rows", type=int, default=20_000)
    q = sub.add_parser("big")
    q.add_argument("--rows", type=int, default=100_000_000)
    q.add_argument("--chunk", type=int, default=10_000_000)
    q = sub.add_parser("kernel")
    q.add_argument("--rows", type=int, default=1_048_576)
    q = sub.add_parser("bound")
    q.add_argument("stats", help="kernel_stats.csv or the results database of the rocprofv3 run")
    q.add_argument("--csv", help="write the statistics rows read from a results database to this file")
    q.add_argument("--rows", type=int, default=1_048_576)
    q.add_argument("--window", type=float, required=True, help="edges evaluated per (row, column), as the kernel run printed it")
    a = ap.parse_args()
    {"e2e": e2e, "big": big, "kernel": kernel, "bound": bound}[a.cmd](a)


if __name__ == "__main__":
    main()
