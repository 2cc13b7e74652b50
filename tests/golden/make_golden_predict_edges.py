"""Generate the fixtures of tests/predict_edges.py (pe_*.npz) from the NumPy oracle.

    python tests/golden/make_golden_predict_edges.py [--jobs N] [id prefix ...]

One file per case of predict_edges.CASES that is marked ``fixture`` - the cases whose two oracle calls (the model and its abs_model)
take more than about 2 s: predictNoisy of a covariance kind beyond ~20 000 (pair, row) steps, predictMissing of GC / VC at m = 63 .. 65.
A file holds the model and the inputs as gpz_amd.predict takes them (float32 where the values are float32-valued, a d x d x n Psi as its
two n x d factors, predict_edges.psi_cube), the oracle's outputs and the term scales s_* (sigma and s_sigma are re-formed from their
terms on loading) and, for a covariance case, e_ref_twin: the oracle against the extended-precision
reference on the diagonal-Gamma twin of the case (predict_edges.reference_error), which test_predict_edges_cpu.py holds to a tenth
of the gate.  Same status as make_golden_predict.py: outputs of oracle/gpz_oracle.py frozen at generation time."""
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import predict_edges as E  # noqa: E402


def write(case_id):
    case = E.CASE_BY_ID[case_id]
    t0 = time.time()
    arr = E.fixture_arrays(case)
    if E.run_method(case)[1] == "C":
        arr["e_ref_twin"] = E.reference_error(case)[0]
    path = E.fixture_path(case)
    np.savez_compressed(path, **arr)
    return "%-32s %6.1f s %7.1f KB  e_ref_twin %.2e" % (case_id, time.time() - t0, os.path.getsize(path) / 1024.0,
                                                       float(arr.get("e_ref_twin", 0.0)))


def main():
    args = sys.argv[1:]
    jobs = 1
    if "--jobs" in args:
        at = args.index("--jobs")
        jobs = int(args[at + 1])
        del args[at:at + 2]
    ids = [c["id"] for c in E.CASES if c["fixture"] and (not args or any(c["id"].startswith(a) for a in args))]
    if jobs > 1:
        with multiprocessing.Pool(jobs) as pool:
            for line in pool.imap_unordered(write, ids):
                print(line, flush=True)
    else:
        for case_id in ids:
            print(write(case_id), flush=True)
    print("wrote %d fixtures of predict_edges" % len(ids))


if __name__ == "__main__":
    main()
