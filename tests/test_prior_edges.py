"""What train() runs once around the optimiser, at the edges of its kernels: getPrior (k_phi_norm*, k_prior_iter*, k_prior_update of
k_gen.hip) twice at the end of every run, the N output of getPHI they start from, and the Dxy of init (k_dxy, k_rows.hip).

getPrior   the wave kernel (m <= 256) with every one of a lane's four columns in use and with a grid-stride loop that wraps
           (n > 4096); the column-strip kernels k_prior_iter<2|4|8|16> (m > 256) at every strip count and with a wrapping row loop
           (n > 1024); more than 16 strips (m > 4096); VC and GL; rows with missing values (the general k_phi_norm) and with input
           noise.  The centres of the last eight basis functions sit on rows of X, so the highest columns carry weight and a column
           nobody wrote cannot hide under a max norm.  Gates: |sum - 1| <= 1e-12; rel(prior, prior_ld) <= 1e-8 (the project's gate;
           float64 is some six orders below it on these inputs); every element above 1e-6 max(prior_ld) to 1e-8 relatively.
           The iteration count in three cases - inside the first batch of ten, in a later batch, at the limit of 100.
N          complete rows against the long-double densities formed from the parameters, a second column block and a striding row
           loop of k_phi_norm_cols; the NaN and Psi rows against the oracle.  Gate: max(phi_tol, 1e-11), the existing one.
Dxy        |D - D_ld| <= (d + 4) 2^-52 (xx + yy) per element, from one point to ny = 70 000 (past the launcher's cap on gridDim.y: the kernel's loop over ny wraps), far from
           the origin and with coincident points.

train_side_reference.py holds the references, inputs and case tables, test_train_side_reference_cpu.py checks their fitness without
a GPU.  Nothing here retries a GPU step.  The figures of every case are printed (run with -s).

Measured on an MI355X (51 tests, 10 s), worst over the cases:
    prior   |sum - 1| 6.3e-17; max-norm error 2.6e-14 (m = 4500); worst element above 1e-6 max 7.6e-14 (m = 2048) - gate 1e-8 each;
            the iteration counts 5, 61 and 100 are the reference's
    N       6.2e-16 in the max norm, 7.6e-16 on the worst column (VC, m = 513); NaN and Psi rows 6.8e-16 - gate 1e-11
    Dxy     error / gate 0.35 (ny = 70 000, d = 2), the oracle's own float64 Dxy has the same 0.35 there
Against the library as it was before k_prior_iter_loop, m = 4097 gave a max-norm error of 1.9e-5 and m = 4500 of 1.5, both with
GPZ_OK and a prior that summed to one.  The ny = 70 000 launch was accepted by the device before the cap as well."""
import numpy as np
import pytest

import gpz_amd
import train_side_reference as R
from oracle import gpz_oracle as O
from test_gpu_parity import phi_tol

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_WHY)]


# ---- getPrior ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.PRIOR_CASES, ids=[c["id"] for c in R.PRIOR_CASES])
def test_prior_against_the_long_double_fixed_point(case):
    model, theta, X, Psi = R.prior_problem(case)
    want, it_ld, _, _ = R.prior_reference(case["id"])
    assert R.tail_weight(want, case["m"]) >= R.PRIOR_TAIL_FITNESS, "the last columns carry no weight: the inputs cannot be judged"
    got, it = gpz_amd.getPrior(X, Psi, theta, model, None, return_iterations=True)
    assert got.shape == (case["m"],) and np.all(np.isfinite(got))
    err_sum = abs(float(np.sum(got.astype(R.LD)) - 1))
    err = R.rel_ld(got, want)
    big = want > 1e-6 * np.max(want)
    err_el = float(np.max(np.abs(got.astype(R.LD)[big] - want[big]) / want[big]))
    print("\n%s: |sum - 1| %.2e, max-norm error %.2e, worst element above 1e-6 max %.2e (%d of %d), iterations %d (reference %d)"
          % (case["id"], err_sum, err, err_el, int(big.sum()), case["m"], it, it_ld))
    assert err_sum <= 1e-12
    assert err <= R.PRIOR_TOL
    assert err_el <= R.PRIOR_TOL
    assert 1 <= it <= 100


@pytest.mark.parametrize("which", list(R.COUNTED))
def test_prior_iteration_count(which):
    """The host applies the test of getPrior.m:18 to a batch of ten priors in order: the count is that of testing after every pass."""
    model, theta, X = R.counted_problem(which)
    want, it_ld, ratios = R.counted_reference(which)
    lo, hi = R.COUNTED[which]
    assert lo <= it_ld <= hi and R.count_is_decidable(it_ld, ratios), "the reference's count is not decidable in float64"
    got, it = gpz_amd.getPrior(X, None, theta, model, None, return_iterations=True)
    print("\n%s: %d iterations (reference %d), error %.2e" % (which, it, it_ld, R.rel_ld(got, want)))
    assert it == it_ld
    assert R.rel_ld(got, want) <= R.PRIOR_TOL


# ---- N of getPHI ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,d,n,m", R.N_CASES)
def test_norm_densities_of_complete_rows(method, d, n, m):
    model, theta, X = R.n_problem(method, d, n, m)
    want = R.norm_densities(model, theta, X)
    PHI, _, _, N = gpz_amd.getPHI(X, None, theta, model, want_N=True)
    tol = max(phi_tol(model, theta), 1e-11)
    err = R.rel_ld(N, want)
    # per column as well: the normalising constants differ by orders between basis functions
    cols = np.max(np.abs(N.astype(R.LD) - want), axis=0) / np.maximum(np.max(want, axis=0), R.LD(1e-300))
    print("\n%s n = %d, m = %d: N error %.2e, worst column %.2e (gate %.2e)" % (method, n, m, err, float(np.max(cols)), tol))
    assert N.shape == (n, m) and err <= tol
    assert float(np.max(cols)) <= tol


@pytest.mark.parametrize("case_id", ["nan-VD-m300", "psi-VD-m300"])
def test_norm_densities_of_the_other_routes(case_id):
    model, theta, X, Psi = R.prior_problem(R.PRIOR_BY_ID[case_id])
    want = O.getPHI(X, Psi, theta, model, None, want_N=True)
    got = gpz_amd.getPHI(X, Psi, theta, model, want_N=True)
    tol = max(phi_tol(model, theta), 1e-11)
    print("\n%s: PHI error %.2e, N error %.2e (gate %.2e)" % (case_id, R.rel_ld(got[0], want[0]), R.rel_ld(got[3], want[3]), tol))
    assert R.rel_ld(got[0], want[0]) <= tol and R.rel_ld(got[3], want[3]) <= tol


# ---- Dxy -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DXY_CASES, ids=[c["id"] for c in R.DXY_CASES])
def test_dxy_against_long_double(case):
    X, Y = R.dxy_inputs(case)
    want, T = R.dxy_reference(case["id"])
    D = gpz_amd.Dxy(X, Y)
    assert D.shape == want.shape and np.all(np.isfinite(D))
    worst = R.dxy_worst(D, want, T, case["d"])
    print("\nDxy %s: error / gate %.3f" % (case["id"], worst))
    assert worst <= 1.0
