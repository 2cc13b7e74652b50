"""The order of the predictor's refusals: every gpz_predictor_* entry and every Predictor method called with two things wrong at once, the
return code and the text of gpz_last_error (or the exception) written out; and a refusal in a late tile, with two tiles in flight,
after which the handle returns the bits and holds the bytes of a fresh one."""

import re

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from test_predictor import catalogue, synth_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D, M, K = 5, 50, 2
ARG, UNSUPPORTED = -1, -5
NOT_FITS = ("input noise on the handle needs predict_noisy_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, k <= 8 and "
            "ceil16(m) <= 256 (method VC, d 5, m 50, k 2); gpz_predictor_run takes Psi for every shape")
FORCED = "input noise needs the fused draws route (GPZ_PREDICT_FORCE_TILES is set)"


@pytest.fixture(scope="module")
def handles():
    """name -> (Predictor, handle): VD on the fused route, VD with force_tiles, VC (outside predict_noisy_fits)."""
    made = {}
    for name, method, force in (("VD", "VD", False), ("VDt", "VD", True), ("VC", "VC", False)):
        p = gpz_amd.Predictor(synth_model(method, M, D, K, True, seed=5), tile_rows=1024, force_tiles=force)
        made[name] = (p, p._handle())
    yield made
    for p, _ in made.values():
        p.close()


def refused(rc, code, text):
    assert rc == code, (rc, _lib.load().gpz_last_error())
    assert _lib.load().gpz_last_error().decode() == text


def host_rows(n=8):
    return np.asfortranarray(np.random.default_rng(1).standard_normal((n, D)))


def outs(n, cols=K, count=4):
    return [np.empty((n, cols), order="F") for _ in range(count)]


def stack_call(lib, h, X, ns, ndraws=0, edges=(0.0, 1.0, 2.0), nbins=2, group=None, ngroups=2, weight=None, shift=None, hist=True):
    e = np.ascontiguousarray(np.tile(np.asarray(edges, dtype=np.float64), (K, 1)))
    C_ = 1 + max(ndraws, 0)
    B, G = max(nbins, 1), max(ngroups, 1)
    o = [np.zeros(C_ * G * K * B), np.zeros(G), np.zeros(C_ * G * K), np.zeros(C_ * G * K)]
    return lib.gpz_predictor_stack(h, _lib.dptr(X), ns, ndraws, 0, None, _lib.dptr(e), nbins,
                                   None if group is None else group.ctypes.data_as(_lib.c_int32_p), ngroups, _lib.dptr(weight),
                                   _lib.dptr(o[0]) if hist else None, _lib.dptr(o[1]), _lib.dptr(o[2]), _lib.dptr(o[3]), _lib.dptr(shift))


# ---- the host entries ---------------------------------------------------------------------------------------------------------------------
def test_run_refusals_in_order(handles):
    lib = _lib.load()
    _, h = handles["VD"]
    X, o = host_rows(), outs(8)
    assert lib.gpz_predictor_run(h, _lib.dptr(X), 0, None, 0, None, None, None, None, None) == 0   # no rows: the outputs are not looked at
    refused(lib.gpz_predictor_run(None, None, -1, None, 0, None, None, None, None, None), ARG, "gpz_predictor_run: null handle")
    refused(lib.gpz_predictor_run(h, None, -1, None, 0, None, None, None, None, None), ARG, "gpz_predictor_run: ns < 0")
    refused(lib.gpz_predictor_run(h, _lib.dptr(X), 8, None, 5, None, *(_lib.dptr(a) for a in o[1:]), None), ARG,
            "gpz_predictor_run: null argument")
    refused(lib.gpz_predictor_run(h, _lib.dptr(X), 8, None, 2, *(_lib.dptr(a) for a in o), None), ARG,
            "gpz_predictor_run: psi_kind 2 does not match Psi")
    Xn = X.copy(order="F")
    Xn[3, 1] = np.nan
    refused(lib.gpz_predictor_run(h, _lib.dptr(Xn), 8, _lib.dptr(X), 2, *(_lib.dptr(a) for a in o), None), ARG,
            "gpz_predictor_run: psi_kind 2 is for the covariance kinds")
    refused(lib.gpz_predictor_run(h, _lib.dptr(Xn), 8, None, 0, *(_lib.dptr(a) for a in o), None), UNSUPPORTED,
            "gpz_predictor_run: the rows have missing values (NaN): group them by pattern and call gpz_predict_missing (predict.m:45-69)")


def test_draws_refusals_in_order(handles):
    lib = _lib.load()
    _, h = handles["VD"]
    X, F = host_rows(), np.empty((8, K, 3), order="F")
    refused(lib.gpz_predictor_draws(None, None, -1, 0, 0, None, None), ARG, "gpz_predictor_draws: null handle")
    refused(lib.gpz_predictor_draws(h, None, -1, 0, 0, None, None), ARG, "gpz_predictor_draws: ns < 0")
    refused(lib.gpz_predictor_draws(h, _lib.dptr(X), 8, 0, 0, None, None), ARG,
            "gpz_predictor_draws: need 1 <= ndraws and ndraws * k <= 16384 (ndraws 0, k 2)")
    refused(lib.gpz_predictor_draws(h, None, 0, 0, 0, None, None), ARG,
            "gpz_predictor_draws: need 1 <= ndraws and ndraws * k <= 16384 (ndraws 0, k 2)")
    refused(lib.gpz_predictor_draws(h, None, 8, 8193, 0, None, _lib.dptr(F)), ARG,
            "gpz_predictor_draws: need 1 <= ndraws and ndraws * k <= 16384 (ndraws 8193, k 2)")
    assert lib.gpz_predictor_draws(h, None, 0, 3, 0, None, None) == 0
    refused(lib.gpz_predictor_draws(h, _lib.dptr(X), 8, 3, 0, None, None), ARG, "gpz_predictor_draws: null argument")


def test_draws_noisy_refusals_in_order(handles):
    lib = _lib.load()
    X, F = host_rows(), np.empty((8, K, 3), order="F")
    who = "gpz_predictor_draws_noisy: "
    refused(lib.gpz_predictor_draws_noisy(handles["VC"][1], _lib.dptr(X), 8, None, 0, 0, None, _lib.dptr(F)), ARG,
            who + "need 1 <= ndraws and ndraws * k <= 16384 (ndraws 0, k 2)")
    refused(lib.gpz_predictor_draws_noisy(handles["VC"][1], _lib.dptr(X), 8, None, 3, 0, None, _lib.dptr(F)), UNSUPPORTED, who + NOT_FITS)
    refused(lib.gpz_predictor_draws_noisy(handles["VDt"][1], _lib.dptr(X), 8, None, 3, 0, None, _lib.dptr(F)), UNSUPPORTED, who + FORCED)
    refused(lib.gpz_predictor_draws_noisy(handles["VDt"][1], None, 0, None, 3, 0, None, None), UNSUPPORTED, who + FORCED)
    h = handles["VD"][1]
    assert lib.gpz_predictor_draws_noisy(h, None, 0, None, 3, 0, None, None) == 0
    refused(lib.gpz_predictor_draws_noisy(h, None, -1, None, 0, 0, None, None), ARG, who + "ns < 0")
    refused(lib.gpz_predictor_draws_noisy(h, _lib.dptr(X), 8, None, 3, 0, None, _lib.dptr(F)), ARG, who + "null argument")
    Xn, Pn = X.copy(order="F"), np.asfortranarray(np.full((8, D), 0.01))
    Xn[2, 0] = np.nan
    Pn[1, 4] = -0.5
    refused(lib.gpz_predictor_draws_noisy(h, _lib.dptr(Xn), 8, _lib.dptr(Pn), 3, 0, None, _lib.dptr(F)), UNSUPPORTED,
            "gpz_predictor_draws: the rows have missing values (NaN): draws are for complete rows")
    refused(lib.gpz_predictor_draws_noisy(h, _lib.dptr(X), 8, _lib.dptr(Pn), 3, 0, None, _lib.dptr(F)), ARG,
            who + "Psi has an element that is NaN, infinite or negative")


def test_stack_refusals_in_order(handles):
    lib = _lib.load()
    _, h = handles["VD"]
    X = host_rows()
    who = "gpz_predictor_stack: "
    bad_lab = np.array([0, 1, -1, 7, 0, 1, 9, 0], dtype=np.int32)
    bad_wt = np.array([1, 1, 1, 1, 1, -2.0, 1, 1], dtype=np.float64)
    inf_shift = np.array([0.0, np.inf])
    Xn = X.copy(order="F")
    Xn[6, 2] = np.nan
    refused(stack_call(lib, None, X, -1, ndraws=-1), ARG, who + "null handle")
    refused(stack_call(lib, h, X, -1, ndraws=-1), ARG, who + "ns < 0")
    refused(stack_call(lib, h, X, 8, ndraws=-1, nbins=0), ARG, who + "need 0 <= ndraws and (1 + ndraws) * k <= 16384 (ndraws -1, k 2)")
    refused(stack_call(lib, h, X, 8, ndraws=8192, nbins=0), ARG,
            who + "need 0 <= ndraws and (1 + ndraws) * k <= 16384 (ndraws 8192, k 2)")
    refused(stack_call(lib, h, X, 8, nbins=0, edges=(0.0, 1.0, 1.0)), ARG, who + "need nbins >= 1 and ngroups >= 1")
    refused(stack_call(lib, h, X, 8, nbins=41, ngroups=100, edges=np.arange(42.0), hist=False), ARG,
            who + "ngroups * nbins = 4100 is over GPZ_STACK_MAX_GROUP_BINS = 4096")
    refused(stack_call(lib, h, X, 8, edges=(0.0, 1.0, 1.0), hist=False), ARG, who + "null argument")
    refused(stack_call(lib, h, X, 8, edges=(0.0, 1.0, 1.0), group=bad_lab), ARG,
            who + "the edges must be finite and strictly increasing (output 0, edge 2)")
    refused(stack_call(lib, h, None, 8, group=bad_lab), ARG, who + "null argument")
    refused(stack_call(lib, h, X, 8, group=bad_lab, weight=bad_wt, shift=inf_shift), ARG, who + "label 7 of row 3 is outside [-1, 2)")
    refused(stack_call(lib, h, X, 8, weight=bad_wt, shift=inf_shift), ARG, who + "mu_shift must be finite")
    refused(stack_call(lib, h, Xn, 8, weight=bad_wt), ARG, who + "the weight of row 5 is negative or not finite")
    refused(stack_call(lib, h, Xn, 8), UNSUPPORTED, who + "the rows have missing values (NaN): stacks are for complete rows")


# ---- the device entries -------------------------------------------------------------------------------------------------------------------
def dev_rows(n=8):
    return torch.from_numpy(np.ascontiguousarray(host_rows(n))).to(DEV)


def test_run_dev_refusals_in_order(handles):
    lib = _lib.load()
    _, h = handles["VD"]
    X = dev_rows()
    v = np.ones(D)
    o = [torch.empty((K, 8), dtype=torch.float64, device=DEV) for _ in range(5)]
    ptr = [t.data_ptr() for t in o]
    who = "gpz_predictor_run_dev: "
    refused(lib.gpz_predictor_run_dev(None, None, 7, -1, 1, 1, None, None, None, *[None] * 6, None), ARG, who + "null handle")
    refused(lib.gpz_predictor_run_dev(h, None, 7, -1, 1, 1, None, None, None, *[None] * 6, None), ARG, who + "ns < 0")
    refused(lib.gpz_predictor_run_dev(h, X.data_ptr(), 7, 8, D, 1, _lib.dptr(v), None, None, *ptr, None, None), ARG,
            who + "x_type 7 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused(lib.gpz_predictor_run_dev(h, None, 0, 8, D, 1, _lib.dptr(v), None, None, *ptr, None, None), ARG,
            who + "muX and sdX go together (both or neither)")
    refused(lib.gpz_predictor_run_dev(h, None, 0, 8, 0, 1, None, None, None, *ptr, None, None), ARG, who + "null argument")
    refused(lib.gpz_predictor_run_dev(h, None, 0, 0, -1, 1, None, None, None, *[None] * 6, None), ARG,
            who + "strides (-1, 1) of 0 rows: a stride must be positive")
    refused(lib.gpz_predictor_run_dev(h, X.data_ptr(), 0, 8, 0, 1, None, None, None, *[None] * 6, None), ARG,
            who + "strides (0, 1) of 8 rows: a stride must be positive")
    assert lib.gpz_predictor_run_dev(h, None, 0, 0, D, 1, None, None, None, *[None] * 6, None) == 0
    refused(lib.gpz_predictor_run_dev(h, X.data_ptr(), 0, 8, D, 1, None, None, None, None, *ptr[1:], None, None), ARG, who + "null argument")


def test_draws_dev_refusals_in_order(handles):
    lib = _lib.load()
    _, h = handles["VD"]
    X = dev_rows()
    who = "gpz_predictor_draws_dev: "
    refused(lib.gpz_predictor_draws_dev(h, X.data_ptr(), 7, -1, D, 1, None, None, None, 0, 0, None, None, None), ARG, who + "ns < 0")
    refused(lib.gpz_predictor_draws_dev(h, X.data_ptr(), 7, 8, D, 1, None, None, None, 0, 0, None, None, None), ARG,
            who + "need 1 <= ndraws and ndraws * k <= 16384 (ndraws 0, k 2)")
    refused(lib.gpz_predictor_draws_dev(h, X.data_ptr(), 7, 8, D, 1, None, None, None, 3, 0, None, None, None), ARG,
            who + "x_type 7 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused(lib.gpz_predictor_draws_dev(h, X.data_ptr(), 1, 8, D, -2, None, None, None, 3, 0, None, None, None), ARG,
            who + "strides (5, -2) of 8 rows: a stride must be positive")
    assert lib.gpz_predictor_draws_dev(h, None, 0, 0, D, 1, None, None, None, 3, 0, None, None, None) == 0
    refused(lib.gpz_predictor_draws_dev(h, X.data_ptr(), 0, 8, D, 1, None, None, None, 3, 0, None, None, None), ARG, who + "null argument")


def test_run_noisy_dev_refusals_in_order(handles):
    lib = _lib.load()
    X, P = dev_rows(), torch.full((8, D), 0.01, dtype=torch.float64, device=DEV)
    v = np.ones(D)
    who = "gpz_predictor_run_noisy_dev: "

    def call(h, x_type=0, psi=P.data_ptr(), psi_type=0, psi_rs=D, sdX=None, sd2=None, ns=8, o=(None,) * 5):
        return lib.gpz_predictor_run_noisy_dev(h, X.data_ptr(), x_type, ns, D, 1, psi, psi_type, psi_rs, 1, _lib.dptr(sdX), _lib.dptr(sdX),
                                               _lib.dptr(sd2), None, *o, None)

    refused(call(handles["VC"][1], x_type=7, ns=-1), ARG, who + "ns < 0")
    refused(call(handles["VC"][1], x_type=7), UNSUPPORTED, who + NOT_FITS)
    h = handles["VDt"][1]                                                 # predictNoisy on the handle does not mind force_tiles
    refused(call(h, x_type=7, psi_type=9), ARG, who + "x_type 7 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused(call(h, psi_type=9, sdX=v), ARG, who + "psi_type 9 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused(call(h, psi=None, sdX=v), ARG, who + "sdX and sd2 go together (both or neither)")
    refused(call(h, psi=None, psi_rs=0), ARG, who + "null Psi")
    refused(call(h, psi_rs=0), ARG, who + "Psi strides (0, 1) of 8 rows: the row stride must be positive")
    assert call(h, ns=0) == 0
    refused(call(h), ARG, who + "null argument")


def test_draws_noisy_dev_refusals_in_order(handles):
    lib = _lib.load()
    X, P = dev_rows(), torch.full((8, D), 0.01, dtype=torch.float64, device=DEV)
    who = "gpz_predictor_draws_noisy_dev: "

    def call(h, ndraws=3, x_type=0, psi=P.data_ptr(), psi_type=0, psi_rs=D, ns=8):
        return lib.gpz_predictor_draws_noisy_dev(h, X.data_ptr(), x_type, ns, D, 1, psi, psi_type, psi_rs, 1, None, None, None, None,
                                                 ndraws, 0, None, None, None)

    refused(call(handles["VC"][1], ndraws=0), ARG, who + "need 1 <= ndraws and ndraws * k <= 16384 (ndraws 0, k 2)")
    refused(call(handles["VC"][1], x_type=7), UNSUPPORTED, who + NOT_FITS)
    refused(call(handles["VDt"][1], x_type=7), UNSUPPORTED, who + FORCED)
    refused(call(handles["VDt"][1], ndraws=0, ns=-1), ARG, who + "ns < 0")
    h = handles["VD"][1]
    refused(call(h, x_type=7, psi=None), ARG, who + "x_type 7 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused(call(h, psi=None, psi_type=9), ARG, who + "psi_type 9 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused(call(h, psi=None), ARG, who + "null Psi")
    refused(call(h, psi_rs=0), ARG, who + "Psi strides (0, 1) of 8 rows: the row stride must be positive")
    assert call(h, ns=0) == 0
    refused(call(h), ARG, who + "null argument")


def test_stack_dev_refusals_in_order(handles):
    lib = _lib.load()
    _, h = handles["VD"]
    X = dev_rows()
    who = "gpz_predictor_stack_dev: "
    inf_shift = np.array([np.nan, 0.0])

    def call(x=X.data_ptr(), x_type=0, ns=8, ndraws=0, edges=(0.0, 1.0, 2.0), nbins=2, ngroups=2, shift=None, hist=True):
        e = np.ascontiguousarray(np.tile(np.asarray(edges, dtype=np.float64), (K, 1)))
        o = [np.full(4 * K * 2, 7.0), np.full(2, 7.0), np.full(2 * K, 7.0), np.full(2 * K, 7.0)]
        rc = lib.gpz_predictor_stack_dev(h, x, x_type, ns, D, 1, None, None, ndraws, 0, None, _lib.dptr(e), nbins, None, ngroups, None,
                                         _lib.dptr(o[0]) if hist else None, _lib.dptr(o[1]), _lib.dptr(o[2]), _lib.dptr(o[3]),
                                         _lib.dptr(shift), None)
        return rc, o

    refused(call(x_type=7, ns=-1, nbins=0)[0], ARG, who + "ns < 0")
    refused(call(x_type=7, ndraws=-1, nbins=0)[0], ARG, who + "need 0 <= ndraws and (1 + ndraws) * k <= 16384 (ndraws -1, k 2)")
    refused(call(x_type=7, nbins=0, edges=(0.0, 1.0, 1.0))[0], ARG, who + "need nbins >= 1 and ngroups >= 1")
    refused(call(x_type=7, hist=False)[0], ARG, who + "null argument")
    refused(call(x_type=7, edges=(0.0, np.inf, 2.0))[0], ARG, who + "the edges must be finite and strictly increasing (output 0, edge 1)")
    refused(call(x=None, x_type=7)[0], ARG, who + "null argument")
    refused(call(x_type=7, shift=inf_shift)[0], ARG, who + "x_type 7 is neither GPZ_X_F64 nor GPZ_X_F32")
    rc, o = call(ns=0, shift=inf_shift)
    refused(rc, ARG, who + "mu_shift must be finite")
    assert all(np.all(a == 7.0) for a in o)                               # refused: the outputs are untouched
    rc, o = call(x=None, ns=0)
    assert rc == 0 and all(np.all(a[:n] == 0.0) for a, n in zip(o, (2 * K * 2, 2, 2 * K, 2 * K)))


# ---- the entries for rows with input noise and with missing inputs ------------------------------------------------------------------------
MISS_FITS = ("missing inputs on the handle need predict_missing_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, k <= 8 and "
             "ceil16(m) <= 256 (method VC, d 5, m 50, k 2); gpz_predict_missing takes every shape")
FULL_MASK = "no dimension is missing in the mask (complete rows go to gpz_predictor_run_dev / _draws_dev)"
PATTERN = "the rows of a group must share one NaN pattern, the one of the mask"
BAD_PSI = "Psi has an element that is NaN, infinite or negative"
BAD_LAB = np.array([0, 1, -1, 7, 0, 1, 9, 0], dtype=np.int32)
BAD_WT = np.array([1, 1, 1, 1, 1, -2.0, 1, 1], dtype=np.float64)
OBS = 0x0f                                                                # dimension 4 is missing


def sevens(*shape):
    return torch.full(shape, 7.0, dtype=torch.float64, device=DEV)


def refused_whole(got, code, text):
    """refused, and the outputs of the call hold the 7.0 they were filled with."""
    rc, o = got
    refused(rc, code, text)
    assert all(bool((a == 7.0).all()) for a in o)


def stack_sevens(ndraws, nbins, ngroups):
    C_, B, G = 1 + max(ndraws, 0), max(nbins, 1), max(ngroups, 1)
    return [np.full(C_ * G * K * B, 7.0), np.full(G, 7.0), np.full(C_ * G * K, 7.0), np.full(C_ * G * K, 7.0)]


def stack_tail(edges, nbins, group, ngroups, weight, o, shift, hist, ptr):
    """edges .. mu_shift of a stack entry; ptr: what turns group and weight into the argument."""
    e = np.ascontiguousarray(np.tile(np.asarray(edges, dtype=np.float64), (K, 1)))
    return (_lib.dptr(e), nbins, ptr(group), ngroups, ptr(weight), _lib.dptr(o[0]) if hist else None, _lib.dptr(o[1]), _lib.dptr(o[2]),
            _lib.dptr(o[3]), _lib.dptr(shift))


def bad_rows():
    """Rows with one NaN, and a Psi with one negative element (both normalised, column-major)."""
    Xn, Pn = host_rows(), np.asfortranarray(np.full((8, D), 0.01))
    Xn[6, 2] = np.nan
    Pn[1, 4] = -0.5
    return Xn, Pn


def missing_rows():
    """Eight rows of the pattern OBS; the same with a second NaN in row 3."""
    Xm = np.ascontiguousarray(host_rows())
    Xm[:, 4] = np.nan
    Xw = Xm.copy()
    Xw[3, 1] = np.nan
    return torch.from_numpy(Xm).to(DEV), torch.from_numpy(Xw).to(DEV)


def test_stack_zeroes_its_outputs_before_it_runs(handles):
    """gpz_predictor_stack alone clears its outputs once its arguments have passed: a refusal of the rows leaves zeros, an earlier one 7.0."""
    lib = _lib.load()
    _, h = handles["VD"]
    Xn, _ = bad_rows()
    e = np.ascontiguousarray(np.tile(np.array([0.0, 1.0, 2.0]), (K, 1)))

    def call(weight=None):
        o = stack_sevens(0, 2, 2)
        ptr = [_lib.dptr(a) for a in o]
        rc = lib.gpz_predictor_stack(h, _lib.dptr(Xn), 8, 0, 0, None, _lib.dptr(e), 2, None, 2, _lib.dptr(weight), *ptr, None)
        return rc, o

    refused_whole(call(weight=BAD_WT), ARG, "gpz_predictor_stack: the weight of row 5 is negative or not finite")
    rc, o = call()
    refused(rc, UNSUPPORTED, "gpz_predictor_stack: the rows have missing values (NaN): stacks are for complete rows")
    assert all(np.all(a == 0.0) for a in o)


def test_stack_noisy_refusals_in_order(handles):
    lib = _lib.load()
    X, P = host_rows(), np.asfortranarray(np.full((8, D), 0.01))
    Xn, Pn = bad_rows()
    inf_shift = np.array([0.0, np.inf])
    who = "gpz_predictor_stack_noisy: "
    vd, vdt, vc = (handles[n][1] for n in ("VD", "VDt", "VC"))

    def call(h, x=X, psi=P, ns=8, ndraws=0, edges=(0.0, 1.0, 2.0), nbins=2, group=None, ngroups=2, weight=None, shift=None, hist=True):
        o = stack_sevens(ndraws, nbins, ngroups)
        lab = lambda a: None if a is None else (a.ctypes.data_as(_lib.c_int32_p) if a.dtype == np.int32 else _lib.dptr(a))
        return lib.gpz_predictor_stack_noisy(h, _lib.dptr(x), ns, _lib.dptr(psi), ndraws, 0, None,
                                             *stack_tail(edges, nbins, group, ngroups, weight, o, shift, hist, lab)), o

    refused_whole(call(None, ns=-1, ndraws=-1), ARG, who + "null handle")
    refused_whole(call(vc, ns=-1, ndraws=-1), ARG, who + "ns < 0")
    refused_whole(call(vc, ndraws=-1, nbins=0), ARG, who + "need 0 <= ndraws and (1 + ndraws) * k <= 16384 (ndraws -1, k 2)")
    refused_whole(call(vc, nbins=0, edges=(0.0, 1.0, 1.0)), ARG, who + "need nbins >= 1 and ngroups >= 1")
    refused_whole(call(vc, nbins=41, ngroups=100, edges=np.arange(42.0), hist=False), ARG,
                  who + "ngroups * nbins = 4100 is over GPZ_STACK_MAX_GROUP_BINS = 4096")
    refused_whole(call(vc, edges=(0.0, 1.0, 1.0), hist=False), ARG, who + "null argument")
    refused_whole(call(vc, x=None, edges=(0.0, 1.0, 1.0)), ARG, who + "the edges must be finite and strictly increasing (output 0, edge 2)")
    refused_whole(call(vc, x=None), ARG, who + "null argument")
    refused_whole(call(vc, psi=None), UNSUPPORTED, who + NOT_FITS)
    refused_whole(call(vdt, psi=None), UNSUPPORTED, who + FORCED)
    refused_whole(call(vdt, x=None, psi=None, ns=0), UNSUPPORTED, who + FORCED)
    refused_whole(call(vd, psi=None, group=BAD_LAB), ARG, who + "null Psi")
    refused_whole(call(vd, group=BAD_LAB, weight=BAD_WT, shift=inf_shift), ARG, who + "label 7 of row 3 is outside [-1, 2)")
    refused_whole(call(vd, weight=BAD_WT, shift=inf_shift), ARG, who + "mu_shift must be finite")
    refused_whole(call(vd, x=Xn, weight=BAD_WT), ARG, who + "the weight of row 5 is negative or not finite")
    rc, o = call(vd, x=None, psi=None, ns=0)
    assert rc == 0 and all(np.all(a == 0.0) for a in o)                   # no rows: zeros
    refused_whole(call(vd, x=Xn, psi=Pn), UNSUPPORTED, who + "the rows have missing values (NaN): stacks are for complete rows")
    refused_whole(call(vd, psi=Pn), ARG, who + BAD_PSI)


def test_stack_noisy_dev_refusals_in_order(handles):
    lib = _lib.load()
    X, P = dev_rows(), torch.full((8, D), 0.01, dtype=torch.float64, device=DEV)
    Xn, Pn = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in bad_rows())
    lab, wt = torch.from_numpy(BAD_LAB).to(DEV), torch.from_numpy(BAD_WT).to(DEV)
    v, nan_shift = np.ones(D), np.array([np.nan, 0.0])
    who = "gpz_predictor_stack_noisy_dev: "
    vd, vdt, vc = (handles[n][1] for n in ("VD", "VDt", "VC"))

    def call(h, x=X.data_ptr(), x_type=0, ns=8, rs=D, psi=P.data_ptr(), psi_type=0, psi_rs=D, mu=None, sd=None, sd2=None, ndraws=0,
             edges=(0.0, 1.0, 2.0), nbins=2, group=None, ngroups=2, weight=None, shift=None, hist=True):
        o = stack_sevens(ndraws, nbins, ngroups)
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib.gpz_predictor_stack_noisy_dev(h, x, x_type, ns, rs, 1, psi, psi_type, psi_rs, 1, _lib.dptr(mu), _lib.dptr(sd),
                                                 _lib.dptr(sd2), ndraws, 0, None,
                                                 *stack_tail(edges, nbins, group, ngroups, weight, o, shift, hist, ptr), None), o

    refused_whole(call(None, ns=-1, ndraws=-1), ARG, who + "null handle")
    refused_whole(call(vc, ns=-1, ndraws=-1), ARG, who + "ns < 0")
    refused_whole(call(vc, ndraws=-1, nbins=0), ARG, who + "need 0 <= ndraws and (1 + ndraws) * k <= 16384 (ndraws -1, k 2)")
    refused_whole(call(vc, nbins=0, hist=False), ARG, who + "need nbins >= 1 and ngroups >= 1")
    refused_whole(call(vc, hist=False, edges=(0.0, np.inf, 2.0)), ARG, who + "null argument")
    refused_whole(call(vc, x=None, edges=(0.0, np.inf, 2.0)), ARG,
                  who + "the edges must be finite and strictly increasing (output 0, edge 1)")
    refused_whole(call(vc, x=None), ARG, who + "null argument")
    refused_whole(call(vc, x_type=7), UNSUPPORTED, who + NOT_FITS)
    refused_whole(call(vdt, x_type=7), UNSUPPORTED, who + FORCED)
    refused_whole(call(vd, x_type=7, psi_type=9), ARG, who + "x_type 7 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused_whole(call(vd, mu=v, psi_type=9), ARG, who + "muX and sdX go together (both or neither)")
    refused_whole(call(vd, rs=0, psi_type=9), ARG, who + "strides (0, 1) of 8 rows: a stride must be positive")
    refused_whole(call(vd, psi_type=9, mu=v, sd=v), ARG, who + "psi_type 9 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused_whole(call(vd, psi=None, mu=v, sd=v), ARG, who + "sdX and sd2 go together (both or neither)")
    refused_whole(call(vd, psi=None, psi_rs=0), ARG, who + "null Psi")
    refused_whole(call(vd, psi_rs=0, shift=nan_shift), ARG, who + "Psi strides (0, 1) of 8 rows: the row stride must be positive")
    refused_whole(call(vd, shift=nan_shift, group=lab), ARG, who + "mu_shift must be finite")
    refused_whole(call(vd, ns=0, shift=nan_shift), ARG, who + "mu_shift must be finite")
    rc, o = call(vd, x=None, psi=None, ns=0)
    assert rc == 0 and all(np.all(a == 0.0) for a in o)                   # no rows: zeros
    # the scan of the rows, Psi, labels and weights
    refused_whole(call(vd, group=lab, weight=wt), ARG, who + "a label is outside [-1, 2)")
    refused_whole(call(vd, x=Xn.data_ptr(), weight=wt), ARG, who + "a weight is negative or not finite")
    refused_whole(call(vd, x=Xn.data_ptr(), psi=Pn.data_ptr()), UNSUPPORTED,
                  who + "the rows have missing values (NaN): stacks are for complete rows")
    refused_whole(call(vd, psi=Pn.data_ptr()), ARG, who + BAD_PSI)


def test_draws_gamma_noisy_dev_refusals_in_order(handles):
    lib = _lib.load()
    X, P = dev_rows(), torch.full((8, D), 0.01, dtype=torch.float64, device=DEV)
    Xn, Pn = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in bad_rows())
    v = np.ones(D)
    who = "gpz_predictor_draws_gamma_noisy_dev: "
    vd, vdt, vc = (handles[n][1] for n in ("VD", "VDt", "VC"))

    def call(h, ndraws=3, x=X.data_ptr(), x_type=0, psi=P.data_ptr(), psi_type=0, psi_rs=D, sdX=None, ns=8, F=True, Gam=True):
        o = [sevens(3, 8, K), sevens(3, 8, K)]
        return lib.gpz_predictor_draws_gamma_noisy_dev(h, x, x_type, ns, D, 1, psi, psi_type, psi_rs, 1, _lib.dptr(sdX), _lib.dptr(sdX), None,
                                                       None, ndraws, 0, None, o[0].data_ptr() if F else None,
                                                       o[1].data_ptr() if Gam else None, None), o

    refused_whole(call(None, ndraws=0, ns=-1), ARG, who + "null handle")
    refused_whole(call(vc, ndraws=0, ns=-1), ARG, who + "ns < 0")
    refused_whole(call(vc, ndraws=0), ARG, who + "need 1 <= ndraws and ndraws * k <= 16384 (ndraws 0, k 2)")
    refused_whole(call(vc, x_type=7), UNSUPPORTED, who + NOT_FITS)
    refused_whole(call(vdt, x_type=7), UNSUPPORTED, who + FORCED)
    refused_whole(call(vd, x_type=7, psi=None), ARG, who + "x_type 7 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused_whole(call(vd, psi=None, psi_type=9), ARG, who + "psi_type 9 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused_whole(call(vd, psi=None, sdX=v), ARG, who + "sdX and sd2 go together (both or neither)")
    refused_whole(call(vd, psi=None, psi_rs=0), ARG, who + "null Psi")
    refused_whole(call(vd, psi_rs=0, Gam=False), ARG, who + "Psi strides (0, 1) of 8 rows: the row stride must be positive")
    assert call(vd, ns=0, F=False, Gam=False)[0] == 0
    refused_whole(call(vd, x=Xn.data_ptr(), Gam=False), ARG, who + "null argument")
    refused_whole(call(vd, x=Xn.data_ptr(), F=False), ARG, who + "null argument")
    refused_whole(call(vd, x=Xn.data_ptr(), psi=Pn.data_ptr()), UNSUPPORTED,
                  who + "the rows have missing values (NaN): draws are for complete rows")
    refused_whole(call(vd, psi=Pn.data_ptr()), ARG, who + BAD_PSI)


def missing_ladder(handles, who, call, outputs_needed):
    """The refusals that gpz_predictor_run_missing_dev, _draws_missing_dev and _draws_gamma_missing_dev share behind their own first
    ones: the model, the mask, the rows' layout, the outputs, then the scan.  call(h, **what is wrong) -> (rc, outputs)."""
    vd, vc = handles["VD"][1], handles["VC"][1]
    Xm, Xw = missing_rows()
    v = np.ones(D)
    refused_whole(call(vc, obs=0x2f), UNSUPPORTED, who + MISS_FITS)
    refused_whole(call(vd, obs=0x2f, x_type=7), ARG, who + "the mask 0x2f has a bit at or above d = 5")
    refused_whole(call(vd, obs=0x1f, x_type=7), ARG, who + FULL_MASK)
    refused_whole(call(vd, x_type=7, mu=v), ARG, who + "x_type 7 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused_whole(call(vd, mu=v, x=None), ARG, who + "muX and sdX go together (both or neither)")
    refused_whole(call(vd, x=None, rs=0), ARG, who + "null argument")
    refused_whole(call(vd, x=Xw.data_ptr(), rs=0), ARG, who + "strides (0, 1) of 8 rows: a stride must be positive")
    assert call(vd, x=None, ns=0, out=False)[0] == 0
    for drop in outputs_needed:
        refused_whole(call(vd, x=Xw.data_ptr(), out=drop), ARG, who + "null argument")
    refused_whole(call(vd, x=Xw.data_ptr()), ARG, who + PATTERN)            # a row with a second NaN
    refused_whole(call(vd, x=dev_rows().data_ptr()), ARG, who + PATTERN)    # complete rows under a mask with a missing dimension
    rc, o = call(vd, x=Xm.data_ptr())
    assert rc == 0 and not bool((o[0] == 7.0).any())                      # the group itself is taken


def test_run_missing_dev_refusals_in_order(handles):
    lib = _lib.load()
    who = "gpz_predictor_run_missing_dev: "

    def call(h, x=None, x_type=0, ns=8, rs=D, mu=None, obs=OBS, out=True):
        o = [sevens(K, 8) for _ in range(5)]
        ptr = [None] * 5 if out is False else [None if i == out and out is not True else t.data_ptr() for i, t in enumerate(o)]
        return lib.gpz_predictor_run_missing_dev(h, x, x_type, ns, rs, 1, _lib.dptr(mu), None, None, None, obs, *ptr, None), o

    refused_whole(call(None, ns=-1, obs=0x2f), ARG, who + "null handle")
    refused_whole(call(handles["VC"][1], ns=-1, obs=0x2f), ARG, who + "ns < 0")
    missing_ladder(handles, who, call, outputs_needed=(0, 2, 3))          # mu, nu, beta; sigma and gamma may be left out


def test_draws_missing_dev_refusals_in_order(handles):
    lib = _lib.load()
    who = "gpz_predictor_draws_missing_dev: "

    def call(h, x=None, x_type=0, ns=8, rs=D, mu=None, obs=OBS, ndraws=3, out=True):
        o = [sevens(3, 8, K)]
        return lib.gpz_predictor_draws_missing_dev(h, x, x_type, ns, rs, 1, _lib.dptr(mu), None, None, None, obs, ndraws, 0, None,
                                                   o[0].data_ptr() if out is True else None, None), o

    refused_whole(call(None, ns=-1, ndraws=0), ARG, who + "null handle")
    refused_whole(call(handles["VC"][1], ns=-1, ndraws=0), ARG, who + "ns < 0")
    refused_whole(call(handles["VC"][1], ndraws=0, obs=0x2f), ARG, who + "need 1 <= ndraws and ndraws * k <= 16384 (ndraws 0, k 2)")
    missing_ladder(handles, who, call, outputs_needed=(0,))


def test_draws_gamma_missing_dev_refusals_in_order(handles):
    lib = _lib.load()
    who = "gpz_predictor_draws_gamma_missing_dev: "

    def call(h, x=None, x_type=0, ns=8, rs=D, mu=None, obs=OBS, ndraws=3, out=True):
        o = [sevens(3, 8, K), sevens(3, 8, K)]
        ptr = [None, None] if out is False else [None if i == out and out is not True else t.data_ptr() for i, t in enumerate(o)]
        return lib.gpz_predictor_draws_gamma_missing_dev(h, x, x_type, ns, rs, 1, _lib.dptr(mu), None, None, None, obs, ndraws, 0, None,
                                                         *ptr, None), o

    refused_whole(call(None, ns=-1, ndraws=0), ARG, who + "null handle")
    refused_whole(call(handles["VC"][1], ns=-1, ndraws=0), ARG, who + "ns < 0")
    refused_whole(call(handles["VC"][1], ndraws=0, obs=0x2f), ARG, who + "need 1 <= ndraws and ndraws * k <= 16384 (ndraws 0, k 2)")
    missing_ladder(handles, who, call, outputs_needed=(0, 1))


def test_stack_missing_dev_refusals_in_order(handles):
    lib = _lib.load()
    Xm, Xw = missing_rows()
    lab, wt = torch.from_numpy(BAD_LAB).to(DEV), torch.from_numpy(BAD_WT).to(DEV)
    v, nan_shift = np.ones(D), np.array([np.nan, 0.0])
    who = "gpz_predictor_stack_missing_dev: "
    vd, vc = handles["VD"][1], handles["VC"][1]

    def call(h, x=Xm.data_ptr(), x_type=0, ns=8, rs=D, mu=None, obs=OBS, ndraws=0, edges=(0.0, 1.0, 2.0), nbins=2, group=None, ngroups=2,
             weight=None, shift=None, hist=True):
        o = stack_sevens(ndraws, nbins, ngroups)
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib.gpz_predictor_stack_missing_dev(h, x, x_type, ns, rs, 1, _lib.dptr(mu), None, None, obs, ndraws, 0, None,
                                                   *stack_tail(edges, nbins, group, ngroups, weight, o, shift, hist, ptr), None), o

    refused_whole(call(None, ns=-1, ndraws=-1), ARG, who + "null handle")
    refused_whole(call(vc, ns=-1, ndraws=-1), ARG, who + "ns < 0")
    refused_whole(call(vc, ndraws=-1, nbins=0), ARG, who + "need 0 <= ndraws and (1 + ndraws) * k <= 16384 (ndraws -1, k 2)")
    refused_whole(call(vc, nbins=0, hist=False), ARG, who + "need nbins >= 1 and ngroups >= 1")
    refused_whole(call(vc, hist=False, edges=(0.0, np.inf, 2.0)), ARG, who + "null argument")
    refused_whole(call(vc, x=None, edges=(0.0, np.inf, 2.0)), ARG,
                  who + "the edges must be finite and strictly increasing (output 0, edge 1)")
    refused_whole(call(vc, x=None, obs=0x2f), ARG, who + "null argument")
    refused_whole(call(vc, obs=0x2f), UNSUPPORTED, who + MISS_FITS)
    refused_whole(call(vd, obs=0x2f, x_type=7), ARG, who + "the mask 0x2f has a bit at or above d = 5")
    refused_whole(call(vd, obs=0x1f, x_type=7), ARG, who + FULL_MASK)
    refused_whole(call(vd, x_type=7, mu=v), ARG, who + "x_type 7 is neither GPZ_X_F64 nor GPZ_X_F32")
    refused_whole(call(vd, mu=v, rs=0), ARG, who + "muX and sdX go together (both or neither)")
    refused_whole(call(vd, rs=0, shift=nan_shift), ARG, who + "strides (0, 1) of 8 rows: a stride must be positive")
    refused_whole(call(vd, shift=nan_shift, group=lab), ARG, who + "mu_shift must be finite")
    refused_whole(call(vd, ns=0, shift=nan_shift), ARG, who + "mu_shift must be finite")
    rc, o = call(vd, x=None, ns=0)
    assert rc == 0 and all(np.all(a == 0.0) for a in o)                   # no rows: zeros
    # the scan of the rows, labels and weights
    refused_whole(call(vd, group=lab, weight=wt), ARG, who + "a label is outside [-1, 2)")
    refused_whole(call(vd, x=Xw.data_ptr(), weight=wt), ARG, who + "a weight is negative or not finite")
    refused_whole(call(vd, x=Xw.data_ptr()), ARG, who + PATTERN)          # a row with a second NaN
    refused_whole(call(vd, x=dev_rows().data_ptr()), ARG, who + PATTERN)  # complete rows under a mask with a missing dimension


# ---- the Python methods -------------------------------------------------------------------------------------------------------------------
def raises(kind, text):
    return pytest.raises(kind, match="^" + re.escape(text))


def test_python_methods_refuse_in_order(handles):
    p, pt, pc = handles["VD"][0], handles["VDt"][0], handles["VC"][0]
    X = catalogue(p.model, 8, seed=2)
    Xn = X.copy()
    Xn[3, 0] = np.nan
    Psi, bad_psi = np.full((8, D), 0.01), np.full((8, D), -1.0)
    T = torch.from_numpy(X)                                               # a host tensor: everything below is refused before the device check
    # draws: shape, NaN rows, the Psi model, Psi values, n_draws, seed, Z
    with raises(ValueError, "X must be n x 5, got shape (8, 4)"):
        p.draws(Xn[:, :4], 0)
    with raises(ValueError, "X has 1 rows with missing values (NaN): draws are for complete rows"):
        p.draws(Xn, 0, Psi=bad_psi)
    with raises(ValueError, "draws with Psi needs a model inside predict_noisy_fits"):
        pc.draws(X, 0, Psi=bad_psi)
    with raises(ValueError, "draws with Psi needs the fused draws route: the predictor was made with force_tiles=True"):
        pt.draws(X, 0, Psi=bad_psi)
    with raises(ValueError, "Psi must be finite and >= 0"):
        p.draws(X, 0, Psi=bad_psi)
    with raises(ValueError, "n_draws must be a positive integer, got 0"):
        p.draws(X, 0, seed=-1, Psi=Psi)
    with raises(ValueError, "n_draws * k = 16386 is over the limit of 16384 per call"):
        p.draws(X, 8193, seed=-1)
    with raises(ValueError, "seed must be an integer in [0, 2^64), got -1"):
        p.draws(X, 3, seed=-1, Z=np.zeros(4))
    with raises(ValueError, "Z must have shape (50, 3, 2), got (4,)"):
        p.draws(X, 3, Z=np.zeros(4))
    # stack: NaN rows, edges, n_draws, seed, Z, groups, n_groups, weights, the size of the histogram
    with raises(ValueError, "X has 1 rows with missing values (NaN): stacks are for complete rows"):
        p.stack(Xn, [0.0])
    with raises(ValueError, "edges must be a vector of at least 2 values, got shape (1,)"):
        p.stack(X, [0.0], n_draws=-1)
    with raises(ValueError, "edges must be finite and strictly increasing"):
        p.stack(X, [0.0, 1.0, 1.0], n_draws=-1)
    with raises(ValueError, "n_draws must be a non-negative integer, got -1"):
        p.stack(X, [0.0, 1.0], n_draws=-1, seed=-1)
    with raises(ValueError, "(1 + n_draws) * k = 16386 is over the limit of 16384 per call"):
        p.stack(X, [0.0, 1.0], n_draws=8192, seed=-1)
    with raises(ValueError, "seed must be an integer in [0, 2^64), got -1"):
        p.stack(X, [0.0, 1.0], seed=-1, Z=np.zeros(4))
    with raises(ValueError, "Z must be None when n_draws is 0"):
        p.stack(X, [0.0, 1.0], Z=np.zeros(4), groups=np.zeros(3, dtype=int))
    with raises(ValueError, "groups must be 8 integer labels"):
        p.stack(X, [0.0, 1.0], groups=np.zeros(3, dtype=int), weights=np.zeros(3))
    with raises(ValueError, "groups must be labels in [-1, n_groups)"):
        p.stack(X, [0.0, 1.0], groups=np.full(8, -2), n_groups=0)
    with raises(ValueError, "n_groups must be a positive integer, got 0"):
        p.stack(X, [0.0, 1.0], groups=np.zeros(8, dtype=int), n_groups=0, weights=np.zeros(3))
    with raises(ValueError, "groups must be labels in [-1, n_groups) with n_groups = 2, got 5"):
        p.stack(X, [0.0, 1.0], groups=np.full(8, 5), n_groups=2, weights=np.zeros(3))
    with raises(ValueError, "weights must be 8 values"):
        p.stack(X, np.arange(4098.0), weights=np.zeros(3))
    with raises(ValueError, "weights must be finite and >= 0"):
        p.stack(X, np.arange(4098.0), weights=np.full(8, -1.0))
    with raises(ValueError, "n_groups * bins = 4097 is over the limit of 4096 per call"):
        p.stack(X, np.arange(4098.0), weights=np.ones(8))
    # the device methods: the type of X, its shape, the mask, then the method's own arguments, the device last
    with raises(TypeError, "predict_dev takes a torch tensor on cuda:0; a NumPy array goes to Predictor.predict"):
        p.predict_dev(X, Psi=Psi)
    with raises(TypeError, "predict_dev takes Psi as a torch tensor on cuda:0; a NumPy array goes to Predictor.predict"):
        p.predict_dev(T, Psi=Psi, return_phi=True)
    with raises(ValueError, "return_phi=True is not available with Psi on the device"):
        pc.predict_dev(T, Psi=torch.from_numpy(Psi), return_phi=True)
    with raises(ValueError, "predict_dev with Psi needs a model inside predict_noisy_fits"):
        pc.predict_dev(T, Psi=torch.from_numpy(Psi))
    with raises(ValueError, "X must be on cuda:0, it is on cpu: the host methods take host arrays"):
        p.predict_dev(T, Psi=torch.from_numpy(Psi))
    with raises(TypeError, "draws_dev takes a torch tensor on cuda:0; a NumPy array goes to Predictor.draws"):
        p.draws_dev(X, 0)
    with raises(ValueError, "n_draws must be a positive integer, got 0"):
        pc.draws_dev(T, 0, Psi=Psi)
    with raises(TypeError, "draws_dev takes Psi as a torch tensor on cuda:0; a NumPy array goes to Predictor.draws"):
        pc.draws_dev(T, 3, Psi=Psi)
    with raises(ValueError, "draws_dev with Psi needs a model inside predict_noisy_fits"):
        pc.draws_dev(T, 3, Psi=torch.from_numpy(Psi))
    with raises(ValueError, "draws_dev with Psi needs the fused draws route: the predictor was made with force_tiles=True"):
        pt.draws_dev(T, 3, Psi=torch.from_numpy(Psi))
    with raises(ValueError, "X must be on cuda:0, it is on cpu: the host methods take host arrays"):
        p.draws_dev(T, 3, Psi=torch.from_numpy(Psi))
    with raises(TypeError, "selection must be a bool torch tensor on the same device as X"):
        p.stack_dev(T, [0.0], selection=np.ones(8, dtype=bool))
    with raises(ValueError, "edges must be a vector of at least 2 values, got shape (1,)"):
        p.stack_dev(T, [0.0], n_draws=-1)
    with raises(ValueError, "edges must be finite and strictly increasing"):
        p.stack_dev(T, [0.0, np.nan], n_draws=-1)
    with raises(ValueError, "n_draws must be a non-negative integer, got -1"):
        p.stack_dev(T, [0.0, 1.0], n_draws=-1, groups=np.zeros(8, dtype=int))
    with raises(ValueError, "groups must be a tensor of 8 integer labels"):
        p.stack_dev(T, [0.0, 1.0], groups=np.zeros(8, dtype=int), weights=np.ones(8))
    with raises(ValueError, "weights must be a float tensor of 8 values"):
        p.stack_dev(T, [0.0, 1.0], weights=np.ones(8), n_groups=0)
    with raises(ValueError, "n_groups must be a positive integer, got 0"):
        p.stack_dev(T, np.arange(4098.0), n_groups=0)
    with raises(ValueError, "n_groups * bins = 8194 is over the limit of 4096 per call"):
        p.stack_dev(T, np.arange(4098.0), n_groups=2)
    with raises(ValueError, "X must be on cuda:0, it is on cpu: the host methods take host arrays"):
        p.stack_dev(T, [0.0, 1.0])
    # a closed predictor says so before it looks at anything else
    q = gpz_amd.Predictor(p.model, tile_rows=1024)
    q.close()
    for call in (lambda: q.predict(Xn[:, :4]), lambda: q.draws(Xn, 0), lambda: q.stack(Xn, [0.0]), lambda: q.predict_dev(X),
                 lambda: q.draws_dev(X, 0), lambda: q.stack_dev(X, [0.0])):
        with raises(RuntimeError, "Predictor is closed"):
            call()


# ---- a refusal with two tiles in flight ---------------------------------------------------------------------------------------------------
NS, BAD_ROW = 3 * 1024 + 5, 2100                                          # four tiles; the bad row is in tile 2


def clean_calls(p, X, Psi, edges, with_psi):
    """predict, draws, stack [, draws with Psi] on clean rows: the arrays of each call and the device bytes held after it."""
    got = []
    calls = [lambda: p.predict(X), lambda: (p.draws(X, 3, seed=4),), lambda: tuple(p.stack(X, edges, n_draws=3, seed=4))]
    if with_psi:
        calls.append(lambda: (p.draws(X, 3, seed=4, Psi=Psi),))
    for call in calls:
        got.append((call(), p.info[1]))
    return got


@pytest.mark.parametrize("method", ["VD", "VC"])
@pytest.mark.parametrize("force_tiles", [False, True])
def test_late_tile_refusal_leaves_the_handle_whole(method, force_tiles):
    """A NaN (through gpz_predictor_run, _draws and _stack with 3 draws) or a negative Psi element (through _draws_noisy, fused route of
    a diagonal kind) at row 2100 of 3 * 1024 + 5, when tiles 0 and 1 are in flight: the documented refusal; then the same handle on the
    clean rows returns the arrays of a fresh handle bit for bit and holds the same device bytes after the same calls."""
    lib = _lib.load()
    with_psi = method == "VD" and not force_tiles
    model = synth_model(method, M, D, K, True, seed=17)
    X = catalogue(model, NS, seed=18)
    Psi = np.random.default_rng(19).gamma(1.0, 0.05, (NS, D))
    edges = np.linspace(-4.0, 4.0, 9)
    with gpz_amd.Predictor(model, tile_rows=1024, force_tiles=force_tiles) as fresh:
        want = clean_calls(fresh, X, Psi, edges, with_psi)
    Xn = np.asfortranarray((X - model.muX) / model.sdX)
    Xbad = Xn.copy(order="F")
    Xbad[BAD_ROW, 2] = np.nan
    Pn = np.asfortranarray(Psi / model.sdX ** 2)
    Pbad = Pn.copy(order="F")
    Pbad[BAD_ROW, 1] = -1e-3
    o = outs(NS)
    F = np.empty((NS, K, 3), order="F")
    nan_rows = "the rows have missing values (NaN): "
    with gpz_amd.Predictor(model, tile_rows=1024, force_tiles=force_tiles) as p:
        h = p._handle()
        assert p.info[2] == int(force_tiles)
        refusals = [
            (lambda: lib.gpz_predictor_run(h, _lib.dptr(Xbad), NS, None, 0, *(_lib.dptr(a) for a in o), None), UNSUPPORTED,
             "gpz_predictor_run: " + nan_rows + "group them by pattern and call gpz_predict_missing (predict.m:45-69)"),
            (lambda: lib.gpz_predictor_draws(h, _lib.dptr(Xbad), NS, 3, 4, None, _lib.dptr(F)), UNSUPPORTED,
             "gpz_predictor_draws: " + nan_rows + "draws are for complete rows"),
            (lambda: stack_call(lib, h, Xbad, NS, ndraws=3, edges=edges, nbins=8, ngroups=1), UNSUPPORTED,
             "gpz_predictor_stack: " + nan_rows + "stacks are for complete rows"),
            (lambda: lib.gpz_predictor_draws_noisy(h, _lib.dptr(Xn), NS, _lib.dptr(Pbad), 3, 4, None, _lib.dptr(F)), ARG,
             "gpz_predictor_draws_noisy: Psi has an element that is NaN, infinite or negative"),
        ]
        calls = [lambda: p.predict(X), lambda: (p.draws(X, 3, seed=4),), lambda: tuple(p.stack(X, edges, n_draws=3, seed=4)),
                 lambda: (p.draws(X, 3, seed=4, Psi=Psi),)]
        for (refuse, code, text), call, (arrays, held) in zip(refusals, calls, want):
            refused(refuse(), code, text)
            got = call()
            assert len(got) == len(arrays) and all(np.array_equal(a, b) for a, b in zip(got, arrays))
            assert p.info[1] == held
