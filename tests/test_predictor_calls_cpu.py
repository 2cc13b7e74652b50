"""The calls the Predictor's Python methods make on the library, without a GPU and without the built library: a recording stand-in behind
``_lib.load`` notes, per gpz_predictor_* (and gpz_predict_missing) call, the entry's name and its scalar arguments, and checks every call
against the binding (argument count and ctypes types), the handle, the stream and the values behind the muX / sdX / sd2 / muY / priors
pointers, at the positions include/gpz_hip.h gives them.  The expected sequences are literals: which entry each method and keyword
combination reaches, with how many rows and which mask of observed dimensions, the NaN-pattern groups in ascending order of their code on
the device and in first-occurrence order on the host.  Below them the Python refusal order of the methods added since
test_predictor_refusals.py::test_python_methods_refuse_in_order was written, two things wrong at once."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib

D, M = 3, 6
HANDLE, STREAM = 0x5EED, 77
MUX, SDX = np.array([1.0, 2.0, 3.0]), np.array([2.0, 4.0, 8.0])
MUY = {1: np.array([0.5]), 2: np.array([0.5, -0.25])}
PRIORS = np.arange(1.0, M + 1) / 21
# bit c of a row's code: dimension c is missing.  0 complete, 4 the last dimension missing, 6 only dimension 0 observed, 7 nothing observed
CODES = [4, 0, 7, 6, 0, 4, 0, 6, 4, 7]
N = len(CODES)
SEL = np.arange(N) >= 4                                                   # drops one row of every pattern: codes 0, 4, 0, 6, 4, 7 stay
LABELS = np.array([0, 1, 2, 0, 1, 0, 1, 0, 1, 0])                         # label 2 on one row only, of the pattern 7, outside SEL
EDGES = np.linspace(-1.0, 1.0, 5)                                         # 4 bins

# argument positions of include/gpz_hip.h (0 = the handle or the descriptor); "out" the first result array, "stream" the last argument
POS = {
    "gpz_predictor_run": dict(rows=2, psi_kind=4, out=5, phi=9),
    "gpz_predictor_draws": dict(rows=2, n_draws=3, seed=4, out=6),
    "gpz_predictor_draws_noisy": dict(rows=2, n_draws=4, seed=5, out=7),
    "gpz_predictor_stack": dict(rows=2, n_draws=3, seed=4, bins=7, groups=9, out=11, muY=15),
    "gpz_predictor_stack_noisy": dict(rows=2, n_draws=4, seed=5, bins=8, groups=10, out=12, muY=16),
    "gpz_predict_missing": dict(priors=4, rows=6, psi_kind=8, out=9),
    "gpz_predictor_run_dev": dict(rows=3, muX=6, sdX=7, muY=8, out=9, phi=14, stream=15),
    "gpz_predictor_draws_dev": dict(rows=3, muX=6, sdX=7, muY=8, n_draws=9, seed=10, out=12, stream=13),
    "gpz_predictor_stack_dev": dict(rows=3, muX=6, sdX=7, n_draws=8, seed=9, bins=12, groups=14, out=16, muY=20, stream=21),
    "gpz_predictor_run_noisy_dev": dict(rows=3, muX=10, sdX=11, sd2=12, muY=13, out=14, stream=19),
    "gpz_predictor_draws_noisy_dev": dict(rows=3, muX=10, sdX=11, sd2=12, muY=13, n_draws=14, seed=15, out=17, stream=18),
    "gpz_predictor_draws_gamma_noisy_dev": dict(rows=3, muX=10, sdX=11, sd2=12, muY=13, n_draws=14, seed=15, out=17, gam=18, stream=19),
    "gpz_predictor_stack_noisy_dev": dict(rows=3, muX=10, sdX=11, sd2=12, n_draws=13, seed=14, bins=17, groups=19, out=21, muY=25,
                                          stream=26),
    "gpz_predictor_run_missing_dev": dict(rows=3, muX=6, sdX=7, muY=8, priors=9, mask=10, out=11, stream=16),
    "gpz_predictor_draws_missing_dev": dict(rows=3, muX=6, sdX=7, muY=8, priors=9, mask=10, n_draws=11, seed=12, out=14, stream=15),
    "gpz_predictor_draws_gamma_missing_dev": dict(rows=3, muX=6, sdX=7, muY=8, priors=9, mask=10, n_draws=11, seed=12, out=14, gam=15,
                                                  stream=16),
    "gpz_predictor_stack_missing_dev": dict(rows=3, muX=6, sdX=7, priors=8, mask=9, n_draws=10, seed=11, bins=14, groups=16, out=18,
                                            muY=22, stream=23),
}
SCALARS = ("rows", "mask", "psi_kind", "n_draws", "seed", "bins", "groups")


def _address(a):
    return a if a is None or isinstance(a, int) else C.cast(a, C.c_void_p).value


class Recorder:
    """Stands in for the loaded library.  ``calls`` is the list of (entry, {scalar: value}); ``out`` the address of each call's first
    result array and ``gam`` of its Gam array, in the same order."""

    def __init__(self, k):
        self.k, self.calls, self.out, self.gam, self.created = k, [], [], [], 0

    def __getattr__(self, name):
        if name not in _lib.SYMBOLS:
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _vector(self, name, what, ptr):
        want = {"muX": MUX, "sdX": SDX, "sd2": SDX ** 2, "muY": MUY[self.k], "priors": PRIORS}[what]
        assert ptr is not None and ptr[:want.size] == want.tolist(), (name, what)

    def _call(self, name, *args):
        types = _lib.SYMBOLS[name][1]
        assert len(args) == len(types), (name, len(args))
        for t, a in zip(types, args):
            t.from_param(a)                                                # TypeError where the binding would refuse the argument
        if name == "gpz_predictor_create":
            args[-1]._obj.value = HANDLE
            self.created += 1
            return 0
        if name == "gpz_predictor_destroy":
            return None
        if name == "gpz_nan_groups":                                       # group ids in first-occurrence order, as the library gives them
            X, n, d, _, gid, ng = args
            nan = np.isnan(np.array(X[:n * d]).reshape((n, d), order="F"))
            seen = {}
            for i in range(n):
                gid[i] = seen.setdefault(nan[i].tobytes(), len(seen))
            ng._obj.value = len(seen)
            return 0
        pos = POS[name]
        if name.startswith("gpz_predictor_"):
            assert getattr(args[0], "value", args[0]) == HANDLE, name
        if "stream" in pos:
            assert pos["stream"] == len(args) - 1 and args[-1] == STREAM, name
        for what in ("muX", "sdX", "sd2", "muY", "priors"):
            if what in pos:
                self._vector(name, what, args[pos[what]])
        rec = {s: int(args[pos[s]]) for s in SCALARS if s in pos}
        if "phi" in pos:
            rec["phi"] = args[pos["phi"]] is not None
        self.calls.append((name, rec))
        self.out.append(_address(args[pos["out"]]))
        self.gam.append(_address(args[pos["gam"]]) if "gam" in pos else None)
        return 0

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def _model(k=1, d=D, m=M, method="VD", priors=PRIORS):
    model = gpz_amd.Model(m=m, d=d, k=k, method=method, muX=MUX[:d] if d <= 3 else np.zeros(d), sdX=SDX[:d] if d <= 3 else np.ones(d),
                          muY=MUY.get(k, np.zeros(k)))
    p = m * d + model.g_dim + m * k + k + 2 * m * k
    model.sets["best"] = {"theta": np.zeros(p), "w": np.zeros((m, k)), "iSigma_w": np.stack([np.eye(m)] * k, axis=2)}
    if priors is not None:
        model.sets["best"]["priors"] = priors
    return model


def _rows(codes=CODES):
    X = np.random.default_rng(3).standard_normal((len(codes), D))
    for i, code in enumerate(codes):
        X[i, [c for c in range(D) if code >> c & 1]] = np.nan
    return X


@pytest.fixture(params=[1, 2])
def rig(request, monkeypatch):
    """(Predictor, Recorder, stream lookups): the stand-in behind _lib.load, host tensors let through the device check and the stream
    lookup answered without a GPU."""
    rec, lookups = Recorder(request.param), []

    class Stream:
        cuda_stream = STREAM
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(gpz_amd.Predictor, "_check_dev_device", lambda self, **tensors: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: lookups.append(device) or Stream())
    p = gpz_amd.Predictor(_model(request.param))
    with np.errstate(all="ignore"):                                        # the stand-in writes no results: the arrays hold anything
        yield p, rec, lookups
    p.close()


def run(name, rows, **scalars):
    return (name, dict(rows=rows, **scalars))


# ---- the host methods ---------------------------------------------------------------------------------------------------------------------
def test_host_methods_reach_their_entries(rig):
    p, rec, lookups = rig
    Xc, Xn, Psi = _rows([0] * N), _rows(), np.full((N, D), 0.01)
    p.predict(Xc)
    assert rec.take() == [run("gpz_predictor_run", 10, psi_kind=0, phi=False)]
    p.predict(Xc, return_phi=True, selection=SEL)
    assert rec.take() == [run("gpz_predictor_run", 6, psi_kind=0, phi=True)]
    p.predict(Xc, Psi=Psi)
    assert rec.take() == [run("gpz_predictor_run", 10, psi_kind=1, phi=False)]
    p.predict(Xc, Psi=np.full(N, 0.01), selection=SEL)                     # one variance per row: fixPsi makes it n x d
    assert rec.take() == [run("gpz_predictor_run", 6, psi_kind=1, phi=False)]
    # rows with NaN: the groups in first-occurrence order (codes 4, 0, 7, 6), complete rows on the handle
    p.predict(Xn)
    assert rec.take() == [run("gpz_predict_missing", 3, psi_kind=0), run("gpz_predictor_run", 3, psi_kind=0, phi=False),
                          run("gpz_predict_missing", 2, psi_kind=0), run("gpz_predict_missing", 2, psi_kind=0)]
    p.predict(Xn, Psi=Psi, selection=SEL, return_phi=True)                 # codes 0, 4, 0, 6, 4, 7
    assert rec.take() == [run("gpz_predictor_run", 2, psi_kind=1, phi=True), run("gpz_predict_missing", 2, psi_kind=1),
                          run("gpz_predict_missing", 1, psi_kind=1), run("gpz_predict_missing", 1, psi_kind=1)]
    p.predict(_rows([6] * N))                                              # one pattern with missing values: one group
    assert rec.take() == [run("gpz_predict_missing", 10, psi_kind=0)]
    F = p.draws(Xc, 3, seed=5)
    assert rec.take() == [run("gpz_predictor_draws", 10, n_draws=3, seed=5)] and F.shape == (3, 10, p._k)
    p.draws(Xc, 3, seed=5, Psi=Psi, selection=SEL)
    assert rec.take() == [run("gpz_predictor_draws_noisy", 6, n_draws=3, seed=5)]
    r = p.stack(Xc, EDGES, n_draws=2, seed=7, groups=LABELS, weights=np.ones(N))
    assert rec.take() == [run("gpz_predictor_stack", 10, n_draws=2, seed=7, bins=4, groups=3)]
    assert rec.out[-1] == r.hist.ctypes.data and r.hist.shape == (3, 3, p._k, 4)
    p.stack(Xc, EDGES, groups=LABELS, selection=SEL)                       # label 2 is outside the selection: two groups
    assert rec.take() == [run("gpz_predictor_stack", 6, n_draws=0, seed=0, bins=4, groups=2)]
    r = p.stack_noisy(Xc, Psi, EDGES, n_draws=2, seed=7, groups=LABELS, weights=np.ones(N))
    assert rec.take() == [run("gpz_predictor_stack_noisy", 10, n_draws=2, seed=7, bins=4, groups=3)]
    assert rec.out[-1] == r.hist.ctypes.data
    p.stack_noisy(Xc, Psi[:, :1], EDGES, n_groups=5, selection=SEL)
    assert rec.take() == [run("gpz_predictor_stack_noisy", 6, n_draws=0, seed=0, bins=4, groups=5)]
    assert rec.created == 1 and lookups == []


def test_host_methods_reach_no_entry_without_rows(rig):
    p, rec, _ = rig
    Xn, Psi, none = _rows(), np.full((N, D), 0.01), np.zeros(N, dtype=bool)
    assert p.predict(Xn, selection=none, return_phi=True)[5].shape == (0, M)
    assert p.predict(Xn, Psi=Psi, selection=none)[0].shape == (0, p._k)
    assert p.draws(Xn, 3, selection=none).shape == (3, 0, p._k)
    assert p.draws(Xn, 3, Psi=Psi, selection=none).shape == (3, 0, p._k)
    assert not p.stack(Xn, EDGES, n_draws=2, selection=none).hist.any()
    assert not p.stack_noisy(Xn, Psi, EDGES, n_draws=2, selection=none).hist.any()
    assert rec.take() == [] and rec.created == 0


# ---- the device methods -------------------------------------------------------------------------------------------------------------------
def test_predict_dev_reaches_its_entries(rig):
    p, rec, lookups = rig
    Xc, Xn, Psi = torch.from_numpy(_rows([0] * N)), torch.from_numpy(_rows()), torch.full((N, D), 0.01, dtype=torch.float64)
    sel = torch.from_numpy(SEL)
    out = p.predict_dev(Xc)
    assert rec.take() == [run("gpz_predictor_run_dev", 10, phi=False)] and rec.out[-1] == out[0].data_ptr()
    p.predict_dev(Xc.float(), return_phi=True, selection=sel)
    assert rec.take() == [run("gpz_predictor_run_dev", 6, phi=True)]
    out = p.predict_dev(Xc, Psi=Psi)
    assert rec.take() == [run("gpz_predictor_run_noisy_dev", 10)] and rec.out[-1] == out[0].data_ptr()
    p.predict_dev(Xc, Psi=Psi[:, 0], selection=sel)                        # one variance per row: broadcast by a stride
    assert rec.take() == [run("gpz_predictor_run_noisy_dev", 6)]
    assert len(lookups) == 4
    # missing=True: ascending code 0, 4, 6, 7 and the mask of the observed dimensions, 7 & ~code
    out = p.predict_dev(Xn, missing=True)
    assert rec.take() == [run("gpz_predictor_run_dev", 3, phi=False), run("gpz_predictor_run_missing_dev", 3, mask=3),
                          run("gpz_predictor_run_missing_dev", 2, mask=1), run("gpz_predictor_run_missing_dev", 2, mask=0)]
    assert out[0].data_ptr() not in rec.out[-4:]                           # every group has results of its own, scattered back
    p.predict_dev(Xn, missing=True, selection=sel)
    assert rec.take() == [run("gpz_predictor_run_dev", 2, phi=False), run("gpz_predictor_run_missing_dev", 2, mask=3),
                          run("gpz_predictor_run_missing_dev", 1, mask=1), run("gpz_predictor_run_missing_dev", 1, mask=0)]
    assert len(lookups) == 6                                               # one lookup per Python call, however many groups
    # one pattern: the whole call, on the caller's own result tensors
    out = p.predict_dev(Xc, missing=True)
    assert rec.take() == [run("gpz_predictor_run_dev", 10, phi=False)] and rec.out[-1] == out[0].data_ptr()
    out = p.predict_dev(torch.from_numpy(_rows([4] * N)), missing=True)
    assert rec.take() == [run("gpz_predictor_run_missing_dev", 10, mask=3)] and rec.out[-1] == out[0].data_ptr()
    assert rec.created == 1


def test_draws_dev_reaches_its_entries(rig):
    p, rec, lookups = rig
    Xc, Xn, Psi = torch.from_numpy(_rows([0] * N)), torch.from_numpy(_rows()), torch.full((N, 1), 0.01, dtype=torch.float64)
    sel = torch.from_numpy(SEL)
    nd = dict(n_draws=3, seed=5)

    def base(t):                                                           # the address of the buffer behind the (n_draws, n, k) view
        return t.data_ptr()
    F = p.draws_dev(Xc, 3, seed=5)
    assert rec.take() == [run("gpz_predictor_draws_dev", 10, **nd)] and rec.out[-1] == base(F) and tuple(F.shape) == (3, 10, p._k)
    F = p.draws_dev(Xc, 3, seed=5, Psi=Psi, selection=sel)
    assert rec.take() == [run("gpz_predictor_draws_noisy_dev", 6, **nd)] and rec.out[-1] == base(F)
    F, Gam = p.draws_dev(Xc, 3, seed=5, Psi=Psi, return_gamma=True)
    assert rec.take() == [run("gpz_predictor_draws_gamma_noisy_dev", 10, **nd)]
    assert (rec.out[-1], rec.gam[-1]) == (base(F), base(Gam))
    F = p.draws_dev(Xn, 3, seed=5, missing=True)
    assert rec.take() == [run("gpz_predictor_draws_dev", 3, **nd), run("gpz_predictor_draws_missing_dev", 3, mask=3, **nd),
                          run("gpz_predictor_draws_missing_dev", 2, mask=1, **nd), run("gpz_predictor_draws_missing_dev", 2, mask=0, **nd)]
    assert base(F) not in rec.out[-4:]
    F, Gam = p.draws_dev(Xn, 3, seed=5, missing=True, return_gamma=True, selection=sel)
    assert rec.take() == [run("gpz_predictor_draws_dev", 2, **nd), run("gpz_predictor_draws_gamma_missing_dev", 2, mask=3, **nd),
                          run("gpz_predictor_draws_gamma_missing_dev", 1, mask=1, **nd),
                          run("gpz_predictor_draws_gamma_missing_dev", 1, mask=0, **nd)]
    assert rec.gam[-4] is None and base(Gam) not in rec.gam[-3:]
    assert tuple(Gam.shape) == (3, 6, p._k) and not Gam[:, [0, 2], :].any()   # complete rows (codes 0, 4, 0, 6, 4, 7): exactly 0.0
    assert len(lookups) == 5
    # one pattern: the whole call, on the caller's own tensors; gamma of complete rows zeroed in place
    F, Gam = p.draws_dev(Xc, 3, seed=5, missing=True, return_gamma=True)
    assert rec.take() == [run("gpz_predictor_draws_dev", 10, **nd)] and rec.out[-1] == base(F) and not Gam.any()
    F, Gam = p.draws_dev(torch.from_numpy(_rows([7] * N)), 3, seed=5, missing=True, return_gamma=True)
    assert rec.take() == [run("gpz_predictor_draws_gamma_missing_dev", 10, mask=0, **nd)]
    assert (rec.out[-1], rec.gam[-1]) == (base(F), base(Gam))
    F = p.draws_dev(torch.from_numpy(_rows([6] * N)), 3, seed=5, missing=True)
    assert rec.take() == [run("gpz_predictor_draws_missing_dev", 10, mask=1, **nd)] and rec.out[-1] == base(F)
    assert rec.created == 1


def test_stack_dev_methods_reach_their_entries(rig):
    p, rec, lookups = rig
    Xc, Xn, Psi = torch.from_numpy(_rows([0] * N)), torch.from_numpy(_rows()), torch.full((N, D), 0.01, dtype=torch.float64)
    sel, lab, wt = torch.from_numpy(SEL), torch.from_numpy(LABELS), torch.ones(N)
    st = dict(n_draws=2, seed=7, bins=4)
    r = p.stack_dev(Xc, EDGES, n_draws=2, seed=7, groups=lab, weights=wt)
    assert rec.take() == [run("gpz_predictor_stack_dev", 10, groups=3, **st)] and rec.out[-1] == r.hist.ctypes.data
    p.stack_dev(Xc, EDGES, n_draws=2, seed=7, groups=lab, selection=sel)    # label 2 is outside the selection: two groups
    assert rec.take() == [run("gpz_predictor_stack_dev", 6, groups=2, **st)]
    r = p.stack_noisy_dev(Xc, Psi, EDGES, n_draws=2, seed=7, groups=lab, weights=wt)
    assert rec.take() == [run("gpz_predictor_stack_noisy_dev", 10, groups=3, **st)] and rec.out[-1] == r.hist.ctypes.data
    p.stack_noisy_dev(Xc, Psi[:, 0], EDGES, n_draws=2, seed=7, n_groups=5, selection=sel)
    assert rec.take() == [run("gpz_predictor_stack_noisy_dev", 6, groups=5, **st)]
    # the missing stack: n_groups over all rows (label 2 sits on one row of the last pattern), the parts in ascending code order
    r = p.stack_missing_dev(Xn, EDGES, n_draws=2, seed=7, groups=lab, weights=wt)
    assert rec.take() == [run("gpz_predictor_stack_dev", 3, groups=3, **st), run("gpz_predictor_stack_missing_dev", 3, mask=3, groups=3, **st),
                          run("gpz_predictor_stack_missing_dev", 2, mask=1, groups=3, **st),
                          run("gpz_predictor_stack_missing_dev", 2, mask=0, groups=3, **st)]
    assert r.hist.ctypes.data not in rec.out[-4:] and r.hist.shape == (3, 3, p._k, 4)
    p.stack_missing_dev(Xn, EDGES, n_draws=2, seed=7, groups=lab, selection=sel)
    assert rec.take() == [run("gpz_predictor_stack_dev", 2, groups=2, **st), run("gpz_predictor_stack_missing_dev", 2, mask=3, groups=2, **st),
                          run("gpz_predictor_stack_missing_dev", 1, mask=1, groups=2, **st),
                          run("gpz_predictor_stack_missing_dev", 1, mask=0, groups=2, **st)]
    assert len(lookups) == 6
    # one pattern: the totals are the part
    r = p.stack_missing_dev(Xc, EDGES, n_draws=2, seed=7, weights=wt)
    assert rec.take() == [run("gpz_predictor_stack_dev", 10, groups=1, **st)] and rec.out[-1] == r.hist.ctypes.data
    r = p.stack_missing_dev(torch.from_numpy(_rows([4] * N)), EDGES, n_draws=2, seed=7)
    assert rec.take() == [run("gpz_predictor_stack_missing_dev", 10, mask=3, groups=1, **st)] and rec.out[-1] == r.hist.ctypes.data
    assert rec.created == 1


def test_device_methods_reach_no_entry_without_rows(rig):
    p, rec, lookups = rig
    Xn, Psi = torch.from_numpy(_rows()), torch.full((N, D), 0.01, dtype=torch.float64)
    none = torch.zeros(N, dtype=torch.bool)
    for kw in ({}, {"Psi": Psi}, {"missing": True}):
        assert tuple(p.predict_dev(Xn, selection=none, **kw)[0].shape) == (0, p._k)
        assert tuple(p.draws_dev(Xn, 3, selection=none, **kw).shape) == (3, 0, p._k)
        if kw:
            assert tuple(p.draws_dev(Xn, 3, selection=none, return_gamma=True, **kw)[1].shape) == (3, 0, p._k)
    assert not p.stack_dev(Xn, EDGES, n_draws=2, selection=none).hist.any()
    assert not p.stack_noisy_dev(Xn, Psi, EDGES, n_draws=2, selection=none).hist.any()
    assert not p.stack_missing_dev(Xn, EDGES, n_draws=2, selection=none).hist.any()
    assert rec.take() == [] and rec.created == 0 and lookups == []


def test_rows_with_nan_are_not_looked_at_without_missing(rig, monkeypatch):
    """Without ``missing`` the device methods hand the rows to the entry as they are (the C entry refuses NaN): no isnan pass."""
    p, rec, _ = rig
    Xn, Psi = torch.from_numpy(_rows()), torch.full((N, D), 0.01, dtype=torch.float64)

    def no_isnan(*a, **kw):
        raise AssertionError("torch.isnan on a route without missing=True")
    monkeypatch.setattr(torch, "isnan", no_isnan)
    p.predict_dev(Xn), p.predict_dev(Xn, Psi=Psi), p.draws_dev(Xn, 3), p.draws_dev(Xn, 3, Psi=Psi, return_gamma=True)
    p.stack_dev(Xn, EDGES), p.stack_noisy_dev(Xn, Psi, EDGES)
    assert [c[0] for c in rec.take()] == ["gpz_predictor_run_dev", "gpz_predictor_run_noisy_dev", "gpz_predictor_draws_dev",
                                          "gpz_predictor_draws_gamma_noisy_dev", "gpz_predictor_stack_dev",
                                          "gpz_predictor_stack_noisy_dev"]
    with pytest.raises(AssertionError, match="torch.isnan"):
        p.predict_dev(Xn, missing=True)


# ---- the refusal order of the later methods -----------------------------------------------------------------------------------------------
def raises(kind, text):
    return pytest.raises(kind, match="^" + re.escape(text))


def test_later_methods_refuse_in_order(monkeypatch):
    """stack_noisy, stack_noisy_dev, stack_missing_dev and draws_dev(return_gamma=True) with two things wrong at once: the text of the
    first.  The library load is made to fail, so a call that got past the checks would raise RuntimeError."""
    def no_library():
        raise RuntimeError("library load disabled by the test")
    monkeypatch.setattr(_lib, "load", no_library)
    p, pt = gpz_amd.Predictor(_model()), gpz_amd.Predictor(_model(), force_tiles=True)
    pc, pm = gpz_amd.Predictor(_model(method="GC")), gpz_amd.Predictor(_model(m=257))
    pp = gpz_amd.Predictor(_model(priors=np.ones(5) / 5))
    X, Xn = _rows([0] * 8), _rows([0, 0, 0, 4, 0, 0, 0, 0])
    Psi, neg = np.full((8, D), 0.01), np.full((8, D), -1.0)
    T, Tp = torch.from_numpy(X), torch.from_numpy(Psi)
    ints, ones = torch.zeros(8, dtype=torch.int64), torch.ones(8)
    # stack_noisy: Psi there, no cube, X, Psi's shape, the mask, NaN rows, the model, Psi's values, then stack's own ladder
    with raises(ValueError, "stack_noisy needs Psi: noise-free rows go to Predictor.stack"):
        p.stack_noisy(X[:, :2], None, [0.0])
    with raises(ValueError, "stack_noisy takes Psi as n x d, n x 1 or n variances: a d x d x n cube"):
        p.stack_noisy(X[:, :2], np.zeros((D, D, 8)), [0.0])
    with raises(ValueError, "X must be n x 3, got shape (8, 2)"):
        p.stack_noisy(X[:, :2], np.zeros((8, 2)), [0.0])
    with raises(ValueError, "Psi must be n x d, n x 1 or d x d x n (n = 8, d = 3), got shape (8, 2)"):
        p.stack_noisy(Xn, np.zeros((8, 2)), [0.0], selection=np.ones(3))
    with raises(ValueError, "selection must be a mask of length 8"):
        p.stack_noisy(Xn, Psi, [0.0], selection=np.ones(3))
    with raises(ValueError, "X has 1 rows with missing values (NaN): stacks are for complete rows"):
        pc.stack_noisy(Xn, neg, [0.0])
    with raises(ValueError, "stack_noisy with Psi needs a model inside predict_noisy_fits"):
        pc.stack_noisy(X, neg, [0.0])
    with raises(ValueError, "stack_noisy with Psi needs the fused draws route: the predictor was made with force_tiles=True"):
        pt.stack_noisy(X, neg, [0.0])
    with raises(ValueError, "Psi must be finite and >= 0"):
        p.stack_noisy(X, neg, [0.0])
    with raises(ValueError, "edges must be a vector of at least 2 values, got shape (1,)"):
        p.stack_noisy(X, Psi, [0.0], n_draws=-1)
    with raises(ValueError, "n_draws must be a non-negative integer, got -1"):
        p.stack_noisy(X, Psi, [0.0, 1.0], n_draws=-1, groups=np.zeros(3, dtype=int))
    with raises(ValueError, "groups must be 8 integer labels"):
        p.stack_noisy(X, Psi, [0.0, 1.0], groups=np.zeros(3, dtype=int), weights=np.zeros(3))
    # stack_noisy_dev: Psi there, X, Psi, the model, the edges, the draws, groups, weights, n_groups, the size, the device last
    with raises(ValueError, "stack_noisy_dev needs Psi: noise-free rows go to Predictor.stack_dev"):
        p.stack_noisy_dev(X, None, [0.0])
    with raises(TypeError, "stack_noisy_dev takes a torch tensor on cuda:0; a NumPy array goes to Predictor.stack_noisy"):
        p.stack_noisy_dev(X, Psi, [0.0])
    with raises(ValueError, "X must be n x 3, got shape (8, 2)"):
        p.stack_noisy_dev(T[:, :2], Psi, [0.0])
    with raises(TypeError, "selection must be a bool torch tensor on the same device as X"):
        p.stack_noisy_dev(T, Psi, [0.0], selection=ones)
    with raises(TypeError, "stack_noisy_dev takes Psi as a torch tensor on cuda:0; a NumPy array goes to Predictor.stack_noisy"):
        pc.stack_noisy_dev(T, Psi, [0.0])
    with raises(ValueError, "Psi must be n x d, n x 1 or n (n = 8, d = 3), got shape (8, 2)"):
        pc.stack_noisy_dev(T, Tp[:, :2], [0.0])
    with raises(ValueError, "stack_noisy_dev with Psi needs a model inside predict_noisy_fits"):
        pc.stack_noisy_dev(T, Tp, [0.0])
    with raises(ValueError, "stack_noisy_dev with Psi needs the fused draws route: the predictor was made with force_tiles=True"):
        pt.stack_noisy_dev(T, Tp, [0.0])
    with raises(ValueError, "edges must be a vector of at least 2 values, got shape (1,)"):
        p.stack_noisy_dev(T, Tp, [0.0], n_draws=-1)
    with raises(ValueError, "n_draws must be a non-negative integer, got -1"):
        p.stack_noisy_dev(T, Tp, [0.0, 1.0], n_draws=-1, groups=ones)
    with raises(ValueError, "groups must be a tensor of 8 integer labels"):
        p.stack_noisy_dev(T, Tp, [0.0, 1.0], groups=ones, weights=ints)
    with raises(ValueError, "weights must be a float tensor of 8 values"):
        p.stack_noisy_dev(T, Tp, [0.0, 1.0], groups=ints, weights=ints, n_groups=0)
    with raises(ValueError, "n_groups must be a positive integer, got 0"):
        p.stack_noisy_dev(T, Tp, np.arange(4098.0), groups=ints, weights=ones, n_groups=0)
    with raises(ValueError, "n_groups * bins = 8194 is over the limit of 4096 per call"):
        p.stack_noisy_dev(T, Tp, np.arange(4098.0), groups=ints, weights=ones, n_groups=2)
    with raises(ValueError, "X must be on cuda:0, it is on cpu: the host methods take host arrays"):
        p.stack_noisy_dev(T, Tp, [0.0, 1.0], groups=ints, weights=ones, n_groups=2)
    # stack_missing_dev: X, the model and the priors, then the ladder of stack_dev
    with raises(TypeError, "stack_dev takes a torch tensor on cuda:0; a NumPy array goes to Predictor.stack"):
        pm.stack_missing_dev(X, [0.0])
    with raises(ValueError, "X must be n x 3, got shape (8, 2)"):
        pm.stack_missing_dev(T[:, :2], [0.0])
    with raises(ValueError, "stack_missing_dev with missing=True needs a model inside predict_missing_fits: m <= 256, not m = 257"):
        pm.stack_missing_dev(T, [0.0])
    with raises(ValueError, "stack_missing_dev with missing=True needs a model inside predict_missing_fits: a diagonal kind"):
        pc.stack_missing_dev(T, [0.0])
    with raises(ValueError, "the priors of the set must be 6 values, got 5"):
        pp.stack_missing_dev(T, [0.0])
    with raises(ValueError, "edges must be a vector of at least 2 values, got shape (1,)"):
        p.stack_missing_dev(T, [0.0], n_draws=-1)
    with raises(ValueError, "n_draws must be a non-negative integer, got -1"):
        p.stack_missing_dev(T, [0.0, 1.0], n_draws=-1, groups=ones)
    with raises(ValueError, "groups must be a tensor of 8 integer labels"):
        p.stack_missing_dev(T, [0.0, 1.0], groups=ones, weights=ints)
    with raises(ValueError, "weights must be a float tensor of 8 values"):
        p.stack_missing_dev(T, [0.0, 1.0], weights=ints, n_groups=0)
    with raises(ValueError, "n_groups must be a positive integer, got 0"):
        p.stack_missing_dev(T, np.arange(4098.0), n_groups=0)
    with raises(ValueError, "n_groups * bins = 8194 is over the limit of 4096 per call"):
        p.stack_missing_dev(T, np.arange(4098.0), n_groups=2)
    with raises(ValueError, "X must be on cuda:0, it is on cpu: the host methods take host arrays"):
        p.stack_missing_dev(T, [0.0, 1.0])
    # draws_dev(return_gamma=True): X, the draws, the keyword's own rule, the missing model, Psi, the noisy model, the device last
    with raises(TypeError, "draws_dev takes a torch tensor on cuda:0; a NumPy array goes to Predictor.draws"):
        p.draws_dev(X, 0, return_gamma=True)
    with raises(ValueError, "X must be n x 3, got shape (8, 2)"):
        p.draws_dev(T[:, :2], 0, return_gamma=True)
    with raises(ValueError, "n_draws must be a positive integer, got 0"):
        p.draws_dev(T, 0, return_gamma=True)
    with raises(ValueError, "seed must be an integer in [0, 2^64), got -1"):
        p.draws_dev(T, 3, seed=-1, return_gamma=True)
    with raises(ValueError, "return_gamma=True needs Psi or missing=True, and not both"):
        pm.draws_dev(T, 3, return_gamma=True)
    with raises(ValueError, "return_gamma=True needs Psi or missing=True, and not both"):
        pm.draws_dev(T, 3, Psi=Psi, missing=True, return_gamma=True)
    with raises(ValueError, "draws_dev with missing=True needs a model inside predict_missing_fits: m <= 256, not m = 257"):
        pm.draws_dev(T, 3, missing=True, return_gamma=True)
    with raises(ValueError, "the priors of the set must be 6 values, got 5"):
        pp.draws_dev(T, 3, missing=True, return_gamma=True)
    with raises(TypeError, "draws_dev takes Psi as a torch tensor on cuda:0; a NumPy array goes to Predictor.draws"):
        pc.draws_dev(T, 3, Psi=Psi, return_gamma=True)
    with raises(ValueError, "Psi must be n x d, n x 1 or n (n = 8, d = 3), got shape (8, 2)"):
        pc.draws_dev(T, 3, Psi=Tp[:, :2], return_gamma=True)
    with raises(ValueError, "draws_dev with Psi needs a model inside predict_noisy_fits"):
        pc.draws_dev(T, 3, Psi=Tp, return_gamma=True)
    with raises(ValueError, "draws_dev with Psi needs the fused draws route: the predictor was made with force_tiles=True"):
        pt.draws_dev(T, 3, Psi=Tp, return_gamma=True)
    with raises(ValueError, "X must be on cuda:0, it is on cpu: the host methods take host arrays"):
        p.draws_dev(T, 3, Psi=Tp, return_gamma=True)
    with raises(ValueError, "X must be on cuda:0, it is on cpu: the host methods take host arrays"):
        p.draws_dev(T, 3, missing=True, return_gamma=True)
