"""The calls host._LBFGSDevice and the device-vector branch of host.minfunc_lbfgs make on the library, without a GPU and without the
built library (the way of test_predictor_calls_cpu.py): a recording stand-in behind ``_lib.load`` checks every call against the
binding and notes, per gpz_lbfgs_direction, whether g came as NULL or as a pointer.  gpz_lbfgs_direction takes NULL for "the g of
the gpz_lbfgs_add just before" and uses that pass's products [S Y]'g; a pointer is always multiplied afresh.  _LBFGSDevice must pass
NULL exactly when its argument is the DevVec OBJECT add_step was just given - so train() keeps its one pass over the memory per
iteration - and a pointer for everything else, an equal vector or the same storage under another object included.

The stand-in computes on CPU tensors (host._LBFGS behind the handle, NumPy for gpz_vec_stats / gpz_vec_axpy), so the whole driver
runs through it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gpz_amd import _lib, host

HANDLE = 0x1BF65


def _view(ptr, p):
    return np.ctypeslib.as_array((C.c_double * p).from_address(ptr))


class Recorder:
    """``calls``: [("add", g address) | ("direction", g address or None)] in order."""

    def __init__(self):
        self.calls, self.mem, self.p, self.last_g = [], None, 0, None

    def __getattr__(self, name):
        if name not in _lib.SYMBOLS:
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _call(self, name, *args):
        types = _lib.SYMBOLS[name][1]
        assert len(args) == len(types), (name, len(args))
        for t, a in zip(types, args):
            t.from_param(a)                                                # TypeError where the binding would refuse the argument
        return getattr(self, "_" + name)(*args)

    def _gpz_lbfgs_create(self, p, corrections, device, stream, out):
        assert self.mem is None and stream is None
        self.mem, self.p = host._LBFGS(p, corrections), p
        out._obj.value = HANDLE
        return 0

    def _gpz_lbfgs_destroy(self, h):
        assert getattr(h, "value", h) == HANDLE
        self.mem = None

    def _gpz_lbfgs_last_error(self):
        return b"stand-in"

    def _gpz_lbfgs_add(self, h, g, g_old, t, d, added):
        assert getattr(h, "value", h) == HANDLE and g and g_old and d
        self.calls.append(("add", g))
        self.last_g = g
        added._obj.value = int(self.mem.add_step(_view(g, self.p).copy(), _view(g_old, self.p).copy(), t, _view(d, self.p).copy()))
        return 0

    def _gpz_lbfgs_direction(self, h, g, d):
        assert getattr(h, "value", h) == HANDLE and d
        self.calls.append(("direction", g))
        if g is None:
            if self.last_g is None:
                return -1                                                  # GPZ_ERR_ARG, as the library answers
            g = self.last_g
        self.last_g = None
        _view(d, self.p)[:] = self.mem.direction(_view(g, self.p).copy())
        return 0

    def _gpz_vec_stats(self, g, d, p, device, stream, out):
        gv = _view(g, p)
        dv = _view(d, p) if d else np.zeros(p)
        out[0], out[1], out[2], out[3] = float(gv @ dv), float(np.abs(gv).max()), float(np.abs(gv).sum()), float(np.abs(dv).max())
        return 0

    def _gpz_vec_axpy(self, out, x, t, d, p, device, stream):
        _view(out, p)[:] = _view(x, p) + t * _view(d, p)
        return 0


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


def vec(a):
    return host.DevVec(torch.tensor(np.asarray(a, dtype=np.float64)))


def test_direction_passes_null_for_the_object_of_the_add_just_before_and_a_pointer_otherwise(rec):
    p = 9
    rng = np.random.default_rng(0)
    g_old, d = rng.standard_normal(p), rng.standard_normal(p)
    g = g_old + 0.5 * d
    mem = host._LBFGSDevice(p, 3)
    G, G_old, D = vec(g), vec(g_old), vec(d)
    A = G.t.data_ptr()
    assert mem.add_step(G, G_old, 1.0, D)
    d1 = mem.direction(G)                                   # the object add_step was given: NULL
    d2 = mem.direction(G)                                   # a direction has come between: by pointer
    assert mem.add_step(G, G_old, 1.0, D)
    d3 = mem.direction(host.DevVec(G.t))                    # the same storage under another object: by pointer
    assert mem.add_step(G, G_old, 1.0, D)
    d4 = mem.direction(G.copy())                            # an equal vector elsewhere: by pointer
    d5 = mem.direction(G)                                   # ... after which G is no longer "the g just before"
    mem.direction(G_old)                                    # never given to add_step as g
    mem.close()
    B = rec.calls[6][1]
    assert rec.calls == [("add", A), ("direction", None), ("direction", A), ("add", A), ("direction", A), ("add", A), ("direction", B),
                         ("direction", A), ("direction", G_old.t.data_ptr())]
    assert B not in (None, A)
    for q in (d1, d2, d3, d4, d5):
        assert isinstance(q, host.DevVec) and q.t.data_ptr() != A and np.all(np.isfinite(q.host()))
    assert np.array_equal(d1.host(), d2.host())


def test_a_failed_add_leaves_nothing_to_refer_to(rec, monkeypatch):
    """add_step forgets the previous g BEFORE the call: if gpz_lbfgs_add raises, the next direction goes by pointer."""
    p = 5
    mem = host._LBFGSDevice(p, 2)
    G, G_old, D = vec(np.arange(1.0, 6.0)), vec(np.zeros(p)), vec(np.ones(p))
    assert mem.add_step(G, G_old, 1.0, D)
    monkeypatch.setattr(rec, "_gpz_lbfgs_add", lambda *a: -2)
    with pytest.raises(_lib.GpzError):
        mem.add_step(G, G_old, 1.0, D)
    mem.direction(G)
    assert rec.calls[-1] == ("direction", G.t.data_ptr())


def test_the_driver_makes_one_null_call_per_iteration(rec):
    """minfunc_lbfgs on device vectors: every iteration after the first is add_step(g, ...) followed by direction of that very
    object, so every gpz_lbfgs_direction call carries NULL; the run ends where the host-vector run ends."""
    rng = np.random.default_rng(1)
    A = rng.standard_normal((12, 12)); A = A @ A.T + np.eye(12)
    b = rng.standard_normal(12)

    def fun(x):
        if isinstance(x, host.DevVec):
            xv = x.host()
            return float(0.5 * xv @ A @ xv - b @ xv), vec(A @ xv - b)
        return float(0.5 * x @ A @ x - b @ x), A @ x - b
    x0 = rng.standard_normal(12)
    xd, fd, flag_d, evals_d, _ = host.minfunc_lbfgs(fun, vec(x0), max_iter=60, corrections=5)
    xh, fh, flag_h, evals_h, _ = host.minfunc_lbfgs(fun, x0, max_iter=60, corrections=5)
    kinds = [k for k, _ in rec.calls]
    assert len(kinds) >= 6 and kinds == ["add", "direction"] * (len(kinds) // 2)
    assert all(g is None for k, g in rec.calls if k == "direction")
    assert flag_d == flag_h and flag_d in (1, 2) and abs(evals_d - evals_h) <= 2
    assert np.allclose(xd.host(), xh, rtol=0, atol=1e-6) and np.allclose(xh, np.linalg.solve(A, b), rtol=0, atol=1e-4)
