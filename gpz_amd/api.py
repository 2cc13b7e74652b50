"""Host-side mirror of the reference's interface for the objective/gradient path.

Same names, argument order and meaning as the MATLAB functions they stand in for
(paths relative to the OxfordML/GPz tree):

    GPz(theta, model, X, Y, Psi, omega, training, validation)   GPz/GPz.m:1
    getPHI(X, Psi, theta, model, selection)                      GPz/getPHI.m:1
    inv_logdet(X)                                                GPz/inv_logdet.m:1
    Dxy(X, Y)                                                    GPz/Dxy.m:1
    predict(X, model, whichSet=..., selection=...)               GPz/predict.m:1 (no-Psi / no-NaN branch)

Everything numeric happens in libgpz_hip.so on the GPU; this file only marshals numpy arrays
(column-major, like MATLAB) across the C ABI.  ``model`` is any object with the reference's struct fields
``m, d, k, method, heteroscedastic`` (+ ``muX, sdX, muY`` and ``sets`` for predict).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib

# the reference's globals (GPz.m:3-7), refreshed by every 2-output GPz() call and left alone by solve-only calls
globals_ = {"trainRMSE": None, "trainLL": None, "validRMSE": None, "validLL": None}


@dataclass
class Model:
    """model struct of init.m:16-20,41-43,86."""
    m: int
    d: int
    k: int = 1
    method: str = "VD"
    heteroscedastic: bool = True
    g_dim: int = 0
    muX: Optional[np.ndarray] = None
    sdX: Optional[np.ndarray] = None
    muY: Optional[np.ndarray] = None
    sets: dict = field(default_factory=dict)

    def __post_init__(self):
        if self.g_dim == 0:
            self.g_dim = {"GL": 1, "VL": self.m, "GD": self.d, "VD": self.m * self.d, "GC": self.d ** 2,
                          "VC": self.d ** 2 * self.m}[self.method]
        if self.muX is None:
            self.muX = np.zeros(self.d)
        if self.sdX is None:
            self.sdX = np.ones(self.d)
        if self.muY is None:
            self.muY = np.zeros(self.k)


def _desc(model, device=0, stream=None, rank=0, world=1, dtype="f64"):
    ds = _lib.gpz_desc()
    if dtype not in ("f64", "f32"):
        raise ValueError("dtype must be 'f64' or 'f32'")
    ds.dtype = 1 if dtype == "f32" else 0
    ds.d, ds.m, ds.k = int(model.d), int(model.m), int(model.k)
    ds.method = str(model.method).encode()
    ds.heteroscedastic = 1 if model.heteroscedastic else 0
    ds.device = int(device)
    ds.stream = stream
    ds.rank, ds.world = int(rank), int(world)
    return ds


def _psi_kind(model, psi):
    """psi_kind of the C ABI from the array's shape: n x d for the diagonal kinds (1), d x d x n cubes for GC/VC (2), and
    n x d per-dimension variances given to GC/VC (3: the diagonal cubes of fixPsi.m:27-31, expanded by the library)."""
    if psi is None:
        return 0
    if psi.ndim == 3:
        return 2
    return 3 if str(model.method)[1] == "C" else 1


def _f64(a, ndim=None):
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    if ndim == 2 and a.ndim == 1:
        a = a[:, None]
    return np.asfortranarray(a)


def _omega(omega, n_tot, k):
    """omega as the reference takes it: n x 1 (one weight per row for every output) or n x k (per-output weights,
    GPz.m:48 ``omega(training,:)``; getOmega.m:19 returns ``(1+Y).^-2``, n x k for a k-column Y)."""
    om = _f64(omega, 2)
    if om is not None and (om.ndim != 2 or om.shape[0] != n_tot or om.shape[1] not in (1, k)):
        raise ValueError("omega must be n x 1 or n x k")
    return om


def _mask(a, n):
    if a is None:
        return None
    a = np.asarray(a)
    if a.size == 0:
        return None
    a = np.ascontiguousarray(a.astype(bool).ravel().astype(np.uint8))
    if a.size != n:
        raise ValueError("mask length must equal the number of rows of X")
    return a


def _last_phi(lib, h):
    out = (C.c_double * 2)()
    _lib.check(lib.gpz_ctx_last_phi(h, out))
    return bool(out[0]), float(out[1])


class GPzContext:
    """The closure ``f = @(theta) GPz(theta,model,X,Y,Psi,omega,training,validation)`` (train.m:40) with the data
    resident on the GPU.  ``X`` must already be normalised and ``Y`` centred, as train.m:30-33 does before
    building the closure."""

    def __init__(self, model, X, Y, Psi=None, omega=None, training=None, validation=None, device=0, stream=None,
                 rank=0, world=1, allreduce=None, dtype="f64", patterns=None):
        """patterns: NaN-pattern table of the whole data set (G x d bool, True = missing, first-occurrence order; see
        gpz_amd.dist.nan_patterns) — needed by row-sharded GC/VC runs with missing values."""
        lib = _lib.load()
        X = _f64(X, 2)
        Y = _f64(Y, 2)
        n_tot = X.shape[0]
        if X.shape[1] != model.d or Y.shape != (n_tot, model.k):
            raise ValueError("X must be n x d and Y n x k")
        om = _omega(omega, n_tot, model.k)
        psi_kind = 0
        psi = None
        if Psi is not None:
            psi = _f64(Psi)
            psi_kind = _psi_kind(model, psi)
        self._tr = _mask(training, n_tot)
        self._va = _mask(validation, n_tot)
        self.model = model
        self._desc = _desc(model, device, stream, rank, world, dtype)
        self._desc.omega_cols = 0 if om is None else om.shape[1]
        h = C.c_void_p()
        pat = None
        if patterns is not None:
            pat = np.ascontiguousarray(np.asarray(patterns, dtype=bool).reshape(-1, model.d).astype(np.uint8))
        _lib.check(lib.gpz_ctx_create_sharded(
            C.byref(self._desc), n_tot, _lib.dptr(X), _lib.dptr(Y), _lib.dptr(psi), psi_kind, _lib.dptr(om),
            None if self._tr is None else self._tr.ctypes.data_as(_lib.c_uint8_p),
            None if self._va is None else self._va.ctypes.data_as(_lib.c_uint8_p),
            None if pat is None else pat.ctypes.data_as(_lib.c_uint8_p), 0 if pat is None else pat.shape[0], C.byref(h)))
        self._h = h
        self._lib = lib
        self.p = int(lib.gpz_theta_len(h))
        self.n_train = int(lib.gpz_n_train(h))
        self.n_valid = int(lib.gpz_n_valid(h))
        self.stats = {}
        self.info = 0
        self.n_global = self.n_train
        self._cb = None
        if allreduce is not None:
            self._cb = _lib.ALLREDUCE_FN(allreduce)
            _lib.check(lib.gpz_ctx_set_allreduce(h, self._cb, None))

    def set_allreduce(self, allreduce):
        """Install (or replace) the caller-supplied all-reduce hook of a sharded context (gpz_ctx_set_allreduce)."""
        self._cb = _lib.ALLREDUCE_FN(allreduce)
        _lib.check(self._lib.gpz_ctx_set_allreduce(self._h, self._cb, None))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpz_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eval(self, theta):
        """[nlogML, grad] = GPz(theta, ...) plus the four global statistics (self.stats)."""
        theta = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        if theta.size != self.p:
            raise ValueError(f"theta must have {self.p} elements")
        f = C.c_double()
        g = np.empty(self.p)
        st = (C.c_double * 4)(float("nan"), float("nan"), float("nan"), float("nan"))
        dg = (C.c_double * 2)()
        _lib.check(self._lib.gpz_eval(self._h, _lib.dptr(theta), C.byref(f), _lib.dptr(g), st, dg))
        self.stats = {"trainRMSE": st[0], "trainLL": st[1]}
        if self._va is not None:     # a mask that selects no row gives NaN, as GPz.m:258-259 does (0/0)
            self.stats.update(validRMSE=st[2], validLL=st[3])
        self.info = int(dg[0])
        self.n_global = int(dg[1])
        return f.value, g

    def eval_dev(self, theta_t):
        """gpz_eval_dev: theta_t is a float64 CUDA tensor on the context's device; returns (f, g) with g a new CUDA
        tensor — theta and the gradient never visit the host."""
        import torch
        if theta_t.numel() != self.p or theta_t.dtype != torch.float64 or not theta_t.is_cuda:
            raise ValueError(f"theta must be a float64 CUDA tensor of {self.p} elements")
        theta_t = theta_t.contiguous()
        g = torch.empty_like(theta_t)
        torch.cuda.current_stream(theta_t.device).synchronize()     # the context runs on its own stream
        f = C.c_double()
        st = (C.c_double * 4)(float("nan"), float("nan"), float("nan"), float("nan"))
        dg = (C.c_double * 2)()
        _lib.check(self._lib.gpz_eval_dev(self._h, theta_t.data_ptr(), C.byref(f), g.data_ptr(), st, dg))
        self.stats = {"trainRMSE": st[0], "trainLL": st[1]}
        if self._va is not None:
            self.stats.update(validRMSE=st[2], validLL=st[3])
        self.info = int(dg[0])
        self.n_global = int(dg[1])
        return f.value, g

    def solve(self, theta):
        """[~, ~, w, iSigma_w] = GPz(theta, ...)  (GPz.m:84-87); also returns the 1 x k partial nlogML."""
        theta = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        m, k = self.model.m, self.model.k
        w = np.empty((m, k), order="F")
        iS = np.empty((m, m, k), order="F")
        part = np.empty(k)
        _lib.check(self._lib.gpz_solve(self._h, _lib.dptr(theta), _lib.dptr(w), _lib.dptr(iS), _lib.dptr(part)))
        return w, iS, part

    def set_pinv_mode(self, mode):
        """Branch of inv_logdet.m:7-12: 0 = Cholesky, SVD pseudo-inverse when SIGMA is nearly singular (default);
        1 = always the truncating SVD route; -1 = never."""
        _lib.check(self._lib.gpz_ctx_set_pinv_mode(self._h, int(mode)))

    def last_pinv(self):
        """(route taken, rank kept, largest singular value, Jacobi sweeps) of the last eval/solve."""
        out = (C.c_double * 4)()
        _lib.check(self._lib.gpz_ctx_last_pinv(self._h, out))
        return bool(out[0]), int(out[1]), float(out[2]), int(out[3])

    def last_phi(self):
        """(fell back, bound) of the last eval: whether the covariance-kind PHI build left the f64 MFMA route (k_phi_quad) for
        k_phi_cov because the bound on its rounding error, max_j B_j, exceeded 2^-33.  (False, 0.0) on every other route."""
        return _last_phi(self._lib, self._h)

    def phi(self):
        """PHI (n_train x m) of the last eval/solve — the 5th output of GPz.m:1."""
        out = np.empty((self.n_train, self.model.m), order="F")
        _lib.check(self._lib.gpz_get_phi(self._h, _lib.dptr(out)))
        return out

    def enable_timing(self, on=True):
        """on = True / 1: HIP events around every stage (eager launches); 2: around the dominant stages only (PHI build, PHI'W PHI,
        T = PHI [inv(SIGMA) | w], moments), the evaluation still replayed as hipGraph segments; False / 0: off."""
        _lib.check(self._lib.gpz_ctx_enable_timing(self._h, int(on)))

    def reset_timings(self):
        _lib.check(self._lib.gpz_ctx_reset_timings(self._h))

    def timings(self):
        """{stage: (total_ms, calls)} measured with HIP events on the context's stream."""
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        calls = (C.c_int64 * cap)()
        n = self._lib.gpz_ctx_timings(self._h, names, ms, calls, cap)
        return {names[i].decode(): (ms[i], int(calls[i])) for i in range(min(n, cap))}

    def route(self):
        """Which kernels this context runs and the state of its evaluation graph (gpz_ctx_route), as one line of text."""
        buf = C.create_string_buffer(512)
        self._lib.gpz_ctx_route(self._h, buf, 512)
        return buf.value.decode()

    def comm_info(self):
        """What the RCCL communicator behind this context's all-reduce reports about itself (gpz_ctx_comm_info):
        {"nccl_count", "nccl_rank", "nccl_device"} (-1 without an in-library communicator), "hip_device", "pci_bus_id"."""
        return _comm_info(lambda info, bus, cap: self._lib.gpz_ctx_comm_info(self._h, info, bus, cap))


class GPzMulti:
    """The same closure on several GPUs behind ONE synchronous call (gpz_mgpu_* of the C ABI): the library splits the
    training-selected rows into contiguous blocks, one per device, drives every device from its own host thread and
    all-reduces the m x m / m x (d^2+d) partials with RCCL itself — no torch.distributed, no Python in the evaluation.
    What a single MATLAB process reaches through the MEX gateway (minFunc.m:314 calls funObj once and waits).

    n_gpus None/0: every device of the node.  reducer "loopback": all shards on ONE device with the library's own
    rank-ordered reducer — how the sharded path is exercised on single-GPU machines."""

    def __init__(self, model, X, Y, Psi=None, omega=None, training=None, validation=None, n_gpus=None, devices=None,
                 reducer="rccl", dtype="f64"):
        lib = _lib.load()
        X = _f64(X, 2)
        Y = _f64(Y, 2)
        n_tot = X.shape[0]
        if X.shape[1] != model.d or Y.shape != (n_tot, model.k):
            raise ValueError("X must be n x d and Y n x k")
        om = _omega(omega, n_tot, model.k)
        psi, psi_kind = None, 0
        if Psi is not None:
            psi = _f64(Psi)
            psi_kind = _psi_kind(model, psi)
        self._tr = _mask(training, n_tot)
        self._va = _mask(validation, n_tot)
        if reducer not in ("rccl", "loopback"):
            raise ValueError("reducer must be 'rccl' or 'loopback'")
        dev = None
        if devices is not None:
            dev = np.ascontiguousarray(np.asarray(devices, dtype=np.int32))
            n_gpus = dev.size
        self.model = model
        self._desc = _desc(model, 0, None, 0, 1, dtype)
        self._desc.omega_cols = 0 if om is None else om.shape[1]
        h = C.c_void_p()
        _lib.check(lib.gpz_mgpu_create(
            C.byref(self._desc), int(n_gpus or 0), None if dev is None else dev.ctypes.data_as(_lib.c_int32_p),
            1 if reducer == "loopback" else 0, n_tot, _lib.dptr(X), _lib.dptr(Y), _lib.dptr(psi), psi_kind, _lib.dptr(om),
            None if self._tr is None else self._tr.ctypes.data_as(_lib.c_uint8_p),
            None if self._va is None else self._va.ctypes.data_as(_lib.c_uint8_p), C.byref(h)))
        self._h, self._lib = h, lib
        self.n_gpus = int(lib.gpz_mgpu_size(h))
        self.p = int(lib.gpz_mgpu_theta_len(h))
        self.rows_per_gpu = [int(lib.gpz_n_train(lib.gpz_mgpu_ctx(h, r))) for r in range(self.n_gpus)]
        self.n_train = sum(self.rows_per_gpu)
        self.stats, self.info, self.n_global = {}, 0, self.n_train

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpz_mgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eval(self, theta):
        theta = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        if theta.size != self.p:
            raise ValueError(f"theta must have {self.p} elements")
        f = C.c_double()
        g = np.empty(self.p)
        st = (C.c_double * 4)(float("nan"), float("nan"), float("nan"), float("nan"))
        dg = (C.c_double * 2)()
        _lib.check(self._lib.gpz_mgpu_eval(self._h, _lib.dptr(theta), C.byref(f), _lib.dptr(g), st, dg))
        self.stats = {"trainRMSE": st[0], "trainLL": st[1]}
        if self._va is not None:
            self.stats.update(validRMSE=st[2], validLL=st[3])
        self.info, self.n_global = int(dg[0]), int(dg[1])
        return f.value, g

    def solve(self, theta):
        theta = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        if theta.size != self.p:
            raise ValueError(f"theta must have {self.p} elements")
        m, k = self.model.m, self.model.k
        w = np.empty((m, k), order="F")
        iS = np.empty((m, m, k), order="F")
        part = np.empty(k)
        _lib.check(self._lib.gpz_mgpu_solve(self._h, _lib.dptr(theta), _lib.dptr(w), _lib.dptr(iS), _lib.dptr(part)))
        return w, iS, part

    def _each(self):
        return [self._lib.gpz_mgpu_ctx(self._h, r) for r in range(self.n_gpus)]

    @property
    def alive(self):
        """False once a rank failed inside a call with the RCCL reducer (communicators aborted): re-create the handle."""
        return bool(self._lib.gpz_mgpu_alive(self._h))

    def debug_fail_at(self, rank, exchange):
        """Test hook (gpz_mgpu_debug_fail_at): the next call fails on `rank` at exchange point 1 or 2."""
        _lib.check(self._lib.gpz_mgpu_debug_fail_at(self._h, int(rank), int(exchange)))

    def comm_info(self, rank=0):
        """gpz_mgpu_comm_info of one rank (see GPzContext.comm_info)."""
        return _comm_info(lambda info, bus, cap: self._lib.gpz_mgpu_comm_info(self._h, int(rank), info, bus, cap))

    def route(self, rank=0):
        buf = C.create_string_buffer(512)
        self._lib.gpz_ctx_route(self._lib.gpz_mgpu_ctx(self._h, int(rank)), buf, 512)
        return buf.value.decode()

    def last_phi(self, rank=0):
        """GPzContext.last_phi of one rank (every rank bounds the rounding error over its own rows)."""
        return _last_phi(self._lib, self._lib.gpz_mgpu_ctx(self._h, int(rank)))

    def enable_timing(self, on=True):
        for c in self._each():
            _lib.check(self._lib.gpz_ctx_enable_timing(c, int(on)))

    def reset_timings(self):
        for c in self._each():
            _lib.check(self._lib.gpz_ctx_reset_timings(c))

    def set_pinv_mode(self, mode):
        for c in self._each():
            _lib.check(self._lib.gpz_ctx_set_pinv_mode(c, int(mode)))

    def timings(self, rank=0):
        """{stage: (total_ms, calls)} of one rank (HIP events on that device's stream)."""
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        calls = (C.c_int64 * cap)()
        n = self._lib.gpz_ctx_timings(self._lib.gpz_mgpu_ctx(self._h, rank), names, ms, calls, cap)
        return {names[i].decode(): (ms[i], int(calls[i])) for i in range(min(n, cap))}


def device_count():
    return int(_lib.load().gpz_device_count())


def _comm_info(call):
    info = (C.c_int32 * 4)()
    bus = C.create_string_buffer(64)
    _lib.check(call(info, bus, 64))
    return {"nccl_count": int(info[0]), "nccl_rank": int(info[1]), "nccl_device": int(info[2]), "hip_device": int(info[3]),
            "pci_bus_id": bus.value.decode()}


def rccl_origin():
    """Which RCCL the library bound to (dlopen at first use): '' when none was needed or found."""
    o = _lib.load().gpz_rccl_origin()
    return o.decode() if o else ""


_cache = {}


def _ctx_for(model, X, Y, Psi, omega, training, validation):
    """One context per closure, keyed on the identity of the model and of the data arrays.  The arrays are treated as
    immutable while cached (MATLAB's value semantics: a modified array is a new array there): editing X, Y, omega, the
    masks or the model IN PLACE between calls is not seen — call ``reset()`` after doing that.  The least recently
    created context is evicted once four are alive."""
    def ident(a):
        return None if a is None else (id(a), getattr(a, "shape", None))
    key = (id(model), model.m, model.d, model.k, model.method, bool(model.heteroscedastic),
           ident(X), ident(Y), ident(Psi), ident(omega), ident(training), ident(validation))
    ctx = _cache.get(key)
    if ctx is None:
        if len(_cache) >= 4:
            old = _cache.pop(next(iter(_cache)))        # FIFO: dicts keep insertion order
            old[0].close()
        ctx = (GPzContext(model, X, Y, Psi, omega, training, validation), (X, Y, Psi, omega, training, validation))
        _cache[key] = ctx
    return ctx[0]


def reset():
    """Drop cached contexts (``clear global`` / new data)."""
    for ctx, _ in _cache.values():
        ctx.close()
    _cache.clear()
    _lib.load().gpz_release_cached_memory()          # and the device buffers the library keeps for its next call


def GPz(theta, model, X, Y, Psi=None, omega=None, training=None, validation=None, nargout=2):
    """[nlogML,grad,w,iSigma_w,PHI] = GPz(theta,model,X,Y,Psi,omega,training,validation)   (GPz.m:1).

    ``nargout`` <= 2 returns (nlogML, grad) and refreshes ``globals_``; > 2 returns
    (nlogML_partial, 0, w, iSigma_w[, PHI]) exactly like the early return at GPz.m:84-87."""
    if Y is None:                      # GPz.m:34-40
        return 0.0, 0.0, 0.0, 0.0
    ctx = _ctx_for(model, X, Y, Psi, omega, training, validation)
    if nargout <= 2:
        f, g = ctx.eval(theta)
        globals_.update(ctx.stats)
        return f, g
    w, iS, part = ctx.solve(theta)
    out = (part, 0.0, w, iS)
    if nargout >= 5:
        out = out + (ctx.phi(),)
    return out


def getPHI(X, Psi, theta, model, selection=None, device=0, want_N=False):
    """[PHI,Gamma,lnBeta_i,N] = getPHI(X,Psi,theta,model,selection)   (getPHI.m:1); Gamma is the expanded
    parameter array of getPHI.m:26-40 (pure reshaping of theta, done on the host).  Psi: n x d for the diagonal
    kinds, d x d x n for GC/VC (the layouts fixPsi.m produces); X may contain NaN (missing inputs)."""
    lib = _lib.load()
    X = np.asarray(X, dtype=np.float64)
    psi = None if Psi is None else np.asarray(Psi, dtype=np.float64)
    if selection is not None:
        sel = np.asarray(selection, dtype=bool)
        X = X[sel]                                                     # getPHI.m:14
        if psi is not None:
            psi = psi[:, :, sel] if psi.ndim == 3 else psi[sel]        # getPHI.m:16-22
    X = _f64(X, 2)
    psi_kind = 0
    if psi is not None:
        psi = np.asfortranarray(psi)
        psi_kind = _psi_kind(model, psi)
    theta = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
    ns = X.shape[0]
    PHI = np.empty((ns, model.m), order="F")
    lnB = np.empty((ns, model.k), order="F")
    N = np.empty((ns, model.m), order="F") if want_N else None
    ds = _desc(model, device)
    _lib.check(lib.gpz_phi(C.byref(ds), _lib.dptr(theta), _lib.dptr(X), ns, _lib.dptr(psi), psi_kind, _lib.dptr(PHI),
                           _lib.dptr(lnB), _lib.dptr(N)))
    out = (PHI, _expand_gamma(theta, model), lnB)
    return out + (N,) if want_N else out


def _expand_gamma(theta, model):
    m, d = model.m, model.d
    G = theta[m * d:m * d + model.g_dim]
    mt = model.method
    if mt == "GL":
        return np.full((m, d), G[0])
    if mt == "VL":
        return np.tile(G.reshape(m, 1), (1, d))
    if mt == "GD":
        return np.tile(G.reshape(1, d), (m, 1))
    if mt == "VD":
        return G.reshape((m, d), order="F")
    if mt == "GC":
        return np.repeat(G.reshape((d, d), order="F")[:, :, None], m, axis=2)
    return G.reshape((d, d, m), order="F")


def inv_logdet(X, device=0, return_info=False):
    """[Xi,logdet] = inv_logdet(X)   (inv_logdet.m:1-15) for symmetric X; info = singular values dropped by the
    truncation of inv_logdet.m:7-12 (0 = none), -1 = X not finite."""
    lib = _lib.load()
    A = _f64(X)
    m = A.shape[0]
    Xi = np.empty((m, m), order="F")
    ld = C.c_double()
    info = C.c_int32()
    _lib.check(lib.gpz_inv_logdet(_lib.dptr(A), m, device, _lib.dptr(Xi), C.byref(ld), C.byref(info)))
    if return_info:
        return Xi, ld.value, int(info.value)
    return Xi, ld.value


def Dxy(X, Y, device=0):
    """D = Dxy(X,Y)   (Dxy.m:1)."""
    lib = _lib.load()
    X = _f64(X, 2)
    Y = _f64(Y, 2)
    D = np.empty((X.shape[0], Y.shape[0]), order="F")
    _lib.check(lib.gpz_dxy(_lib.dptr(X), X.shape[0], _lib.dptr(Y), Y.shape[0], X.shape[1], device, _lib.dptr(D)))
    return D


def nan_groups(X, device=0):
    """Group id per row by NaN pattern, in first-occurrence order (the loop of getPHI.m:43-54)."""
    lib = _lib.load()
    X = _f64(X, 2)
    n, d = X.shape
    gid = np.empty(n, dtype=np.int32)
    ng = C.c_int32()
    _lib.check(lib.gpz_nan_groups(_lib.dptr(X), n, d, device, gid.ctypes.data_as(_lib.c_int32_p), C.byref(ng)))
    return gid, int(ng.value)


def predict(X, model, whichSet="best", Psi=None, selection=None, device=0, n_gpus=None):
    """[mu,sigma,nu,beta_i,gamma,PHI,w,iSigma_w] = predict(X,model,...)   (predict.m:1).  Rows are grouped by NaN
    pattern as predict.m:45-57 does; a group without missing values runs predictFull / predictNoisy, a group with
    missing values predictMissing / predictNoisyMissing (predictDiag.m:127-297, predictCov.m:134-337).
    n_gpus (0 = every GPU of the node): every group's rows are split into contiguous blocks over the GPUs
    (gpz_mgpu_predict; more blocks than GPUs = several blocks per GPU)."""
    lib = _lib.load()
    X = np.asarray(X, dtype=np.float64)
    psi = None if Psi is None else np.asarray(Psi, dtype=np.float64)
    if selection is not None:
        sel = np.asarray(selection, dtype=bool)
        X = X[sel]                                                   # predict.m:25
        if psi is not None:                                          # predict.m:27-33
            psi = psi[:, :, sel] if (model.method[1] == "C" and psi.ndim == 3) else psi[sel]
    st = model.sets[whichSet]                                        # predict.m:10-14
    Xn = _f64((X - model.muX) / model.sdX, 2)                        # predict.m:35-36
    theta = np.ascontiguousarray(np.asarray(st["theta"], dtype=np.float64).ravel())
    w = _f64(st["w"], 2)
    iS = np.asfortranarray(np.asarray(st["iSigma_w"], dtype=np.float64).reshape(model.m, model.m, model.k))
    ns, k, m = Xn.shape[0], model.k, model.m
    psin = None
    if psi is not None:
        from .host import fixPsi
        psin = np.asfortranarray(fixPsi(psi, ns, model.sdX, model.method))   # predict.m:43
    cube = psin is not None and psin.ndim == 3
    ds = _desc(model, device)
    mu = nu = beta_i = gamma = PHI = None            # allocated below unless the data is one group (then the outputs ARE the results)
    # predict.m:45-57: groups of identical NaN patterns.  The grouping itself is the library's (gpz_nan_groups, ids in first-
    # occurrence order as the reference's loop forms them; np.unique over the rows took a third of a 1e5-row predictFull); complete
    # data is one group and is passed through without gathering.
    if ns and np.isnan(Xn).any():
        gid, n_groups = nan_groups(Xn, device)
        order = np.argsort(gid, kind="stable")
        bounds = np.concatenate(([0], np.cumsum(np.bincount(gid, minlength=n_groups))))
        groups = [order[bounds[g]:bounds[g + 1]] for g in range(n_groups)]
    else:
        groups = [slice(None)] if ns else []
    for idx in groups:
        whole = isinstance(idx, slice)
        Xg = Xn if whole else _f64(Xn[idx], 2)
        ng = Xg.shape[0]
        first_missing = bool(np.isnan(Xg[0]).any())
        Pg = None if psin is None else (psin if whole else np.asfortranarray(psin[:, :, idx] if cube else psin[idx]))
        o_mu = np.empty((ng, k), order="F"); o_nu = np.empty((ng, k), order="F"); o_be = np.empty((ng, k), order="F")
        o_ga = np.zeros((ng, k), order="F"); o_ph = np.empty((ng, m), order="F")
        if n_gpus is not None:
            pri = st.get("priors")
            pri = np.full(m, 1.0 / m) if pri is None else np.ascontiguousarray(np.asarray(pri, dtype=np.float64).ravel())
            _lib.check(lib.gpz_mgpu_predict(C.byref(ds), int(n_gpus), None, _lib.dptr(theta), _lib.dptr(w), _lib.dptr(iS),
                                            _lib.dptr(pri), _lib.dptr(Xg), ng, _lib.dptr(Pg),
                                            0 if Pg is None else (2 if cube else 1), _lib.dptr(o_mu), _lib.dptr(o_nu),
                                            _lib.dptr(o_be), _lib.dptr(o_ga), _lib.dptr(o_ph)))
        elif not first_missing:
            if Pg is None:                                           # predictFull, gamma = 0 (predictDiag.m:74)
                _lib.check(lib.gpz_predict_full(C.byref(ds), _lib.dptr(theta), _lib.dptr(w), _lib.dptr(iS), _lib.dptr(Xg), ng,
                                                _lib.dptr(o_mu), _lib.dptr(o_nu), _lib.dptr(o_be), _lib.dptr(o_ph)))
            else:
                _lib.check(lib.gpz_predict_noisy(C.byref(ds), _lib.dptr(theta), _lib.dptr(w), _lib.dptr(iS), _lib.dptr(Xg), ng,
                                                 _lib.dptr(Pg), 2 if cube else 1, _lib.dptr(o_mu), _lib.dptr(o_nu),
                                                 _lib.dptr(o_be), _lib.dptr(o_ga), _lib.dptr(o_ph)))
        else:
            pri = st.get("priors")
            pri = np.full(m, 1.0 / m) if pri is None else np.ascontiguousarray(np.asarray(pri, dtype=np.float64).ravel())
            _lib.check(lib.gpz_predict_missing(C.byref(ds), _lib.dptr(theta), _lib.dptr(w), _lib.dptr(iS), _lib.dptr(pri),
                                               _lib.dptr(Xg), ng, _lib.dptr(Pg), 0 if Pg is None else (2 if cube else 1),
                                               _lib.dptr(o_mu), _lib.dptr(o_nu), _lib.dptr(o_be), _lib.dptr(o_ga),
                                               _lib.dptr(o_ph)))
        if whole:
            mu, nu, beta_i, gamma, PHI = o_mu, o_nu, o_be, o_ga, o_ph
        else:
            if mu is None:
                mu = np.zeros((ns, k)); nu = np.zeros((ns, k)); beta_i = np.zeros((ns, k)); gamma = np.zeros((ns, k))
                PHI = np.zeros((ns, m))
            mu[idx] = o_mu; nu[idx] = o_nu; beta_i[idx] = o_be; gamma[idx] = o_ga; PHI[idx] = o_ph
    if mu is None:                                                   # no rows
        mu = np.zeros((ns, k)); nu = np.zeros((ns, k)); beta_i = np.zeros((ns, k)); gamma = np.zeros((ns, k)); PHI = np.zeros((ns, m))
    sigma = nu + beta_i + gamma                                      # predict.m:72
    mu = mu + model.muY                                              # predict.m:73
    return mu, sigma, nu, beta_i, gamma, PHI, w, iS


GPZ_PREDICT_FORCE_TILES = 1   # gpz_predictor_create flags (include/gpz_hip.h)
GPZ_DRAWS_MAX_COLUMNS = 16384   # n_draws * k per gpz_predictor_draws call (include/gpz_hip.h)
GPZ_STACK_MAX_GROUP_BINS = 4096   # n_groups * n_bins per gpz_predictor_stack call (include/gpz_hip.h)

StackResult = namedtuple("StackResult", ["hist", "sum_w", "sum_mu", "sum_mu2", "edges"])


class Predictor:
    """A trained model held on one GPU for prediction over any number of rows (gpz_predictor_*).

        with gpz_amd.Predictor(model, whichSet="best", device=0) as p:
            mu, sigma, nu, beta_i, gamma = p.predict(X, Psi=None, selection=None)
            mu, sigma, nu, beta_i, gamma, PHI = p.predict(X, Psi=Psi, return_phi=True)

    The same results as ``predict`` (normalisation, ``selection``, fixPsi, sigma = nu + beta_i + gamma, + muY), but the model's
    once-per-model work is done once and rows stream through tile-sized device buffers, so device memory does not grow with the
    number of rows and PHI only leaves the device when asked for.  Complete rows go through the handle (a fused kernel where
    ceil16(m + 2k) <= 256 and d <= 20, else the PHI kernel + T-GEMM per tile; rows with Psi per tile through predictNoisy, and on the
    handle's own tiles from ``predict_dev`` / ``draws`` / ``draws_dev`` with ``Psi=`` for a diagonal kind, d <= 20, k <= 8, m <= 256); rows with
    missing values are grouped by NaN pattern and go to gpz_predict_missing as in ``predict``.  Shapes are checked before the GPU is
    touched; the handle itself is created on first use.  ``route`` / ``info`` (tile rows, device bytes held, route 0 fused / 1 tiles,
    runs) describe it."""

    def __init__(self, model, whichSet="best", device=0, tile_rows=None, force_tiles=False):
        if whichSet not in getattr(model, "sets", {}):
            raise ValueError(f"whichSet {whichSet!r} is not one of the model's sets {sorted(getattr(model, 'sets', {}))}")
        m, d, k = int(model.m), int(model.d), int(model.k)
        method = str(model.method)
        if method not in ("GL", "VL", "GD", "VD", "GC", "VC"):
            raise ValueError(f"unknown method {method!r}")
        st = model.sets[whichSet]
        g_dim = {"GL": 1, "VL": m, "GD": d, "VD": m * d, "GC": d * d, "VC": d * d * m}[method]
        p = m * d + g_dim + m * k + k + (2 * m * k if model.heteroscedastic else 0)
        self._theta = np.ascontiguousarray(np.asarray(st["theta"], dtype=np.float64).ravel())
        if self._theta.size != p:
            raise ValueError(f"theta has {self._theta.size} entries, the model needs {p}")
        self._w = _f64(st["w"], 2)
        if self._w.shape != (m, k):
            raise ValueError(f"w must be {m} x {k}")
        iS = np.asarray(st["iSigma_w"], dtype=np.float64)
        if iS.size != m * m * k:
            raise ValueError(f"iSigma_w must be {m} x {m} x {k}")
        self._iS = np.asfortranarray(iS.reshape(m, m, k))
        pri = st.get("priors")
        self._priors = np.full(m, 1.0 / m) if pri is None else np.ascontiguousarray(np.asarray(pri, dtype=np.float64).ravel())
        if tile_rows is not None and (int(tile_rows) != tile_rows or tile_rows < 1):
            raise ValueError("tile_rows must be a positive integer or None")
        self.model, self.whichSet, self.device = model, whichSet, int(device)
        self._m, self._d, self._k, self._method = m, d, k, method
        self._tile_rows = 0 if tile_rows is None else int(tile_rows)
        self._flags = GPZ_PREDICT_FORCE_TILES if force_tiles else 0
        self._h = None
        self._closed = False
        self._lib = None

    def _check_open(self):
        if self._closed:
            raise RuntimeError("Predictor is closed")

    def _handle(self):
        self._check_open()
        if self._h is None:
            self._lib = _lib.load()
            ds = _desc(self.model, self.device)
            h = C.c_void_p()
            _lib.check(self._lib.gpz_predictor_create(C.byref(ds), _lib.dptr(self._theta), _lib.dptr(self._w), _lib.dptr(self._iS),
                                                      self._tile_rows, self._flags, C.byref(h)))
            self._h = h
        return self._h

    def close(self):
        if self._h is not None:
            self._lib.gpz_predictor_destroy(self._h)
            self._h = None
        self._closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def route(self):
        """Which kernels the handle runs (gpz_predictor_route), as one line of text."""
        h = self._handle()
        buf = C.create_string_buffer(256)
        n = self._lib.gpz_predictor_route(h, buf, 256)
        if n >= 256:                                                     # a long factor list after draws: the whole text
            buf = C.create_string_buffer(n + 1)
            self._lib.gpz_predictor_route(h, buf, n + 1)
        return buf.value.decode()

    @property
    def info(self):
        """(tile rows, device bytes held, route: 0 fused / 1 tiles, runs) of gpz_predictor_info."""
        h = self._handle()
        out = (C.c_int64 * 4)()
        _lib.check(self._lib.gpz_predictor_info(h, out))
        return tuple(int(v) for v in out)

    def _check_inputs(self, X, Psi, selection):
        d = self._d
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1 and d == 1:
            X = X[:, None]
        if X.ndim != 2 or X.shape[1] != d:
            raise ValueError(f"X must be n x {d}, got shape {X.shape}")
        n = X.shape[0]
        psi = None
        if Psi is not None:
            psi = np.asarray(Psi, dtype=np.float64)
            ok = ((psi.ndim == 1 and psi.shape[0] == n) or (psi.ndim == 2 and psi.shape[0] == n and psi.shape[1] in (1, d))
                  or (psi.ndim == 3 and psi.shape == (d, d, n)))
            if not ok:
                raise ValueError(f"Psi must be n x d, n x 1 or d x d x n (n = {n}, d = {d}), got shape {psi.shape}")
        if selection is not None:
            sel = np.asarray(selection)
            if sel.shape != (n,):
                raise ValueError(f"selection must be a mask of length {n}")
            sel = sel.astype(bool)
            X = X[sel]                                                   # predict.m:25
            if psi is not None:                                          # predict.m:27-33
                psi = psi[:, :, sel] if psi.ndim == 3 else psi[sel]
        return X, psi

    def _normalised(self, X):
        """(X - muX) / sdX (predict.m:35-36), one pass into the column-major layout."""
        Xn = np.empty(X.shape, order="F")
        np.subtract(X, self.model.muX, out=Xn)
        np.divide(Xn, self.model.sdX, out=Xn)
        return Xn

    def _run(self, Xg, Pg, cube, want_phi):
        ng, k, m = Xg.shape[0], self._k, self._m
        o = [np.empty((ng, k), order="F") for _ in range(4)]
        ph = np.empty((ng, m), order="F") if want_phi else None
        _lib.check(self._lib.gpz_predictor_run(self._h, _lib.dptr(Xg), ng, _lib.dptr(Pg), 0 if Pg is None else (2 if cube else 1),
                                               *(_lib.dptr(a) for a in o), _lib.dptr(ph)))
        return o[0], o[1], o[2], o[3], ph

    def predict(self, X, Psi=None, selection=None, return_phi=False):
        """mu, sigma, nu, beta_i, gamma [, PHI] of ``predict`` (predict.m:1) for the rows of X (n x d, not normalised)."""
        self._check_open()
        model, k, m = self.model, self._k, self._m
        X, psi = self._check_inputs(X, Psi, selection)
        Xn = self._normalised(X)
        ns = Xn.shape[0]
        psin = None
        if psi is not None:
            from .host import fixPsi
            psin = np.asfortranarray(fixPsi(psi, ns, model.sdX, model.method))   # predict.m:43
        cube = psin is not None and psin.ndim == 3
        if ns == 0:
            z = np.zeros((0, k))
            out = (z + model.muY, z.copy(), z.copy(), z.copy(), z.copy())
            return out + (np.zeros((0, m)),) if return_phi else out
        self._handle()
        if np.isnan(Xn.sum()) and np.isnan(Xn).any():                    # predict.m:45-57: groups of identical NaN patterns
            gid, n_groups = nan_groups(Xn, self.device)
            order = np.argsort(gid, kind="stable")
            bounds = np.concatenate(([0], np.cumsum(np.bincount(gid, minlength=n_groups))))
            groups = [order[bounds[g]:bounds[g + 1]] for g in range(n_groups)]
            mu = np.zeros((ns, k)); nu = np.zeros((ns, k)); beta_i = np.zeros((ns, k)); gamma = np.zeros((ns, k))
            PHI = np.zeros((ns, m)) if return_phi else None
            ds = _desc(model, self.device)
            for idx in groups:
                Xg = _f64(Xn[idx], 2)
                Pg = None if psin is None else np.asfortranarray(psin[:, :, idx] if cube else psin[idx])
                if not np.isnan(Xg[0]).any():
                    r = self._run(Xg, Pg, cube, return_phi)
                else:
                    ng = Xg.shape[0]
                    r = [np.empty((ng, k), order="F") for _ in range(4)] + [np.empty((ng, m), order="F")]
                    _lib.check(self._lib.gpz_predict_missing(C.byref(ds), _lib.dptr(self._theta), _lib.dptr(self._w),
                                                             _lib.dptr(self._iS), _lib.dptr(self._priors), _lib.dptr(Xg), ng,
                                                             _lib.dptr(Pg), 0 if Pg is None else (2 if cube else 1),
                                                             *(_lib.dptr(a) for a in r)))
                mu[idx] = r[0]; nu[idx] = r[1]; beta_i[idx] = r[2]; gamma[idx] = r[3]
                if return_phi:
                    PHI[idx] = r[4]
        else:                                                            # complete rows: no gather copy
            mu, nu, beta_i, gamma, PHI = self._run(Xn, psin, cube, return_phi)
        sigma = nu + beta_i + gamma                                      # predict.m:72
        mu = mu + model.muY                                              # predict.m:73
        out = (mu, sigma, nu, beta_i, gamma)
        return out + (PHI,) if return_phi else out

    def draws(self, X, n_draws, seed=0, Z=None, selection=None, Psi=None):
        """Posterior draws of the predictive mean (gpz_predictor_draws): an array of shape (n_draws, n, k) whose draws[s] has the shape
        and meaning of ``predict``'s mu (normalisation, ``selection``, + muY) under one draw w_s ~ N(w, iSigma_w) of the weights, the
        same draw for every row.  The spread of an aggregate of the rows across draws (a bin's mean redshift, a stacked n(z)) is its
        error from the finite training set, cross-row covariance included; y-draws add sqrt(beta_i) times independent normals per row.
        With ``Psi`` (a host array as ``predict`` takes it; gpz_predictor_draws_noisy) draws[s] is ``predict(X, Psi=Psi)``'s mu under draw
        s, E_x[PHI] w_s + muY: the mean is linear in the weights, so this is exact.  Psi needs a model inside predict_noisy_fits (a
        diagonal kind, d <= 20, k <= 8, m <= 256), else ValueError.

        ``seed`` (an integer in [0, 2^64)) selects the standard normals, generated on the device from Philox4x32-10: draw s of a seed
        is the same on every call and for every n_draws > s.  ``Z`` (m x n_draws x k, or m x n_draws when k = 1) gives them instead;
        ``Z = eye(m)`` with n_draws = m makes (draws - mu) an exact square root of the joint covariance of the rows' means.  Complete
        rows only: rows with NaN are refused.  At most n_draws * k = 16384 columns per call."""
        self._check_open()
        model, k = self.model, self._k
        X, psi = self._check_inputs(X, Psi, selection)
        nbad = int(np.isnan(X).any(axis=1).sum()) if X.size else 0
        if nbad:
            raise ValueError(f"X has {nbad} rows with missing values (NaN): draws are for complete rows")
        if psi is not None:
            self._check_noisy_model("draws", draws=True)
            if not np.all(np.isfinite(psi)) or np.any(psi < 0):
                raise ValueError("Psi must be finite and >= 0")
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 1)
        ns = X.shape[0]
        F = np.empty((ns, k, n_draws), order="F")                        # column-major ns x k x n_draws, as the C entry writes it
        if ns:
            Xn = self._normalised(X)
            psin = None
            if psi is not None:
                from .host import fixPsi
                psin = np.asfortranarray(fixPsi(psi, ns, model.sdX, model.method))   # predict.m:43: n x d for a diagonal kind
            h = self._handle()
            if psin is None:
                _lib.check(self._lib.gpz_predictor_draws(h, _lib.dptr(Xn), ns, n_draws, int(seed), _lib.dptr(z), _lib.dptr(F)))
            else:
                _lib.check(self._lib.gpz_predictor_draws_noisy(h, _lib.dptr(Xn), ns, _lib.dptr(psin), n_draws, int(seed), _lib.dptr(z),
                                                               _lib.dptr(F)))
        out = F.transpose(2, 0, 1)                                       # (n_draws, n, k) view
        out += np.asarray(model.muY, dtype=np.float64).reshape(k)        # predict.m:73
        return out

    def stack(self, X, edges, n_draws=0, seed=0, Z=None, groups=None, n_groups=None, weights=None, selection=None):
        """Stacked predictive densities on the device (gpz_predictor_stack): the n(z) of every group of rows under the posterior-mean
        weights and under each of ``n_draws`` weight draws, without any per-row result leaving the GPU.

        ``edges`` (B + 1 strictly increasing values in the units of y, the same for every output) are the bins; ``groups`` an integer
        label per row in [-1, n_groups) (-1 leaves the row out; default: one group; ``n_groups`` defaults to max label + 1);
        ``weights`` a weight >= 0 per row (default 1).  Column 0 uses ``predict``'s mu and sigma, column 1 + s uses ``draws``' draw s
        (same ``seed`` / ``Z``) with the noise variance beta_i as its width.  Returns a StackResult:

            hist     (1 + n_draws, G, k, B)   sum over the group's rows of weight * (normal mass of the row in the bin)
            sum_w    (G,)                     sum of the weights
            sum_mu   (1 + n_draws, G, k)      sum of weight * mu        (mu with muY, as ``predict`` returns it)
            sum_mu2  (1 + n_draws, G, k)      sum of weight * mu^2
            edges    (B + 1,)

        ``sum_mu / sum_w`` is a group's mean under a column, and the spread of ``hist[1:]`` or of that mean over the draws is the error
        from the finite training set.  Mass outside [edges[0], edges[-1]] is not counted.  Normalisation and ``selection`` (applied
        to the rows, labels and weights alike) as in ``predict``.  Complete, noise-free rows only.  Every field but ``edges`` is a plain
        sum over rows, so the results of several calls add: a catalogue read in chunks is a loop over ``stack`` and a ``+=`` per field.
        The same call on the same handle returns the same bits every time; another ``tile_rows`` may change the last ones."""
        return self._stack_host(X, None, edges, n_draws, seed, Z, groups, n_groups, weights, selection)

    def stack_noisy(self, X, Psi, edges, n_draws=0, seed=0, Z=None, groups=None, n_groups=None, weights=None, selection=None):
        """``stack`` for rows with input noise (gpz_predictor_stack_noisy): ``Psi`` is the rows' input-noise variances as a host array of
        shape (n, d), (n, 1) or (n,) (through ``fixPsi``; a d x d x n cube is refused), everything else as for ``stack``.  Column 0 uses
        ``predict_dev(X, Psi=Psi)``'s mu and sigma = (nu + beta_i) + gamma.  Column 1 + s uses ``draws(X, ..., Psi=Psi)``'s draw s and
        the width beta_i + max(gamma_s, 0), where gamma_s is predictNoisy's gamma under the weights of draw s, the variance of
        PHI(x) w_s over the input noise (``draws_dev(..., Psi=Psi, return_gamma=True)`` returns it).  Needs a model inside
        predict_noisy_fits (a diagonal kind, d <= 20, k <= 8, m <= 256) on the fused route, else ValueError.  ``selection`` applies to
        rows, Psi, labels and weights alike.  Returns a StackResult with the bits of ``stack_noisy_dev`` on the same handle and rows."""
        if Psi is None:
            raise ValueError("stack_noisy needs Psi: noise-free rows go to Predictor.stack")
        return self._stack_host(X, Psi, edges, n_draws, seed, Z, groups, n_groups, weights, selection)

    def _stack_host(self, X, Psi, edges, n_draws, seed, Z, groups, n_groups, weights, selection):
        """``stack`` (Psi None) and ``stack_noisy``: the checks, all before the library is loaded, then the entry."""
        self._check_open()
        n_all = np.asarray(X).shape[0] if np.ndim(X) else 0             # rows before the selection: labels and weights go with them
        if Psi is not None and np.ndim(Psi) == 3:
            raise ValueError("stack_noisy takes Psi as n x d, n x 1 or n variances: a d x d x n cube is for the covariance kinds, "
                             "which are outside predict_noisy_fits")
        X, psi = self._check_inputs(X, Psi, selection)
        sel = None if selection is None else np.asarray(selection).astype(bool)
        nbad = int(np.isnan(X).any(axis=1).sum()) if X.size else 0
        if nbad:
            raise ValueError(f"X has {nbad} rows with missing values (NaN): stacks are for complete rows")
        if psi is not None:
            self._check_noisy_model("stack_noisy", draws=True)
            if not np.all(np.isfinite(psi)) or np.any(psi < 0):
                raise ValueError("Psi must be finite and >= 0")
        e, B = self._check_edges(edges)
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 0)
        ns = X.shape[0]
        lab = None
        if groups is not None:
            ga = np.asarray(groups)
            if ga.shape != (n_all,) or ga.dtype.kind not in "iu":
                raise ValueError(f"groups must be {n_all} integer labels")
            if sel is not None:
                ga = ga[sel]
            top = int(ga.max()) + 1 if ga.size else 0
            if n_groups is None:
                n_groups = max(top, 1)
            if ga.size and int(ga.min()) < -1:
                raise ValueError("groups must be labels in [-1, n_groups)")
        elif n_groups is None:
            n_groups = 1
        if isinstance(n_groups, (bool, np.bool_)) or not isinstance(n_groups, (int, np.integer)) or n_groups < 1:
            raise ValueError(f"n_groups must be a positive integer, got {n_groups!r}")
        G = int(n_groups)
        if groups is not None:
            if ga.size and int(ga.max()) >= G:
                raise ValueError(f"groups must be labels in [-1, n_groups) with n_groups = {G}, got {int(ga.max())}")
            lab = np.ascontiguousarray(ga, dtype=np.int32)
        wt = None
        if weights is not None:
            wa = np.asarray(weights, dtype=np.float64)
            if wa.shape != (n_all,):
                raise ValueError(f"weights must be {n_all} values")
            if sel is not None:
                wa = wa[sel]
            if not np.all(np.isfinite(wa)) or np.any(wa < 0):
                raise ValueError("weights must be finite and >= 0")
            wt = np.ascontiguousarray(wa)
        if G * B > GPZ_STACK_MAX_GROUP_BINS:
            raise ValueError(f"n_groups * bins = {G * B} is over the limit of {GPZ_STACK_MAX_GROUP_BINS} per call")
        hist, sum_w, sum_mu, sum_mu2 = self._stack_arrays(n_draws, G, B)
        if ns:
            Xn = self._normalised(X)
            muY = self._norm_vectors()[2]
            es = self._stack_edges(e, muY)
            tail = (n_draws, int(seed), _lib.dptr(z), _lib.dptr(es), B, None if lab is None else lab.ctypes.data_as(_lib.c_int32_p), G,
                    _lib.dptr(wt), _lib.dptr(hist), _lib.dptr(sum_w), _lib.dptr(sum_mu), _lib.dptr(sum_mu2),
                    _lib.dptr(muY))                                      # predict.m:73 inside the sums
            if psi is None:
                h = self._handle()
                _lib.check(self._lib.gpz_predictor_stack(h, _lib.dptr(Xn), ns, *tail))
            else:
                from .host import fixPsi
                psin = np.asfortranarray(fixPsi(psi, ns, self.model.sdX, self.model.method))   # predict.m:43: n x d for a diagonal kind
                h = self._handle()
                _lib.check(self._lib.gpz_predictor_stack_noisy(h, _lib.dptr(Xn), ns, _lib.dptr(psin), *tail))
        return StackResult(hist, sum_w, sum_mu, sum_mu2, e.copy())

    # ---- device-resident entries: the catalogue is a torch tensor on the handle's GPU, per-row results stay there -------------------
    def _check_dev_rows(self, X, selection, what):
        """X (and the mask) of a *_dev call by type, dtype and shape; nothing here touches a GPU.  Returns X as n x d."""
        import torch
        d = self._d
        if isinstance(X, np.ndarray):
            raise TypeError(f"{what}_dev takes a torch tensor on cuda:{self.device}; a NumPy array goes to Predictor.{what}")
        if not isinstance(X, torch.Tensor):
            raise TypeError(f"X must be a torch.Tensor on cuda:{self.device}, got {type(X).__name__}")
        if X.dtype not in (torch.float64, torch.float32):
            raise TypeError(f"X must be float64 or float32, got {X.dtype}")
        if X.dim() == 1 and d == 1:
            X = X[:, None]
        if X.dim() != 2 or X.shape[1] != d:
            raise ValueError(f"X must be n x {d}, got shape {tuple(X.shape)}")
        if selection is not None:
            if not isinstance(selection, torch.Tensor) or selection.dtype != torch.bool:
                raise TypeError("selection must be a bool torch tensor on the same device as X")
            if tuple(selection.shape) != (X.shape[0],):
                raise ValueError(f"selection must be a mask of length {X.shape[0]}")
        return X

    def _check_noisy_model(self, what, draws=False):
        """predict_noisy_fits (k_predict_noisy.hip) for this model, before the GPU is touched."""
        if self._method[1] == "C" or self._d > 20 or self._k > 8 or self._m > 256:
            raise ValueError(f"{what} with Psi needs a model inside predict_noisy_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, "
                             f"k <= 8 and m <= 256; this one is {self._method} with d = {self._d}, m = {self._m}, k = {self._k} "
                             "(Predictor.predict takes Psi for every shape)")
        if draws and self._flags & GPZ_PREDICT_FORCE_TILES:
            raise ValueError(f"{what} with Psi needs the fused draws route: the predictor was made with force_tiles=True")

    def _check_missing_model(self, what, Psi):
        """predict_missing_fits (k_predict_missing.hip) for this model and call, before the GPU is touched."""
        if Psi is not None:
            raise ValueError(f"{what} with missing=True does not take Psi: rows with both input noise and missing values "
                             "(predictNoisyMissing) are not on the handle; Predictor.predict takes them")
        bad = []
        if self._method[1] == "C":
            bad.append(f"a diagonal kind (GL, VL, GD, VD), not {self._method}")
        if self._d > 20:
            bad.append(f"d <= 20, not d = {self._d}")
        if self._k > 8:
            bad.append(f"k <= 8, not k = {self._k}")
        if self._m > 256:
            bad.append(f"m <= 256, not m = {self._m}")
        if bad:
            raise ValueError(f"{what} with missing=True needs a model inside predict_missing_fits: " + "; ".join(bad) +
                             " (Predictor.predict takes rows with missing values for every shape)")
        if self._priors.shape != (self._m,):
            raise ValueError(f"the priors of the set must be {self._m} values, got {self._priors.size}")

    def _nan_groups_dev(self, X):
        """The rows of X (n x d, on the device) grouped by NaN pattern (predict.m:45-57) with torch on X's device: a list of
        (code, index tensor) with bit c of code set where dimension c is missing, in ascending code order; the index tensor lists
        the group's rows in their order in X, and is None when all rows share one pattern.  Only the distinct codes and the group
        sizes come to the host."""
        import torch
        bits = 2 ** torch.arange(self._d, device=X.device, dtype=torch.int64)
        code = (torch.isnan(X).to(torch.int64) * bits).sum(dim=1)
        codes, inv = torch.unique(code, return_inverse=True)
        if codes.numel() == 1:
            return [(int(codes[0]), None)]
        order = torch.argsort(inv, stable=True)
        bounds = [0] + torch.cumsum(torch.bincount(inv, minlength=codes.numel()), 0).tolist()
        return [(c, order[bounds[g]:bounds[g + 1]]) for g, c in enumerate(codes.tolist())]

    def _check_dev_psi(self, Psi, n, what):
        """Psi of a *_dev call by type, dtype and shape ((n, d), (n, 1) or (n,)); nothing here touches a GPU.  Returns it as n x 1 or n x d."""
        import torch
        d = self._d
        if isinstance(Psi, np.ndarray):
            raise TypeError(f"{what}_dev takes Psi as a torch tensor on cuda:{self.device}; a NumPy array goes to Predictor.{what}")
        if not isinstance(Psi, torch.Tensor):
            raise TypeError(f"Psi must be a torch.Tensor on cuda:{self.device}, got {type(Psi).__name__}")
        if Psi.dtype not in (torch.float64, torch.float32):
            raise TypeError(f"Psi must be float64 or float32, got {Psi.dtype}")
        if Psi.dim() == 1:
            Psi = Psi[:, None]
        if Psi.dim() != 2 or Psi.shape[0] != n or Psi.shape[1] not in (1, d):
            raise ValueError(f"Psi must be n x d, n x 1 or n (n = {n}, d = {d}), got shape {tuple(Psi.shape)}")
        return Psi

    def _check_dev_device(self, **tensors):
        """Every tensor of a *_dev call lives on cuda:<self.device> (checked after the shapes and before the GPU is touched)."""
        for name, t in tensors.items():
            if t is None:
                continue
            if not t.is_cuda:
                raise ValueError(f"{name} must be on cuda:{self.device}, it is on {t.device}: the host methods take host arrays")
            if t.device.index != self.device:
                raise ValueError(f"{name} is on {t.device}, the predictor on cuda:{self.device}")

    def _check_draw_args(self, n_draws, seed, Z, least):
        k, m = self._k, self._m
        if isinstance(n_draws, (bool, np.bool_)) or not isinstance(n_draws, (int, np.integer)) or n_draws < least:
            raise ValueError(f"n_draws must be a {'positive' if least else 'non-negative'} integer, got {n_draws!r}")
        n_draws = int(n_draws)
        if (1 - least + n_draws) * k > GPZ_DRAWS_MAX_COLUMNS:
            raise ValueError(f"{'n_draws' if least else '(1 + n_draws)'} * k = {(1 - least + n_draws) * k} is over the limit of "
                             f"{GPZ_DRAWS_MAX_COLUMNS} per call")
        if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        z = None
        if Z is not None:
            if n_draws == 0:
                raise ValueError("Z must be None when n_draws is 0")
            z = np.asarray(Z, dtype=np.float64)
            if k == 1 and z.shape == (m, n_draws):
                z = z[:, :, None]
            if z.shape != (m, n_draws, k):
                want = f"({m}, {n_draws}, {k})" + (f" or ({m}, {n_draws})" if k == 1 else "")
                raise ValueError(f"Z must have shape {want}, got {np.asarray(Z).shape}")
            z = np.asfortranarray(z)
        return n_draws, z

    @staticmethod
    def _check_edges(edges):
        """The bin edges of a stack call as a float64 vector, and the number of bins."""
        e = np.asarray(edges, dtype=np.float64)
        if e.ndim != 1 or e.size < 2:
            raise ValueError(f"edges must be a vector of at least 2 values, got shape {e.shape}")
        if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
            raise ValueError("edges must be finite and strictly increasing")
        return e, e.size - 1

    def _stack_arrays(self, n_draws, G, B):
        """The zeroed fields of a StackResult: hist, sum_w, sum_mu, sum_mu2."""
        C_, k = 1 + n_draws, self._k
        return np.zeros((C_, G, k, B)), np.zeros(G), np.zeros((C_, G, k)), np.zeros((C_, G, k))

    @staticmethod
    def _stack_edges(e, muY):
        """The edges as the entry takes them: k x (B + 1), without muY as the entry's mu is."""
        return np.ascontiguousarray(e[None, :] - muY[:, None])

    def _norm_vectors(self):
        """model.muX, model.sdX (d values each) and model.muY (k values) as contiguous float64 host vectors."""
        def vec(a, n):
            a = np.asarray(a, dtype=np.float64).reshape(-1)
            return np.ascontiguousarray(np.broadcast_to(a, (n,)) if a.size == 1 else a.reshape(n))
        return vec(self.model.muX, self._d), vec(self.model.sdX, self._d), vec(self.model.muY, self._k)

    @staticmethod
    def _x_args(X):
        """(address, element type, rows, row stride, column stride) of gpz_predictor_*_dev: the tensor as it lies, never copied."""
        import torch
        return X.data_ptr(), 1 if X.dtype == torch.float32 else 0, X.shape[0], X.stride(0), X.stride(1)

    def _psi_args(self, Psi, n):
        """(address, element type, row stride, column stride) of Psi for gpz_predictor_*_noisy_dev: n x 1 is broadcast by a stride of 0."""
        import torch
        P = Psi.expand(n, self._d)                                       # a view: never a copy
        return P.data_ptr(), 1 if P.dtype == torch.float32 else 0, P.stride(0), P.stride(1)

    def predict_dev(self, X, selection=None, return_phi=False, Psi=None, missing=False):
        """``predict`` for a catalogue that is on the GPU already (gpz_predictor_run_dev): X is a float64 or float32 torch tensor of
        shape (n, d) on cuda:<device> with any strides (row-major as torch makes it, a transposed or sliced view: it is read as it lies,
        never copied), ``selection`` a bool tensor there.  Returns mu, sigma, nu, beta_i, gamma [, PHI] as float64 tensors of shape
        (n, k) [(n, m)] on the same device, column-major (``.T`` of a contiguous (k, n) tensor).  Same meaning and, for the same rows,
        the same bits as ``predict``: normalisation by model.muX / sdX, + muY, sigma = nu + beta_i + gamma.  No row and no result
        crosses to the host.  The call is ordered after the work queued on torch's current stream of that device (no synchronise is
        needed before it) and is complete when it returns.  Complete rows only: rows with NaN are refused (GpzError).
        ``Psi`` (gpz_predictor_run_noisy_dev): the rows' input-noise variances as a float64 or float32 tensor on the same device, of
        shape (n, d), (n, 1) or (n,), with any strides (read as it lies; one variance per row is broadcast, not copied).  The five
        tensors are then ``predict(X, Psi=Psi)``'s, gamma no longer zero, computed on the handle's tiles by k_predict_noisy_small; a
        row's results do not depend on the tile size or the row order.  It needs a model inside predict_noisy_fits (a diagonal kind,
        d <= 20, k <= 8, m <= 256) and does not return PHI; an element of Psi that is NaN, infinite or negative is refused (GpzError).
        ``missing=True`` (gpz_predictor_run_missing_dev): rows with NaN are taken instead of refused.  The rows are grouped by NaN
        pattern with torch on the device; complete rows get exactly what they get without the keyword, every other group
        predictMissing (predictDiag.m:127-209) on the handle's tiles with the priors of the set (1 / m without any), gamma > 0 there.
        It needs a model inside predict_missing_fits (a diagonal kind, d <= 20, k <= 8, m <= 256), takes neither Psi nor return_phi,
        and a row's results do not depend on the tile size, the row order or the other rows of the call.
        Type, dtype and shape are checked first, the device last, all before the GPU is touched."""
        import torch
        self._check_open()
        k, m = self._k, self._m
        X = self._check_dev_rows(X, selection, "predict")
        if missing:
            self._check_missing_model("predict_dev", Psi)
            if return_phi:
                raise ValueError("return_phi=True is not available with missing=True: Predictor.predict returns PHI for such rows")
        if Psi is not None:
            Psi = self._check_dev_psi(Psi, X.shape[0], "predict")
            if return_phi:
                raise ValueError("return_phi=True is not available with Psi on the device: Predictor.predict returns PHI for noisy rows")
            self._check_noisy_model("predict_dev")
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        if selection is not None:
            X = X[selection]                                             # predict.m:25
            if Psi is not None:
                Psi = Psi[selection]                                     # predict.m:27-33
        n = X.shape[0]
        # the tensors are referenced by this frame for the whole call, which returns when the device is done: no record_stream needed
        out = [torch.empty((k, n), dtype=torch.float64, device=X.device).T for _ in range(5)]
        PHI = torch.empty((m, n), dtype=torch.float64, device=X.device).T if return_phi else None
        if n:
            muX, sdX, muY = self._norm_vectors()
            h = self._handle()
            if missing:
                full, stream = (1 << self._d) - 1, torch.cuda.current_stream(X.device).cuda_stream
                for code, idx in self._nan_groups_dev(X):
                    Xg = X if idx is None else X[idx]
                    og = out if idx is None else [torch.empty((k, Xg.shape[0]), dtype=torch.float64, device=X.device).T for _ in range(5)]
                    if code == 0:
                        _lib.check(self._lib.gpz_predictor_run_dev(h, *self._x_args(Xg), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                                   *(t.data_ptr() for t in og), None, stream))
                    else:
                        _lib.check(self._lib.gpz_predictor_run_missing_dev(h, *self._x_args(Xg), _lib.dptr(muX), _lib.dptr(sdX),
                                                                           _lib.dptr(muY), _lib.dptr(self._priors), full & ~code,
                                                                           *(t.data_ptr() for t in og), stream))
                    if idx is not None:
                        for t, g in zip(out, og):
                            t[idx] = g
            elif Psi is None:
                _lib.check(self._lib.gpz_predictor_run_dev(h, *self._x_args(X), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                           *(t.data_ptr() for t in out), None if PHI is None else PHI.data_ptr(),
                                                           torch.cuda.current_stream(X.device).cuda_stream))
            else:
                sd2 = np.ascontiguousarray(sdX ** 2)                     # fixPsi.m: Psi ./ sdX.^2
                _lib.check(self._lib.gpz_predictor_run_noisy_dev(h, *self._x_args(X), *self._psi_args(Psi, n), _lib.dptr(muX),
                                                                 _lib.dptr(sdX), _lib.dptr(sd2), _lib.dptr(muY),
                                                                 *(t.data_ptr() for t in out),
                                                                 torch.cuda.current_stream(X.device).cuda_stream))
        return tuple(out) + (PHI,) if return_phi else tuple(out)

    def draws_dev(self, X, n_draws, seed=0, Z=None, selection=None, Psi=None, missing=False, return_gamma=False):
        """``draws`` for a catalogue on the GPU (gpz_predictor_draws_dev): X and ``selection`` as for ``predict_dev``, ``n_draws``,
        ``seed`` and ``Z`` (a host array: it is m x n_draws x k) as for ``draws``.  Returns a float64 tensor of shape (n_draws, n, k) on
        the device, a view of the column-major n x k x n_draws buffer, with the bits of ``draws`` for the same rows.  Any statistic of
        the draws is then a torch reduction over it; nothing comes to the host unless asked.  ``Psi`` as for ``predict_dev``
        (gpz_predictor_draws_noisy_dev): the draws of ``predict(X, Psi=Psi)``'s mu, with the bits of ``draws(X, ..., Psi=Psi)``.
        ``missing=True`` as for ``predict_dev`` (gpz_predictor_draws_missing_dev): for a row with missing values draws[s] is
        PHI_missing w_s + muY, the mu of predictMissing under weight draw s; one weight draw serves all rows of all groups.
        ``return_gamma=True`` (with ``Psi``; gpz_predictor_draws_gamma_noisy_dev) returns ``(F, Gam)``: Gam is a float64 tensor of shape
        (n_draws, n, k), predictNoisy's gamma under the weights of draw s - the variance of PHI(x) w_s over the input noise, not
        clamped at 0.  A y-draw of row i under draw s has variance beta_i + Gam[s, i].
        ``return_gamma=True`` with ``missing=True`` (gpz_predictor_draws_gamma_missing_dev) returns the same pair with predictMissing's
        gamma under the weights of draw s: the variance of PHI(x) w_s over the missing dimensions of the row, exactly 0.0 on complete
        rows.  A row's Gam has the same bits for any tile size, row order, other rows of the call and any n_draws > s.  The scope is
        that of ``missing=True`` (diagonal kinds, d <= 20, k <= 8, m <= 256); ``Psi`` together with missing values, the covariance
        kinds and host arrays are not on the handle.  With neither ``Psi`` nor ``missing``, or with both, it is a ValueError."""
        import torch
        self._check_open()
        k = self._k
        X = self._check_dev_rows(X, selection, "draws")
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 1)
        if return_gamma and (Psi is None) != bool(missing):
            raise ValueError("return_gamma=True needs Psi or missing=True, and not both: gamma under a draw is the variance over the "
                             "input noise or over the missing dimensions")
        if missing:
            self._check_missing_model("draws_dev", Psi)
        if Psi is not None:
            Psi = self._check_dev_psi(Psi, X.shape[0], "draws")
            self._check_noisy_model("draws_dev", draws=True)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        if selection is not None:
            X = X[selection]
            if Psi is not None:
                Psi = Psi[selection]
        n = X.shape[0]
        # referenced by this frame for the whole (host-synchronous) call: no record_stream needed
        F = torch.empty((n_draws, k, n), dtype=torch.float64, device=X.device)   # column-major n x k x n_draws, as the C entry writes it
        Gam = torch.empty((n_draws, k, n), dtype=torch.float64, device=X.device) if return_gamma else None
        if n:
            muX, sdX, muY = self._norm_vectors()
            h = self._handle()
            if missing:
                full, stream = (1 << self._d) - 1, torch.cuda.current_stream(X.device).cuda_stream
                for code, idx in self._nan_groups_dev(X):
                    Xg = X if idx is None else X[idx]
                    Fg = F if idx is None else torch.empty((n_draws, k, Xg.shape[0]), dtype=torch.float64, device=X.device)
                    Gg = None
                    if return_gamma:                                     # complete rows: exactly 0.0
                        Gg = Gam if idx is None else torch.zeros((n_draws, k, Xg.shape[0]), dtype=torch.float64, device=X.device)
                    if code == 0:
                        _lib.check(self._lib.gpz_predictor_draws_dev(h, *self._x_args(Xg), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                                     n_draws, int(seed), _lib.dptr(z), Fg.data_ptr(), stream))
                        if return_gamma and idx is None:
                            Gam.zero_()
                    elif return_gamma:
                        _lib.check(self._lib.gpz_predictor_draws_gamma_missing_dev(h, *self._x_args(Xg), _lib.dptr(muX), _lib.dptr(sdX),
                                                                                   _lib.dptr(muY), _lib.dptr(self._priors), full & ~code,
                                                                                   n_draws, int(seed), _lib.dptr(z), Fg.data_ptr(),
                                                                                   Gg.data_ptr(), stream))
                    else:
                        _lib.check(self._lib.gpz_predictor_draws_missing_dev(h, *self._x_args(Xg), _lib.dptr(muX), _lib.dptr(sdX),
                                                                             _lib.dptr(muY), _lib.dptr(self._priors), full & ~code,
                                                                             n_draws, int(seed), _lib.dptr(z), Fg.data_ptr(), stream))
                    if idx is not None:
                        F[:, :, idx] = Fg
                        if return_gamma:
                            Gam[:, :, idx] = Gg
            elif Psi is None:
                _lib.check(self._lib.gpz_predictor_draws_dev(h, *self._x_args(X), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY), n_draws,
                                                             int(seed), _lib.dptr(z), F.data_ptr(),
                                                             torch.cuda.current_stream(X.device).cuda_stream))
            elif not return_gamma:
                sd2 = np.ascontiguousarray(sdX ** 2)                     # fixPsi.m: Psi ./ sdX.^2
                _lib.check(self._lib.gpz_predictor_draws_noisy_dev(h, *self._x_args(X), *self._psi_args(Psi, n), _lib.dptr(muX),
                                                                   _lib.dptr(sdX), _lib.dptr(sd2), _lib.dptr(muY), n_draws, int(seed),
                                                                   _lib.dptr(z), F.data_ptr(),
                                                                   torch.cuda.current_stream(X.device).cuda_stream))
            else:
                sd2 = np.ascontiguousarray(sdX ** 2)
                _lib.check(self._lib.gpz_predictor_draws_gamma_noisy_dev(h, *self._x_args(X), *self._psi_args(Psi, n), _lib.dptr(muX),
                                                                         _lib.dptr(sdX), _lib.dptr(sd2), _lib.dptr(muY), n_draws,
                                                                         int(seed), _lib.dptr(z), F.data_ptr(), Gam.data_ptr(),
                                                                         torch.cuda.current_stream(X.device).cuda_stream))
        if return_gamma:
            return F.permute(0, 2, 1), Gam.permute(0, 2, 1)
        return F.permute(0, 2, 1)                                        # (n_draws, n, k) view

    def stack_dev(self, X, edges, n_draws=0, seed=0, Z=None, groups=None, n_groups=None, weights=None, selection=None):
        """``stack`` for a catalogue on the GPU (gpz_predictor_stack_dev): X and ``selection`` as for ``predict_dev``; ``groups`` an
        integer tensor and ``weights`` a float tensor on the same device (converted there to int32 / float64), one value per row of X
        before the selection; everything else as for ``stack``.  Returns the same NumPy StackResult, with the bits of ``stack`` on the
        same handle and rows.  ``n_groups`` defaults to ``groups.max() + 1`` (one scalar read back).  Labels outside [-1, n_groups)
        and negative or non-finite weights are found on the device and refused with a GpzError, as rows with NaN are."""
        return self._stack_dev(X, None, edges, n_draws, seed, Z, groups, n_groups, weights, selection)

    def stack_noisy_dev(self, X, Psi, edges, n_draws=0, seed=0, Z=None, groups=None, n_groups=None, weights=None, selection=None):
        """``stack_noisy`` for a catalogue on the GPU (gpz_predictor_stack_noisy_dev): X, ``groups``, ``weights`` and ``selection`` as
        for ``stack_dev``, ``Psi`` as for ``predict_dev`` (float64 or float32, (n, d), (n, 1) or (n,), any strides).  Returns the same
        NumPy StackResult, with the bits of ``stack_noisy`` on the same handle and rows.  An element of Psi that is NaN, infinite or
        negative is found on the device and refused with a GpzError, as bad labels, weights and rows with NaN are."""
        if Psi is None:
            raise ValueError("stack_noisy_dev needs Psi: noise-free rows go to Predictor.stack_dev")
        return self._stack_dev(X, Psi, edges, n_draws, seed, Z, groups, n_groups, weights, selection)

    def stack_missing_dev(self, X, edges, n_draws=0, seed=0, Z=None, groups=None, n_groups=None, weights=None, selection=None):
        """``stack_dev`` for a catalogue with missing inputs (non-detections, NaN) on the GPU: arguments and result as for ``stack_dev``.
        The rows are grouped by NaN pattern with torch on the device, as ``predict_dev(X, missing=True)`` groups them.  The complete
        rows go to gpz_predictor_stack_dev (a catalogue without NaN gives ``stack_dev``'s bits), every other group with its labels and
        weights to gpz_predictor_stack_missing_dev, and the groups' results are added field by field in ascending order of the
        pattern code: the fields are plain sums, so the call is deterministic and equals the ``+=`` of the single-pattern calls bit
        for bit.  For a row with missing values column 0 uses ``predict_dev(X, missing=True)``'s mu and sigma = (nu + beta_i) + gamma,
        column 1 + s ``draws_dev(X, ..., missing=True)``'s draw s and the width beta_i + max(gamma_s, 0), where gamma_s is
        predictMissing's gamma under the weights of draw s (``draws_dev(..., missing=True, return_gamma=True)`` returns it).
        ``n_groups`` and the range of the labels are decided over all rows.  It needs a model inside predict_missing_fits (a diagonal
        kind, d <= 20, k <= 8, m <= 256), else ValueError; host arrays, ``Psi`` together with missing values and the covariance
        kinds are not on the handle (``Predictor.predict`` takes such rows)."""
        return self._stack_dev(X, None, edges, n_draws, seed, Z, groups, n_groups, weights, selection, missing=True)

    def _stack_dev(self, X, Psi, edges, n_draws, seed, Z, groups, n_groups, weights, selection, missing=False):
        """``stack_dev`` (Psi None), ``stack_noisy_dev`` and ``stack_missing_dev``: the checks, the device last, all before the GPU is
        touched; then the entry, or with ``missing`` one entry per NaN-pattern group."""
        import torch
        self._check_open()
        X = self._check_dev_rows(X, selection, "stack" if Psi is None else "stack_noisy")
        n_all = X.shape[0]
        if missing:
            self._check_missing_model("stack_missing_dev", None)
        if Psi is not None:
            Psi = self._check_dev_psi(Psi, n_all, "stack_noisy")
            self._check_noisy_model("stack_noisy_dev", draws=True)
        e, B = self._check_edges(edges)
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 0)
        if groups is not None:
            if not isinstance(groups, torch.Tensor) or groups.dtype.is_floating_point or groups.dtype.is_complex or \
                    groups.dtype == torch.bool or tuple(groups.shape) != (n_all,):
                raise ValueError(f"groups must be a tensor of {n_all} integer labels")
        if weights is not None:
            if not isinstance(weights, torch.Tensor) or not weights.dtype.is_floating_point or tuple(weights.shape) != (n_all,):
                raise ValueError(f"weights must be a float tensor of {n_all} values")
        if n_groups is not None and (isinstance(n_groups, (bool, np.bool_)) or not isinstance(n_groups, (int, np.integer))
                                     or n_groups < 1):
            raise ValueError(f"n_groups must be a positive integer, got {n_groups!r}")
        if n_groups is not None and int(n_groups) * B > GPZ_STACK_MAX_GROUP_BINS:
            raise ValueError(f"n_groups * bins = {int(n_groups) * B} is over the limit of {GPZ_STACK_MAX_GROUP_BINS} per call")
        self._check_dev_device(X=X, selection=selection, groups=groups, weights=weights, Psi=Psi)
        lab = wt = None
        if selection is not None:
            X = X[selection]
            if Psi is not None:
                Psi = Psi[selection]
        if groups is not None:
            lab = (groups if selection is None else groups[selection]).to(torch.int32).contiguous()
        if weights is not None:
            wt = (weights if selection is None else weights[selection]).to(torch.float64).contiguous()
        if n_groups is None:
            n_groups = max(int(lab.max()) + 1, 1) if lab is not None and lab.numel() else 1
            if n_groups * B > GPZ_STACK_MAX_GROUP_BINS:
                raise ValueError(f"n_groups * bins = {n_groups * B} is over the limit of {GPZ_STACK_MAX_GROUP_BINS} per call")
        G = int(n_groups)
        n = X.shape[0]
        hist, sum_w, sum_mu, sum_mu2 = self._stack_arrays(n_draws, G, B)
        if n:
            muX, sdX, muY = self._norm_vectors()
            es = self._stack_edges(e, muY)
            h = self._handle()
            # X, lab and wt are referenced by this frame for the whole (host-synchronous) call: no record_stream needed
            tail = (n_draws, int(seed), _lib.dptr(z), _lib.dptr(es), B, None if lab is None else lab.data_ptr(), G,
                    None if wt is None else wt.data_ptr(), _lib.dptr(hist), _lib.dptr(sum_w), _lib.dptr(sum_mu), _lib.dptr(sum_mu2),
                    _lib.dptr(muY), torch.cuda.current_stream(X.device).cuda_stream)
            if missing:
                full = (1 << self._d) - 1
                for code, idx in self._nan_groups_dev(X):                # ascending code: one fixed order of the sums
                    Xg, lg, wg = (X, lab, wt) if idx is None else (X[idx], None if lab is None else lab[idx],
                                                                   None if wt is None else wt[idx])
                    part = self._stack_arrays(n_draws, G, B)
                    gtail = (n_draws, int(seed), _lib.dptr(z), _lib.dptr(es), B, None if lg is None else lg.data_ptr(), G,
                             None if wg is None else wg.data_ptr(), *(_lib.dptr(a) for a in part), _lib.dptr(muY), tail[-1])
                    if code == 0:
                        _lib.check(self._lib.gpz_predictor_stack_dev(h, *self._x_args(Xg), _lib.dptr(muX), _lib.dptr(sdX), *gtail))
                    else:
                        _lib.check(self._lib.gpz_predictor_stack_missing_dev(h, *self._x_args(Xg), _lib.dptr(muX), _lib.dptr(sdX),
                                                                             _lib.dptr(self._priors), full & ~code, *gtail))
                    if idx is None:
                        hist, sum_w, sum_mu, sum_mu2 = part
                    else:
                        for total, a in zip((hist, sum_w, sum_mu, sum_mu2), part):
                            total += a
            elif Psi is None:
                _lib.check(self._lib.gpz_predictor_stack_dev(h, *self._x_args(X), _lib.dptr(muX), _lib.dptr(sdX), *tail))
            else:
                sd2 = np.ascontiguousarray(sdX ** 2)                     # fixPsi.m: Psi ./ sdX.^2
                _lib.check(self._lib.gpz_predictor_stack_noisy_dev(h, *self._x_args(X), *self._psi_args(Psi, n), _lib.dptr(muX),
                                                                   _lib.dptr(sdX), _lib.dptr(sd2), *tail))
        return StackResult(hist, sum_w, sum_mu, sum_mu2, e.copy())


def getPrior(X, Psi, theta, model, selection=None, device=0, return_iterations=False):
    """prior = getPrior(X,Sx,theta,model,set)   (getPrior.m:1); X / Psi already normalised as train.m passes them."""
    lib = _lib.load()
    X = np.asarray(X, dtype=np.float64)
    psi = None if Psi is None else np.asarray(Psi, dtype=np.float64)
    if selection is not None:
        sel = np.asarray(selection, dtype=bool)
        X = X[sel]
        if psi is not None:
            psi = psi[:, :, sel] if psi.ndim == 3 else psi[sel]
    X = _f64(X, 2)
    psi_kind = 0
    if psi is not None:
        psi = np.asfortranarray(psi)
        psi_kind = _psi_kind(model, psi)
    theta = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
    prior = np.empty(model.m)
    it = C.c_int32()
    ds = _desc(model, device)
    _lib.check(lib.gpz_prior(C.byref(ds), _lib.dptr(theta), _lib.dptr(X), X.shape[0], _lib.dptr(psi), psi_kind,
                             _lib.dptr(prior), C.byref(it)))
    return (prior, int(it.value)) if return_iterations else prior
