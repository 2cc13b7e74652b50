"""The streaming predictor: a trained model held on one GPU (gpz_predictor_* of the C ABI) behind ``Predictor``.

The methods ask one of four questions (run: the moments of ``predict``; draws; draws with gamma per draw; stack) of rows of one of four
kinds (clean, noisy: with Psi, missing: one NaN-pattern group, noisy_missing: such a group with Psi); noisy_cov is the noisy kind of a
covariance model (GC, VC), which has all four questions through methods of its own (``*_noisy_cov_dev``), and missing_cov the
missing kind of such a model, which has all four too (``predict_missing_cov_dev``, ``draws_missing_cov_dev`` with ``return_gamma``,
``stack_missing_cov_dev``); noisy_missing_cov is such a group with Psi, with all four as well
(``predict_noisy_missing_cov_dev``, ``draws_noisy_missing_cov_dev`` with ``return_gamma``, ``stack_noisy_missing_cov_dev``);
psi_cube is the noisy kind of a covariance model whose rows have a full d x d Psi each, the d x d x n cube, with all four
(``predict_psi_cube_dev``, ``draws_psi_cube_dev`` with ``return_gamma``, ``stack_psi_cube_dev``); psi_cube_missing is a NaN-pattern
group of such rows, with all four (``predict_psi_cube_missing_dev``, ``draws_psi_cube_missing_dev`` with ``return_gamma``,
``stack_psi_cube_missing_dev``).
``_DEV_ENTRIES`` names the device-resident entry of each pair, ``Predictor._dev_entry`` builds the arguments the entries of a pair
share, and ``Predictor._dev_groups`` is the one loop over the groups of a call; the host methods choose between two entries each by
whether Psi is there (``_HOST_ENTRIES``).  Everything numeric happens in the library; ``torch`` is only imported by the device methods.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from .api import _desc, _f64, nan_row_groups

GPZ_PREDICT_FORCE_TILES = 1   # gpz_predictor_create flags (include/gpz_hip.h)
GPZ_PREDICT_LARGE_M = 2       # complete rows with Psi stay on the handle up to GPZ_PREDICT_LARGE_M_MAX basis functions
GPZ_PREDICT_LARGE_M_MAX = 1024
GPZ_PREDICT_LARGE_M_MISSING = 4   # one NaN-pattern group of a diagonal kind stays on the handle up to the same limit
GPZ_DRAWS_MAX_COLUMNS = 16384   # n_draws * k per gpz_predictor_draws call (include/gpz_hip.h)
GPZ_STACK_MAX_GROUP_BINS = 4096   # n_groups * n_bins per gpz_predictor_stack call (include/gpz_hip.h)

StackResult = namedtuple("StackResult", ["hist", "sum_w", "sum_mu", "sum_mu2", "edges"])

# (question, row kind) -> the device-resident entry.  Complete rows have no gamma entry: their gamma is exactly 0.
_DEV_ENTRIES = {
    ("run", "clean"): "gpz_predictor_run_dev", ("run", "noisy"): "gpz_predictor_run_noisy_dev",
    ("run", "noisy_cov"): "gpz_predictor_run_noisy_cov_dev", ("draws", "noisy_cov"): "gpz_predictor_draws_noisy_cov_dev",
    ("run", "missing"): "gpz_predictor_run_missing_dev", ("run", "noisy_missing"): "gpz_predictor_run_noisy_missing_dev",
    ("run", "missing_cov"): "gpz_predictor_run_missing_cov_dev", ("draws", "missing_cov"): "gpz_predictor_draws_missing_cov_dev",
    ("draws", "clean"): "gpz_predictor_draws_dev", ("draws", "noisy"): "gpz_predictor_draws_noisy_dev",
    ("draws", "missing"): "gpz_predictor_draws_missing_dev", ("draws", "noisy_missing"): "gpz_predictor_draws_noisy_missing_dev",
    ("draws_gamma", "noisy"): "gpz_predictor_draws_gamma_noisy_dev", ("draws_gamma", "missing"): "gpz_predictor_draws_gamma_missing_dev",
    ("draws_gamma", "noisy_missing"): "gpz_predictor_draws_gamma_noisy_missing_dev",
    ("draws_gamma", "noisy_cov"): "gpz_predictor_draws_gamma_noisy_cov_dev", ("stack", "noisy_cov"): "gpz_predictor_stack_noisy_cov_dev",
    ("stack", "clean"): "gpz_predictor_stack_dev", ("stack", "noisy"): "gpz_predictor_stack_noisy_dev",
    ("stack", "missing"): "gpz_predictor_stack_missing_dev", ("stack", "noisy_missing"): "gpz_predictor_stack_noisy_missing_dev",
    ("draws_gamma", "missing_cov"): "gpz_predictor_draws_gamma_missing_cov_dev", ("stack", "missing_cov"): "gpz_predictor_stack_missing_cov_dev",
    ("run", "noisy_missing_cov"): "gpz_predictor_run_noisy_missing_cov_dev",
    ("draws", "noisy_missing_cov"): "gpz_predictor_draws_noisy_missing_cov_dev",
    ("draws_gamma", "noisy_missing_cov"): "gpz_predictor_draws_gamma_noisy_missing_cov_dev",
    ("stack", "noisy_missing_cov"): "gpz_predictor_stack_noisy_missing_cov_dev",
    ("run", "psi_cube"): "gpz_predictor_run_psi_cube_dev", ("draws", "psi_cube"): "gpz_predictor_draws_psi_cube_dev",
    ("draws_gamma", "psi_cube"): "gpz_predictor_draws_gamma_psi_cube_dev", ("stack", "psi_cube"): "gpz_predictor_stack_psi_cube_dev",
    ("run", "psi_cube_missing"): "gpz_predictor_run_psi_cube_missing_dev",
    ("draws", "psi_cube_missing"): "gpz_predictor_draws_psi_cube_missing_dev",
    ("draws_gamma", "psi_cube_missing"): "gpz_predictor_draws_gamma_psi_cube_missing_dev",
    ("stack", "psi_cube_missing"): "gpz_predictor_stack_psi_cube_missing_dev",
}
# (question, Psi there) -> the host entry
_HOST_ENTRIES = {("draws", False): "gpz_predictor_draws", ("draws", True): "gpz_predictor_draws_noisy",
                 ("stack", False): "gpz_predictor_stack", ("stack", True): "gpz_predictor_stack_noisy"}
# what the entries of one *_dev call share: the handle, torch's current stream and the normalisation vectors (host, float64)
_DevCall = namedtuple("_DevCall", ["h", "stream", "muX", "sdX", "sd2", "muY", "div"])


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
    runs) describe it.

    ``large_m=True`` (GPZ_PREDICT_LARGE_M) keeps complete rows with Psi on the handle up to m = 1024 where the limit is otherwise
    m = 256: the methods of a diagonal kind with ``Psi=`` (``predict_dev``, ``draws``, ``draws_dev``, ``stack_noisy``,
    ``stack_noisy_dev``), ``*_noisy_cov_dev`` and ``*_psi_cube_dev``.  The methods for rows with missing values keep m <= 256.  It
    costs nothing before the first call with Psi and changes nothing for m <= 256; beyond, the first call builds a table of
    m (m + 1) / 2 pair records (0.1 to 0.4 GB at m = 1024, and for GC / VC a temporary of (1 + d + d * d) doubles per pair while it
    is built) and every row costs m (m + 1) / 2 pair densities, 524 800 at m = 1024.  With ``force_tiles=True`` as well, the draws of
    a diagonal kind with Psi run as E_x[PHI] of a tile (k_predict_noisy_phi) against the weights on the T-GEMM at any m.

    ``large_m_missing=True`` (GPZ_PREDICT_LARGE_M_MISSING, and GPZ_PREDICT_LARGE_M with it for the complete rows of a catalogue with
    Psi) widens the methods for rows with missing values of a diagonal kind to m = 1024 as well: ``predict_dev(X, missing=True)``,
    ``draws_dev(X, n, missing=True[, return_gamma=True])``, ``stack_missing_dev``, ``predict_noisy_missing_dev``,
    ``draws_noisy_missing_dev`` and ``stack_noisy_missing_dev``; the ``*_missing_cov_dev``, ``*_noisy_missing_cov_dev`` and
    ``*_psi_cube_missing_dev`` methods of GC / VC keep m <= 256.  It changes nothing for m <= 256; beyond, the first call for a group
    builds the pattern's tables, m (m + 1) / 2 x ceil16(m) doubles of U (0.54 GB at m = 512, 4.3 GB at m = 1024), rebuilt in place
    when the pattern or the priors change, and every such row costs m (m + 1) / 2 x ceil16(m) multiply-adds on the f64 MFMA."""

    def __init__(self, model, whichSet="best", device=0, tile_rows=None, force_tiles=False, large_m=False, large_m_missing=False):
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
        self._flags = (GPZ_PREDICT_FORCE_TILES if force_tiles else 0) | (GPZ_PREDICT_LARGE_M if large_m else 0) | \
                      (GPZ_PREDICT_LARGE_M | GPZ_PREDICT_LARGE_M_MISSING if large_m_missing else 0)
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
        route, buf = self._lib.gpz_predictor_route, C.create_string_buffer(256)
        n = route(h, buf, 256)
        if n >= 256:                                                     # a long factor list after draws: the whole text
            buf = C.create_string_buffer(n + 1)
            route(h, buf, n + 1)
        return buf.value.decode()

    @property
    def info(self):
        """(tile rows, device bytes held, route: 0 fused / 1 tiles, runs) of gpz_predictor_info."""
        h = self._handle()
        out = (C.c_int64 * 4)()
        _lib.check(self._lib.gpz_predictor_info(h, out))
        return tuple(int(v) for v in out)

    # ---- the host methods: the catalogue is a NumPy array ------------------------------------------------------------------------------
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

    @staticmethod
    def _refuse_nan_rows(X, what):
        """draws and stacks on the host are for complete rows; ``what`` is "draws" or "stacks"."""
        nbad = int(np.isnan(X).any(axis=1).sum()) if X.size else 0
        if nbad:
            raise ValueError(f"X has {nbad} rows with missing values (NaN): {what} are for complete rows")

    @staticmethod
    def _refuse_bad_psi(psi):
        if not np.all(np.isfinite(psi)) or np.any(psi < 0):
            raise ValueError("Psi must be finite and >= 0")

    def _fixed_psi(self, psi, ns):
        """fixPsi of the selected rows' Psi (predict.m:43; n x d for a diagonal kind), column-major; None without Psi."""
        if psi is None:
            return None
        from .host import fixPsi
        return np.asfortranarray(fixPsi(psi, ns, self.model.sdX, self.model.method))

    def _normalised(self, X):
        """(X - muX) / sdX (predict.m:35-36), one pass into the column-major layout."""
        Xn = np.empty(X.shape, order="F")
        np.subtract(X, self.model.muX, out=Xn)
        np.divide(Xn, self.model.sdX, out=Xn)
        return Xn

    def _host_entry(self, question, Xn, psin):
        """The bound host entry of ``question`` and its leading arguments: the handle, the rows and, where there is one, Psi."""
        lead = [self._handle(), _lib.dptr(Xn), Xn.shape[0]] + ([] if psin is None else [_lib.dptr(psin)])
        return getattr(self._lib, _HOST_ENTRIES[question, psin is not None]), lead

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
        psin = self._fixed_psi(psi, ns)
        cube = psin is not None and psin.ndim == 3
        if ns == 0:
            z = np.zeros((0, k))
            out = (z + model.muY, z.copy(), z.copy(), z.copy(), z.copy())
            return out + (np.zeros((0, m)),) if return_phi else out
        self._handle()
        if np.isnan(Xn.sum()) and np.isnan(Xn).any():                    # predict.m:45-57: groups of identical NaN patterns
            groups = nan_row_groups(Xn, self.device)
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
        diagonal kind, d <= 20, k <= 8, m <= 256, or 1024 on a predictor made with large_m=True), else ValueError.

        ``seed`` (an integer in [0, 2^64)) selects the standard normals, generated on the device from Philox4x32-10: draw s of a seed
        is the same on every call and for every n_draws > s.  ``Z`` (m x n_draws x k, or m x n_draws when k = 1) gives them instead;
        ``Z = eye(m)`` with n_draws = m makes (draws - mu) an exact square root of the joint covariance of the rows' means.  Complete
        rows only: rows with NaN are refused.  At most n_draws * k = 16384 columns per call."""
        self._check_open()
        model, k = self.model, self._k
        X, psi = self._check_inputs(X, Psi, selection)
        self._refuse_nan_rows(X, "draws")
        if psi is not None:
            self._check_noisy_model("draws", draws=True)
            self._refuse_bad_psi(psi)
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 1)
        ns = X.shape[0]
        F = np.empty((ns, k, n_draws), order="F")                        # column-major ns x k x n_draws, as the C entry writes it
        if ns:
            fn, lead = self._host_entry("draws", self._normalised(X), self._fixed_psi(psi, ns))
            _lib.check(fn(*lead, n_draws, int(seed), _lib.dptr(z), _lib.dptr(F)))
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
        predict_noisy_fits (a diagonal kind, d <= 20, k <= 8, m <= 256, or 1024 with large_m=True) on the fused route (any route with large_m=True), else ValueError.  ``selection`` applies to
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
        self._refuse_nan_rows(X, "stacks")
        if psi is not None:
            self._check_noisy_model("stack_noisy", draws=True)
            self._refuse_bad_psi(psi)
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
        totals = self._stack_arrays(n_draws, G, B)
        if ns:
            Xn = self._normalised(X)
            muY = self._norm_vectors()[2]
            es = self._stack_edges(e, muY)
            fn, lead = self._host_entry("stack", Xn, self._fixed_psi(psi, ns))
            _lib.check(fn(*lead, n_draws, int(seed), _lib.dptr(z), _lib.dptr(es), B,
                          None if lab is None else lab.ctypes.data_as(_lib.c_int32_p), G, _lib.dptr(wt),
                          *(_lib.dptr(a) for a in totals), _lib.dptr(muY)))   # predict.m:73 inside the sums
        return StackResult(*totals, e.copy())

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
        large = bool(self._flags & GPZ_PREDICT_LARGE_M)
        if large and (self._method[1] == "C" or self._d > 20 or self._k > 8 or self._m > GPZ_PREDICT_LARGE_M_MAX):
            raise ValueError(f"{what} with Psi needs a model inside predict_noisy_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, "
                             f"k <= 8 and, with large_m=True, m <= {GPZ_PREDICT_LARGE_M_MAX}; this one is {self._method} with "
                             f"d = {self._d}, m = {self._m}, k = {self._k} (Predictor.predict takes Psi for every shape)")
        if large:
            return                                                       # (its draws with Psi run off the fused route too)
        if self._method[1] == "C" or self._d > 20 or self._k > 8 or self._m > 256:
            raise ValueError(f"{what} with Psi needs a model inside predict_noisy_fits: a diagonal kind (GL, VL, GD, VD), d <= 20, "
                             f"k <= 8 and m <= 256; this one is {self._method} with d = {self._d}, m = {self._m}, k = {self._k} "
                             "(Predictor.predict takes Psi for every shape)")
        if draws and self._flags & GPZ_PREDICT_FORCE_TILES:
            raise ValueError(f"{what} with Psi needs the fused draws route: the predictor was made with force_tiles=True")

    def _check_noisy_cov_shape(self, name):
        """predict_noisy_cov_fits (k_predict_noisy_cov.hip) for this model: m <= 256, or m <= 1024 on a predictor with large_m=True."""
        inside = 1 <= self._d <= 10 and 1 <= self._k <= 8
        if self._flags & GPZ_PREDICT_LARGE_M:
            if not (inside and 1 <= self._m <= GPZ_PREDICT_LARGE_M_MAX):
                raise ValueError(f"{name} needs a model inside predict_noisy_cov_fits: GC or VC, d <= 10, k <= 8 and, with large_m=True, "
                                 f"m <= {GPZ_PREDICT_LARGE_M_MAX}; this one is {self._method} with d = {self._d}, m = {self._m}, "
                                 f"k = {self._k} (Predictor.predict takes Psi for every shape)")
        elif not (inside and 1 <= self._m <= 256):
            raise ValueError(f"{name} needs a model inside predict_noisy_cov_fits: GC or VC, d <= 10, k <= 8 and m <= 256; this one is "
                             f"{self._method} with d = {self._d}, m = {self._m}, k = {self._k} (Predictor.predict takes Psi for every "
                             "shape)")

    def _check_missing_model(self, what, Psi, how=" with missing=True"):
        """predict_missing_fits (k_predict_missing.hip) for this model and call, before the GPU is touched."""
        if Psi is not None:
            raise ValueError(f"{what} with missing=True does not take Psi: rows with both input noise and missing values "
                             "(predictNoisyMissing) go to predict_noisy_missing_dev / draws_noisy_missing_dev")
        most = GPZ_PREDICT_LARGE_M_MAX if self._flags & GPZ_PREDICT_LARGE_M_MISSING else 256   # (predict_missing_large_fits)
        bad = [text for outside, text in ((self._method[1] == "C", f"a diagonal kind (GL, VL, GD, VD), not {self._method}"),
                                          (self._d > 20, f"d <= 20, not d = {self._d}"), (self._k > 8, f"k <= 8, not k = {self._k}"),
                                          (self._m > most, f"m <= {most}, not m = {self._m}")) if outside]
        if bad:
            raise ValueError(f"{what}{how} needs a model inside predict_missing_fits: " + "; ".join(bad) +
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

    @staticmethod
    def _selected(selection, X, Psi):
        """The rows and their Psi under the mask (predict.m:25-33): as they are without one.  A d x d x n cube has its rows last."""
        if selection is None:
            return X, Psi
        return X[selection], None if Psi is None else Psi[:, :, selection] if Psi.dim() == 3 else Psi[selection]

    def _dev_begin(self, device):
        """What the entries of one *_dev call share: the normalisation vectors (sd2 for fixPsi.m's Psi ./ sdX.^2), the handle and
        torch's current stream of the device, looked up once.  The call is ordered after the work queued on that stream."""
        import torch
        muX, sdX, muY = self._norm_vectors()
        h = self._handle()
        sd2 = np.ascontiguousarray(sdX ** 2)
        # fixPsi.m:36's divisors sdX' sdX of a Psi cube as the packed lower triangle, (r, c) at r (r + 1) / 2 + c; on the diagonal they
        # must be the sd2 that a variance per dimension is divided by, so that a cube of diagonals gets that route's bits
        r, c = np.tril_indices(self._d)
        div = np.ascontiguousarray(sdX[r] * sdX[c])
        assert np.array_equal(div[r == c], sd2), "the divisor triangle's diagonal must be sdX ** 2 bit for bit"
        return _DevCall(h, torch.cuda.current_stream(device).cuda_stream, muX, sdX, sd2, muY, div)

    def _dev_groups(self, X, missing, *per_row):
        """The one loop over the groups of a *_dev call: yields (code, idx, Xg, the per-row tensors of the group ...).  Without
        ``missing`` the rows are not looked at and the whole call is the one group (0, None, X, ...); rows with NaN are then refused by
        the entry.  With it the groups of ``_nan_groups_dev`` in ascending code order, gathered by idx (None, and nothing gathered,
        where all rows share one pattern).  A per-row tensor that is None stays None; a d x d x n cube has its rows last."""
        if not missing:
            yield (0, None, X) + per_row
            return
        for code, idx in self._nan_groups_dev(X):
            yield (code, idx, X if idx is None else X[idx]) + tuple(
                t if idx is None or t is None else t[:, :, idx] if t.dim() == 3 else t[idx] for t in per_row)

    @staticmethod
    def _merge(idx, whole, part, axis):
        """One group's results into the call's: written to the rows idx along ``axis`` of each tensor, or (axis None: the fields of a
        stack, plain sums) added to the totals.  The group that is the whole call (idx None) wrote the call's own arrays."""
        if idx is None:
            return
        for t, g in zip(whole, part):
            if axis is None:
                t += g
            elif g is not None:
                t[(slice(None),) * axis + (idx,)] = g

    def _dev_entry(self, question, call, code, Xg, Pg, cov=False):
        """The bound entry of ``_DEV_ENTRIES`` for one group and the arguments up to where the questions differ, in the order of
        include/gpz_hip.h: the handle, the rows, Psi for rows with one, muX, sdX, sd2 for rows with Psi; then muY and, for a group with
        missing values, the priors and the mask of the observed dimensions.  ``run`` and ``draws`` take muY there, in front of the
        priors; ``stack`` takes the priors straight after sdX and muY at the end of its own arguments.  ``cov``: complete rows with Psi
        of a covariance kind, whose entries take the noisy kind's arguments, or a group with missing values of such a kind, whose
        entries take the missing kind's (with Psi too: the noisy missing kind's).  ``cov == "cube"``: a d x d x n Psi, three strides
        and the divisor triangle in place of sd2, for complete rows and for a group with missing values; a group with nothing observed
        has no Psi to read and is the missing kind's of the model.  Returns (entry, arguments, row kind)."""
        cube = cov == "cube"
        if cube and code == (1 << self._d) - 1:
            Pg = None
        noisy = Pg is not None
        cube = cube and noisy
        kind = ("psi_cube_missing" if code else "psi_cube") if cube else \
            (("noisy_missing_cov" if cov else "noisy_missing") if noisy else "missing_cov" if cov else "missing") if code else \
            (("noisy_cov" if cov else "noisy") if noisy else "clean")
        lead = [call.h, *self._x_args(Xg)]
        if cube:
            import torch
            lead += [Pg.data_ptr(), 1 if Pg.dtype == torch.float32 else 0, Pg.stride(0), Pg.stride(1), Pg.stride(2)]
        elif noisy:
            lead += self._psi_args(Pg, Xg.shape[0])
        lead += [_lib.dptr(call.muX), _lib.dptr(call.sdX)]
        if noisy:
            lead.append(_lib.dptr(call.div if cube else call.sd2))
        if question != "stack":
            lead.append(_lib.dptr(call.muY))
        if code:
            lead += [_lib.dptr(self._priors), ((1 << self._d) - 1) & ~code]
        return getattr(self._lib, _DEV_ENTRIES[question, kind]), lead, kind

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
        d <= 20, k <= 8, m <= 256, or 1024 with large_m=True) and does not return PHI; an element of Psi that is NaN, infinite or negative is refused (GpzError).
        ``missing=True`` (gpz_predictor_run_missing_dev): rows with NaN are taken instead of refused.  The rows are grouped by NaN
        pattern with torch on the device; complete rows get exactly what they get without the keyword, every other group
        predictMissing (predictDiag.m:127-209) on the handle's tiles with the priors of the set (1 / m without any), gamma > 0 there.
        It needs a model inside predict_missing_fits (a diagonal kind, d <= 20, k <= 8, m <= 256), takes neither Psi
        (``predict_noisy_missing_dev`` does) nor return_phi, and a row's results do not depend on the tile size, the row order or the
        other rows of the call.
        Type, dtype and shape are checked first, the device last, all before the GPU is touched."""
        self._check_open()
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
        return self._moments_dev(X, Psi, selection, missing, return_phi)

    def _moments_dev(self, X, Psi, selection, missing, return_phi=False, cov=False):
        """The checked call of ``predict_dev``, ``predict_noisy_missing_dev`` and ``predict_noisy_cov_dev``: the selection, the
        result tensors and one entry per group of ``_dev_groups``."""
        import torch
        k, m = self._k, self._m
        X, Psi = self._selected(selection, X, Psi)
        n = X.shape[0]
        # the tensors are referenced by this frame for the whole call, which returns when the device is done: no record_stream needed
        out = [torch.empty((k, n), dtype=torch.float64, device=X.device).T for _ in range(5)]
        PHI = torch.empty((m, n), dtype=torch.float64, device=X.device).T if return_phi else None
        if n:
            call = self._dev_begin(X.device)
            for code, idx, Xg, Pg in self._dev_groups(X, missing, Psi):
                og = out if idx is None else [torch.empty((k, Xg.shape[0]), dtype=torch.float64, device=X.device).T for _ in range(5)]
                fn, lead, kind = self._dev_entry("run", call, code, Xg, Pg, cov)
                phi = [None if PHI is None else PHI.data_ptr()] if kind == "clean" else []   # the clean entry alone returns PHI
                _lib.check(fn(*lead, *(t.data_ptr() for t in og), *phi, call.stream))
                self._merge(idx, out, og, 0)
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
        that of ``missing=True`` (diagonal kinds, d <= 20, k <= 8, m <= 256); the covariance kinds and host arrays are not on the handle
        (gamma per draw over the input noise of a covariance kind is ``draws_noisy_cov_dev(..., return_gamma=True)``'s, over its
        missing dimensions ``draws_missing_cov_dev(..., return_gamma=True)``'s);
        gamma per draw for ``Psi`` together with missing values is ``draws_noisy_missing_dev(..., return_gamma=True)``'s.  With neither ``Psi`` nor ``missing``, or with both, it is a ValueError."""
        self._check_open()
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
        return self._draws_dev(X, Psi, selection, missing, n_draws, seed, z, return_gamma)

    def _draws_dev(self, X, Psi, selection, missing, n_draws, seed, z, return_gamma=False, cov=False):
        """The checked call of ``draws_dev``, ``draws_noisy_missing_dev`` and ``draws_noisy_cov_dev``: the selection, the result
        tensors and one entry per group of ``_dev_groups``, all under the one weight draw of (seed, z)."""
        import torch
        k = self._k
        X, Psi = self._selected(selection, X, Psi)
        n = X.shape[0]
        # referenced by this frame for the whole (host-synchronous) call: no record_stream needed
        F = torch.empty((n_draws, k, n), dtype=torch.float64, device=X.device)   # column-major n x k x n_draws, as the C entry writes it
        Gam = torch.empty((n_draws, k, n), dtype=torch.float64, device=X.device) if return_gamma else None
        if n:
            call = self._dev_begin(X.device)
            for code, idx, Xg, Pg in self._dev_groups(X, missing, Psi):
                Fg = F if idx is None else torch.empty((n_draws, k, Xg.shape[0]), dtype=torch.float64, device=X.device)
                Gg = Gam                                                 # None without return_gamma; complete rows: exactly 0.0
                if return_gamma and idx is not None:
                    Gg = torch.zeros((n_draws, k, Xg.shape[0]), dtype=torch.float64, device=X.device)
                gamma = return_gamma and (code != 0 or Pg is not None)   # complete rows have no gamma entry
                fn, lead, _ = self._dev_entry("draws_gamma" if gamma else "draws", call, code, Xg, Pg, cov)
                _lib.check(fn(*lead, n_draws, int(seed), _lib.dptr(z), Fg.data_ptr(), *([Gg.data_ptr()] if gamma else []), call.stream))
                if return_gamma and not gamma and idx is None:
                    Gam.zero_()
                self._merge(idx, (F, Gam), (Fg, Gg), 2)
        F = F.permute(0, 2, 1)                                           # (n_draws, n, k) view
        return (F, Gam.permute(0, 2, 1)) if return_gamma else F

    def _check_noisy_missing(self, what, X, Psi, selection, draws=False):
        """The checks the two methods for rows with Psi and missing values share, none of which touches a GPU: types, dtypes and shapes
        of X and Psi, the model's shape (predict_missing_fits), the priors; for the draws the route of the complete rows.  Returns X
        as n x d and Psi as n x 1 or n x d."""
        X = self._check_dev_rows(X, selection, what)
        if Psi is None:
            raise ValueError(f"{what}_noisy_missing_dev needs Psi: rows without input noise go to " +
                             ("stack_missing_dev(X, ...)" if what == "stack" else f"{what}_dev(X, missing=True)"))
        Psi = self._check_dev_psi(Psi, X.shape[0], what)
        self._check_missing_model(f"{what}_noisy_missing_dev", None, how="")
        if draws and self._flags & GPZ_PREDICT_FORCE_TILES:
            raise ValueError(f"{what}_noisy_missing_dev needs the fused draws route for its complete rows: the predictor was made with "
                             "force_tiles=True")
        return X, Psi

    def predict_noisy_missing_dev(self, X, Psi, selection=None):
        """``predict_dev`` for a catalogue whose rows have input noise and, some of them, missing values (a flux error in every band,
        NaN for the non-detections): X, ``selection`` and ``Psi`` (variances, (n, d), (n, 1) or (n,), float64 or float32, any strides)
        as for ``predict_dev``.  Returns mu, sigma, nu, beta_i, gamma as ``predict(X, Psi=Psi)`` does, as float64 tensors of shape
        (n, k) on the device.  The rows are grouped by NaN pattern with torch on the device: the complete rows go to
        gpz_predictor_run_noisy_dev and get the bits of ``predict_dev(X[full], Psi=Psi[full])``; every other group is gathered with its
        Psi and goes to gpz_predictor_run_noisy_missing_dev, predictNoisyMissing (predictDiag.m:211-297) on the handle's tiles with
        the priors of the set (1 / m without any).  Psi must be finite and >= 0 in a row's observed dimensions (else GpzError); in its
        missing dimensions it is not read, whatever it holds.  It needs a model inside predict_missing_fits (a diagonal kind,
        d <= 20, k <= 8, m <= 256), else ValueError; PHI, host arrays and the covariance kinds are not on
        this route (``Predictor.predict`` takes such rows for every shape).  A row's results do not depend on the tile size, the row
        order or the other rows of the call.  Type, dtype and shape are checked first, the device last, all before the GPU is
        touched."""
        self._check_open()
        X, Psi = self._check_noisy_missing("predict", X, Psi, selection)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        return self._moments_dev(X, Psi, selection, True)

    def draws_noisy_missing_dev(self, X, Psi, n_draws, seed=0, Z=None, selection=None, return_gamma=False):
        """``draws_dev`` for such a catalogue (gpz_predictor_draws_noisy_missing_dev): X, ``Psi`` and ``selection`` as for
        ``predict_noisy_missing_dev``, ``n_draws``, ``seed`` and ``Z`` as for ``draws_dev``.  Returns a float64 tensor of shape
        (n_draws, n, k) on the device: draws[s] is ``predict_noisy_missing_dev``'s mu under weight draw s, PHI w_s + muY with the PHI
        of predictNoisy or predictNoisyMissing - the mean is linear in the weights, so this is exact.  One weight draw serves all
        rows of all groups; complete rows get the bits of ``draws_dev(X[full], ..., Psi=Psi[full])``.  The predictor must not have
        been made with force_tiles=True.
        ``return_gamma=True`` returns ``(F, Gam)``: Gam (n_draws, n, k) is predictNoisyMissing's gamma under the weights of draw s,
        the variance of PHI(x) w_s over the input noise and the missing dimensions together, not clamped at 0
        (gpz_predictor_draws_gamma_noisy_missing_dev); complete rows get ``draws_dev(..., Psi=, return_gamma=True)``'s, the variance
        over their input noise, which is not zero.  A row's Gam has the same bits for any tile size, row order, other rows of the
        call and any n_draws > s."""
        self._check_open()
        X, Psi = self._check_noisy_missing("draws", X, Psi, selection, draws=True)
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 1)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        return self._draws_dev(X, Psi, selection, True, n_draws, seed, z, bool(return_gamma))

    def _check_noisy_cov(self, what, X, Psi, selection):
        """The checks the three methods for rows with Psi of a covariance kind share, none of which touches a GPU: X, then where such
        rows go when this is not their route (no Psi, a full Psi cube, a diagonal kind, a shape outside predict_noisy_cov_fits of
        k_predict_noisy_cov.hip), then Psi's type, dtype and shape.  Returns X as n x d and Psi as n x 1 or n x d."""
        X = self._check_dev_rows(X, selection, what)
        name = f"{what}_noisy_cov_dev"
        clean, diag = (f"{what}_dev(X, edges)", "stack_noisy_dev(X, Psi, edges)") if what == "stack" else \
            (f"{what}_dev(X)", f"{what}_dev(X, Psi=Psi)")
        if Psi is None:
            raise ValueError(f"{name} needs Psi: rows without input noise go to {clean}")
        if np.ndim(Psi) == 3 or (hasattr(Psi, "dim") and Psi.dim() == 3):
            raise ValueError(f"{name} takes Psi as n x d, n x 1 or n variances: a full d x d x n Psi stays on "
                             "Predictor.predict(X, Psi=Psi)")
        if self._method[1] != "C":
            raise ValueError(f"{name} is for the covariance kinds (GC, VC): a diagonal kind such as {self._method} goes to {diag}")
        self._check_noisy_cov_shape(name)
        if what == "stack" and isinstance(Psi, np.ndarray):               # (no host stack takes Psi of a covariance kind)
            raise TypeError(f"{name} takes Psi as a torch tensor on cuda:{self.device}; host arrays of a covariance kind stay on "
                            "Predictor.predict(X, Psi=Psi)")
        return X, self._check_dev_psi(Psi, X.shape[0], what)

    def predict_noisy_cov_dev(self, X, Psi, selection=None):
        """``predict_dev(X, Psi=Psi)`` for a covariance kind (GC, VC; gpz_predictor_run_noisy_cov_dev): X, ``selection`` and ``Psi``
        (variances per input dimension, (n, d), (n, 1) or (n,), float64 or float32, any strides) as for ``predict_dev``.  Returns mu,
        sigma, nu, beta_i, gamma as ``predict(X, Psi=Psi)`` does, as float64 tensors of shape (n, k) on the device: predictNoisy of
        predictCov.m on the handle's tiles by k_predict_noisy_cov_small, with the variances on the diagonal of each row's Psi as fixPsi
        puts them there.  A row's results do not depend on the tile size, the row order or the other rows of the call.  It needs a
        model inside predict_noisy_cov_fits (GC or VC, d <= 10, k <= 8, m <= 256, or 1024 with large_m=True), else ValueError; a full d x d x n Psi, PHI, host
        arrays and rows with missing values are not on this route (``Predictor.predict`` takes them); the stack of such rows is
        ``stack_noisy_cov_dev``'s and gamma per draw ``draws_noisy_cov_dev(..., return_gamma=True)``'s.  Rows
        with NaN and an element of Psi that is NaN, infinite or negative are refused (GpzError).  Type, dtype and shape are checked
        first, the device last, all before the GPU is touched."""
        self._check_open()
        X, Psi = self._check_noisy_cov("predict", X, Psi, selection)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        return self._moments_dev(X, Psi, selection, False, cov=True)

    def draws_noisy_cov_dev(self, X, Psi, n_draws, seed=0, Z=None, selection=None, return_gamma=False):
        """``draws_dev(X, ..., Psi=Psi)`` for a covariance kind (gpz_predictor_draws_noisy_cov_dev): X, ``Psi`` and ``selection`` as for
        ``predict_noisy_cov_dev``, ``n_draws``, ``seed`` and ``Z`` as for ``draws_dev``.  Returns a float64 tensor of shape
        (n_draws, n, k) on the device: draws[s] is ``predict_noisy_cov_dev``'s mu under weight draw s, E_x[PHI] w_s + muY - the mean is
        linear in the weights, so this is exact.  E_x[PHI] of a tile comes from k_predict_noisy_cov_phi and meets the draws' weights on
        the T-GEMM, whatever route the handle's noise-free draws take.
        ``return_gamma=True`` (gpz_predictor_draws_gamma_noisy_cov_dev) returns ``(F, Gam)``: F with the bits it has without the keyword,
        Gam a float64 tensor of shape (n_draws, n, k), predictNoisy's gamma of predictCov.m under the weights of draw s - the variance
        of PHI(x) w_s over the input noise, not clamped at 0 (k_predict_noisy_cov_gamma).  A y-draw of row i under draw s has variance
        beta_i + Gam[s, i].  A row's Gam has the same bits for any tile size, row order, other rows of the call and any n_draws > s."""
        self._check_open()
        X, Psi = self._check_noisy_cov("draws", X, Psi, selection)
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 1)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        return self._draws_dev(X, Psi, selection, False, n_draws, seed, z, bool(return_gamma), cov=True)

    def _check_psi_cube(self, what, X, Psi, selection):
        """The checks the three methods for rows with a d x d x n Psi of a covariance kind share, none of which touches a GPU, in the
        order of ``_check_noisy_cov``: X, then where such rows go when this is not their route (no Psi, a variance per dimension, a
        diagonal kind, a shape outside predict_noisy_cov_fits), then Psi's type, dtype and shape.  Returns X as n x d and Psi."""
        import torch
        X = self._check_dev_rows(X, selection, what)
        name, d, n = f"{what}_psi_cube_dev", self._d, X.shape[0]
        clean, diag = (f"{what}_dev(X, edges)", "stack_noisy_dev(X, Psi, edges)") if what == "stack" else \
            (f"{what}_dev(X)", f"{what}_dev(X, Psi=Psi)")
        if Psi is None:
            raise ValueError(f"{name} needs Psi: rows without input noise go to {clean}")
        ndim = Psi.dim() if hasattr(Psi, "dim") else np.ndim(Psi)
        if ndim in (1, 2):
            raise ValueError(f"{name} takes Psi as the d x d x n cube: n x d, n x 1 or n variances go to {what}_noisy_cov_dev")
        if self._method[1] != "C":
            raise ValueError(f"{name} is for the covariance kinds (GC, VC): fixPsi gives a diagonal kind such as {self._method} only "
                             f"the cube's diagonal, which goes to {diag}")
        self._check_noisy_cov_shape(name)
        if isinstance(Psi, np.ndarray):
            raise TypeError(f"{name} takes Psi as a torch tensor on cuda:{self.device}; host arrays stay on "
                            "Predictor.predict(X, Psi=Psi)")
        if not isinstance(Psi, torch.Tensor):
            raise TypeError(f"Psi must be a torch.Tensor on cuda:{self.device}, got {type(Psi).__name__}")
        if Psi.dtype not in (torch.float64, torch.float32):
            raise TypeError(f"Psi must be float64 or float32, got {Psi.dtype}")
        if tuple(Psi.shape) != (d, d, n):
            raise ValueError(f"Psi must be d x d x n (d = {d}, n = {n}; an n x d x d tensor goes in as .permute(1, 2, 0)), got shape "
                             f"{tuple(Psi.shape)}")
        return X, Psi

    def predict_psi_cube_dev(self, X, Psi, selection=None):
        """``predict_noisy_cov_dev`` for rows with a full input-noise covariance each (GC, VC; gpz_predictor_run_psi_cube_dev): ``Psi``
        is a float64 or float32 tensor of shape (d, d, n) on the device, the reference's cube (fixPsi.m, predictCov.m:109), with any
        strides - an (n, d, d) tensor under ``.permute(1, 2, 0)`` is read where it lies.  Only the lower triangle (row >= column) of
        each row's matrix is read and scanned; the upper triangle may hold anything.  Element (r, c) enters the kernels as
        double(Psi[r, c, i]) / (sdX[r] * sdX[c]), fixPsi.m:36's bits.  Returns mu, sigma, nu, beta_i, gamma as
        ``predict(X, Psi=Psi)`` does, float64 (n, k) on the device, from k_predict_psi_cube_small on the handle's tiles: the packed
        Cholesky of S + Psi_i per row and record.  A cube with zeros off the diagonal gives the bits of ``predict_noisy_cov_dev`` on
        its diagonal; a row's results do not depend on the tile size, the row order or the other rows of the call.  An element of a
        lower triangle that is NaN or infinite (itself or after its division), a negative diagonal element and rows with NaN in X are
        refused (GpzError), outputs untouched.  A matrix that passes this scan but is not positive semidefinite is the caller's error:
        that row's results are unspecified, and no other row is affected.  It needs a model inside predict_noisy_cov_fits (GC or VC,
        d <= 10, k <= 8, m <= 256, or 1024 with large_m=True), else ValueError; a diagonal kind takes the cube's diagonal through ``predict_dev(X, Psi=)``; rows
        with NaN together with a cube, PHI and host arrays stay on ``Predictor.predict``.  Type, dtype and shape are checked first,
        the device last, all before the GPU is touched."""
        self._check_open()
        X, Psi = self._check_psi_cube("predict", X, Psi, selection)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        return self._moments_dev(X, Psi, selection, False, cov="cube")

    def draws_psi_cube_dev(self, X, Psi, n_draws, seed=0, Z=None, selection=None, return_gamma=False):
        """``draws_noisy_cov_dev`` for such rows (gpz_predictor_draws_psi_cube_dev): X, ``Psi`` (d x d x n, its lower triangles read)
        and ``selection`` as for ``predict_psi_cube_dev``, everything else and the result as for ``draws_noisy_cov_dev``: draws[s] is
        ``predict_psi_cube_dev``'s mu under weight draw s, E_x[PHI] w_s + muY with E_x[PHI] from k_predict_psi_cube_phi.
        ``return_gamma=True`` (gpz_predictor_draws_gamma_psi_cube_dev) returns ``(F, Gam)``: Gam[s] is predictNoisy's gamma of
        predictCov.m under the weights of draw s, not clamped at 0 (k_predict_psi_cube_gamma).  A row's F and Gam have the same bits
        for any tile size, row order, other rows of the call and any n_draws > s; a matrix that is not positive semidefinite makes its
        own row's results unspecified and touches no other row."""
        self._check_open()
        X, Psi = self._check_psi_cube("draws", X, Psi, selection)
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 1)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        return self._draws_dev(X, Psi, selection, False, n_draws, seed, z, bool(return_gamma), cov="cube")

    def stack_psi_cube_dev(self, X, Psi, edges, n_draws=0, seed=0, Z=None, groups=None, n_groups=None, weights=None, selection=None):
        """``stack_noisy_cov_dev`` for such rows (gpz_predictor_stack_psi_cube_dev): X, ``Psi`` (d x d x n, its lower triangles read)
        and ``selection`` as for ``predict_psi_cube_dev``, everything else as for ``stack_dev``.  Returns a NumPy StackResult.  Column 0
        uses ``predict_psi_cube_dev``'s mu and that call's sigma = (nu + beta_i) + gamma, bit for bit; column 1 + s
        ``draws_psi_cube_dev``'s draw s and the width beta_i + max(gamma_s, 0), where gamma_s is that method's ``return_gamma=True``.
        The fields are plain sums over the rows, so calls over parts of a catalogue add.  Rows with NaN, a bad element of a lower
        triangle, a label outside [-1, n_groups) and a negative or non-finite weight are found on the device before the first tile and
        refused with a GpzError; a matrix that is not positive semidefinite makes its own row's contribution unspecified."""
        return self._stack_dev(X, Psi, edges, n_draws, seed, Z, groups, n_groups, weights, selection, cov="cube")

    def _check_psi_cube_missing(self, what, X, Psi, selection):
        """The checks the three methods for rows with a d x d x n Psi and missing values of a covariance kind share, none of which
        touches a GPU, in the order of ``_check_psi_cube``: X, then where such rows go when this is not their route (no Psi, a variance
        per dimension, a diagonal kind, a shape outside predict_missing_cov_fits), then Psi's type, dtype and shape and the priors.
        Returns X as n x d and Psi."""
        import torch
        name = f"{what}_psi_cube_missing_dev"
        if isinstance(X, np.ndarray):
            raise TypeError(f"{name} takes a torch tensor on cuda:{self.device}; a NumPy catalogue with a Psi cube and missing values "
                            "goes to Predictor.predict(X, Psi=Psi)")
        X = self._check_dev_rows(X, selection, what)
        d, n = self._d, X.shape[0]
        if Psi is None:
            raise ValueError(f"{name} needs Psi: rows of a covariance kind without input noise go to {what}_missing_cov_dev(X)")
        ndim = Psi.dim() if hasattr(Psi, "dim") else np.ndim(Psi)
        if ndim in (1, 2):
            raise ValueError(f"{name} takes Psi as the d x d x n cube: n x d, n x 1 or n variances go to "
                             f"{what}_noisy_missing_cov_dev(X, Psi)")
        if self._method[1] != "C":
            raise ValueError(f"{name} is for the covariance kinds (GC, VC): fixPsi gives a diagonal kind such as {self._method} only "
                             f"the cube's diagonal, which goes to {what}_noisy_missing_dev(X, Psi)")
        if not (1 <= d <= 10 and 1 <= self._k <= 8 and 1 <= self._m <= 256):
            raise ValueError(f"{name} needs a model inside predict_missing_cov_fits: GC or VC, d <= 10, k <= 8 and m <= 256; this one "
                             f"is {self._method} with d = {d}, m = {self._m}, k = {self._k} (Predictor.predict takes rows with a Psi "
                             "cube and missing values for every shape)")
        if isinstance(Psi, np.ndarray):
            raise TypeError(f"{name} takes Psi as a torch tensor on cuda:{self.device}; host arrays stay on "
                            "Predictor.predict(X, Psi=Psi)")
        if not isinstance(Psi, torch.Tensor):
            raise TypeError(f"Psi must be a torch.Tensor on cuda:{self.device}, got {type(Psi).__name__}")
        if Psi.dtype not in (torch.float64, torch.float32):
            raise TypeError(f"Psi must be float64 or float32, got {Psi.dtype}")
        if tuple(Psi.shape) != (d, d, n):
            raise ValueError(f"Psi must be d x d x n (d = {d}, n = {n}; an n x d x d tensor goes in as .permute(1, 2, 0)), got shape "
                             f"{tuple(Psi.shape)}")
        if self._priors.shape != (self._m,):
            raise ValueError(f"the priors of the set must be {self._m} values, got {self._priors.size} (Predictor.predict reports "
                             "the same for such rows)")
        return X, Psi

    def predict_psi_cube_missing_dev(self, X, Psi, selection=None):
        """``predict_noisy_missing_cov_dev`` for rows with a full input-noise covariance each (GC, VC;
        gpz_predictor_run_psi_cube_missing_dev): a catalogue with correlated input errors and, in some rows, missing values.  X and
        ``selection`` as for ``predict_dev``; ``Psi`` the d x d x n cube as for ``predict_psi_cube_dev`` (float64 or float32, any
        strides, element (r, c) entering as double(Psi[r, c, i]) / (sdX[r] * sdX[c])).  Returns mu, sigma, nu, beta_i, gamma as
        ``predict(X, Psi=Psi)`` does, float64 (n, k) on the device.  The rows are grouped by NaN pattern with torch on the device: the
        complete rows go to gpz_predictor_run_psi_cube_dev and get the bits of ``predict_psi_cube_dev`` on them alone, rows with
        nothing observed read no Psi and get the bits of ``predict_missing_cov_dev``, and every other group is gathered with its
        matrices and gets predictNoisyMissing of predictCov.m:233-337 on the handle's tiles (k_predict_psi_cube_missing_pairs) with the
        priors of the set.  Only the lower triangle of the observed x observed block of a row's matrix is read and scanned: there an
        element that is NaN or infinite (itself or after its division) or a negative diagonal element is refused (GpzError, outputs
        untouched); a missing row or column of the matrix is never read and may hold NaN.  A cube with zeros off the diagonal gives the
        bits of ``predict_noisy_missing_cov_dev`` on its diagonal.  A matrix that passes the scan but is not positive semidefinite is
        the caller's error: that row gets NaN, and no other row is affected.  It needs a model inside predict_missing_cov_fits (GC or
        VC, d <= 10, k <= 8, m <= 256), else ValueError; a diagonal kind takes the cube's diagonal through
        ``predict_noisy_missing_dev``, variances per dimension go to ``predict_noisy_missing_cov_dev``, and PHI and host arrays stay
        on ``Predictor.predict``.  A row's results do not depend on the tile size, the row order or the other rows of the call.  Type,
        dtype and shape are checked first, the device last, all before the GPU is touched."""
        self._check_open()
        X, Psi = self._check_psi_cube_missing("predict", X, Psi, selection)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        return self._moments_dev(X, Psi, selection, True, cov="cube")

    def draws_psi_cube_missing_dev(self, X, Psi, n_draws, seed=0, Z=None, selection=None, return_gamma=False):
        """``draws_noisy_missing_cov_dev`` for such rows (gpz_predictor_draws_psi_cube_missing_dev): X, ``Psi`` (d x d x n) and
        ``selection`` as for ``predict_psi_cube_missing_dev``, everything else and the result as for ``draws_noisy_missing_cov_dev``:
        draws[s] is ``predict_psi_cube_missing_dev``'s mu under weight draw s; one weight draw serves all rows of all groups, complete
        rows get the bits of ``draws_psi_cube_dev`` and rows with nothing observed those of ``draws_missing_cov_dev``.
        ``return_gamma=True`` (gpz_predictor_draws_gamma_psi_cube_missing_dev) returns ``(F, Gam)``: Gam[s] is predictNoisyMissing's
        gamma under the weights of draw s, not clamped at 0 (k_predict_psi_cube_missing_gamma).  A row's F and Gam have the same bits
        for any tile size, row order, other rows of the call and any n_draws > s."""
        self._check_open()
        X, Psi = self._check_psi_cube_missing("draws", X, Psi, selection)
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 1)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        return self._draws_dev(X, Psi, selection, True, n_draws, seed, z, bool(return_gamma), cov="cube")

    def stack_psi_cube_missing_dev(self, X, Psi, edges, n_draws=64, seed=0, Z=None, groups=None, n_groups=None, weights=None,
                                   selection=None):
        """``stack_noisy_missing_cov_dev`` for such rows (gpz_predictor_stack_psi_cube_missing_dev): X, ``Psi`` (d x d x n) and
        ``selection`` as for ``predict_psi_cube_missing_dev``, everything else as for ``stack_dev``; ``n_draws`` defaults to 64.  The
        complete rows go to gpz_predictor_stack_psi_cube_dev (a catalogue without NaN gives ``stack_psi_cube_dev``'s bits), rows with
        nothing observed to gpz_predictor_stack_missing_cov_dev, every other group with its matrices, labels and weights to
        gpz_predictor_stack_psi_cube_missing_dev, and the groups' results are added field by field in ascending order of the pattern
        code; one weight draw serves all groups.  For a row with missing values column 0 uses ``predict_psi_cube_missing_dev``'s mu
        and that call's sigma = (nu + beta_i) + gamma, bit for bit; column 1 + s ``draws_psi_cube_missing_dev``'s draw s and the width
        beta_i + max(gamma_s, 0), where gamma_s is that method's ``return_gamma=True``.  Refusals as for
        ``predict_psi_cube_missing_dev``; a label outside [-1, n_groups) and a negative or non-finite weight are found on the device
        before the first tile and refused with a GpzError."""
        return self._stack_dev(X, Psi, edges, n_draws, seed, Z, groups, n_groups, weights, selection, missing=True, both=True,
                               cov="cube")

    def _check_noisy_missing_cov(self, what, X, Psi, selection):
        """The checks the three methods for rows with Psi and missing values of a covariance kind share, none of which touches a GPU: X by
        type, dtype and shape, then where such rows go when this is not their route (no Psi, a full Psi cube, a diagonal kind, a shape
        outside predict_missing_cov_fits of k_predict_missing_cov.hip), then Psi's type, dtype and shape and the priors.  Returns X as
        n x d and Psi as n x 1 or n x d."""
        name = f"{what}_noisy_missing_cov_dev"
        if isinstance(X, np.ndarray):
            raise TypeError(f"{name} takes a torch tensor on cuda:{self.device}; a NumPy catalogue with input noise and missing values "
                            "goes to Predictor.predict(X, Psi=Psi)")
        X = self._check_dev_rows(X, selection, what)
        if Psi is None:
            raise ValueError(f"{name} needs Psi: rows of a covariance kind without input noise go to {what}_missing_cov_dev(X)")
        if np.ndim(Psi) == 3 or (hasattr(Psi, "dim") and Psi.dim() == 3):
            raise ValueError(f"{name} takes Psi as n x d, n x 1 or n variances: a full d x d x n Psi stays on "
                             "Predictor.predict(X, Psi=Psi)")
        if self._method[1] != "C":
            raise ValueError(f"{name} is for the covariance kinds (GC, VC): a diagonal kind such as {self._method} goes to "
                             f"{what}_noisy_missing_dev(X, Psi)")
        if not (1 <= self._d <= 10 and 1 <= self._k <= 8 and 1 <= self._m <= 256):
            raise ValueError(f"{name} needs a model inside predict_missing_cov_fits: GC or VC, d <= 10, k <= 8 and m <= 256; this one "
                             f"is {self._method} with d = {self._d}, m = {self._m}, k = {self._k} (Predictor.predict takes rows with "
                             "input noise and missing values for every shape)")
        Psi = self._check_dev_psi(Psi, X.shape[0], what)
        if self._priors.shape != (self._m,):
            raise ValueError(f"the priors of the set must be {self._m} values, got {self._priors.size} (Predictor.predict reports "
                             "the same for such rows)")
        return X, Psi

    def predict_noisy_missing_cov_dev(self, X, Psi, selection=None):
        """``predict_noisy_missing_dev`` for a covariance kind (GC, VC; gpz_predictor_run_noisy_missing_cov_dev): a catalogue whose rows
        have input noise and, some of them, missing values.  X, ``selection`` and ``Psi`` (variances per input dimension, (n, d),
        (n, 1) or (n,), float64 or float32, any strides) as for ``predict_noisy_cov_dev``.  Returns mu, sigma, nu, beta_i, gamma as
        ``predict(X, Psi=Psi)`` does, as float64 tensors of shape (n, k) on the device.  The rows are grouped by NaN pattern with torch
        on the device: the complete rows go to gpz_predictor_run_noisy_cov_dev and get the bits of ``predict_noisy_cov_dev`` on them
        alone; every other group is gathered with its Psi and gets predictNoisyMissing of predictCov.m:233-337 on the handle's tiles
        (k_predict_noisy_missing_cov_pairs) with the priors of the set (1 / m without any).  Psi must be finite and >= 0 in a row's
        observed dimensions (else GpzError); in its missing dimensions it is not read, whatever it holds, and a row with nothing
        observed gets the bits of ``predict_missing_cov_dev``.  It needs a model inside predict_missing_cov_fits (GC or VC, d <= 10,
        k <= 8, m <= 256), else ValueError; a full d x d x n Psi, PHI and host arrays stay on ``Predictor.predict``, a diagonal kind
        goes to ``predict_noisy_missing_dev`` and rows without Psi to ``predict_missing_cov_dev``.  A row's results do not depend on the
        tile size, the row order or the other rows of the call.  Type, dtype and shape are checked first, the device last, all before
        the GPU is touched."""
        self._check_open()
        X, Psi = self._check_noisy_missing_cov("predict", X, Psi, selection)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        return self._moments_dev(X, Psi, selection, True, cov=True)

    def draws_noisy_missing_cov_dev(self, X, Psi, n_draws, seed=0, Z=None, selection=None, return_gamma=False):
        """``draws_noisy_missing_dev`` for a covariance kind (gpz_predictor_draws_noisy_missing_cov_dev): X, ``Psi`` and ``selection`` as
        for ``predict_noisy_missing_cov_dev``, ``n_draws``, ``seed`` and ``Z`` as for ``draws_dev``.  Returns a float64 tensor of shape
        (n_draws, n, k) on the device: draws[s] is ``predict_noisy_missing_cov_dev``'s mu under weight draw s, PHI w_s + muY with the PHI
        of predictNoisy or predictNoisyMissing - the mean is linear in the weights, so this is exact.  One weight draw serves all rows
        of all groups; complete rows get the bits of ``draws_noisy_cov_dev`` on them alone.
        ``return_gamma=True`` (gpz_predictor_draws_gamma_noisy_missing_cov_dev) returns ``(F, Gam)``: F with the bits it has without the
        keyword, Gam a float64 tensor of shape (n_draws, n, k), predictNoisyMissing's gamma of predictCov.m under the weights of draw
        s - the variance of PHI(x) w_s over the input noise and the missing dimensions together, not clamped at 0
        (k_predict_noisy_missing_cov_gamma); complete rows get ``draws_noisy_cov_dev(..., return_gamma=True)``'s and rows with nothing
        observed ``draws_missing_cov_dev(..., return_gamma=True)``'s.  A y-draw of row i under draw s has variance beta_i + Gam[s, i].
        A row's Gam has the same bits for any tile size, row order, other rows of the call and any n_draws > s."""
        self._check_open()
        X, Psi = self._check_noisy_missing_cov("draws", X, Psi, selection)
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 1)
        self._check_dev_device(X=X, selection=selection, Psi=Psi)
        return self._draws_dev(X, Psi, selection, True, n_draws, seed, z, bool(return_gamma), cov=True)

    def stack_noisy_missing_cov_dev(self, X, Psi, edges, n_draws=64, seed=0, Z=None, groups=None, n_groups=None, weights=None,
                                    selection=None):
        """``stack_noisy_missing_dev`` for a covariance kind (GC, VC; gpz_predictor_stack_noisy_missing_cov_dev): a catalogue whose rows
        have input noise and, some of them, missing values.  X, ``Psi`` and ``selection`` as for ``predict_noisy_missing_cov_dev``
        (Psi is not read in a row's missing dimensions), everything else as for ``stack_dev``; ``n_draws`` defaults to 64.  The rows are
        grouped by NaN pattern with torch on the device.  The complete rows go to gpz_predictor_stack_noisy_cov_dev (a catalogue
        without NaN gives ``stack_noisy_cov_dev``'s bits), every other group with its Psi, labels and weights to
        gpz_predictor_stack_noisy_missing_cov_dev (rows with nothing observed get ``stack_missing_cov_dev``'s), and the groups' results
        are added field by field in ascending order of the pattern code, so the call equals the ``+=`` of the single-pattern calls bit
        for bit; one weight draw serves all groups.  For a row with missing values column 0 uses ``predict_noisy_missing_cov_dev``'s mu
        and that call's sigma = (nu + beta_i) + gamma, bit for bit; column 1 + s ``draws_noisy_missing_cov_dev``'s draw s and the width
        beta_i + max(gamma_s, 0), where gamma_s is that method's ``return_gamma=True``.  ``n_groups`` and the range of the labels are
        decided over all rows.  It needs a model inside predict_missing_cov_fits (GC or VC, d <= 10, k <= 8, m <= 256), else
        ValueError; a diagonal kind goes to ``stack_noisy_missing_dev``, rows without Psi to ``stack_missing_cov_dev``, and a full
        d x d x n Psi and host arrays stay on ``Predictor.predict``.  A label outside [-1, n_groups) and a negative or non-finite
        weight are found on the device before the first tile and refused with a GpzError."""
        return self._stack_dev(X, Psi, edges, n_draws, seed, Z, groups, n_groups, weights, selection, missing=True, both=True, cov=True)

    def _check_missing_cov(self, what, X, Psi, selection):
        """The checks the three methods for rows with missing values of a covariance kind share, none of which touches a GPU: X by type,
        dtype and shape, then where such rows go when this is not their route (Psi, a diagonal kind, a shape outside
        predict_missing_cov_fits of k_predict_missing_cov.hip), then the priors.  Returns X as n x d."""
        name = f"{what}_missing_cov_dev"
        if isinstance(X, np.ndarray):
            raise TypeError(f"{name} takes a torch tensor on cuda:{self.device}; a NumPy catalogue with missing values goes to "
                            "Predictor.predict")
        X = self._check_dev_rows(X, selection, what)
        if Psi is not None:
            raise ValueError(f"{name} does not take Psi: rows of a covariance kind with both input noise and missing values "
                             "(predictNoisyMissing) go to Predictor.predict(X, Psi=Psi)")
        if self._method[1] != "C":
            raise ValueError(f"{name} is for the covariance kinds (GC, VC): a diagonal kind such as {self._method} goes to " +
                             ("stack_missing_dev(X, edges)" if what == "stack" else f"{what}_dev(X, missing=True)"))
        if not (1 <= self._d <= 10 and 1 <= self._k <= 8 and 1 <= self._m <= 256):
            raise ValueError(f"{name} needs a model inside predict_missing_cov_fits: GC or VC, d <= 10, k <= 8 and m <= 256; this one "
                             f"is {self._method} with d = {self._d}, m = {self._m}, k = {self._k} (Predictor.predict takes rows with "
                             "missing values for every shape)")
        if self._priors.shape != (self._m,):
            raise ValueError(f"the priors of the set must be {self._m} values, got {self._priors.size} (Predictor.predict reports "
                             "the same for such rows)")
        return X

    def _check_missing_cov_device(self, X, selection):
        """``_check_dev_device`` for those two methods, saying where a catalogue in host memory goes."""
        try:
            self._check_dev_device(X=X, selection=selection)
        except ValueError as e:
            raise ValueError(f"{e} (Predictor.predict takes a catalogue with missing values from host arrays)") from None

    def predict_missing_cov_dev(self, X, selection=None, Psi=None):
        """``predict_dev(X, missing=True)`` for a covariance kind (GC, VC; gpz_predictor_run_missing_cov_dev): X and ``selection`` as
        for ``predict_dev``.  Returns mu, sigma, nu, beta_i, gamma as ``predict(X)`` does, as float64 tensors of shape (n, k) on the
        device.  The rows are grouped by NaN pattern with torch on the device; complete rows go to gpz_predictor_run_dev and get
        exactly what ``predict_dev`` gives them (gamma 0.0), every other group predictMissing of predictCov.m:134-232 on the handle's
        tiles with the priors of the set (1 / m without any), gamma > 0 there.  A row's results do not depend on the tile size, the
        row order or the other rows of the call.  It needs a model inside predict_missing_cov_fits (GC or VC, d <= 10, k <= 8,
        m <= 256), else ValueError; ``Psi`` is refused (rows with both stay on ``Predictor.predict``, as host arrays and PHI do), and
        a diagonal kind goes to ``predict_dev(X, missing=True)``.  Type, dtype and shape are checked first, the device last, all
        before the GPU is touched."""
        self._check_open()
        X = self._check_missing_cov("predict", X, Psi, selection)
        self._check_missing_cov_device(X, selection)
        return self._moments_dev(X, None, selection, True, cov=True)

    def draws_missing_cov_dev(self, X, n_draws, seed=0, Z=None, selection=None, Psi=None, return_gamma=False):
        """``draws_dev(X, n_draws, missing=True)`` for a covariance kind (gpz_predictor_draws_missing_cov_dev): X and ``selection`` as
        for ``predict_missing_cov_dev``, ``n_draws``, ``seed`` and ``Z`` as for ``draws_dev``.  Returns a float64 tensor of shape
        (n_draws, n, k) on the device: for a row with missing values draws[s] is PHI_missing w_s + muY, ``predict_missing_cov_dev``'s
        mu under weight draw s - the mean is linear in the weights, so this is exact.  One weight draw serves all rows of all groups;
        complete rows get the bits of ``draws_dev`` on them alone.
        ``return_gamma=True`` (gpz_predictor_draws_gamma_missing_cov_dev) returns ``(F, Gam)``: F with the bits it has without the keyword,
        Gam a float64 tensor of shape (n_draws, n, k), predictMissing's gamma of predictCov.m under the weights of draw s - the variance
        of PHI(x) w_s over the missing dimensions of the row, not clamped at 0 and exactly 0.0 on complete rows
        (k_predict_missing_cov_gamma).  A y-draw of row i under draw s has variance beta_i + Gam[s, i].  A row's Gam has the same bits
        for any tile size, row order, other rows of the call and any n_draws > s."""
        self._check_open()
        X = self._check_missing_cov("draws", X, Psi, selection)
        n_draws, z = self._check_draw_args(n_draws, seed, Z, 1)
        self._check_missing_cov_device(X, selection)
        return self._draws_dev(X, None, selection, True, n_draws, seed, z, bool(return_gamma), cov=True)

    def stack_missing_cov_dev(self, X, edges, n_draws=0, seed=0, Z=None, groups=None, n_groups=None, weights=None, selection=None):
        """``stack_missing_dev`` for a covariance kind (GC, VC; gpz_predictor_stack_missing_cov_dev): arguments and result as for
        ``stack_dev``.  The rows are grouped by NaN pattern with torch on the device, as ``predict_missing_cov_dev`` groups them.  The
        complete rows go to gpz_predictor_stack_dev (a catalogue without NaN gives ``stack_dev``'s bits), every other group with its
        labels and weights to gpz_predictor_stack_missing_cov_dev, and the groups' results are added field by field in ascending order
        of the pattern code, so the call equals the ``+=`` of the single-pattern calls bit for bit.  For a row with missing values
        column 0 uses ``predict_missing_cov_dev``'s mu and that call's sigma = (nu + beta_i) + gamma, bit for bit; column 1 + s
        ``draws_missing_cov_dev``'s draw s and the width beta_i + max(gamma_s, 0), where gamma_s is that method's ``return_gamma=True``.
        ``n_groups`` and the range of the labels are decided over all rows.  It needs a model inside predict_missing_cov_fits (GC or
        VC, d <= 10, k <= 8, m <= 256), else ValueError; a diagonal kind goes to ``stack_missing_dev``, rows with ``Psi`` to
        ``stack_noisy_missing_cov_dev``, and host arrays are not on the handle (``Predictor.predict`` takes such rows).  A label outside [-1, n_groups)
        and a negative or non-finite weight are found on the device before the first tile and refused with a GpzError."""
        return self._stack_dev(X, None, edges, n_draws, seed, Z, groups, n_groups, weights, selection, missing=True, cov=True)

    def stack_noisy_cov_dev(self, X, Psi, edges, n_draws=0, seed=0, Z=None, groups=None, n_groups=None, weights=None, selection=None):
        """``stack_noisy_dev`` for a covariance kind (GC, VC; gpz_predictor_stack_noisy_cov_dev): X, ``Psi`` and ``selection`` as for
        ``predict_noisy_cov_dev``, everything else as for ``stack_dev``.  Returns a NumPy StackResult.  Column 0 uses
        ``predict_noisy_cov_dev``'s mu and that call's sigma = (nu + beta_i) + gamma, bit for bit; column 1 + s
        ``draws_noisy_cov_dev``'s draw s and the width beta_i + max(gamma_s, 0), where gamma_s is that method's ``return_gamma=True``.
        The fields are plain sums over the rows, so calls over parts of a catalogue add.  It needs a model inside
        predict_noisy_cov_fits (GC or VC, d <= 10, k <= 8, m <= 256, or 1024 with large_m=True), else ValueError, and takes any route of the handle; a diagonal
        kind goes to ``stack_noisy_dev``.  Rows with NaN, a bad element of Psi, a label outside [-1, n_groups) and a negative or
        non-finite weight are found on the device before the first tile and refused with a GpzError."""
        return self._stack_dev(X, Psi, edges, n_draws, seed, Z, groups, n_groups, weights, selection, cov=True)

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
        kind, d <= 20, k <= 8, m <= 256), else ValueError; host arrays and ``Psi`` together with missing values are not on the handle
        (``Predictor.predict`` takes such rows), and the covariance kinds go to ``stack_missing_cov_dev``."""
        return self._stack_dev(X, None, edges, n_draws, seed, Z, groups, n_groups, weights, selection, missing=True)

    def stack_noisy_missing_dev(self, X, Psi, edges, n_draws=0, seed=0, Z=None, groups=None, n_groups=None, weights=None,
                                selection=None):
        """``stack_noisy_dev`` for a catalogue whose rows have input noise and, some of them, missing values (a flux error in every
        band, NaN for the non-detections): arguments and result as for ``stack_noisy_dev``, ``Psi`` as for
        ``predict_noisy_missing_dev`` (not read in a row's missing dimensions).  The rows are grouped by NaN pattern with torch on the
        device.  The complete rows go to gpz_predictor_stack_noisy_dev (a catalogue without NaN gives ``stack_noisy_dev``'s bits),
        every other group with its Psi, labels and weights to gpz_predictor_stack_noisy_missing_dev, and the groups' results are
        added field by field in ascending order of the pattern code, so the call equals the ``+=`` of the single-pattern calls bit
        for bit.  For a row with missing values column 0 uses ``predict_noisy_missing_dev``'s mu and sigma = (nu + beta_i) + gamma,
        column 1 + s ``draws_noisy_missing_dev``'s draw s and the width beta_i + max(gamma_s, 0), where gamma_s is
        predictNoisyMissing's gamma under the weights of draw s (``draws_noisy_missing_dev(..., return_gamma=True)`` returns it).
        ``n_groups`` and the range of the labels are decided over all rows.  It needs a model inside predict_missing_fits (a diagonal
        kind, d <= 20, k <= 8, m <= 256, or 1024 with large_m=True), else ValueError, and a predictor that was not made with force_tiles=True (unless with large_m=True); host arrays are
        not on the handle, and the covariance kinds go to ``stack_noisy_missing_cov_dev``."""
        return self._stack_dev(X, Psi, edges, n_draws, seed, Z, groups, n_groups, weights, selection, missing=True, both=True)

    def _stack_dev(self, X, Psi, edges, n_draws, seed, Z, groups, n_groups, weights, selection, missing=False, both=False, cov=False):
        """``stack_dev`` (Psi None), ``stack_noisy_dev``, ``stack_missing_dev``, (``both``: Psi and ``missing`` together)
        ``stack_noisy_missing_dev``, (``cov``: Psi of a covariance kind) ``stack_noisy_cov_dev``, (``cov`` with ``missing``)
        ``stack_missing_cov_dev`` and (``cov`` with ``both``) ``stack_noisy_missing_cov_dev``: the checks, the device last, all before the GPU is touched; then the entry, or with ``missing``
        one entry per NaN-pattern group."""
        import torch
        self._check_open()
        if both and cov == "cube":
            X, Psi = self._check_psi_cube_missing("stack", X, Psi, selection)
        elif both and cov:
            X, Psi = self._check_noisy_missing_cov("stack", X, Psi, selection)
        elif both:
            X, Psi = self._check_noisy_missing("stack", X, Psi, selection, draws=True)
        elif cov == "cube":
            X, Psi = self._check_psi_cube("stack", X, Psi, selection)
        elif cov and missing:
            X = self._check_missing_cov("stack", X, Psi, selection)
        elif cov:
            X, Psi = self._check_noisy_cov("stack", X, Psi, selection)
        else:
            X = self._check_dev_rows(X, selection, "stack" if Psi is None else "stack_noisy")
        n_all = X.shape[0]
        if missing and not both and not cov:
            self._check_missing_model("stack_missing_dev", None)
        if Psi is not None and not both and not cov:
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
        try:
            self._check_dev_device(X=X, selection=selection, groups=groups, weights=weights, Psi=Psi)
        except ValueError as err:
            if not (cov and missing) or both:
                raise
            raise ValueError(f"{err} (Predictor.predict takes a catalogue with missing values from host arrays)") from None
        lab = wt = None
        X, Psi = self._selected(selection, X, Psi)
        if groups is not None:
            lab = (groups if selection is None else groups[selection]).to(torch.int32).contiguous()
        if weights is not None:
            wt = (weights if selection is None else weights[selection]).to(torch.float64).contiguous()
        if n_groups is None:
            n_groups = max(int(lab.max()) + 1, 1) if lab is not None and lab.numel() else 1
            if n_groups * B > GPZ_STACK_MAX_GROUP_BINS:
                raise ValueError(f"n_groups * bins = {n_groups * B} is over the limit of {GPZ_STACK_MAX_GROUP_BINS} per call")
        G = int(n_groups)
        totals = self._stack_arrays(n_draws, G, B)
        if X.shape[0]:
            call = self._dev_begin(X.device)
            es = self._stack_edges(e, call.muY)
            # X, lab and wt are referenced by this frame for the whole (host-synchronous) call: no record_stream needed
            for code, idx, Xg, Pg, lg, wg in self._dev_groups(X, missing, Psi, lab, wt):   # ascending code: one fixed order of the sums
                part = totals if idx is None else self._stack_arrays(n_draws, G, B)
                fn, lead, _ = self._dev_entry("stack", call, code, Xg, Pg, cov)
                _lib.check(fn(*lead, n_draws, int(seed), _lib.dptr(z), _lib.dptr(es), B, None if lg is None else lg.data_ptr(), G,
                              None if wg is None else wg.data_ptr(), *(_lib.dptr(a) for a in part), _lib.dptr(call.muY), call.stream))
                self._merge(idx, totals, part, None)
        return StackResult(*totals, e.copy())
