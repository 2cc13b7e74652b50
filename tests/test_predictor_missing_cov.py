"""Rows with missing inputs of the covariance kinds on the predictor handle (Predictor.predict_missing_cov_dev / draws_missing_cov_dev,
k_predict_missing_cov.hip) against the one-shot predictMissing route and the oracle: parity over GC and VC, every width and every number
of observed dimensions, the edges in m of the blocks, the chunk rule and the slab rule, every row count of a group, the same bits over
tile sizes, row orders, company and splits, every layout of X, the draws, the refusals of the C entries and constant memory.

Gates: per output, ten times the largest nrel against gpz_amd.predict seen on an MI355X at the shapes of this file, rounded up to a
power of ten (GATES; none looser than 1e-9), and rel <= 1e-8 against oracle.gpz_oracle.predict_any (the project's oracle gate).
Largest values seen: GATE_SEEN below."""

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, nrel, synth_model
from test_predictor_draws_cpu import philox_normals
from test_predictor_missing import check_gamma_sign, knock_out, model_with_priors, reference
from test_predictor_missing_cov_cpu import chunks_rule, slabs_rule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COV = ("GC", "VC")
NAMES = ("mu", "sigma", "nu", "beta_i", "gamma")
NAN = float("nan")
GATE_SEEN = {"mu": 2.8e-15, "sigma": 1.3e-14, "nu": 1.1e-15, "beta_i": 2.8e-16, "gamma": 2.5e-14}   # over the 69 comparisons of this file
GATES = {"mu": 1e-13, "sigma": 1e-12, "nu": 1e-13, "beta_i": 1e-14, "gamma": 1e-12}
# (against the oracle on 60 rows at m = 7, at most: mu 9.8e-16, sigma 5.8e-15, nu 9.5e-16, beta_i 4.9e-16, gamma 8.1e-15)


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def check_parity(out, ref):
    """nrel within GATES on all five outputs over the rows predict() gave; rel <= 1e-8 on the rows that are the oracle's."""
    ref, orc_rows = ref
    for name, a, b in zip(NAMES, out, ref):
        a = host(a) if isinstance(a, torch.Tensor) else a
        assert a.shape == b.shape, (name, a.shape, b.shape)
        keep = slice(None) if orc_rows is None else ~orc_rows
        print(f"nrel {name}: {nrel(a[keep], b[keep]):.3e}")
        assert nrel(a[keep], b[keep]) <= GATES[name], (name, nrel(a[keep], b[keep]))
        if orc_rows is not None:
            assert rel(a[orc_rows], b[orc_rows]) <= 1e-8, (name, rel(a[orc_rows], b[orc_rows]))


def both(p, x, nd=3, seed=9, **kw):
    return tuple(p.predict_missing_cov_dev(x, **kw)) + (p.draws_missing_cov_dev(x, nd, seed=seed, **kw),)


def same(a, b, what=""):
    for i, (s, t) in enumerate(zip(a, b)):
        assert torch.equal(s, t), (what, i)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_parity_with_predict_and_the_oracle(method, hetero, k):
    """2500 rows over 1024-row tiles: dimension 1 missing on 20 % and dimension 4 on 10 % of the rows independently, one row with only
    dimension 0 observed and one with nothing observed.  m = 250 passes its pair-component records through many slabs."""
    d, ns = 5, 2500
    for m in (7, 50, 250):
        model = model_with_priors(method, m, d, k, hetero, seed=3000 * COV.index(method) + 100 * hetero + 10 * k + m)
        X = knock_out(catalogue(model, ns, seed=m), seed=m + 1)
        X[5, 1:] = NAN
        X[9, :] = NAN
        full = ~np.isnan(X).any(axis=1)
        ref = reference(X, model)
        with gpz_amd.Predictor(model, tile_rows=1024) as p:
            out = p.predict_missing_cov_dev(dev(X))
            assert p.route.endswith(f"; missing: k_predict_missing_cov_pairs ({chunks_rule(m)} pair chunks)"), p.route
            check_parity(out, ref)
            check_gamma_sign(out, X)
            alone = p.predict_dev(dev(X[full]))
            fd = torch.from_numpy(full).to(DEV)
            assert all(torch.equal(a[fd], b) for a, b in zip(out, alone))
            if m == 7:
                orc = O.predict_any(X[:60], model)
                for name, a, b in zip(NAMES, out, orc):
                    print(f"oracle rel {name}: {rel(host(a)[:60], b):.3e}")
                    assert rel(host(a)[:60], b) <= 1e-8, (name, rel(host(a)[:60], b))
        if m == 250:
            assert max(slabs_rule(m, no) for no in (0, 1, 3, 4)) > 1


# ---- 2. every width and every number of observed dimensions --------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 11)))
def test_every_width_and_every_number_of_observed_dimensions(d):
    """Bit 0 alone missing, bit d - 1 alone missing, a single observed dimension (each of the two ends), nothing observed: NO = d - 1,
    1 and 0 at every d, so NO = 0 .. 9 between them."""
    n, m, k = 300, 20, 1 if d % 2 else 8
    for method in COV:
        model = model_with_priors(method, m, d, k, True, seed=400 + d)
        X = catalogue(model, n, seed=d)
        X[0:60, 0] = NAN
        if d > 1:
            X[60:120, d - 1] = NAN
            X[120:125, 1:] = NAN                                           # only dimension 0 observed
            X[125:130, :d - 1] = NAN                                       # only dimension d - 1 observed
            X[130, :] = NAN
        ref = reference(X, model)
        with gpz_amd.Predictor(model) as p:
            out = p.predict_missing_cov_dev(dev(X))
            check_parity(out, ref)
            check_gamma_sign(out, X)
            F = p.draws_missing_cov_dev(dev(X), 2, Z=np.zeros((m, 2, k)))
            assert nrel(host(F[1]), host(out[0])) <= 1e-12


# ---- 3. the edges in m ---------------------------------------------------------------------------------------------------------------------
CHUNK_EDGES = [m for m in range(2, 257) if chunks_rule(m) != chunks_rule(m - 1)]
SLAB_EDGES = [m for m in range(2, 257) if slabs_rule(m, 2) != slabs_rule(m - 1, 2)]        # where the number of slabs changes at no = 2
EDGES_M = sorted({1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256} | {m - e for m in CHUNK_EDGES + SLAB_EDGES for e in (0, 1)})


@pytest.mark.parametrize("m", EDGES_M)
def test_edges_in_m(m):
    """m at the edges of the 16-record stages and the 64-record stages, and every m where the chunk rule or, at no = 2, the slab rule
    gives another count, with m - 1.  One pattern: dimension 1 missing of d = 3."""
    assert CHUNK_EDGES == [11, 16, 23, 32] and SLAB_EDGES == [141, 178, 224]
    d, n, k = 3, 300, 1 if m % 2 else 2
    model = model_with_priors("VC", m, d, k, bool(m % 3), seed=800 + 10 * m)
    X = catalogue(model, n, seed=m)
    X[:, 1] = NAN
    ref = reference(X, model)
    with gpz_amd.Predictor(model) as p:
        out = p.predict_missing_cov_dev(dev(X))
        check_parity(out, ref)
        check_gamma_sign(out, X)
        assert p.route.endswith(f"({chunks_rule(m)} pair chunks)"), p.route
        F = p.draws_missing_cov_dev(dev(X), 2, Z=np.zeros((m, 2, k)))
        assert nrel(host(F[0]), host(out[0])) <= 1e-12


# ---- 4. every row count of a group ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_every_row_count_of_a_group(k):
    """A group of n rows at the edges of the 64-row workgroups and the 256-row blocks of the Ex and PHI kernels: every shorter call is
    the first rows of the longest bit for bit, moments and draws."""
    d, m, nd = 5, 17, 3
    model = model_with_priors("VC", m, d, k, True, seed=950 + k)
    X = catalogue(model, 257, seed=93)
    X[:, 2] = NAN
    ref = reference(X, model)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        Xd = dev(X)
        full = p.predict_missing_cov_dev(Xd)
        Ff = p.draws_missing_cov_dev(Xd, nd, seed=3)
        check_parity(full, ref)
        for n in (1, 63, 64, 65, 255, 256):
            out = p.predict_missing_cov_dev(Xd[:n])
            assert all(o.shape == (n, k) and torch.equal(o, f[:n]) for o, f in zip(out, full)), n
            assert torch.equal(p.draws_missing_cov_dev(Xd[:n], nd, seed=3), Ff[:, :n]), n


# ---- 5. the same bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,m,k", [("VC", 60, 1), ("GC", 40, 3)])
def test_same_bits_over_tiles_row_orders_company_and_splits(method, m, k):
    n, d = 3000, 5
    model = model_with_priors(method, m, d, k, True, seed=45 + m)
    X = knock_out(catalogue(model, n, seed=46), seed=47)
    perm = np.random.default_rng(48).permutation(n)
    Xd, pd = dev(X), torch.from_numpy(perm).to(DEV)
    outs = []
    for tile in (256, 1024, None):
        with gpz_amd.Predictor(model, tile_rows=tile) as p:
            outs.append(both(p, Xd))
            if tile == 1024:
                shuf = both(p, Xd[pd])
                rows = [int(np.flatnonzero(np.isnan(X[:, 1]) & ~np.isnan(X[:, 4]))[3]), int(np.flatnonzero(np.isnan(X[:, 4]))[0]),
                        int(np.flatnonzero(~np.isnan(X).any(axis=1))[2])]
                single = [both(p, Xd[r:r + 1]) for r in rows]
                only = torch.from_numpy(np.isnan(X[:, 1]) & ~np.isnan(X[:, 4])).to(DEV)   # one group, the others removed
                group = both(p, Xd[only])
                halves = [both(p, Xd[:1300]), both(p, Xd[1300:])]                          # the catalogue split into two calls
    base = outs[0]
    for o in outs[1:]:
        same(o, base, "tiles")
    same(shuf[:5], [b[pd] for b in base[:5]], "permutation")
    assert torch.equal(shuf[5], base[5][:, pd])
    for r, s in zip(rows, single):
        same(s[:5], [b[r:r + 1] for b in base[:5]], r)
        assert torch.equal(s[5], base[5][:, r:r + 1]), r
    same(group[:5], [b[only] for b in base[:5]], "one group")
    assert torch.equal(group[5], base[5][:, only])
    same([torch.cat((a, b)) for a, b in zip(halves[0][:5], halves[1][:5])], base[:5], "split")
    assert torch.equal(torch.cat((halves[0][5], halves[1][5]), dim=1), base[5])


# ---- 6. layouts ----------------------------------------------------------------------------------------------------------------------------
def test_layouts_of_x_give_the_same_bits():
    """float32, a column-strided view and a transposed storage: each is the call on a contiguous float64 copy of the same values."""
    n, d = 700, 5
    model = model_with_priors("VC", 40, d, 2, True, seed=84)
    X32 = knock_out(catalogue(model, 2 * n, seed=85), seed=86).astype(np.float32)
    Xd = dev(X32.astype(np.float64))
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        ref = both(p, Xd.contiguous())
        same(both(p, dev(X32, torch.float32)), ref, "float32")
        same(both(p, Xd.T.contiguous().T), ref, "transposed storage")
        same(both(p, dev(X32, torch.float32).T.contiguous().T), ref, "float32 transposed storage")
        wide = torch.full((2 * n, 2 * d), 3.0, dtype=torch.float64, device=DEV)
        wide[:, ::2] = Xd
        same(both(p, wide[:, ::2]), ref, "column-strided view")
        half = both(p, Xd[::2].contiguous())
        same(both(p, Xd[::2]), half, "row-sliced view")
        same([t[::2] if t.dim() == 2 else t[:, ::2] for t in ref], half, "rows of the whole call")
        sel = torch.zeros(2 * n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        same(both(p, Xd, selection=sel), half, "selection")


# ---- 7. draws ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,k", [("VC", 1), ("GC", 2)])
def test_draws_are_phi_missing_against_the_weight_draws(method, k):
    n, d, m, nd = 200, 4, 30, 7
    model = model_with_priors(method, m, d, k, True, seed=75 + k)
    X = knock_out(catalogue(model, n, seed=76), seed=77, cols=((0, 0.3), (2, 0.3)))
    Xd = dev(X)
    full = ~np.isnan(X).any(axis=1)
    st = model.sets["best"]
    with gpz_amd.Predictor(model) as p:
        PHI = np.array(gpz_amd.predict(X, model)[5])
        mu = host(p.predict_missing_cov_dev(Xd)[0])
        F0 = host(p.draws_missing_cov_dev(Xd, 3, Z=np.zeros((m, 3, k))))
        assert all(nrel(F0[s], mu) <= 1e-12 for s in range(3))             # Z = 0 gives mu
        seeded = p.draws_missing_cov_dev(Xd, nd, seed=12345)
        Z = philox_normals(12345, m, nd, k)
        want = np.empty((nd, n, k))
        for o in range(k):
            S = 0.5 * (st["iSigma_w"][:, :, o] + st["iSigma_w"][:, :, o].T)
            W = st["w"][:, o:o + 1] + np.linalg.cholesky(S) @ Z[:, :, o]   # m x nd
            want[:, :, o] = (PHI @ W).T + model.muY[o]
        print(f"draws against PHI (w + R z) + muY: {nrel(host(seeded), want):.3e}")
        assert nrel(host(seeded), want) <= 1e-10, nrel(host(seeded), want)
        assert nrel(host(seeded), host(p.draws_missing_cov_dev(Xd, nd, Z=Z))) <= 1e-12
        # draw s is one weight draw for the rows of every group: the complete rows are the draws of a call without the others
        fd = torch.from_numpy(full).to(DEV)
        assert torch.equal(seeded[:, fd], p.draws_dev(Xd[fd], nd, seed=12345))
        with pytest.raises(ValueError, match="predict_missing_fits"):      # and the keyword keeps refusing these kinds
            p.draws_dev(Xd, nd, seed=12345, missing=True)
        with pytest.raises(_lib.GpzError, match="missing values"):
            p.predict_dev(Xd)


# ---- 8. refusals at the C entries -------------------------------------------------------------------------------------------------------------
def raw_call(p, x, obs, k, nd=3):
    """Both C entries on x with the mask obs: (rc of run, rc of draws, the outputs, the run's message)."""
    n = x.shape[0]
    muX, sdX, muY = p._norm_vectors()
    stream = torch.cuda.current_stream(x.device).cuda_stream
    out = [torch.full((k, n), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
    F = torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV)
    rc1 = p._lib.gpz_predictor_run_missing_cov_dev(p._handle(), *p._x_args(x), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                   _lib.dptr(p._priors), obs, *(t.data_ptr() for t in out), stream)
    msg = p._lib.gpz_last_error().decode() if rc1 else ""
    rc2 = p._lib.gpz_predictor_draws_missing_cov_dev(p._handle(), *p._x_args(x), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                     _lib.dptr(p._priors), obs, nd, 5, None, F.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc1, rc2, out + [F], msg


def test_bad_groups_are_refused_with_the_outputs_untouched():
    n, d, k = 20_000, 5, 2
    model = model_with_priors("VC", 20, d, k, True, seed=88)
    Xh = catalogue(model, n, seed=89)
    Xh[:, 3] = NAN
    X = dev(Xh)
    mask = 0b10111
    with gpz_amd.Predictor(model, tile_rows=1 << 12) as p:
        good = p.predict_missing_cov_dev(X[:500])
        rc1, rc2, outs, _ = raw_call(p, X, mask, k)
        assert rc1 == 0 and rc2 == 0 and all(bool((t != -7.0).all()) for t in outs)
        assert all(torch.equal(a[:500], b) for a, b in zip(outs[:5], good))
        two = X.clone()
        two[15_000:, 0] = NAN                                              # two patterns in one group
        nan_obs = X.clone()
        nan_obs[19_999, 4] = NAN                                           # a NaN in an observed dimension
        num_miss = X.clone()
        num_miss[12_345, 3] = 0.5                                          # a number in a missing one
        untouched = torch.full((k, n), -7.0, dtype=torch.float64, device=DEV).T
        for what, x, obs, text in (("two patterns", two, mask, "share one NaN pattern"), ("NaN in o", nan_obs, mask, "share one NaN pattern"),
                                   ("number in u", num_miss, mask, "share one NaN pattern"),
                                   ("full mask", X, 0b11111, "no dimension is missing"), ("mask past d", X, 0b110111, "above d")):
            rc1, rc2, outs, msg = raw_call(p, x, obs, k)
            assert rc1 == -1 and rc2 == -1, (what, rc1, rc2)               # GPZ_ERR_ARG
            assert text in msg, (what, msg)
            assert all(host(t).tobytes() == host(untouched).tobytes() for t in outs[:5]), what   # refused before any tile kernel has run
            assert bool((outs[5] == -7.0).all()), what
            again = p.predict_missing_cov_dev(X[:500])                      # the handle works on the next call
            assert all(torch.equal(a, b) for a, b in zip(again, good))
        none = torch.full((300, d), NAN, dtype=torch.float64, device=DEV)   # nothing observed: a valid mask
        rc1, rc2, outs, _ = raw_call(p, none, 0, k)
        assert rc1 == 0 and rc2 == 0
        assert all(bool((t == t[0:1]).all()) for t in outs[:5])            # Pio = priors / sum: every density a constant


@pytest.mark.parametrize("kw", [{"m": 257}, {"d": 11}, {"k": 9}, {"method": "VD"}])
def test_shapes_outside_the_route_are_refused_by_the_c_entry(kw):
    a = {"method": "VC", "m": 20, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    X = catalogue(model, 40, seed=6)
    X[:, 1] = NAN
    text = "gpz_predictor_run_missing_dev" if a["method"] == "VD" else "predict_missing_cov_fits"
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match="diagonal kind" if a["method"] == "VD" else "predict_missing_cov_fits"):
            p.predict_missing_cov_dev(dev(X))
        muX, sdX, muY = p._norm_vectors()
        out = [torch.empty((a["k"], 40), dtype=torch.float64, device=DEV).T for _ in range(5)]
        F = torch.empty((2, a["k"], 40), dtype=torch.float64, device=DEV)
        h = p._handle()
        with pytest.raises(_lib.GpzError, match=text) as ei:
            _lib.check(p._lib.gpz_predictor_run_missing_cov_dev(h, *p._x_args(dev(X)), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                                None, (1 << a["d"]) - 3, *(t.data_ptr() for t in out), None))
        assert ei.value.code == -5                                         # GPZ_ERR_UNSUPPORTED
        with pytest.raises(_lib.GpzError, match=text) as ei:
            _lib.check(p._lib.gpz_predictor_draws_missing_cov_dev(h, *p._x_args(dev(X)), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(muY),
                                                                  None, (1 << a["d"]) - 3, 2, 0, None, F.data_ptr(), None))
        assert ei.value.code == -5
        assert "missing" not in p.route


# ---- 9. memory -----------------------------------------------------------------------------------------------------------------------------
def test_memory_is_added_once_and_never_grows_with_rows_or_patterns():
    d, nd = 5, 4
    model = model_with_priors("VC", 30, d, 1, True, seed=97)
    n = 100_000
    gen = torch.Generator(device=DEV).manual_seed(98)
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=gen) * torch.from_numpy(model.sdX).to(DEV) + \
        torch.from_numpy(model.muX).to(DEV)
    two = X.clone()
    two[torch.rand(n, device=DEV, generator=gen) < 0.2, 1] = NAN
    eight = X.clone()
    for c in (0, 2, 4):
        eight[torch.rand(n, device=DEV, generator=gen) < 0.3, c] = NAN
    with gpz_amd.Predictor(model, tile_rows=1 << 16) as p, gpz_amd.Predictor(model, tile_rows=1 << 16) as q:
        q.predict_dev(X[:1000]); q.draws_dev(X[:1000], nd)                   # a handle that never makes these calls ...
        p.predict_dev(X[:1000]); p.draws_dev(X[:1000], nd)
        held = p.info[1]
        assert held == q.info[1]
        small = p.predict_missing_cov_dev(two[:1000])
        p.draws_missing_cov_dev(two[:1000], nd)
        first = p.info[1]
        assert first > held
        out = p.predict_missing_cov_dev(two)
        p.draws_missing_cov_dev(two[:50_000], nd)
        assert p.info[1] == first                                            # 100 000 rows: the same bytes
        assert all(torch.equal(a, b[:1000]) for a, b in zip(small, out))
        assert len(p._nan_groups_dev(eight)) == 8
        p.predict_missing_cov_dev(eight[:20_000])
        p.draws_missing_cov_dev(eight[:20_000], nd)
        assert p.info[1] == first                                            # eight patterns: the same bytes
        q.predict_dev(X); q.draws_dev(X[:50_000], nd)
        assert q.info[1] == held                                             # ... holds what it held


# ---- 10. rows with input noise and rows with missing inputs on one handle ----------------------------------------------------------------------
def test_noisy_and_missing_rows_share_a_handle_in_either_order():
    """VC, m = 20, d = 3, k = 2, 300 rows on 256-row tiles.  predict_noisy_cov_dev and predict_missing_cov_dev take the model's Sigma_j,
    ln|Sigma_j| and raw pair records from one helper, the first into temporaries of the call, the second into the handle: in either
    order each call returns the bits of the same call on a fresh handle, and the handle grows by what the two calls add separately
    (counted from a handle that has made a device call, predict_dev, as both do for their complete rows or their staging)."""
    m, d, k, n = 20, 3, 2, 300
    model = model_with_priors("VC", m, d, k, True, seed=4242)
    X = catalogue(model, n, seed=3)
    Xd, Xm = dev(X), dev(knock_out(X, seed=4, cols=((0, 0.3), (2, 0.2))))
    Psi = dev(np.random.default_rng(5).gamma(1.0, 0.05, (n, d)))
    calls = {"noisy": lambda p: p.predict_noisy_cov_dev(Xd, Psi), "missing": lambda p: p.predict_missing_cov_dev(Xm)}

    def fresh():
        p = gpz_amd.Predictor(model, tile_rows=256)
        p.predict_dev(Xd)
        return p

    alone, added = {}, {}
    for name, call in calls.items():
        with fresh() as p:
            base = p.info[1]
            alone[name] = call(p)
            added[name] = p.info[1] - base
            assert added[name] > 0, name
    for order in (("noisy", "missing"), ("missing", "noisy")):
        with fresh() as p:
            base = p.info[1]
            for name in order:
                same(calls[name](p), alone[name], (order, name))
            print(order, p.info[1] - base, added)
            assert p.info[1] - base == added["noisy"] + added["missing"], order
            assert "k_predict_noisy_cov_small" in p.route and "k_predict_missing_cov_pairs" in p.route, p.route
