"""Rows with a full input-noise covariance and missing inputs on the predictor handle (Predictor.predict_psi_cube_missing_dev /
draws_psi_cube_missing_dev / stack_psi_cube_missing_dev; k_predict_psi_cube_missing.hip, k_predict_psi_cube_missing_gamma.hip) against
the one-shot route ``gpz_amd.predict(X, model, Psi=cube)``, the oracle and the sibling entries of the handle: parity over GC and VC,
every edge in m, every number of observed dimensions and every row count of a group; the bit identities with the per-dimension
methods (a cube of diagonals), the cube methods (complete rows) and the methods without Psi (nothing observed), over tiles, orders,
company, splits and layouts; the draws; gamma under every draw against parent code; the stack; the refusals of the C entries with the
outputs untouched; and constant memory.  Psi_i = u u' + diag(g) as tests/predict_edges.py:psi_cube builds it; 256-row tiles unless said.

Gates.  Every test prints its figures before it asserts.  Against ``predict`` the gate of an output is ten times the largest norm ratio
seen on an MI355X over the comparisons of this file (GATE_SEEN), rounded up to a power of ten, and never looser than 1e-9 - the rule of
tests/test_predictor_noisy_missing_cov.py.  gamma_s is held against parent code by DESIGN.md section 32's rule: ten times the spread
of the parent's own two routes on the w_s model (gpz_amd.predict and Predictor.predict with the cube), never tighter than 1e-12, never
looser than 1e-9.  The oracle: 1e-8."""
import math

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from predict_edges import psi_cube, twin_psi
from test_predictor import catalogue, nrel
from test_predictor_draws_cpu import philox_normals
from test_predictor_missing import knock_out, model_with_priors
from test_predictor_missing_cov_cpu import chunks_rule
from test_predictor_noisy import noise
from test_predictor_noisy_missing_cov_cpu import slabs_rule
from test_predictor_stack import EPS, assert_close, setting
from test_predictor_stack_missing_cov import exact_model, exact_weights, same_stack, torch_reference
from test_predictor_stack_noisy import with_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COV = ("GC", "VC")
NAMES = ("mu", "sigma", "nu", "beta_i", "gamma")
NAN = float("nan")
ERR_ARG, ERR_UNSUPPORTED = -1, -5                                       # include/gpz_hip.h
# the largest nrel against gpz_amd.predict(X, model, Psi=cube) seen on an MI355X over the parity comparisons of this file, per output
GATE_SEEN = {"mu": 2.1e-15, "sigma": 3.2e-14, "nu": 5.4e-15, "beta_i": 2.3e-16, "gamma": 4.3e-14}   # over the 20 cases of tests 1
# ten times that, rounded up to a power of ten; none may be looser than 1e-9
GATES = {name: 10.0 ** math.ceil(math.log10(10.0 * v) - 1e-12) for name, v in GATE_SEEN.items()}
assert GATES == {"mu": 1e-13, "sigma": 1e-12, "nu": 1e-13, "beta_i": 1e-14, "gamma": 1e-12} and all(g <= 1e-9 for g in GATES.values())
# (against the oracle on 60 rows at m = 7, at most 1.4e-14.  The draws: under Z = 0 against predict's mu at most 4.0e-16, seeded against
# PHI w_s at most 4.6e-16.  gamma_s against gpz_amd.predict of the w_s model: at most 7.7e-15 over the column counts with exact weights
# and 1.3e-14 with seeded draws; the parent's two routes with a cube and NaN are one code path, their spread is 0, and the gate is the
# rule's floor of 1e-12)


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def cube_of(n, d, seed):
    """u u' + diag(g) per row: exactly symmetric and positive definite, d x d x n."""
    return psi_cube(noise(n, d, seed), 0.3 * np.random.default_rng(seed + 7919).standard_normal((n, d)))


def gate_of(spread):
    """10 x the spread of the parent's two routes, never tighter than 1e-12, never looser than 1e-9."""
    return min(max(10.0 * spread, 1e-12), 1e-9)


def reference(X, cube, model):
    """(predict() on all rows it accepts, None), or, where it refuses the rows with nothing observed, (predict() on the others with the
    oracle's values in those rows, their mask).  The cube is the clean one, always."""
    try:
        return [np.array(a) for a in gpz_amd.predict(X, model, Psi=cube)[:5]], None
    except _lib.GpzError:
        none = np.isnan(X).all(axis=1)
        assert none.any() and not none.all()
        part = gpz_amd.predict(X[~none], model, Psi=np.ascontiguousarray(cube[:, :, ~none]))[:5]
        orc = O.predict_any(X[none], model, Psi=np.ascontiguousarray(cube[:, :, none]))[:5]
        out = [np.empty((X.shape[0], model.k)) for _ in range(5)]
        for o, a, b in zip(out, part, orc):
            o[~none] = a
            o[none] = b
        return out, none


def check_parity(out, ref, what):
    """nrel within GATES on all five outputs over the rows predict() gave; rel <= 1e-8 on the rows that are the oracle's."""
    ref, orc_rows = ref
    keep = slice(None) if orc_rows is None else ~orc_rows
    fig = {}
    for name, a, b in zip(NAMES, out, ref):
        a = host(a) if isinstance(a, torch.Tensor) else a
        assert a.shape == b.shape, (name, a.shape, b.shape)
        fig[name] = nrel(a[keep], b[keep])
        print(f"nrel {what} {name} {fig[name]:.3e}")
        if orc_rows is not None:
            assert rel(a[orc_rows], b[orc_rows]) <= 1e-8, (name, rel(a[orc_rows], b[orc_rows]))
    for name in NAMES:
        assert fig[name] <= GATES[name], (what, name, fig[name])


def three(p, x, psi, nd=3, seed=4, **kw):
    """The five moments, the draws and gamma under every draw."""
    return tuple(p.predict_psi_cube_missing_dev(x, psi, **kw)) + \
        tuple(p.draws_psi_cube_missing_dev(x, psi, nd, seed=seed, return_gamma=True, **kw))


def same(a, b, what):
    for i, (s, t) in enumerate(zip(a, b)):
        assert s.shape == t.shape and torch.equal(s, t), (what, i)


def rows_of(out, idx):
    """Rows idx of the seven tensors of three(): (n, k) moments, (nd, n, k) draws and gamma."""
    return [t[idx] if t.dim() == 2 else t[:, idx] for t in out]


def pairs_tail(m):
    return f"; noise cube missing: k_predict_psi_cube_missing_pairs ({chunks_rule(m)} pair chunks)"


def gamma_tail(m, stack=False):
    return (f"; noise cube missing per draw: k_predict_psi_cube_missing_gamma ({chunks_rule(m)} pair chunks)" +
            (" + k_stack_tile_w" if stack else ""))


def groups_catalogue(model, seed):
    """d = 5.  Groups of 300, 65, 64, 63 and 1 rows - dimension 1 missing ([o u] = [0 2 3 4 1] is no involution: the `unshuffle` case),
    dimension 0 missing, dimensions 1 and 4, dimension 4, dimensions 0, 1 and 2 - so NO = 4, 4, 3, 4, 2; one row with only dimension 0
    observed (NO = 1), one row with nothing observed, 20 complete rows; then shuffled."""
    n = 300 + 65 + 64 + 63 + 1 + 1 + 1 + 20
    X = catalogue(model, n, seed=seed)
    at = 0
    for rows, gone in ((300, (1,)), (65, (0,)), (64, (1, 4)), (63, (4,)), (1, (0, 1, 2)), (1, (1, 2, 3, 4)), (1, (0, 1, 2, 3, 4))):
        X[at:at + rows, list(gone)] = NAN
        at += rows
    return X[np.random.default_rng(seed + 1).permutation(n)]


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
@pytest.mark.parametrize("m", [1, 2, 7, 15, 16, 17, 33, 50])
def test_parity_at_the_edges_in_m(method, m):
    """m at the edges of the record stages and of the chunk rule; k in {1, 3, 8}, heteroscedastic and not, by m; every NO = 1 .. 4 of
    d = 5 and the row counts 1, 63, 64, 65, 300 per group (groups_catalogue).  At m = 7 the first 60 rows against the oracle."""
    d = 5
    i = [1, 2, 7, 15, 16, 17, 33, 50].index(m) + COV.index(method)
    k, hetero = (1, 3, 8)[i % 3], bool(i % 2)
    model = model_with_priors(method, m, d, k, hetero, seed=26000 + 100 * COV.index(method) + m)
    X = groups_catalogue(model, seed=m)
    n = X.shape[0]
    cube = cube_of(n, d, seed=m + 2)
    ref = reference(X, cube, model)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        out = p.predict_psi_cube_missing_dev(dev(X), dev(cube))
        assert p.route.endswith(pairs_tail(m)), p.route
        assert "k_predict_noisy_missing_cov_pairs" not in p.route        # the per-dimension kernel has not run on this handle
        check_parity(out, ref, f"{method} m{m} k{k} h{int(hetero)}")
        nan = np.isnan(X).any(axis=1)
        assert np.all(host(out[4])[nan] > 0.0)
        if m == 7:
            orc = O.predict_any(X[:60], model, Psi=np.ascontiguousarray(cube[:, :, :60]))
            for name, a, b in zip(NAMES, out, orc):
                print(f"oracle rel {method} {name}: {rel(host(a)[:60], b):.3e}")
                assert rel(host(a)[:60], b) <= 1e-8, (name, rel(host(a)[:60], b))


@pytest.mark.parametrize("method,m,d,gone,k", [("VC", 250, 5, (1,), 1), ("GC", 250, 5, (0,), 3), ("VC", 240, 10, (3,), 1),
                                               ("GC", 240, 10, (9,), 8)])
def test_parity_at_several_slabs_and_at_the_largest_lds(method, m, d, gone, k):
    """m = 250 at d = 5: the pair-component records pass through several slabs.  m = 240 at d = 10 with NO = 9: the largest dynamic LDS
    (the Pio block of 240 components and the widest records) and the widest triangle, 45 values in registers.  130 rows: two full
    workgroups and a last one of two rows."""
    n = 130
    if d == 5:
        assert slabs_rule(m, d, d - len(gone)) > 1
    model = model_with_priors(method, m, d, k, True, seed=27000 + m + d)
    X = catalogue(model, n, seed=m + d)
    X[:, list(gone)] = NAN
    cube = cube_of(n, d, seed=m + d + 1)
    ref = reference(X, cube, model)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        out = p.predict_psi_cube_missing_dev(dev(X), dev(cube))
        check_parity(out, ref, f"{method} m{m} d{d} k{k}")
        F = p.draws_psi_cube_missing_dev(dev(X), dev(cube), 2, Z=np.zeros((m, 2, k)))
        assert nrel(host(F[1]), host(out[0])) <= GATES["mu"]


# ---- 2. bit identities -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,d,m,k", [("VC", 5, 40, 1), ("GC", 10, 33, 3), ("VC", 2, 20, 8)])
def test_a_cube_of_diagonals_is_the_per_dimension_route_bit_for_bit(method, d, m, k):
    """torch.equal on every output of all four questions against the noisy_missing_cov methods with the diagonal as variances: M + 0.0
    off the diagonal, the same division on it, the same factor and density functions, the same records and the same order of every sum."""
    n, nd = 700, 5
    model = model_with_priors(method, m, d, k, True, seed=26200 + m)
    X = knock_out(catalogue(model, n, seed=m), seed=m + 3, cols=((1, 0.3), (d - 1, 0.2)) if d > 2 else ((1, 0.4),))
    X[5, :] = NAN
    Psi = noise(n, d, seed=m + 1)
    Xd, Pd, Cd = dev(X), dev(Psi), dev(twin_psi(Psi))
    groups, weights = setting(n, 3, seed=m)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=256) as p, gpz_amd.Predictor(model, tile_rows=256) as q:
        ref = tuple(q.predict_noisy_missing_cov_dev(Xd, Pd)) + tuple(q.draws_noisy_missing_cov_dev(Xd, Pd, nd, seed=4, return_gamma=True))
        same(three(p, Xd, Cd, nd=nd), ref, "moments, draws and gamma per draw")
        edges = np.linspace(*np.percentile(host(ref[0]), [3, 97]), 41)
        kw = dict(n_draws=nd, seed=4, groups=gd, n_groups=3, weights=wd)
        same_stack(p.stack_psi_cube_missing_dev(Xd, Cd, edges, **kw), q.stack_noisy_missing_cov_dev(Xd, Pd, edges, **kw), "stack")
        same(three(q, Xd, Cd, nd=nd), ref, "on the handle that has served the per-dimension route")


def test_complete_rows_rows_with_nothing_observed_and_nan_in_the_missing_part_of_the_cube():
    """Complete rows of a mixed catalogue have the bits of the psi_cube methods on those rows alone, and a catalogue without NaN the bits
    of those methods; rows with nothing observed the bits of the missing_cov methods; NaN written into every missing row and column of
    the cube changes no bit."""
    n, d, m, k, nd = 900, 5, 24, 2, 3
    model = model_with_priors("VC", m, d, k, True, seed=26301)
    X = knock_out(catalogue(model, n, seed=302), seed=303)
    X[[7, 11, 500], :] = NAN
    cube = cube_of(n, d, seed=304)
    nan = np.isnan(X)
    dirty = cube.copy()
    for i in np.flatnonzero(nan.any(axis=1)):
        dirty[nan[i], :, i] = NAN
        dirty[:, nan[i], i] = NAN
    Xd, Cd = dev(X), dev(cube)
    groups, weights = setting(n, 2, seed=5)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        ref = three(p, Xd, Cd, nd=nd)
        assert all(bool(torch.isfinite(t).all()) for t in ref)
        full = torch.from_numpy(~nan.any(axis=1)).to(DEV)
        alone = tuple(p.predict_psi_cube_dev(Xd[full], Cd[:, :, full])) + \
            tuple(p.draws_psi_cube_dev(Xd[full], Cd[:, :, full], nd, seed=4, return_gamma=True))
        same(rows_of(ref, full), alone, "complete rows")
        same(three(p, Xd[full], Cd[:, :, full], nd=nd), alone, "a catalogue without NaN")
        none = torch.from_numpy(nan.all(axis=1)).to(DEV)
        plain = tuple(p.predict_missing_cov_dev(Xd[none])) + tuple(p.draws_missing_cov_dev(Xd[none], nd, seed=4, return_gamma=True))
        same(rows_of(ref, none), plain, "nothing observed")
        same(three(p, Xd, dev(dirty), nd=nd), ref, "NaN in the missing rows and columns of the cube")
        edges = np.linspace(*np.percentile(host(ref[0]), [3, 97]), 31)
        kw = dict(n_draws=nd, seed=4, groups=gd, n_groups=2, weights=wd)
        whole = p.stack_psi_cube_missing_dev(Xd, Cd, edges, **kw)
        same_stack(p.stack_psi_cube_missing_dev(Xd, dev(dirty), edges, **kw), whole, "stack with NaN in the missing part")
        same_stack(p.stack_psi_cube_missing_dev(Xd[full], Cd[:, :, full], edges, n_draws=nd, seed=4, groups=gd[full], n_groups=2,
                                                weights=wd[full]),
                   p.stack_psi_cube_dev(Xd[full], Cd[:, :, full], edges, n_draws=nd, seed=4, groups=gd[full], n_groups=2, weights=wd[full]),
                   "stack of a catalogue without NaN")


@pytest.mark.parametrize("method,m,k", [("VC", 40, 1), ("GC", 24, 3)])
def test_same_bits_over_tiles_row_orders_company_splits_and_draw_counts(method, m, k):
    n, d, nd = 1500, 5, 3
    model = model_with_priors(method, m, d, k, True, seed=26400 + m)
    X = knock_out(catalogue(model, n, seed=46), seed=47)
    cube = cube_of(n, d, seed=49)
    perm = np.random.default_rng(48).permutation(n)
    Xd, Cd, pd = dev(X), dev(cube), torch.from_numpy(perm).to(DEV)
    outs = []
    for tile in (256, 1024, None):
        with gpz_amd.Predictor(model, tile_rows=tile) as p:
            outs.append(three(p, Xd, Cd, nd=nd))
            if tile == 256:
                shuf = three(p, Xd[pd], Cd[:, :, pd], nd=nd)
                only = torch.from_numpy(np.isnan(X[:, 1]) & ~np.isnan(X[:, 4])).to(DEV)   # one group, the others removed
                group = three(p, Xd[only], Cd[:, :, only], nd=nd)
                halves = [three(p, Xd[:700], Cd[:, :, :700], nd=nd), three(p, Xd[700:], Cd[:, :, 700:], nd=nd)]
                more = three(p, Xd, Cd, nd=nd + 4)
    base = outs[0]
    for o in outs[1:]:
        same(o, base, "tile size")
    same(shuf, rows_of(base, pd), "row order")
    same(group, rows_of(base, only), "company")
    same([torch.cat([a, b], dim=0 if a.dim() == 2 else 1) for a, b in zip(*halves)], base, "two calls")
    same(more[:5] + (more[5][:nd], more[6][:nd]), base, "draw s does not depend on the draws behind it")


def test_layouts_of_the_cube_give_the_same_bits():
    """The cube contiguous as (d, d, n), as (n, d, d) under permute, column-major, as a strided view into a larger tensor of NaN, as
    float32 holding the same values, with its strict upper triangle overwritten with NaN; a selection."""
    n, d = 600, 5
    model = model_with_priors("VC", 30, d, 2, True, seed=26501)
    X = knock_out(catalogue(model, n, seed=182), seed=184)
    C32 = cube_of(n, d, seed=183).astype(np.float32)
    Xd, Cd = dev(X), dev(C32.astype(np.float64))
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        ref = three(p, Xd, Cd.contiguous())
        ndd = Cd.permute(2, 0, 1).contiguous()
        same(three(p, Xd, ndd.permute(1, 2, 0)), ref, "(n, d, d) under permute(1, 2, 0)")
        fortran = dev(np.asfortranarray(C32.astype(np.float64)).T.copy()).permute(2, 1, 0)
        assert fortran.stride() == (1, d, d * d)
        same(three(p, Xd, fortran), ref, "column-major d x d x n")
        big = torch.full((d + 1, d + 2, 2 * n + 3), NAN, dtype=torch.float64, device=DEV)
        big[1:, 2:, 3::2] = Cd
        same(three(p, Xd, big[1:, 2:, 3::2]), ref, "a strided view into a larger tensor")
        same(three(p, Xd, dev(C32, torch.float32)), ref, "float32")
        upper = Cd.clone()
        iu = torch.triu_indices(d, d, 1, device=DEV)
        upper[iu[0], iu[1], :] = NAN
        same(three(p, Xd, upper), ref, "NaN above the diagonal")
        sel = torch.zeros(n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        same(three(p, Xd, Cd, selection=sel), three(p, Xd[::2].contiguous(), Cd[:, :, ::2].contiguous()), "selection")


# ---- 3. draws ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
def test_draws_are_phi_times_the_drawn_weights(method):
    """Under Z = 0 every draw is predict's mu; seeded draws are PHI (w + R z_s) + muY with PHI from gpz_amd.predict(X, model, Psi=cube),
    R the Cholesky factor of the symmetric part of iSigma_w and z the Philox normals of the seed - both within the mu gate."""
    m, d, k, nd, n, seed = 40, 5, 2, 4, 500, 31
    model = model_with_priors(method, m, d, k, True, seed=26600)
    X = knock_out(catalogue(model, n, seed=78), seed=79)
    cube = cube_of(n, d, seed=80)
    res = gpz_amd.predict(X, model, Psi=cube)
    mu, PHI = np.array(res[0]), np.array(res[5])
    z = philox_normals(seed, m, nd, k)
    iS, w, muY = model.sets["best"]["iSigma_w"], model.sets["best"]["w"], np.asarray(model.muY).reshape(-1)
    L = [np.linalg.cholesky(0.5 * (iS[:, :, o] + iS[:, :, o].T)) for o in range(k)]
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F0 = host(p.draws_psi_cube_missing_dev(dev(X), dev(cube), nd, Z=np.zeros((m, nd, k))))
        F = host(p.draws_psi_cube_missing_dev(dev(X), dev(cube), nd, seed=seed))
    for s in range(nd):
        ws = np.stack([w[:, o] + L[o] @ z[:, s, o] for o in range(k)], axis=1)
        a, b = nrel(F0[s], mu), nrel(F[s], PHI @ ws + muY)
        print(f"{method} draw {s}: Z = 0 against predict's mu {a:.3e}; seeded against PHI w_s {b:.3e}")
        assert a <= GATES["mu"] and b <= GATES["mu"], (s, a, b)


# ---- 4. gamma per draw, against parent code ----------------------------------------------------------------------------------------------------
def parent_gamma(ms, X, cube):
    """gamma of the model ms by the parent's two routes with a cube and NaN: gpz_amd.predict(X, ms, Psi=cube) and the handle's host
    method Predictor.predict(X, Psi=cube); their spread."""
    a = np.array(gpz_amd.predict(X, ms, Psi=cube)[4])
    with gpz_amd.Predictor(ms) as q:
        b = np.array(q.predict(X, Psi=cube)[4])
    return a, nrel(b, a)


# (columns, k, d): NO = d - 1.  d = 3: 1, 16, 17, 64, 65, 128 | 129 (the pass edge of 8 blocks) and 257 (a third pass of one column);
# d = 7, NO = 6: 64 | 65, its pass edge of 4 blocks; d = 10, the widest NO: 128 | 129
@pytest.mark.parametrize("ncol,k,d", [(1, 1, 3), (16, 1, 3), (17, 1, 3), (64, 8, 3), (65, 1, 3), (128, 8, 3), (129, 1, 3), (257, 1, 3),
                                      (64, 1, 7), (65, 1, 7), (128, 8, 10), (129, 1, 10)])
def test_gamma_per_draw_with_exact_weights_over_the_column_counts(ncol, k, d):
    """iSigma_w = 2^-10 I, so w_s = w + 2^-5 z_s is the same double on host and device.  m = 17, the last dimension missing, 100 rows
    (a workgroup of 64 and one of 36), the first, the middle and the last draw."""
    m, n, nd = 17, 100, ncol // k
    model = exact_model(COV[ncol % 2], m, d, k, True, seed=26700 + ncol + d)
    X = catalogue(model, n, seed=ncol)
    X[:, d - 1] = NAN
    cube = cube_of(n, d, seed=ncol + 1)
    Z = np.random.default_rng(ncol).standard_normal((m, nd, k))
    W = exact_weights(model, Z)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        F, Gam = p.draws_psi_cube_missing_dev(dev(X), dev(cube), nd, Z=Z, return_gamma=True)
        assert p.route.endswith(gamma_tail(m)), p.route
        assert torch.equal(F, p.draws_psi_cube_missing_dev(dev(X), dev(cube), nd, Z=Z))
    Gam = host(Gam)
    assert Gam.shape == (nd, n, k) and np.isfinite(Gam).all()
    worst, spread = 0.0, 0.0
    for s in sorted({0, nd // 2, nd - 1}):
        ref, sp = parent_gamma(with_weights(model, W[:, s, :]), X, cube)
        worst, spread = max(worst, nrel(Gam[s], ref)), max(spread, sp)
    print(f"ncol={ncol} k={k} d={d}: worst nrel of gamma_s against predict of the w_s model {worst:.3g}; spread of the parent's two "
          f"routes {spread:.3g}")
    assert worst <= gate_of(spread), (worst, spread)


@pytest.mark.parametrize("method", COV)
def test_gamma_per_draw_with_seeded_draws(method):
    """Seeded draws of a general iSigma_w; w_s formed on the host as w + chol(sym(iSigma_w)) z_s with the Philox normals of the seed.
    Four patterns and complete rows (whose gamma_s is draws_psi_cube_dev's)."""
    m, d, k, nd, n, seed = 40, 5, 2, 3, 400, 31
    model = model_with_priors(method, m, d, k, True, seed=26800)
    X = knock_out(catalogue(model, n, seed=78), seed=79)
    cube = cube_of(n, d, seed=80)
    z = philox_normals(seed, m, nd, k)
    iS = model.sets["best"]["iSigma_w"]
    L = [np.linalg.cholesky(0.5 * (iS[:, :, o] + iS[:, :, o].T)) for o in range(k)]
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        Gam = host(p.draws_psi_cube_missing_dev(dev(X), dev(cube), nd, seed=seed, return_gamma=True)[1])
    figures = []
    for s in range(nd):
        ws = np.stack([model.sets["best"]["w"][:, o] + L[o] @ z[:, s, o] for o in range(k)], axis=1)
        ref, spread = parent_gamma(with_weights(model, ws), X, cube)
        figures.append((nrel(Gam[s], ref), spread))
        print(f"{method} draw {s}: nrel(gamma_s, predict of w_s) {figures[-1][0]:.3g}; spread of the parent's two routes {spread:.3g}")
    for s, (got, spread) in enumerate(figures):
        assert got <= gate_of(spread), (s, got, spread)


# ---- 5. stack ----------------------------------------------------------------------------------------------------------------------------
def stack_inputs(p, model, Xd, Cd, edges, n_draws, draw_kw, groups, weights, G):
    """torch_reference fed with the device's own per-row numbers (predict_psi_cube_missing_dev and draws_psi_cube_missing_dev with
    return_gamma=True), and the derived tolerances of tests/test_predictor_stack_missing.py with s_min over the new widths."""
    mu_t, sigma_t, _, beta_t = p.predict_psi_cube_missing_dev(Xd, Cd)[:4]
    Ft = S2t = None
    if n_draws:
        Ft, Gt = p.draws_psi_cube_missing_dev(Xd, Cd, n_draws, return_gamma=True, **draw_kw)
        Ft, S2t = Ft.contiguous(), beta_t[None] + torch.clamp(Gt, min=0.0)
    ref = torch_reference(mu_t, sigma_t, Ft, S2t, dev(edges), dev(groups, torch.int64), dev(weights), G)
    mu, sigma = host(mu_t), host(sigma_t)
    F, S2 = (None, None) if Ft is None else (host(Ft), host(S2t))
    n, k = mu.shape
    g, w = np.asarray(groups), np.asarray(weights, dtype=np.float64)
    cols = [mu] + ([] if F is None else list(F))
    muY = np.asarray(model.muY).reshape(-1)
    E = max(np.max(np.abs(np.asarray(edges)[None, :] - muY[:, None])), 0.0) + max(np.max(np.abs(c - muY)) for c in cols)
    s_min = np.sqrt(min(sigma.min(), S2.min() if S2 is not None else sigma.min()))
    W = np.array([w[g == gi].sum() for gi in range(G)])
    ng = np.array([(g == gi).sum() for gi in range(G)])
    tol_h = EPS * W * (ng + 64.0 * (1.0 + E / s_min))
    tol_m = np.empty((len(cols), G, k, 2))
    for c, m_ in enumerate(cols):
        for gi in range(G):
            r = g == gi
            tol_m[c, gi, :, 0] = ng[gi] * EPS * (w[r] @ np.abs(m_[r]))
            tol_m[c, gi, :, 1] = ng[gi] * EPS * (w[r] @ (m_[r] * m_[r]))
    return ref, tol_h, tol_m, ng * EPS * W


@pytest.mark.parametrize("method,k", [("VC", 1), ("GC", 3)])
def test_stack(method, k):
    """1500 rows in four patterns and complete rows on 256-row tiles, three groups with rows left out and random weights, 37 bins, no draws
    and 5 seeded draws, against the torch reduction of the device's own per-row numbers; column 0 of the call with draws is the call
    without draws bit for bit (predict_psi_cube_missing_dev's mu and sigma); the parts of a split into two calls add to the whole."""
    d, n, G, m, B = 5, 1500, 3, 30, 37
    model = model_with_priors(method, m, d, k, True, seed=26900 + k)
    X = knock_out(catalogue(model, n, seed=k + 40), seed=k + 42)
    X[13, :] = NAN
    cube = cube_of(n, d, seed=k + 41)
    Xd, Cd = dev(X), dev(cube)
    groups, weights = setting(n, G, seed=m)
    gd, wd = dev(groups, torch.int64), dev(weights)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        mu0 = host(p.predict_psi_cube_missing_dev(Xd, Cd)[0])
        edges = np.linspace(*np.percentile(mu0, [3, 97]), B + 1)
        res = {}
        for nd in (0, 5):
            ref, th, tm, tw = stack_inputs(p, model, Xd, Cd, edges, nd, dict(seed=77), groups, weights, G)
            kw = dict(n_draws=nd, seed=77, n_groups=G)
            res[nd] = p.stack_psi_cube_missing_dev(Xd, Cd, edges, groups=gd, weights=wd, **kw)
            assert res[nd].hist.shape == (1 + nd, G, k, B)
            assert_close(res[nd], ref, th, tm, tw, f"{method} k={k} draws={nd}")
            same_stack(res[nd], p.stack_psi_cube_missing_dev(Xd, Cd, edges, groups=gd, weights=wd, **kw), "the same call twice")
            parts = [p.stack_psi_cube_missing_dev(Xd[i:j], Cd[:, :, i:j], edges, groups=gd[i:j], weights=wd[i:j], **kw)
                     for i, j in ((0, 700), (700, n))]
            total = [parts[0][f] + parts[1][f] for f in range(4)]
            assert_close(gpz_amd.api.StackResult(*total, edges), ref, th, tm, tw, "two calls")
            for u, v, w in zip(parts[0][:4], parts[1][:4], res[nd][:4]):
                assert np.allclose(u + v, w, rtol=1e-12, atol=1e-12 * np.abs(w).max())
        same_stack([res[5].hist[:1], res[5].sum_w, res[5].sum_mu[:1], res[5].sum_mu2[:1]], res[0][:4], "column 0 of the call with draws")
        assert res[5].hist[1:].sum() > 0.0
        assert p.route.endswith(gamma_tail(m, stack=True)), p.route


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def raw_entries(p, x, cube, obs, k, nd=3, B=7):
    """The four C entries on one group with the outputs pre-filled with a sentinel: the return codes, the messages and the outputs."""
    n = x.shape[0]
    call = p._dev_begin(x.device)
    out = [torch.full((k, n), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
    F, F2, Gm = (torch.full((nd, k, n), -7.0, dtype=torch.float64, device=DEV) for _ in range(3))
    hist, sw, sm, sm2 = (np.full(s, -7.0) for s in ((1 + nd, 1, k, B), (1,), (1 + nd, 1, k), (1 + nd, 1, k)))
    edges = np.ascontiguousarray(np.tile(np.linspace(-3.0, 3.0, B + 1), (k, 1)))
    psi = (cube.data_ptr(), 1 if cube.dtype == torch.float32 else 0, cube.stride(0), cube.stride(1), cube.stride(2))
    lead = (call.h, *p._x_args(x), *psi, _lib.dptr(call.muX), _lib.dptr(call.sdX), _lib.dptr(call.div))
    pat = (_lib.dptr(p._priors), obs)
    rcs, msgs = [], []

    def note(rc):
        rcs.append(rc)
        msgs.append(p._lib.gpz_last_error().decode() if rc else "")

    L = p._lib
    note(L.gpz_predictor_run_psi_cube_missing_dev(*lead, _lib.dptr(call.muY), *pat, *(t.data_ptr() for t in out), call.stream))
    note(L.gpz_predictor_draws_psi_cube_missing_dev(*lead, _lib.dptr(call.muY), *pat, nd, 5, None, F.data_ptr(), call.stream))
    note(L.gpz_predictor_draws_gamma_psi_cube_missing_dev(*lead, _lib.dptr(call.muY), *pat, nd, 5, None, F2.data_ptr(), Gm.data_ptr(),
                                                          call.stream))
    note(L.gpz_predictor_stack_psi_cube_missing_dev(*lead, *pat, nd, 5, None, _lib.dptr(edges), B, None, 1, None, _lib.dptr(hist),
                                                    _lib.dptr(sw), _lib.dptr(sm), _lib.dptr(sm2), None, call.stream))
    torch.cuda.synchronize()
    return tuple(rcs), msgs, out + [F, F2, Gm] + [torch.from_numpy(a) for a in (hist, sw, sm, sm2)]


def test_bad_cubes_and_bad_rows_are_refused_with_the_outputs_untouched():
    """One group through the C entries, dimension 1 of 5 missing (mask 0b11101).  NaN, infinite or negative-diagonal Psi in an observed
    position, an overflow after the division and a row off the mask: GPZ_ERR_ARG, every output still the sentinel, and the handle works
    on the next call.  The same values in a missing row or column are never read."""
    n, d, k, obs = 2000, 5, 2, 0b11101
    model = model_with_priors("VC", 20, d, k, True, seed=27185)
    model.sdX = np.array(model.sdX, dtype=np.float64)
    model.sdX[0] = 1e-155                                                 # sdX[0]^2 is subnormal: a division by it can overflow
    scale = (model.sdX[:, None] * model.sdX[None, :])[:, :, None]
    Xh = catalogue(model, n, seed=186)
    Xh[:, 1] = NAN
    X, C = dev(Xh), dev(cube_of(n, d, seed=187) * scale)
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        good = three(p, X[:300], C[:, :, :300])
        assert all(bool(torch.isfinite(t).all()) for t in good)
        rcs, msgs, clean = raw_entries(p, X, C, obs, k)
        assert rcs == (0, 0, 0, 0), (rcs, msgs)
        assert all(bool((t != -7.0).all()) for t in clean)
        same(clean[:5], p.predict_psi_cube_missing_dev(X, C), "the C entry is what the method calls")
        off = X.clone()
        off[1501, 1] = 0.5                                                # a complete row in the group
        off2 = X.clone()
        off2[77, 3] = NAN                                                 # a row with one more dimension missing
        cases = [("a row off the mask", off, C), ("a row off the mask", off2, C)]
        for what, v, r, c, at in (("NaN on the diagonal", NAN, 4, 4, 1999), ("+inf on the diagonal", float("inf"), 0, 0, 0),
                                  ("a negative diagonal element", -1e-300, 2, 2, 1333), ("NaN below the diagonal", NAN, 3, 2, 77),
                                  ("an overflow after the division", 1e200, 2, 0, 1024)):
            bad = C.clone()
            bad[r, c, at] = v
            cases.append((what, X, bad))
        for what, x, cube in cases:
            rcs, msgs, outs = raw_entries(p, x, cube, obs, k)
            assert rcs == (ERR_ARG,) * 4, (what, rcs, msgs)
            assert all("psi_cube_missing_dev" in t for t in msgs), msgs
            assert all(bool((t == -7.0).all()) for t in outs), what        # refused before any tile kernel has run
            if x is X:                                                     # (the methods would regroup a row off the mask)
                with pytest.raises(_lib.GpzError, match="observed dimensions"):
                    p.predict_psi_cube_missing_dev(x, cube)
                with pytest.raises(_lib.GpzError):
                    p.draws_psi_cube_missing_dev(x, cube, 3, return_gamma=True)
                with pytest.raises(_lib.GpzError):
                    p.stack_psi_cube_missing_dev(x, cube, np.linspace(-3.0, 3.0, 8), n_draws=2)
            same(three(p, X[:300], C[:, :, :300]), good, "the handle works on the next call")
        unread = C.clone()
        unread[1, :, :] = NAN                                              # the missing row and column, and above the diagonal
        unread[:, 1, :] = float("inf")
        unread[0, 2, 99] = NAN
        rcs, _, outs = raw_entries(p, X, unread, obs, k)
        assert rcs == (0, 0, 0, 0)
        same(outs, clean, "Psi in the missing dimension is never read")
        # a mask without a missing dimension and a mask with a bit at d: the arguments' own refusals
        assert raw_entries(p, X, C, 0b11111, k)[0] == (ERR_ARG,) * 4 and raw_entries(p, X, C, 0b111101, k)[0] == (ERR_ARG,) * 4


def test_models_outside_the_scope_are_refused_by_name():
    """A diagonal kind, d = 11 and m = 257 through the C entries: GPZ_ERR_UNSUPPORTED naming the function and where such rows go, the
    outputs untouched; a 2-D Psi is a ValueError of the methods before the GPU is touched."""
    for kw, word in ((dict(method="VD", m=20, d=5), "diagonal kind"), (dict(method="VC", m=20, d=11), "predict_missing_cov_fits"),
                     (dict(method="GC", m=257, d=3), "predict_missing_cov_fits")):
        d, k = kw["d"], 1
        model = model_with_priors(kw["method"], kw["m"], d, k, True, seed=27300 + d)
        Xh = catalogue(model, 50, seed=d)
        Xh[:, 1] = NAN
        X, C = dev(Xh), dev(cube_of(50, d, seed=d + 1))
        with gpz_amd.Predictor(model) as p:
            rcs, msgs, outs = raw_entries(p, X, C, ((1 << d) - 1) & ~2, k)
            assert rcs == (ERR_UNSUPPORTED,) * 4, (kw, rcs, msgs)
            assert all(word in t and "psi_cube_missing_dev" in t for t in msgs), msgs
            assert all(bool((t == -7.0).all()) for t in outs), kw
            with pytest.raises(ValueError, match=word.replace("_", ".")):
                p.predict_psi_cube_missing_dev(X, C)
            with pytest.raises(ValueError, match="d x d x n cube"):
                p.predict_psi_cube_missing_dev(X, C[0].T.contiguous())
            assert bool(torch.isfinite(p.predict_dev(dev(catalogue(model, 50, seed=d)))[0]).all())   # the handle is usable


def test_a_matrix_that_is_not_positive_semidefinite_gives_nan_on_its_row_only():
    n, d, k = 500, 5, 2
    model = model_with_priors("VC", 24, d, k, True, seed=27400)
    Xh = knock_out(catalogue(model, n, seed=5), seed=6)
    Xh[123, :] = catalogue(model, 1, seed=7)[0]
    Xh[123, 1] = NAN
    X, C = dev(Xh), dev(cube_of(n, d, seed=8))
    odd = C.clone()
    odd[2, 0, 123] = odd[0, 2, 123] = -1e6                                  # passes the scan; M + Psi_oo has a negative pivot
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[123] = False
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        ref, broken = three(p, X, C), three(p, X, odd)
    same(rows_of(broken, keep), rows_of(ref, keep), "every row but the indefinite one")
    assert bool(torch.isnan(broken[0][123]).all()) and bool(torch.isnan(broken[4][123]).all())


# ---- 7. memory ---------------------------------------------------------------------------------------------------------------------------
def test_memory_is_added_once_and_never_grows_with_rows_or_patterns():
    """a handle that has served the noisy_missing_cov entries on the same pattern and the psi_cube entries holds
    everything the new entries need - the first call adds no byte; ten times the rows and eight patterns add none either; and a handle
    that never makes these calls keeps its bytes and its route text."""
    d, nd, m, k, T = 5, 4, 30, 1, 256
    model = model_with_priors("VC", m, d, k, True, seed=27500)
    n = 4000
    Xh = catalogue(model, n, seed=196)
    one = Xh[:400].copy()
    one[:, 1] = NAN
    rng = np.random.default_rng(9)
    many = Xh.copy()
    pats = [(0,), (1,), (2,), (3,), (4,), (0, 1), (2, 3), (1, 2, 4)]
    for i in range(n):
        many[i, list(pats[rng.integers(0, 8)])] = NAN
    Psi, C = dev(noise(n, d, seed=197)), dev(cube_of(n, d, seed=198))
    X1, Xm, Xc = dev(one), dev(many), dev(Xh)
    with gpz_amd.Predictor(model, tile_rows=T) as p, gpz_amd.Predictor(model, tile_rows=T) as q:
        for h in (p, q):
            h.draws_noisy_missing_cov_dev(X1, Psi[:400], nd, return_gamma=True)
            h.predict_noisy_missing_cov_dev(X1, Psi[:400])
            h.draws_psi_cube_dev(Xc[:400], C[:, :, :400], nd, return_gamma=True)
            h.predict_psi_cube_dev(Xc[:400], C[:, :, :400])
        held, text = p.info[1], p.route
        assert (held, text) == (q.info[1], q.route)
        small = three(p, X1, C[:, :, :400], nd=nd)
        assert p.info[1] == held, (p.info[1] - held)                        # nothing is built twice
        assert p.route == text + pairs_tail(m) + gamma_tail(m), p.route
        three(p, Xm, C, nd=nd)
        three(p, X1, C[:, :, :400], nd=nd)
        assert p.info[1] == held
        same(three(p, X1, C[:, :, :400], nd=nd), small, "the same bits afterwards")
        assert (q.info[1], q.route) == (held, text)
    with gpz_amd.Predictor(model, tile_rows=T) as r:                        # on a fresh handle: the same bytes for 400 rows and 4000
        three(r, X1, C[:, :, :400], nd=nd)
        first = r.info[1]
        three(r, Xm, C, nd=nd)
        assert r.info[1] == first
