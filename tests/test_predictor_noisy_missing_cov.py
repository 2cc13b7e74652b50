"""Rows with input noise and missing inputs for the covariance kinds on the predictor handle (Predictor.predict_noisy_missing_cov_dev /
draws_noisy_missing_cov_dev, gpz_predictor_run_noisy_missing_cov_dev / _draws_noisy_missing_cov_dev; k_predict_noisy_missing_cov.hip)
against the one-shot predictNoisyMissing route, gpz_amd.predict(X, model, Psi=Psi), and the oracle: parity over GC and VC, every width and
every number of observed dimensions, the edges in m, the row counts of a group, the same bits over tiles, orders, company, splits and
layouts, Psi in the missing dimensions, Psi = 0, the draws, the refusals of the C entries and the memory of the handle.  Several patterns
of these tests have an [observed | missing] order that is not its own inverse, where predictCov.m:271-273 scatters T Psi T' through
`unshuffle`: the route keeps that, or parity with predict() would stop at 1e-2."""
import math

import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from helpers import rel
from oracle import gpz_oracle as O
from test_predictor import catalogue, nrel, synth_model
from test_predictor_draws_cpu import philox_normals
from test_predictor_missing import knock_out, model_with_priors
from test_predictor_missing_cov_cpu import chunks_rule
from test_predictor_noisy import noise
from test_predictor_noisy_missing import check_gamma_sign, reference
from test_predictor_noisy_missing_cov_cpu import slabs_rule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COV = ("GC", "VC")
NAMES = ("mu", "sigma", "nu", "beta_i", "gamma")
NAN = float("nan")
# the largest nrel against gpz_amd.predict(X, model, Psi=Psi) seen on an MI355X over the comparisons of this file, per output
GATE_SEEN = {"mu": 1.4e-15, "sigma": 1.5e-14, "nu": 1.2e-15, "beta_i": 2.4e-16, "gamma": 2.2e-14}   # over the 55 comparisons of this file
# ten times that, rounded up to a power of ten (the rule of tests/test_predictor_missing_cov.py); none may be looser than 1e-9
GATES = {name: 10.0 ** math.ceil(math.log10(10.0 * v) - 1e-12) for name, v in GATE_SEEN.items()}
assert GATES == {"mu": 1e-13, "sigma": 1e-12, "nu": 1e-13, "beta_i": 1e-14, "gamma": 1e-12} and all(g <= 1e-9 for g in GATES.values())
# (against the oracle on 60 rows at m = 7, at most: mu 1.5e-15, sigma 1.8e-14, nu 1.6e-15, beta_i 4.5e-16, gamma 2.8e-14)


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


def both(p, x, psi, nd=3, seed=9, **kw):
    return tuple(p.predict_noisy_missing_cov_dev(x, psi, **kw)) + (p.draws_noisy_missing_cov_dev(x, psi, nd, seed=seed, **kw),)


def same(a, b, what=""):
    for i, (s, t) in enumerate(zip(a, b)):
        assert torch.equal(s, t), (what, i)


def suffix(m):
    return f"; noisy missing: k_predict_noisy_missing_cov_pairs ({chunks_rule(m)} pair chunks)"


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", COV)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_parity_with_predict_and_the_oracle(method, hetero, k):
    """m = 7 and 50: 2500 rows over 1024-row tiles, Psi on every row, dimension 1 missing on 20 % and dimension 4 on 10 % of the rows
    independently, one row with only dimension 0 observed and one with nothing observed.  m = 250: 300 rows in two patterns, whose
    pair-component records pass through several slabs."""
    d = 5
    for m in (7, 50, 250):
        ns = 300 if m == 250 else 2500
        model = model_with_priors(method, m, d, k, hetero, seed=7000 * COV.index(method) + 100 * hetero + 10 * k + m)
        X = catalogue(model, ns, seed=m)
        if m == 250:
            X[:150, 1] = NAN
            X[150:, 4] = NAN
            assert slabs_rule(m, d, 4) > 1
        else:
            X = knock_out(X, seed=m + 1)
            X[5, 1:] = NAN
            X[9, :] = NAN
        Psi = noise(ns, d, seed=m + 2)
        full = ~np.isnan(X).any(axis=1)
        ref = reference(X, Psi, model)
        with gpz_amd.Predictor(model, tile_rows=1024) as p:
            out = p.predict_noisy_missing_cov_dev(dev(X), dev(Psi))
            assert p.route.endswith(suffix(m)), p.route
            check_parity(out, ref)
            check_gamma_sign(out, X)
            if full.any():
                alone = p.predict_noisy_cov_dev(dev(X[full]), dev(Psi[full]))
                fd = torch.from_numpy(full).to(DEV)
                assert all(torch.equal(a[fd], b) for a, b in zip(out, alone))
            if m == 7:
                orc = O.predict_any(X[:60], model, Psi=Psi[:60])
                for name, a, b in zip(NAMES, out, orc):
                    print(f"oracle rel {name}: {rel(host(a)[:60], b):.3e}")
                    assert rel(host(a)[:60], b) <= 1e-8, (name, rel(host(a)[:60], b))


# ---- 2. every width and every number of observed dimensions --------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(range(1, 11)))
def test_every_width_and_every_number_of_observed_dimensions(d):
    """Bit 0 alone missing, bit d - 1 alone missing, a single observed dimension (each of the two ends), nothing observed: NO = d - 1,
    1 and 0 at every d, so NO = 0 .. 9 between them."""
    n, m, k = 300, 20, 1 if d % 2 else 8
    for method in COV:
        model = model_with_priors(method, m, d, k, True, seed=1400 + d)
        X = catalogue(model, n, seed=d)
        X[0:60, 0] = NAN
        if d > 1:
            X[60:120, d - 1] = NAN
            X[120:125, 1:] = NAN                                           # only dimension 0 observed
            X[125:130, :d - 1] = NAN                                       # only dimension d - 1 observed
            X[130, :] = NAN
        Psi = noise(n, d, seed=d + 50)
        ref = reference(X, Psi, model)
        with gpz_amd.Predictor(model) as p:
            out = p.predict_noisy_missing_cov_dev(dev(X), dev(Psi))
            check_parity(out, ref)
            check_gamma_sign(out, X)
            F = p.draws_noisy_missing_cov_dev(dev(X), dev(Psi), 2, Z=np.zeros((m, 2, k)))
            assert nrel(host(F[1]), host(out[0])) <= 1e-12


# ---- 3. the edges in m ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 15, 16, 17, 31, 32, 33, 255, 256])
def test_edges_in_m(m):
    """m at the edges of the record stages and of the chunk rule (pairs / 32: it changes at m = 11, 16, 23, 32).  One pattern: dimension 1
    missing of d = 3; at most 128 rows at the large m."""
    d, n, k = 3, 128 if m > 64 else 300, 1 if m % 2 else 2
    model = model_with_priors("VC", m, d, k, bool(m % 3), seed=1800 + 10 * m)
    X = catalogue(model, n, seed=m)
    X[:, 1] = NAN
    Psi = noise(n, d, seed=m + 9)
    ref = reference(X, Psi, model)
    with gpz_amd.Predictor(model) as p:
        out = p.predict_noisy_missing_cov_dev(dev(X), dev(Psi))
        check_parity(out, ref)
        check_gamma_sign(out, X)
        assert p.route.endswith(suffix(m)), p.route
        F = p.draws_noisy_missing_cov_dev(dev(X), dev(Psi), 2, Z=np.zeros((m, 2, k)))
        assert nrel(host(F[0]), host(out[0])) <= 1e-12


# ---- 4. every row count of a group ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_every_row_count_of_a_group(k):
    """A group of n rows at the edges of the 64-row workgroups and the 256-row blocks of the Ex and PHI kernels and one above the handle's
    tile: parity on the longest call, and every shorter one is its first rows bit for bit, moments and draws."""
    d, m, nd = 5, 17, 3
    model = model_with_priors("VC", m, d, k, True, seed=1950 + k)
    X = catalogue(model, 1025, seed=93)
    X[:, 2] = NAN
    Psi = noise(1025, d, seed=94)
    ref = reference(X, Psi, model)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        Xd, Pd = dev(X), dev(Psi)
        full = both(p, Xd, Pd, nd, seed=3)
        check_parity(full[:5], ref)
        for n in (1, 63, 64, 65, 255, 256, 257):
            out = both(p, Xd[:n], Pd[:n], nd, seed=3)
            assert all(o.shape == (n, k) and torch.equal(o, f[:n]) for o, f in zip(out[:5], full[:5])), n
            assert torch.equal(out[5], full[5][:, :n]), n


# ---- 5. the same bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,m,k", [("VC", 40, 1), ("GC", 24, 3)])
def test_same_bits_over_tiles_row_orders_company_and_splits(method, m, k):
    n, d, nd = 3000, 5, 5
    model = model_with_priors(method, m, d, k, True, seed=145 + m)
    X = knock_out(catalogue(model, n, seed=46), seed=47)
    Psi = noise(n, d, seed=49)
    perm = np.random.default_rng(48).permutation(n)
    Xd, Pd, pd = dev(X), dev(Psi), torch.from_numpy(perm).to(DEV)
    outs = []
    for tile in (1024, None):
        with gpz_amd.Predictor(model, tile_rows=tile) as p:
            outs.append(both(p, Xd, Pd, nd))
            if tile == 1024:
                shuf = both(p, Xd[pd], Pd[pd], nd)
                only = torch.from_numpy(np.isnan(X[:, 1]) & ~np.isnan(X[:, 4])).to(DEV)   # one group, the others removed
                group = both(p, Xd[only], Pd[only], nd)
                halves = [both(p, Xd[:1300], Pd[:1300], nd), both(p, Xd[1300:], Pd[1300:], nd)]
    base = outs[0]
    same(outs[1], base, "tile size")
    same(shuf[:5], [b[pd] for b in base[:5]], "row order")
    assert torch.equal(shuf[5], base[5][:, pd])
    same(group[:5], [b[only] for b in base[:5]], "company")
    assert torch.equal(group[5], base[5][:, only])
    same([torch.cat([a, b]) for a, b in zip(halves[0][:5], halves[1][:5])], base[:5], "split")
    assert torch.equal(torch.cat([halves[0][5], halves[1][5]], dim=1), base[5])


def test_layouts_of_x_and_psi_give_the_same_bits():
    """float32, transposed storage, row-sliced views, Psi as (n, 1) and (n,): each is the call on a contiguous float64 copy of the same
    values, bit for bit."""
    n, d, nd = 700, 5, 4
    model = model_with_priors("VC", 20, d, 2, True, seed=184)
    X32 = knock_out(catalogue(model, 2 * n, seed=85), seed=86).astype(np.float32)
    P32 = noise(2 * n, d, seed=87).astype(np.float32)
    Xd, Pd = dev(X32.astype(np.float64)), dev(P32.astype(np.float64))     # the same values as float64
    with gpz_amd.Predictor(model, tile_rows=256) as p:
        ref = both(p, Xd.contiguous(), Pd.contiguous(), nd)
        same(both(p, dev(X32, torch.float32), dev(P32, torch.float32), nd), ref, "float32")
        same(both(p, Xd, dev(P32, torch.float32), nd), ref, "float32 Psi")
        same(both(p, Xd.T.contiguous().T, Pd.T.contiguous().T, nd), ref, "transposed storage")
        half = both(p, Xd[::2].contiguous(), Pd[::2].contiguous(), nd)
        same(both(p, Xd[::2], Pd[::2], nd), half, "row-sliced views")
        same([t[::2] if t.dim() == 2 else t[:, ::2] for t in ref], half, "rows of the whole call")
        col = Pd[:, 2].contiguous()
        bc = both(p, Xd, col[:, None].expand(2 * n, d).contiguous(), nd)
        same(both(p, Xd, col[:, None], nd), bc, "Psi (n, 1)")
        same(both(p, Xd, Pd[:, 2], nd), bc, "Psi (n,) strided")
        sel = torch.zeros(2 * n, dtype=torch.bool, device=DEV)
        sel[::2] = True
        same(both(p, Xd, Pd, nd, selection=sel), half, "selection")


# ---- 6. Psi in the missing dimensions ------------------------------------------------------------------------------------------------------
def raw_call(p, Xg, psi, obs, k, nd=3):
    """The two C entries on one group with the outputs preset to -7: (rc of run, rc of draws, the six outputs, the run's message)."""
    ng = Xg.shape[0]
    muX, sdX, muY = p._norm_vectors()
    sd2 = np.ascontiguousarray(sdX ** 2)
    stream = torch.cuda.current_stream(Xg.device).cuda_stream
    out = [torch.full((k, ng), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
    F = torch.full((nd, k, ng), -7.0, dtype=torch.float64, device=DEV)
    lead = [p._handle(), *p._x_args(Xg), *p._psi_args(psi, ng), _lib.dptr(muX), _lib.dptr(sdX), _lib.dptr(sd2), _lib.dptr(muY),
            _lib.dptr(p._priors), obs]
    rc1 = p._lib.gpz_predictor_run_noisy_missing_cov_dev(*lead, *(t.data_ptr() for t in out), stream)
    msg = p._lib.gpz_last_error().decode() if rc1 else ""
    rc2 = p._lib.gpz_predictor_draws_noisy_missing_cov_dev(*lead, nd, 5, None, F.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc1, rc2, out + [F], msg


def test_psi_in_missing_dimensions_is_not_read():
    """NaN, inf and -1 in Psi where X is NaN change no bit; the same values in an observed dimension are refused by the C entries with the
    outputs untouched; a group with nothing observed reads no Psi and has the bits of the entries without Psi."""
    n, d, k, nd, m = 2000, 5, 2, 3, 20
    model = model_with_priors("VC", m, d, k, True, seed=188)
    X = knock_out(catalogue(model, n, seed=89), seed=90)
    X[7, :] = NAN
    X[11, :] = NAN
    Psi = noise(n, d, seed=91)
    nan = np.isnan(X)
    Xd, Pd = dev(X), dev(Psi)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        ref = both(p, Xd, Pd, nd, seed=2)
        for v in (NAN, float("inf"), -1.0):
            bad = Psi.copy()
            bad[nan] = v
            same(both(p, Xd, dev(bad), nd, seed=2), ref, v)
        none = torch.from_numpy(nan.all(axis=1)).to(DEV)                    # nothing observed: the entries without Psi, bit for bit
        plain = tuple(p.predict_missing_cov_dev(Xd[none])) + (p.draws_missing_cov_dev(Xd[none], nd, seed=2),)
        same([t[none] for t in ref[:5]] + [ref[5][:, none]], plain, "nothing observed")
        g = np.flatnonzero(~nan[:, 1] & nan[:, 4])                          # one group through the C entries: dimension 4 missing
        Xg, Pg, ng = dev(X[g]), Psi[g].copy(), g.size
        good = p.predict_noisy_missing_cov_dev(Xg, dev(Pg))
        rc1, rc2, outs, _ = raw_call(p, Xg, dev(Pg), 0b01111, k)
        assert rc1 == 0 and rc2 == 0 and all(bool((t != -7.0).all()) for t in outs)
        same(outs[:5], good, "the C entry")
        for v, at, c in ((NAN, ng - 1, 3), (float("inf"), 0, 0), (-1e-300, ng // 2, 2)):
            bad = Pg.copy()
            bad[at, c] = v
            rc1, rc2, outs, msg = raw_call(p, Xg, dev(bad), 0b01111, k)
            assert rc1 == -1 and rc2 == -1, (v, rc1, rc2)                   # GPZ_ERR_ARG
            assert "Psi has an element that is NaN, infinite or negative" in msg, msg
            assert all(bool((t == -7.0).all()) for t in outs), v            # refused before any tile kernel has run
            miss = Pg.copy()
            miss[at, 4] = v                                                 # the same value where the group's X is NaN: taken
            rc1, rc2, outs, _ = raw_call(p, Xg, dev(miss), 0b01111, k)
            assert rc1 == 0 and rc2 == 0
            same(outs[:5], good, v)
        with pytest.raises(_lib.GpzError, match="Psi"):                     # and through the method: in the row's observed dimensions
            p.predict_noisy_missing_cov_dev(Xd, dev(np.where(nan, Psi, -1.0)))


# ---- 7. Psi = 0 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,k", [("VC", 1), ("GC", 3)])
def test_zero_noise_is_the_prediction_for_missing_inputs(method, k):
    """On the rows with missing values all five outputs and the draws agree with predict_missing_cov_dev / draws_missing_cov_dev within the
    gates of this file (the record form differs, so the bits need not be the same)."""
    n, d, m, nd = 600, 5, 30, 3
    model = model_with_priors(method, m, d, k, True, seed=160 + k)
    X = knock_out(catalogue(model, n, seed=61), seed=62, cols=((1, 0.4), (4, 0.3)))
    X[3, :] = NAN
    miss = np.isnan(X).any(axis=1)
    Xd = dev(X[miss])
    zero = torch.zeros((int(miss.sum()), d), dtype=torch.float64, device=DEV)
    with gpz_amd.Predictor(model) as p:
        z = both(p, Xd, zero, nd)
        f = tuple(p.predict_missing_cov_dev(Xd)) + (p.draws_missing_cov_dev(Xd, nd, seed=9),)
    assert miss.sum() > 100
    for name, a, b in zip(NAMES, z, f):
        print(f"zero noise nrel {name}: {nrel(host(a), host(b)):.3e}")
        assert nrel(host(a), host(b)) <= GATES[name], (name, nrel(host(a), host(b)))
    assert nrel(host(z[5]), host(f[5])) <= GATES["mu"]


# ---- 8. draws ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_draws_are_phi_against_the_weight_draws(k):
    n, d, m = 200, 4, 30
    model = model_with_priors("VC", m, d, k, True, seed=175 + k)
    X = knock_out(catalogue(model, n, seed=76), seed=77, cols=((0, 0.3), (2, 0.3)))
    Psi = noise(n, d, seed=78)
    Xd, Pd = dev(X), dev(Psi)
    with gpz_amd.Predictor(model) as p:
        PHI = np.array(gpz_amd.predict(X, model, Psi=Psi)[5])
        mu = host(p.predict_noisy_missing_cov_dev(Xd, Pd)[0])
        F0 = host(p.draws_noisy_missing_cov_dev(Xd, Pd, 3, Z=np.zeros((m, 3, k))))
        assert all(nrel(F0[s], mu) <= 1e-12 for s in range(3))
        seeded = p.draws_noisy_missing_cov_dev(Xd, Pd, 7, seed=12345)
        Z = philox_normals(12345, m, 7, k)
        st = model.sets["best"]
        want = np.empty((7, n, k))
        for o in range(k):
            S = 0.5 * (st["iSigma_w"][:, :, o] + st["iSigma_w"][:, :, o].T)
            W = st["w"][:, o:o + 1] + np.linalg.cholesky(S) @ Z[:, :, o]   # m x nd
            want[:, :, o] = (PHI @ W).T + model.muY[o]
        print(f"draws against PHI (w + R z) + muY: {nrel(host(seeded), want):.3e}")
        assert nrel(host(seeded), want) <= 1e-12, nrel(host(seeded), want)
        assert nrel(host(seeded), host(p.draws_noisy_missing_cov_dev(Xd, Pd, 7, Z=Z))) <= 1e-12
        full = torch.from_numpy(~np.isnan(X).any(axis=1)).to(DEV)          # one weight draw serves all groups: the complete rows alone
        assert torch.equal(seeded[:, full], p.draws_noisy_cov_dev(Xd[full], Pd[full], 7, seed=12345))
        more = p.draws_noisy_missing_cov_dev(Xd, Pd, 11, seed=12345)       # draw s is the same for any n_draws > s
        assert torch.equal(more[:7], seeded)


# ---- 9. refusals at the C entries -----------------------------------------------------------------------------------------------------------
def test_a_mixed_pattern_is_refused_with_the_outputs_untouched():
    n, d, k = 3000, 5, 2
    model = model_with_priors("VC", 12, d, k, True, seed=288)
    Xh = catalogue(model, n, seed=89)
    Xh[:, 3] = NAN
    X, Psi = dev(Xh), dev(noise(n, d, seed=92))
    mask = 0b10111
    with gpz_amd.Predictor(model, tile_rows=1 << 11) as p:
        good = p.predict_noisy_missing_cov_dev(X[:500], Psi[:500])
        rc1, rc2, outs, _ = raw_call(p, X, Psi, mask, k)
        assert rc1 == 0 and rc2 == 0 and all(bool((t != -7.0).all()) for t in outs)
        same([a[:500] for a in outs[:5]], good)
        two = X.clone()
        two[2500:, 0] = NAN                                                # two patterns in one group
        for what, x, obs, text in (("two patterns", two, mask, "share one NaN pattern"),
                                   ("full mask", X, 0b11111, "no dimension is missing"), ("mask past d", X, 0b110111, "above d")):
            rc1, rc2, outs, msg = raw_call(p, x, Psi, obs, k)
            assert rc1 == -1 and rc2 == -1, (what, rc1, rc2)               # GPZ_ERR_ARG
            assert text in msg, (what, msg)
            assert all(bool((t == -7.0).all()) for t in outs), what         # refused before any tile kernel has run
        same(p.predict_noisy_missing_cov_dev(X[:500], Psi[:500]), good)     # the handle works on the next call


@pytest.mark.parametrize("kw", [{"method": "VD"}, {"d": 11}, {"m": 257}, {"k": 9}])
def test_shapes_outside_the_route_are_refused_by_the_c_entries(kw):
    a = {"method": "VC", "m": 12, "d": 5, "k": 1}
    a.update(kw)
    model = synth_model(a["method"], a["m"], a["d"], a["k"], True, seed=5)
    n = 40
    X = catalogue(model, n, seed=6)
    X[:, 1] = NAN
    Psi = noise(n, a["d"], seed=7)
    diag = a["method"] == "VD"
    with gpz_amd.Predictor(model) as p:
        with pytest.raises(ValueError, match=r"predict_noisy_missing_dev\(X, Psi\)" if diag else "Predictor.predict"):
            p.predict_noisy_missing_cov_dev(dev(X), dev(Psi))
        muX, sdX, muY = p._norm_vectors()
        out = [torch.full((a["k"], n), -7.0, dtype=torch.float64, device=DEV).T for _ in range(5)]
        F = torch.full((4, a["k"], n), -7.0, dtype=torch.float64, device=DEV)
        lead = [p._handle(), *p._x_args(dev(X)), *p._psi_args(dev(Psi), n), _lib.dptr(muX), _lib.dptr(sdX),
                _lib.dptr(np.ascontiguousarray(sdX ** 2)), _lib.dptr(muY), None, (1 << a["d"]) - 3]
        for name, call in (("gpz_predictor_run_noisy_missing_cov_dev",
                            lambda: p._lib.gpz_predictor_run_noisy_missing_cov_dev(*lead, *(t.data_ptr() for t in out), None)),
                           ("gpz_predictor_draws_noisy_missing_cov_dev",
                            lambda: p._lib.gpz_predictor_draws_noisy_missing_cov_dev(*lead, 4, 0, None, F.data_ptr(), None))):
            with pytest.raises(_lib.GpzError, match="gpz_predictor_run_noisy_missing_dev" if diag else name) as ei:
                _lib.check(call())
            assert ei.value.code == -5                                     # GPZ_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in out + [F])
        assert "missing" not in p.route


# ---- 10. memory ----------------------------------------------------------------------------------------------------------------------------
def test_memory_is_added_once_and_never_grows_with_rows_or_patterns():
    d, nd = 5, 4
    model = model_with_priors("VC", 16, d, 1, True, seed=197)
    n = 30_000
    gen = torch.Generator(device=DEV).manual_seed(98)
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=gen) * torch.from_numpy(model.sdX).to(DEV) + \
        torch.from_numpy(model.muX).to(DEV)
    Psi = 0.05 * torch.rand((n, d), dtype=torch.float64, device=DEV, generator=gen)
    two = X.clone()
    two[torch.rand(n, device=DEV, generator=gen) < 0.2, 1] = NAN
    six = two.clone()
    for c in (0, 4):
        six[torch.rand(n, device=DEV, generator=gen) < 0.3, c] = NAN
    with gpz_amd.Predictor(model, tile_rows=1 << 12) as p, gpz_amd.Predictor(model, tile_rows=1 << 12) as q:
        def usual(h):                                                        # the row kinds a covariance handle had before
            h.predict_dev(X[:1000]); h.draws_dev(X[:1000], nd)
            h.predict_noisy_cov_dev(X[:1000], Psi[:1000]); h.draws_noisy_cov_dev(X[:1000], Psi[:1000], nd)
            h.predict_missing_cov_dev(two[:1000]); h.draws_missing_cov_dev(two[:1000], nd)
        usual(q)                                                             # a handle that never makes such a call ...
        usual(p)
        held, route = p.info[1], p.route
        assert held == q.info[1] and route == q.route and "noisy missing" not in route
        small = p.predict_noisy_missing_cov_dev(two[:3000], Psi[:3000])
        p.draws_noisy_missing_cov_dev(two[:3000], Psi[:3000], nd)
        first = p.info[1]
        assert first > held and p.route.startswith(route) and p.route[len(route):] == suffix(16), p.route
        out = p.predict_noisy_missing_cov_dev(two, Psi)
        p.draws_noisy_missing_cov_dev(two, Psi, nd)
        assert p.info[1] == first                                            # ten times the rows: the same bytes
        assert all(torch.equal(a, b[:3000]) for a, b in zip(small, out))
        assert len(p._nan_groups_dev(two)) == 2 and len(p._nan_groups_dev(six)) == 8   # four more patterns, and two more
        p.predict_noisy_missing_cov_dev(six[:5000], Psi[:5000])
        p.draws_noisy_missing_cov_dev(six[:5000], Psi[:5000], nd)
        assert p.info[1] == first                                            # more patterns: the same bytes
        usual(q)
        assert q.info[1] == held and q.route == route                        # ... holds what it held and says what it said
