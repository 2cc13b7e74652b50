"""Device-resident entries of the streaming predictor (Predictor.predict_dev / draws_dev / stack_dev) on the GPU.  The yardstick is the
host entry of the same handle: the same tile kernels on the same normalised bits must give the same bits, so every comparison is
np.array_equal, never a tolerance."""
import numpy as np
import pytest
import torch

import gpz_amd
from gpz_amd import _lib
from test_predictor import METHODS, catalogue, synth_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def host(t):
    return t.cpu().numpy()


def layouts(X):
    """X (n x d, float64, on the device) as row-major, column-major and as every second column of an (n, 2d) tensor."""
    wide = torch.empty((X.shape[0], 2 * X.shape[1]), dtype=X.dtype, device=X.device)
    wide[:, ::2] = X
    wide[:, 1::2] = float("nan")                                         # never read
    return {"row-major": X.contiguous(), "column-major": X.T.contiguous().T, "strided view": wide[:, ::2]}


def assert_same(dev, ref, what):
    assert len(dev) == len(ref)
    for i, (a, b) in enumerate(zip(dev, ref)):
        a = host(a)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape)
        assert np.array_equal(a, b), (what, i, float(np.max(np.abs(a - b))))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("hetero", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_bit_parity_with_predict(method, hetero, k):
    """ns = 2500 over 1024-row tiles (the last one partial), the fused route (m = 50) and the tile route (m = 300), every layout of X."""
    d, ns = 5, 2500
    for m in (50, 300):
        model = synth_model(method, m, d, k, hetero, seed=1000 * METHODS.index(method) + 100 * hetero + 10 * k + m)
        Xh = catalogue(model, ns, seed=m)
        X = torch.from_numpy(Xh).to(DEV)
        with gpz_amd.Predictor(model, tile_rows=1024) as p:
            assert p.info[2] == (0 if m == 50 else 1), p.route
            ref = p.predict(Xh)
            ref_phi = p.predict(Xh, return_phi=True)
            runs = p.info[3]
            for name, Xl in layouts(X).items():
                assert torch.equal(Xl, X)
                assert_same(p.predict_dev(Xl), ref, (m, name))
                assert_same(p.predict_dev(Xl, return_phi=True), ref_phi, (m, name, "phi"))
            assert p.info[3] == runs + 6 and p.route.endswith("; device entries: k_pred_stage"), p.route
            X32 = X.float()
            ref32 = p.predict(host(X32.double()), return_phi=True)
            assert_same(p.predict_dev(X32, return_phi=True), ref32, (m, "float32"))
            assert_same(p.predict_dev(X32.T.contiguous().T), ref32[:5], (m, "float32 column-major"))
            out = p.predict_dev(X)
            assert all(t.shape == (ns, k) and t.stride() == (1, ns) and t.dtype == torch.float64 for t in out)
        if m == 50:   # the tile route where the fused kernel fits
            with gpz_amd.Predictor(model, tile_rows=1024, force_tiles=True) as p:
                assert p.info[2] == 1
                ref = p.predict(Xh, return_phi=True)
                for name, Xl in layouts(X).items():
                    assert_same(p.predict_dev(Xl, return_phi=True), ref, (m, "forced tiles", name))


@pytest.mark.parametrize("d", [7, 24, 1])
def test_wide_and_padded_inputs(d):
    """d = 24: the runtime-d route and two LDS column chunks of the stage kernel; d = 7: de = 8, the padding dimension stays zero;
    d = 1: a vector X."""
    model = synth_model("VD", 40, d, 2, True, seed=3 + d)
    Xh = catalogue(model, 1500, seed=4)
    X = torch.from_numpy(Xh).to(DEV)
    sel = np.random.default_rng(5).random(1500) < 0.7
    with gpz_amd.Predictor(model, tile_rows=1000) as p:
        ref = p.predict(Xh, return_phi=True)
        for name, Xl in layouts(X).items():
            assert_same(p.predict_dev(Xl, return_phi=True), ref, (d, name))
        assert_same(p.predict_dev(X.float()), p.predict(host(X.float().double())), (d, "float32"))
        assert_same(p.predict_dev(X, selection=torch.from_numpy(sel).to(DEV)), p.predict(Xh, selection=sel), (d, "selection"))
        if d == 1:
            assert_same(p.predict_dev(X[:, 0]), ref[:5], (d, "vector"))
        empty = p.predict_dev(X[:0], return_phi=True)
        assert [tuple(t.shape) for t in empty] == [(0, 2)] * 5 + [(0, 40)]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("force_tiles", [False, True])
def test_draws_bit_parity(k, force_tiles):
    m, d, ns = 60, 5, 2500
    model = synth_model("VC", m, d, k, True, seed=20 + k)
    Xh = catalogue(model, ns, seed=21)
    X = torch.from_numpy(Xh).to(DEV)
    rng = np.random.default_rng(22)
    with gpz_amd.Predictor(model, tile_rows=1024, force_tiles=force_tiles) as p:
        got = {}
        for nd in (1, 16, 70):
            ref = p.draws(Xh, nd, seed=5)
            for name, Xl in layouts(X).items():
                f = p.draws_dev(Xl, nd, seed=5)
                assert f.shape == (nd, ns, k) and f.is_cuda
                assert np.array_equal(host(f), ref), (nd, name)
            got[nd] = host(p.draws_dev(X, nd, seed=5))
            Z = rng.standard_normal((m, nd, k))
            assert np.array_equal(host(p.draws_dev(X, nd, Z=Z)), p.draws(Xh, nd, Z=Z)), nd
            assert np.array_equal(host(p.draws_dev(X.float(), nd, seed=9)), p.draws(host(X.float().double()), nd, seed=9)), nd
        assert np.array_equal(got[16], got[70][:16]) and np.array_equal(got[1], got[16][:1])


def same_stack(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n_draws", [0, 8])
@pytest.mark.parametrize("force_tiles", [False, True])
def test_stack_bit_parity(n_draws, force_tiles):
    m, d, k, ns, G, B = 60, 5, 2, 5000, 3, 40
    model = synth_model("VD", m, d, k, True, seed=30)
    Xh = catalogue(model, ns, seed=31)
    rng = np.random.default_rng(32)
    lab = rng.integers(-1, G, ns)                                        # int64, with -1
    wt = rng.uniform(0.0, 2.0, ns).astype(np.float32)
    sel = rng.random(ns) < 0.8
    edges = np.linspace(-4.0, 4.0, B + 1)
    X = torch.from_numpy(Xh).to(DEV)
    labd, wtd, seld = torch.from_numpy(lab).to(DEV), torch.from_numpy(wt).to(DEV), torch.from_numpy(sel).to(DEV)
    with gpz_amd.Predictor(model, tile_rows=1024, force_tiles=force_tiles) as p:
        ref = p.stack(Xh, edges, n_draws=n_draws, seed=3, groups=lab, n_groups=G, weights=wt, selection=sel)
        for name, Xl in layouts(X).items():
            r = p.stack_dev(Xl, edges, n_draws=n_draws, seed=3, groups=labd, n_groups=G, weights=wtd, selection=seld)
            assert isinstance(r, gpz_amd.api.StackResult) and all(isinstance(f, np.ndarray) for f in r)
            assert same_stack(r, ref), name
        assert same_stack(p.stack_dev(X, edges, n_draws=n_draws, seed=3, groups=labd), p.stack(Xh, edges, n_draws=n_draws, seed=3, groups=lab))
        assert same_stack(p.stack_dev(X, edges, n_draws=n_draws, seed=3), p.stack(Xh, edges, n_draws=n_draws, seed=3))
        assert "stack: k_stack_tile" in p.route
        # two chunks: the field-wise sums agree bit for bit
        cut = 2300
        a = p.stack_dev(X[:cut], edges, n_draws=n_draws, seed=3, groups=labd[:cut], n_groups=G, weights=wtd[:cut])
        b = p.stack_dev(X[cut:], edges, n_draws=n_draws, seed=3, groups=labd[cut:], n_groups=G, weights=wtd[cut:])
        ha = p.stack(Xh[:cut], edges, n_draws=n_draws, seed=3, groups=lab[:cut], n_groups=G, weights=wt[:cut])
        hb = p.stack(Xh[cut:], edges, n_draws=n_draws, seed=3, groups=lab[cut:], n_groups=G, weights=wt[cut:])
        for f in range(4):
            assert np.array_equal(a[f] + b[f], ha[f] + hb[f]), f


def test_stream_order():
    """On a side stream: X is the end of a chain of 50 in-place updates, predict_dev is called at once, and a torch reduction over the
    returned mu is queued behind it, all without a synchronise in between."""
    n, d = 2_000_000, 5
    model = synth_model("VD", 100, d, 1, True, seed=40)
    base = torch.from_numpy(catalogue(model, n, seed=41)).to(DEV)
    with gpz_amd.Predictor(model) as p:
        p.predict_dev(base[:1000])                                       # the handle exists before the chain starts
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            X = torch.full_like(base, float("nan"))                      # what a call that ran too early would read
            for i in range(50):
                X.copy_(base) if i == 0 else X.mul_(1.0009765625).sub_(0.001)
            out = p.predict_dev(X)
            total, top, low = out[0].sum(), out[0].max(), out[0].min()
        side.synchronize()
        ref = p.predict(host(X))
        assert_same(out, ref, "side stream")
        assert float(top) == ref[0].max() and float(low) == ref[0].min()
        # any order of the n additions is within (n - 1) eps sum |mu| of the exact sum, NumPy's and torch's alike
        assert abs(float(total) - float(np.sum(ref[0]))) <= 2 * n * 2.3e-16 * float(np.abs(ref[0]).sum())


def test_constant_memory_over_many_tiles():
    n, d, nd = 3_000_000, 5, 8
    model = synth_model("VD", 100, d, 1, True, seed=50)
    gen = torch.Generator(device=DEV).manual_seed(51)
    X = torch.randn((n, d), dtype=torch.float64, device=DEV, generator=gen) * torch.from_numpy(model.sdX).to(DEV) + \
        torch.from_numpy(model.muX).to(DEV)
    sub = np.sort(np.random.default_rng(52).choice(n, 10_000, replace=False))
    Xs = host(X[torch.from_numpy(sub).to(DEV)])
    with gpz_amd.Predictor(model) as hp, gpz_amd.Predictor(model) as p:
        ref = hp.predict(Xs)
        ref_draws = hp.draws(Xs, nd, seed=6)
        p.predict_dev(X[:1000])
        held = p.info[1]
        out = p.predict_dev(X)
        assert p.info[1] == held and p.info[3] == 2 and p.info[0] == 1 << 17
        chunks = []
        for c in range(3):
            chunks.append(p.draws_dev(X[c * 1_000_000:(c + 1) * 1_000_000], nd, seed=6))
            if c == 0:
                held_draws = p.info[1]
        assert p.info[1] == held_draws
        assert p.info[1] <= hp.info[1] + 64 * 1024, (p.info, hp.info)       # the parameter / flag buffer, nothing that grows with n
        assert_same([o[torch.from_numpy(sub).to(DEV)] for o in out], ref, "sampled rows")
        F = torch.cat(chunks, dim=1)
        assert np.array_equal(host(F[:, torch.from_numpy(sub).to(DEV)]), ref_draws)


def test_refusals_on_the_device():
    n, d, G = 2_000_000, 5, 4
    model = synth_model("VD", 100, d, 1, True, seed=60)
    X = torch.from_numpy(catalogue(model, n, seed=61)).to(DEV)
    good = X[:5000].clone()
    edges = np.linspace(-4.0, 4.0, 41)
    bad = X.clone()
    bad[1_700_000, 3] = float("nan")
    lab = torch.zeros(n, dtype=torch.int64, device=DEV)
    wt = torch.ones(n, dtype=torch.float64, device=DEV)
    with gpz_amd.Predictor(model) as p:
        before = (p.predict_dev(good), p.draws_dev(good, 4, seed=1), p.stack_dev(good, edges, n_draws=4, seed=1))
        for call in (lambda x: p.predict_dev(x), lambda x: p.draws_dev(x, 4, seed=1), lambda x: p.stack_dev(x, edges, n_draws=4, seed=1),
                     lambda x: p.predict_dev(x.float()), lambda x: p.predict_dev(x.T.contiguous().T), lambda x: p.predict_dev(x[:, :])):
            with pytest.raises(_lib.GpzError, match="missing values") as ei:
                call(bad)
            assert ei.value.code == -5                                   # GPZ_ERR_UNSUPPORTED
            assert torch.equal(p.predict_dev(good)[0], before[0][0])     # the handle works on the next call
        for kw in ({"groups": lab.clone().index_fill_(0, torch.tensor([1_234_567], device=DEV), G), "n_groups": G},
                   {"groups": lab.clone().index_fill_(0, torch.tensor([7], device=DEV), -2), "n_groups": G},
                   {"weights": wt.clone().index_fill_(0, torch.tensor([1_999_999], device=DEV), -1.0)},
                   {"weights": wt.clone().index_fill_(0, torch.tensor([0], device=DEV), float("inf"))},
                   {"weights": wt.clone().index_fill_(0, torch.tensor([64], device=DEV), float("nan"))}):
            with pytest.raises(_lib.GpzError) as ei:
                p.stack_dev(X, edges, n_draws=4, seed=1, **kw)
            assert ei.value.code == -1, kw                               # GPZ_ERR_ARG
        after = (p.predict_dev(good), p.draws_dev(good, 4, seed=1), p.stack_dev(good, edges, n_draws=4, seed=1))
        assert all(torch.equal(a, b) for a, b in zip(before[0], after[0])) and torch.equal(before[1], after[1])
        assert same_stack(before[2], after[2])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU to form a tensor on another device")
def test_tensor_on_another_device_is_refused():
    model = synth_model("VD", 20, 5, 1, True, seed=70)
    with gpz_amd.Predictor(model, device=0) as p:
        with pytest.raises(ValueError, match="cuda:1"):
            p.predict_dev(torch.zeros((4, 5), dtype=torch.float64, device="cuda:1"))


def test_host_and_device_entries_share_a_handle():
    """The host methods after device calls return what they returned before, bit for bit, and the reverse."""
    model = synth_model("VC", 80, 5, 2, True, seed=80)
    Xh = catalogue(model, 3000, seed=81)
    X = torch.from_numpy(Xh).to(DEV)
    edges = np.linspace(-4.0, 4.0, 31)
    with gpz_amd.Predictor(model, tile_rows=1024) as p:
        h0 = (p.predict(Xh, return_phi=True), p.draws(Xh, 6, seed=2), p.stack(Xh, edges, n_draws=6, seed=2))
        d0 = (p.predict_dev(X, return_phi=True), p.draws_dev(X, 6, seed=2), p.stack_dev(X, edges, n_draws=6, seed=2))
        h1 = (p.predict(Xh, return_phi=True), p.draws(Xh, 6, seed=2), p.stack(Xh, edges, n_draws=6, seed=2))
        d1 = (p.predict_dev(X, return_phi=True), p.draws_dev(X, 6, seed=2), p.stack_dev(X, edges, n_draws=6, seed=2))
        for h in (h0, h1):
            assert_same(d0[0], h[0], "predict")
            assert np.array_equal(host(d0[1]), h[1]) and same_stack(d0[2], h[2])
        assert_same(d1[0], h0[0], "predict again")
        assert np.array_equal(host(d1[1]), h0[1]) and same_stack(d1[2], h0[2])
    with gpz_amd.Predictor(model, tile_rows=1024) as p:                  # device calls first on a fresh handle
        d2 = (p.predict_dev(X, return_phi=True), p.draws_dev(X, 6, seed=2), p.stack_dev(X, edges, n_draws=6, seed=2))
        h2 = (p.predict(Xh, return_phi=True), p.draws(Xh, 6, seed=2), p.stack(Xh, edges, n_draws=6, seed=2))
        assert_same(d2[0], h0[0], "fresh handle")
        assert np.array_equal(host(d2[1]), h0[1]) and same_stack(d2[2], h0[2])
        assert_same([torch.from_numpy(a) for a in h2[0]], h0[0], "host after device")
        assert np.array_equal(h2[1], h0[1]) and same_stack(h2[2], h0[2])
