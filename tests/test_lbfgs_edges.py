"""The kernels train() runs around the objective in every L-BFGS iteration (k_lbfgs.hip: gpz_lbfgs_add, gpz_lbfgs_direction,
gpz_vec_stats, gpz_vec_axpy) at their edges, against the long-double two-loop of train_side_reference.py: p below a wave, at the 64-,
256- and 4096-row boundaries, corrections = 1 and 128 (the largest the library admits), rings that wrap, rejected pairs, a direction
before any pair, both ways gpz_lbfgs_direction comes by [S Y]'g, and a buffer overwritten in place between add and direction.

Gate of the direction: rel(d_gpu, d_ld) <= 32 max(e_ref, 2^-52), e_ref the larger error of two float64 CPU evaluations (host._LBFGS's
two-loop, the Gram form restated in NumPy) against the same long-double two-loop, computed per case; fitness e_ref <= 1e-13.
test_train_side_reference_cpu.py checks the checker and the fitness of every row without a GPU.  Nothing here retries a GPU step.
The worst error / gate per case is printed (run with -s).

Measured on an MI355X (44 tests, 4 s), worst error / gate per row of the table, both ways of coming by [S Y]'g:
    p = 1: 0.021, 63: 0.012, 64: 0.019, 65: 0.018, 255: 0.011, 257: 0.014, 4095: 0.003, 4096: 0.003, (4097, 128 corrections): 0.012,
    8193: 0.006, 12289: 0.002; the buffer overwritten in place 0.013
- errors of 2.1e-16 to 1.0e-15 against e_ref of 3.4e-16 to 3.4e-15: the device's directions are as close to the long-double two-loop as
the float64 two-loop of the host.  Against the library as it was before gpz_lbfgs_direction stopped comparing addresses, the
overwritten buffer gave an error of 0.19 (the direction of the old vector) and GPZ_OK."""
import ctypes as C

import numpy as np
import pytest

import train_side_reference as R
from gpz_amd import _lib, host

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_WHY)]

GPZ_ERR_ARG = -1
EDGES = [1, 255, 256, 257, 4095, 4096, 4097, 12289]          # p of the vector kernels: one workgroup's 4096 rows, a 256-thread pass
SPOTS = [0, 255, 256, 4095, 4096]                            # ... and where a NaN or an Inf is put, plus p - 1


def dev(a):
    return host.DevVec.from_host(np.asarray(a, dtype=np.float64))


def last_error():
    return (_lib.load().gpz_lbfgs_last_error() or b"").decode()


# ---- gpz_lbfgs_add / gpz_lbfgs_direction -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,corr,steps", R.LBFGS_CASES)
def test_direction_and_added_flag_against_the_long_double_two_loop(p, corr, steps):
    """Every step: the `added` flag is the reference's; the direction from the products gpz_lbfgs_add kept (the call train() makes)
    and the direction of a copy of g at another address (the library multiplies [S Y]'g itself) are both inside the gate."""
    ref = R.lbfgs_case(p, corr, steps, host._LBFGS)
    assert ref["e_ref"] <= R.LBFGS_FITNESS, "the inputs cannot be judged"
    if steps > corr:
        assert ref["accepted"] >= corr + R.LBFGS_WRAP_MARGIN, "the ring does not wrap"
    gate = R.lbfgs_gate(ref["e_ref"])
    mem = host._LBFGSDevice(p, corr)
    worst = 0.0
    try:
        for it, (g, g_old, t, d) in enumerate(ref["steps"]):
            G = dev(g)
            assert mem.add_step(G, dev(g_old), t, dev(d)) == ref["added"][it], it
            for what, vec in (("kept products", G), ("own products", dev(g))):
                err = R.rel_ld(mem.direction(vec).host(), ref["d_ld"][it])
                worst = max(worst, err)
                assert err <= gate, (it, what, err, gate)
    finally:
        mem.close()
    print("\np = %d, corrections = %d, %d steps (%d accepted): e_ref %.2e, worst error %.2e, error / gate %.3f"
          % (p, corr, steps, ref["accepted"], ref["e_ref"], worst, worst / gate))


@pytest.mark.parametrize("p,corr,steps", [(4097, 128, 175), (257, 5, 12)])
def test_kept_products_equal_own_products_bit_for_bit(p, corr, steps):
    """k_lb_dots promises the same sums in the same order whether g rides along with [s y] in gpz_lbfgs_add or comes alone."""
    ref = R.lbfgs_case(p, corr, steps, host._LBFGS)
    mem = host._LBFGSDevice(p, corr)
    try:
        for it, (g, g_old, t, d) in enumerate(ref["steps"]):
            G = dev(g)
            mem.add_step(G, dev(g_old), t, dev(d))
            kept = mem.direction(G).host()
            own = mem.direction(dev(g)).host()
            assert np.array_equal(kept, own), it
    finally:
        mem.close()


@pytest.mark.parametrize("p", [1, 65, 4097])
def test_direction_before_any_pair_is_minus_g(p):
    g = np.random.default_rng(p).standard_normal(p)
    mem = host._LBFGSDevice(p, 3)
    try:
        assert np.array_equal(mem.direction(dev(g)).host(), -g)
        # ... and still after a pair that was rejected
        assert not mem.add_step(dev(g), dev(g + 1.0), 1.0, dev(np.ones(p)))          # y's = -p
        assert np.array_equal(mem.direction(dev(g)).host(), -g)
    finally:
        mem.close()


def test_create_refuses_what_the_memory_cannot_hold():
    lib = _lib.load()
    for p, corr in ((10, 129), (10, 0), (0, 5)):
        h = C.c_void_p()
        assert lib.gpz_lbfgs_create(p, corr, 0, None, C.byref(h)) == GPZ_ERR_ARG and not h.value
        assert "gpz_lbfgs_create" in last_error()
    h = C.c_void_p()
    assert lib.gpz_lbfgs_create(10, 128, 0, None, C.byref(h)) == 0 and h.value
    lib.gpz_lbfgs_destroy(h)


def test_direction_at_a_buffer_overwritten_in_place():
    """add(g at address A), A overwritten with another vector, direction(A): the direction of what A holds NOW.  (Until
    gpz_lbfgs_direction stopped comparing addresses it returned the direction of the old vector, without an error.)"""
    import torch
    p, corr, steps = 257, 5, 12
    ref = R.lbfgs_case(p, corr, steps, host._LBFGS)
    lib = _lib.load()
    mem = host._LBFGSDevice(p, corr)
    try:
        for g, g_old, t, d in ref["steps"]:
            G = dev(g)
            mem.add_step(G, dev(g_old), t, dev(d))
        g2 = np.random.default_rng(7).standard_normal(p)
        want = ref["ring"].direction(g2)
        e_ref = max(R.rel_ld(ref["two_loop_f64"].direction(g2), want), R.rel_ld(ref["gram_f64"].direction(g2, ref["ring"].hdiag), want))
        assert e_ref <= R.LBFGS_FITNESS
        G.t.copy_(torch.from_numpy(g2))                                       # in place: the address stays
        out = torch.empty_like(G.t)
        _lib.check_plain(lib.gpz_lbfgs_direction(mem._h, G.t.data_ptr(), out.data_ptr()))
        err = R.rel_ld(out.cpu().numpy(), want)
        print("\noverwritten in place: e_ref %.2e, error %.2e, error / gate %.3f" % (e_ref, err, err / R.lbfgs_gate(e_ref)))
        assert err <= R.lbfgs_gate(e_ref), (err, R.rel_ld(out.cpu().numpy(), ref["d_ld"][-1]))
    finally:
        mem.close()


def test_null_g_stands_for_the_g_of_the_add_just_before_and_for_nothing_else():
    import torch
    p = 300
    rng = np.random.default_rng(2)
    lib = _lib.load()
    mem = host._LBFGSDevice(p, 4)
    try:
        out = torch.empty(p, dtype=torch.float64, device="cuda")
        assert lib.gpz_lbfgs_direction(mem._h, None, out.data_ptr()) == GPZ_ERR_ARG          # no add yet
        assert "gpz_lbfgs_add" in last_error()
        g_old, d = rng.standard_normal(p), rng.standard_normal(p)
        g = g_old + 0.3 * d
        G, G_old, D = dev(g), dev(g_old), dev(d)
        added = C.c_int32()
        assert lib.gpz_lbfgs_add(mem._h, G.t.data_ptr(), G_old.t.data_ptr(), 1.0, D.t.data_ptr(), C.byref(added)) == 0 and added.value == 1
        assert lib.gpz_lbfgs_direction(mem._h, None, out.data_ptr()) == 0
        first = out.cpu().numpy().copy()
        assert lib.gpz_lbfgs_direction(mem._h, None, out.data_ptr()) == GPZ_ERR_ARG          # used up
        assert lib.gpz_lbfgs_direction(mem._h, G.t.data_ptr(), out.data_ptr()) == 0
        assert np.array_equal(out.cpu().numpy(), first)
        assert lib.gpz_lbfgs_add(mem._h, G.t.data_ptr(), G_old.t.data_ptr(), 1.0, D.t.data_ptr(), C.byref(added)) == 0
        assert lib.gpz_lbfgs_direction(mem._h, G_old.t.data_ptr(), out.data_ptr()) == 0      # another direction comes between
        assert lib.gpz_lbfgs_direction(mem._h, None, out.data_ptr()) == GPZ_ERR_ARG
        assert last_error()
    finally:
        mem.close()


# ---- gpz_vec_stats / gpz_vec_axpy ------------------------------------------------------------------------------------------------------
def stats(g, d, p):
    out = (C.c_double * 4)()
    _lib.check_plain(_lib.load().gpz_vec_stats(g.data_ptr(), None if d is None else d.data_ptr(), p, 0, None, out))
    return list(out)


def integers(p, seed):
    """integer-valued vectors in [-8, 8]: every sum below 2^53 is exact in any order"""
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, p).astype(np.float64), rng.integers(-8, 9, p).astype(np.float64)


@pytest.mark.parametrize("p", EDGES)
def test_vec_stats_exact_on_integers(p):
    g, d = integers(p, p)
    G, D = dev(g), dev(d)
    want = [float(g @ d), float(np.abs(g).max()), float(np.abs(g).sum()), float(np.abs(d).max())]
    assert stats(G.t, D.t, p) == want
    assert stats(G.t, None, p) == [0.0, want[1], want[2], 0.0]
    assert G.legal() and G.amax() == want[1] and G.asum() == want[2] and (G @ D) == want[0]


@pytest.mark.parametrize("p", EDGES)
def test_vec_stats_nan_and_inf_at_every_edge(p):
    """out[1] is NaN exactly when g holds a NaN, out[3] exactly when d does; an Inf gives inf; isLegal.m sees either in g."""
    g, d = integers(p, p + 1)
    mg, md = float(np.abs(g).max()), float(np.abs(d).max())
    for pos in sorted({q for q in SPOTS + [p - 1] if q < p}):
        for bad in (np.nan, np.inf, -np.inf):
            for in_g in (True, False):
                a, b = g.copy(), d.copy()
                (a if in_g else b)[pos] = bad
                A, B = dev(a), dev(b)
                out = stats(A.t, B.t, p)
                where = (p, pos, bad, "g" if in_g else "d")
                if bad != bad:
                    assert np.isnan(out[1]) == in_g and np.isnan(out[3]) == (not in_g), where
                    assert (out[3] == md) if in_g else (out[1] == mg), where
                else:
                    assert (out[1] == np.inf and out[3] == md) if in_g else (out[3] == np.inf and out[1] == mg), where
                if in_g:
                    assert not A.legal(), where
                    assert not dev(a).legal(), where                       # on its own (d = NULL)
                    o1 = stats(A.t, None, p)
                    assert (np.isnan(o1[1]) if bad != bad else o1[1] == np.inf) and o1[3] == 0.0, where
                else:
                    assert A.legal() and not B.legal(), where


@pytest.mark.parametrize("p", EDGES)
def test_vec_axpy_exact_on_integers(p):
    """dyadic t, integer-valued x and d: x + t d is exact, so every element must match bit for bit; out may alias x."""
    import torch
    x, d = integers(p, p + 2)
    lib = _lib.load()
    for t in (1.0, -2.0, 0.25, -0.0078125, 1024.0):
        X, D = dev(x), dev(d)
        out = torch.full_like(X.t, 7.5)
        _lib.check_plain(lib.gpz_vec_axpy(out.data_ptr(), X.t.data_ptr(), t, D.t.data_ptr(), p, 0, None))
        assert np.array_equal(out.cpu().numpy(), x + t * d), (p, t)
        assert np.array_equal(X.host(), x) and np.array_equal(D.host(), d)
        assert np.array_equal((X + t * D).host(), x + t * d) and np.array_equal((-X).host(), -x)
        _lib.check_plain(lib.gpz_vec_axpy(X.t.data_ptr(), X.t.data_ptr(), t, D.t.data_ptr(), p, 0, None))      # out = x
        assert np.array_equal(X.host(), x + t * d), (p, t)
