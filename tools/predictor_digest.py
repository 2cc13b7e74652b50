"""SHA-256 of everything the streaming predictor returns, for comparing two builds of the library bit for bit
(profiles/r11_predictor_refactor.txt: the host code of gpz_predictor.hip before and after it was folded onto one pipeline;
profiles/r14_predictor_row_kinds.txt: before and after clean, noisy and missing rows were folded onto one set of runners and the unit
was cut into gpz_predictor.hip, gpz_predictor_host.hip and gpz_predictor_dev.hip behind gpz_predictor.h;
profiles/r18_predict_group_kernels.txt: before and after the four pair kernels of a group of rows with missing inputs were folded onto
the one body of k_predict_group_impl.h;
profiles/r20_predict_gamma_fold.txt: before and after k_predict_noisy_gamma and k_predict_noisy_cov_gamma were folded onto the one body
of k_predict_gamma_impl.h and the host's covariance-kind model tables onto one helper;
profiles/r25_predict_ncov_fold.txt: before and after the tile kernels and gamma policies of GC / VC rows with Psi, a variance per
dimension or a full matrix per row, were folded onto the bodies of k_predict_ncov_impl.h and one Psi policy).

    python tools/predictor_digest.py > digest.txt        # in each tree, on the same machine; then diff the two files

Seeded models of both kinds (VD, VC) on both routes (fused, force_tiles) with k = 1 and 3, d = 5, m = 50; 2500 rows in 1024-row tiles
(the last one partial).  Every entry of the handle is called: predict with and without PHI and with Psi, draws by seed and by an
explicit Z and with Psi, stack with and without draws, groups and weights, and the device entries on float64, float32 and strided
rows; on the VD models the stacks of rows with input noise (host and device) and gamma per draw beside the draws, and, on the same
rows with four NaN patterns knocked out, predict_dev, draws_dev (with and without gamma) and the stack of rows with missing inputs,
and the same with Psi (predict_noisy_missing_dev, draws_noisy_missing_dev with and without gamma, stack_noisy_missing_dev plain, with
draws and groups, and with Z and a selection); a third handle meets the missing stack first, then the noisy one, then predict.  One
more VD model has m = 128 and k = 3: predict_missing_chunks is 8 there and the KM = 8 pair kernels walk more than one group per chunk.
Then the entries of the covariance kinds and the gamma kernels at their edges (run_edges): GC and VC at d = 1, 7, 8, 9, 10 and VD at
d = 1, 20, each with m = 20, k = 1 (one gamma chunk; 1, 64 and 129 or, from d = 8 on, 65 columns: one more than a pass holds) and
m = 91, k = 3 (two gamma chunks, the last stage partial; 3 and 129 or 66 columns), 80 rows on 128-row tiles (a full workgroup and 16 rows)
and one call over two tiles: predict_noisy_cov_dev, draws_noisy_cov_dev with and without gamma, stack_noisy_cov_dev,
predict_missing_cov_dev and draws_missing_cov_dev (VD: gamma per draw and stack_noisy_dev), and two more handles that meet a call for
rows with missing inputs first and one for rows with input noise second, and the other way round.  Behind them, on handles of their
own so that the lines above stay what they were (profiles/r21_predict_stack_missing_cov.txt): draws_missing_cov_dev with gamma (the
first call of its handle, then predict_missing_cov_dev, which reads the slab that call filled) and stack_missing_cov_dev with 1 and
with 129 or 66 columns, groups and weights, and a handle that meets stack_noisy_cov_dev first and stack_missing_cov_dev second.
Behind those again, on one more handle (profiles/r23_predict_stack_noisy_missing_cov.txt): the same rows with Psi through
draws_noisy_missing_cov_dev with gamma (the first call of its handle), predict_noisy_missing_cov_dev and stack_noisy_missing_cov_dev.
Last, on handles of their own again (run_cube, profiles/r25_predict_ncov_fold.txt): rows with a full Psi each, Psi_i = u_i u_i' +
diag(g_i) as tools/predict_psi_cube_timing.py draws it, on GC and VC at d = 1 (no off-diagonal element), 6 and 7 (pcg_blocks changes
between them), 9, 10 (the widths above 256 registers), each with m = 20, k = 1 and m = 91, k = 3, 80 rows on 128-row tiles and 200 rows
over two tiles: predict_psi_cube_dev, draws_psi_cube_dev with and without gamma, stack_psi_cube_dev with 1 draw and with one column
more than a gamma pass holds; one handle that meets a cube call first and predict_noisy_cov_dev / stack_noisy_cov_dev second, and one
the other way round (the two kinds share cbrec, cprec, nout, npart, cphi and gpart).
Behind those (run_cube_missing, profiles/r27_predict_nmcov_fold.txt: before and after the tile and gamma kernels of GC / VC groups
with Psi and missing inputs were folded onto the bodies of k_predict_nmcov_impl.h): such rows with NaN patterns on GC and VC at d = 5
(one pattern per NO = 1 .. 4), 10 (NO = 9) and 2 (NO = 1), m = 7 and 17, k = 1 and 2, 200 rows that mix complete rows, rows with
nothing observed and the patterns: predict_psi_cube_missing_dev, draws_psi_cube_missing_dev with and without gamma (17 and 65 columns)
and stack_psi_cube_missing_dev with 3 groups, on a float64 cube and a float32 one with other strides; two handles that serve
predict_noisy_missing_cov_dev and the cube calls on one pattern in both orders; and m = 250, where the pattern's table takes several slabs.
After each call one line: the call, the digest of each array it returned, and the handle's route and info."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpz_amd  # noqa: E402
from test_predictor import catalogue, synth_model  # noqa: E402

D, M, NS, TILE, DRAWS, DEV = 5, 50, 2500, 1024, 5, "cuda:0"


def digest(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return hashlib.sha256(str(a.shape).encode() + np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def report(tag, p, out):
    out = out if isinstance(out, tuple) else (out,)
    print(f"{tag}: {' '.join(digest(a) for a in out)} | {p.route} | {p.info}", flush=True)


def four_patterns(X):
    """tests/test_predictor_stack_missing.py's: of every ten rows five without the last dimension, one with dimension 0 only, one with
    nothing observed, three complete."""
    X = X.copy()
    r = np.arange(X.shape[0]) % 10
    X[r < 5, X.shape[1] - 1] = np.nan
    X[r == 5, 1:] = np.nan
    X[r == 6, :] = np.nan
    return X


def run(method, k, force, M=M):
    tag = f"{method} k={k} {'tiles' if force else 'fused'}" + ("" if M == 50 else f" m={M}")
    model = synth_model(method, M, D, k, True, seed=100 * k + (method == "VC"))
    rng = np.random.default_rng(7 * k)
    X = catalogue(model, NS, seed=k)
    Psi = rng.gamma(1.0, 0.05, (NS, D))
    Z = rng.standard_normal((M, DRAWS, k))
    edges = np.linspace(-3.0, 3.0, 13)
    groups = rng.integers(-1, 3, NS)
    weights = rng.uniform(0.5, 1.5, NS)
    sel = rng.random(NS) < 0.7
    noisy = method == "VD"                                               # predict_noisy_fits: input noise on the handle
    Xd = torch.from_numpy(X).to(DEV)
    wide = torch.zeros((NS, 2 * D + 1), dtype=torch.float64, device=DEV)
    wide[:, 1::2] = Xd
    layouts = {"f64": Xd, "f32": Xd.to(torch.float32), "cols": Xd.T.contiguous().T, "strided": wide[:, 1::2]}
    Pd, gd, wd, sd = (torch.from_numpy(a).to(DEV) for a in (Psi, groups, weights, sel))
    with gpz_amd.Predictor(model, tile_rows=TILE, force_tiles=force) as p:
        report(f"{tag} predict", p, p.predict(X))
        report(f"{tag} predict phi", p, p.predict(X, return_phi=True))
        report(f"{tag} predict sel", p, p.predict(X, selection=sel))
        report(f"{tag} predict psi", p, p.predict(X[:300], Psi=Psi[:300], return_phi=True))
        report(f"{tag} draws seed", p, p.draws(X, DRAWS, seed=11))
        report(f"{tag} draws Z", p, p.draws(X, DRAWS, Z=Z))
        if noisy and not force:
            report(f"{tag} draws psi", p, p.draws(X, DRAWS, seed=11, Psi=Psi))
            report(f"{tag} draws psi Z", p, p.draws(X, DRAWS, Z=Z, Psi=Psi[:, :1]))
        report(f"{tag} stack", p, tuple(p.stack(X, edges)))
        report(f"{tag} stack draws", p, tuple(p.stack(X, edges, n_draws=DRAWS, seed=11, groups=groups, n_groups=3, weights=weights)))
        report(f"{tag} stack Z sel", p, tuple(p.stack(X, edges, n_draws=DRAWS, Z=Z, groups=groups, weights=weights, selection=sel)))
        for name, x in layouts.items():
            report(f"{tag} predict_dev {name}", p, p.predict_dev(x, return_phi=name != "f32"))
            report(f"{tag} draws_dev {name}", p, p.draws_dev(x, DRAWS, seed=11))
            report(f"{tag} stack_dev {name}", p, tuple(p.stack_dev(x, edges, n_draws=DRAWS, seed=11, groups=gd, n_groups=3, weights=wd)))
            if noisy:
                report(f"{tag} predict_dev psi {name}", p, p.predict_dev(x, Psi=Pd.to(x.dtype)))
            if noisy and not force:
                report(f"{tag} draws_dev psi {name}", p, p.draws_dev(x, DRAWS, Z=Z, Psi=Pd[:, 0]))
        report(f"{tag} predict_dev sel", p, p.predict_dev(Xd, selection=sd))
        report(f"{tag} draws_dev Z sel", p, p.draws_dev(Xd, DRAWS, Z=Z, selection=sd))
        report(f"{tag} stack_dev plain", p, tuple(p.stack_dev(Xd, edges, selection=sd)))
        by_group = dict(groups=groups, n_groups=3, weights=weights)
        by_group_d = dict(groups=gd, n_groups=3, weights=wd)
        if noisy and not force:                                          # the stacks with Psi and gamma per draw need the fused draws route
            report(f"{tag} stack_noisy", p, tuple(p.stack_noisy(X, Psi, edges)))
            report(f"{tag} stack_noisy draws", p, tuple(p.stack_noisy(X, Psi, edges, n_draws=DRAWS, seed=11, **by_group)))
            report(f"{tag} stack_noisy Z sel", p, tuple(p.stack_noisy(X, Psi, edges, n_draws=DRAWS, Z=Z, selection=sel, **by_group)))
            report(f"{tag} stack_noisy_dev", p, tuple(p.stack_noisy_dev(Xd, Pd, edges)))
            report(f"{tag} stack_noisy_dev draws", p, tuple(p.stack_noisy_dev(Xd, Pd, edges, n_draws=DRAWS, seed=11, **by_group_d)))
            report(f"{tag} stack_noisy_dev Z sel", p, tuple(p.stack_noisy_dev(Xd, Pd, edges, n_draws=DRAWS, Z=Z, selection=sd, **by_group_d)))
            report(f"{tag} draws_dev psi gamma", p, p.draws_dev(Xd, DRAWS, seed=11, Psi=Pd, return_gamma=True))
        if noisy:                                                        # predict_missing_fits: rows with missing inputs on the handle
            Xm = torch.from_numpy(four_patterns(X)).to(DEV)
            report(f"{tag} predict_dev missing", p, p.predict_dev(Xm, missing=True))
            report(f"{tag} draws_dev missing", p, p.draws_dev(Xm, DRAWS, seed=11, missing=True))
            report(f"{tag} draws_dev missing gamma", p, p.draws_dev(Xm, DRAWS, Z=Z, missing=True, return_gamma=True))
            report(f"{tag} stack_missing_dev", p, tuple(p.stack_missing_dev(Xm, edges)))
            report(f"{tag} stack_missing_dev draws", p, tuple(p.stack_missing_dev(Xm, edges, n_draws=DRAWS, seed=11, **by_group_d)))
            report(f"{tag} stack_missing_dev Z sel", p, tuple(p.stack_missing_dev(Xm, edges, n_draws=DRAWS, Z=Z, selection=sd, **by_group_d)))
            report(f"{tag} predict_noisy_missing_dev", p, p.predict_noisy_missing_dev(Xm, Pd))
        if noisy and not force:                                          # with Psi the draws and the stack need the fused draws route
            report(f"{tag} draws_noisy_missing_dev", p, p.draws_noisy_missing_dev(Xm, Pd, DRAWS, seed=11))
            report(f"{tag} draws_noisy_missing_dev gamma", p, p.draws_noisy_missing_dev(Xm, Pd, DRAWS, Z=Z, return_gamma=True))
            report(f"{tag} stack_noisy_missing_dev", p, tuple(p.stack_noisy_missing_dev(Xm, Pd, edges)))
            report(f"{tag} stack_noisy_missing_dev draws", p,
                   tuple(p.stack_noisy_missing_dev(Xm, Pd, edges, n_draws=DRAWS, seed=11, **by_group_d)))
            report(f"{tag} stack_noisy_missing_dev Z sel", p,
                   tuple(p.stack_noisy_missing_dev(Xm, Pd, edges, n_draws=DRAWS, Z=Z, selection=sd, **by_group_d)))
    with gpz_amd.Predictor(model, tile_rows=TILE, force_tiles=force) as p:   # a handle that meets the stack first, then PHI
        report(f"{tag} second handle stack_dev", p, tuple(p.stack_dev(Xd, edges, n_draws=2, seed=3)))
        report(f"{tag} second handle stack", p, tuple(p.stack(X, edges, n_draws=DRAWS, seed=3)))
        report(f"{tag} second handle predict_dev phi", p, p.predict_dev(Xd, return_phi=True))
        report(f"{tag} second handle predict phi", p, p.predict(X, return_phi=True))
    if noisy and not force:   # a handle that meets the missing stack first, then the noisy one, then predict: the per-kind state the other way
        with gpz_amd.Predictor(model, tile_rows=TILE) as p:
            report(f"{tag} third handle stack_missing_dev", p, tuple(p.stack_missing_dev(Xm, edges, n_draws=2, seed=3)))
            report(f"{tag} third handle stack_noisy_dev", p, tuple(p.stack_noisy_dev(Xd, Pd, edges, n_draws=DRAWS, seed=3)))
            report(f"{tag} third handle stack_noisy", p, tuple(p.stack_noisy(X, Psi, edges, n_draws=2, seed=3)))
            report(f"{tag} third handle predict", p, p.predict(X))


def run_edges(method, d, m, k):
    tag = f"{method} d={d} m={m} k={k}"
    cov = method != "VD"
    model = synth_model(method, m, d, k, True, seed=1000 * d + 10 * m + k + (method == "GC"))
    rng = np.random.default_rng(d + m)
    X = catalogue(model, 200, seed=d)
    Xm = X.copy()
    Xm[0::3, 0] = np.nan
    Xm[1::3, d - 1] = np.nan
    Xd, Xmd, Pd = (torch.from_numpy(a).to(DEV) for a in (X, Xm, rng.gamma(1.0, 0.05, (200, d))))
    edges = np.linspace(-3.0, 3.0, 13)
    over = 65 if cov and d >= 8 else 129                                 # one column more than a pass of the gamma kernel holds
    draws = (1, 64, over) if k == 1 else (1, -(-over // k))

    def noisy(p, rows, nd):
        x, psi = Xd[:rows], Pd[:rows]
        if cov:
            report(f"{tag} draws_noisy_cov_dev {nd} x {rows}", p, p.draws_noisy_cov_dev(x, psi, nd, seed=11))
            report(f"{tag} draws_noisy_cov_dev gamma {nd} x {rows}", p, p.draws_noisy_cov_dev(x, psi, nd, seed=11, return_gamma=True))
            report(f"{tag} stack_noisy_cov_dev {nd} x {rows}", p, tuple(p.stack_noisy_cov_dev(x, psi, edges, n_draws=nd, seed=11)))
        else:
            report(f"{tag} draws_dev psi gamma {nd} x {rows}", p, p.draws_dev(x, nd, seed=11, Psi=psi, return_gamma=True))
            report(f"{tag} stack_noisy_dev {nd} x {rows}", p, tuple(p.stack_noisy_dev(x, psi, edges, n_draws=nd, seed=11)))

    def missing(p, rows):
        report(f"{tag} predict_missing_cov_dev x {rows}", p, p.predict_missing_cov_dev(Xmd[:rows]))
        report(f"{tag} draws_missing_cov_dev x {rows}", p, p.draws_missing_cov_dev(Xmd[:rows], 3, seed=11))

    with gpz_amd.Predictor(model, tile_rows=128) as p:
        if cov:
            report(f"{tag} predict_noisy_cov_dev", p, p.predict_noisy_cov_dev(Xd[:80], Pd[:80]))
        for nd in draws:
            noisy(p, 80, nd)
        noisy(p, 200, draws[-1])                                         # two tiles
        if cov:
            missing(p, 80)
            missing(p, 200)
    if cov:
        with gpz_amd.Predictor(model, tile_rows=128) as p:               # rows with missing inputs first, rows with input noise second
            missing(p, 80)
            report(f"{tag} missing first, predict_noisy_cov_dev", p, p.predict_noisy_cov_dev(Xd[:80], Pd[:80]))
            noisy(p, 80, draws[0])
        with gpz_amd.Predictor(model, tile_rows=128) as p:               # and the other way round, the draws (no pairs) in front
            report(f"{tag} noisy first, draws_noisy_cov_dev", p, p.draws_noisy_cov_dev(Xd[:80], Pd[:80], 2, seed=11))
            report(f"{tag} noisy first, predict_noisy_cov_dev", p, p.predict_noisy_cov_dev(Xd[:80], Pd[:80]))
            missing(p, 80)
        gd = torch.from_numpy(rng.integers(-1, 3, 200)).to(DEV)
        wd = torch.from_numpy(rng.uniform(0.5, 1.5, 200)).to(DEV)
        with gpz_amd.Predictor(model, tile_rows=128) as p:               # gamma per draw and the stack of rows with missing inputs
            for nd in (draws[0], draws[-1]):
                report(f"{tag} draws_missing_cov_dev gamma {nd} x 200", p, p.draws_missing_cov_dev(Xmd, nd, seed=11, return_gamma=True))
                missing(p, 200)
                report(f"{tag} stack_missing_cov_dev {nd} x 200", p,
                       tuple(p.stack_missing_cov_dev(Xmd, edges, n_draws=nd, seed=11, groups=gd, n_groups=3, weights=wd)))
            report(f"{tag} stack_missing_cov_dev plain x 80", p, tuple(p.stack_missing_cov_dev(Xmd[:80], edges)))
        with gpz_amd.Predictor(model, tile_rows=128) as p:               # the noisy stack first, the missing one second: gpart is shared
            report(f"{tag} noisy first, stack_noisy_cov_dev", p, tuple(p.stack_noisy_cov_dev(Xd[:80], Pd[:80], edges, n_draws=3, seed=11)))
            report(f"{tag} noisy first, stack_missing_cov_dev", p, tuple(p.stack_missing_cov_dev(Xmd, edges, n_draws=draws[-1], seed=11)))
        with gpz_amd.Predictor(model, tile_rows=128) as p:               # the same with Psi: gamma first, then the moments, which read its slab
            for nd in (draws[0], draws[-1]):
                report(f"{tag} draws_noisy_missing_cov_dev gamma {nd} x 200", p,
                       p.draws_noisy_missing_cov_dev(Xmd, Pd, nd, seed=11, return_gamma=True))
                report(f"{tag} predict_noisy_missing_cov_dev x 200", p, p.predict_noisy_missing_cov_dev(Xmd, Pd))
                report(f"{tag} stack_noisy_missing_cov_dev {nd} x 200", p,
                       tuple(p.stack_noisy_missing_cov_dev(Xmd, Pd, edges, n_draws=nd, seed=11, groups=gd, n_groups=3, weights=wd)))
            report(f"{tag} stack_noisy_missing_cov_dev plain x 80", p, tuple(p.stack_noisy_missing_cov_dev(Xmd[:80], Pd[:80], edges, n_draws=0)))


def run_cube(method, d, m, k):
    from predict_psi_cube_timing import catalogue as cube_rows           # (X, the variances g, the cube u u' + diag(g), groups), seed 2
    tag = f"{method} d={d} m={m} k={k} cube"
    model = synth_model(method, m, d, k, True, seed=1000 * d + 10 * m + k + (method == "GC"))
    Xd = torch.from_numpy(catalogue(model, 200, seed=d)).to(DEV)
    _, Pd, Cd, _ = cube_rows(200, d, torch.device(DEV))
    edges = np.linspace(-3.0, 3.0, 13)
    over = 65 if d >= 7 else 129                                         # one column more than a pass of k_predict_psi_cube_gamma holds
    draws = (1, over) if k == 1 else (1, -(-over // k))

    def cube(p, rows, nd, pre=""):
        x, c = Xd[:rows], Cd[:, :, :rows]
        report(f"{tag} {pre}predict_psi_cube_dev x {rows}", p, p.predict_psi_cube_dev(x, c))
        report(f"{tag} {pre}draws_psi_cube_dev {nd} x {rows}", p, p.draws_psi_cube_dev(x, c, nd, seed=11))
        report(f"{tag} {pre}draws_psi_cube_dev gamma {nd} x {rows}", p, p.draws_psi_cube_dev(x, c, nd, seed=11, return_gamma=True))
        report(f"{tag} {pre}stack_psi_cube_dev {nd} x {rows}", p, tuple(p.stack_psi_cube_dev(x, c, edges, n_draws=nd, seed=11)))

    def diagonal(p, rows, nd, pre=""):
        x, psi = Xd[:rows], Pd[:rows]
        report(f"{tag} {pre}predict_noisy_cov_dev x {rows}", p, p.predict_noisy_cov_dev(x, psi))
        report(f"{tag} {pre}stack_noisy_cov_dev {nd} x {rows}", p, tuple(p.stack_noisy_cov_dev(x, psi, edges, n_draws=nd, seed=11)))

    with gpz_amd.Predictor(model, tile_rows=128) as p:
        for nd in draws:
            cube(p, 80, nd)
        cube(p, 200, draws[-1])                                          # two tiles
    with gpz_amd.Predictor(model, tile_rows=128) as p:                   # a full Psi first, a variance per dimension second
        cube(p, 80, draws[0], "cube first, ")
        diagonal(p, 80, draws[-1], "cube first, ")
    with gpz_amd.Predictor(model, tile_rows=128) as p:                   # and the other way round
        diagonal(p, 80, draws[0], "diagonal first, ")
        cube(p, 80, draws[-1], "diagonal first, ")


def run_cube_missing(method, d, m, k):
    """Rows with a full Psi each and missing inputs (profiles/r27_predict_nmcov_fold.txt): of every eight rows two complete, one with
    nothing observed and the others on the patterns of d - one per NO = 1 .. 4 at d = 5, dimension 1 of 5 missing among them, NO = 9
    at d = 10 and NO = 1 at d = 2.  All four questions on a float64 cube and on a float32 one with other strides, gamma per draw at 17
    and 65 columns (18 and 66 at k = 2), a stack with 3 groups, and two handles that serve the diagonal form and the cube on one
    pattern in both orders (they share the slab and its flag)."""
    from predict_edges import psi_cube
    tag = f"{method} d={d} m={m} k={k} cube missing"
    n = 200
    model = synth_model(method, m, d, k, True, seed=2000 * d + 10 * m + k + (method == "GC"))
    rng = np.random.default_rng(27 * d + m + k)
    X = catalogue(model, n, seed=d + m)
    missing = {5: ((1,), (0, 4), (0, 2, 4), (0, 1, 3, 4)), 10: ((3,),), 2: ((0,),)}[d]   # the dimensions each pattern lacks
    r = np.arange(n) % 8
    X[r == 2, :] = np.nan
    for slot, dims in zip((3, 4, 5, 6), missing):
        X[np.ix_(r == slot, dims)] = np.nan
    X[np.ix_(r == 7, missing[0])] = np.nan
    sd = np.asarray(model.sdX).reshape(-1)
    g = rng.gamma(1.0, 0.05, (n, d)) * sd ** 2
    C = psi_cube(g.copy(), 0.2 * rng.standard_normal((n, d)) * sd)
    Xd, Pd, Cd = (torch.from_numpy(a).to(DEV) for a in (X, g, C))
    C32 = torch.from_numpy(np.ascontiguousarray(C.transpose(2, 0, 1)).astype(np.float32)).to(DEV).permute(1, 2, 0)   # strides (d, 1, d d)
    gd = torch.from_numpy(rng.integers(-1, 3, n)).to(DEV)
    wd = torch.from_numpy(rng.uniform(0.5, 1.5, n)).to(DEV)
    edges = np.linspace(-3.0, 3.0, 13)
    first = torch.from_numpy(np.flatnonzero((r == 3) | (r == 7))).to(DEV)   # the rows of one pattern
    with gpz_amd.Predictor(model, tile_rows=128) as p:
        for name, c in (("f64", Cd), ("f32", C32)):
            report(f"{tag} predict {name}", p, p.predict_psi_cube_missing_dev(Xd, c))
            report(f"{tag} draws {name}", p, p.draws_psi_cube_missing_dev(Xd, c, 3, seed=11))
            for cols in (17, 65):
                nd = -(-cols // k)
                report(f"{tag} draws gamma {nd} {name}", p, p.draws_psi_cube_missing_dev(Xd, c, nd, seed=11, return_gamma=True))
            report(f"{tag} stack {name}", p,
                   tuple(p.stack_psi_cube_missing_dev(Xd, c, edges, n_draws=5, seed=11, groups=gd, n_groups=3, weights=wd)))
        report(f"{tag} stack plain", p, tuple(p.stack_psi_cube_missing_dev(Xd[:80], Cd[:, :, :80], edges, n_draws=0)))
    x1, p1, c1 = Xd[first], Pd[first], Cd[:, :, first]
    with gpz_amd.Predictor(model, tile_rows=128) as p:                   # a variance per dimension first, the cube second
        report(f"{tag} diagonal first, predict_noisy_missing_cov_dev", p, p.predict_noisy_missing_cov_dev(x1, p1))
        report(f"{tag} diagonal first, predict", p, p.predict_psi_cube_missing_dev(x1, c1))
        report(f"{tag} diagonal first, draws gamma", p, p.draws_psi_cube_missing_dev(x1, c1, 3, seed=11, return_gamma=True))
    with gpz_amd.Predictor(model, tile_rows=128) as p:                   # and the other way round, gamma in front
        report(f"{tag} cube first, draws gamma", p, p.draws_psi_cube_missing_dev(x1, c1, 3, seed=11, return_gamma=True))
        report(f"{tag} cube first, predict_noisy_missing_cov_dev", p, p.predict_noisy_missing_cov_dev(x1, p1))
        report(f"{tag} cube first, stack_noisy_missing_cov_dev", p, tuple(p.stack_noisy_missing_cov_dev(x1, p1, edges, n_draws=3, seed=11)))
        report(f"{tag} cube first, predict", p, p.predict_psi_cube_missing_dev(x1, c1))


def run_cube_missing_slabs(method):
    """m = 250, d = 5: the pair-component table of a pattern with NO = 4 passes through several slabs.  70 rows of that pattern."""
    from predict_edges import psi_cube
    m, d, k, n = 250, 5, 1, 70
    tag = f"{method} d={d} m={m} k={k} cube missing slabs"
    model = synth_model(method, m, d, k, True, seed=2750 + (method == "GC"))
    rng = np.random.default_rng(275)
    X = catalogue(model, n, seed=27)
    X[:, 1] = np.nan
    sd = np.asarray(model.sdX).reshape(-1)
    C = psi_cube(rng.gamma(1.0, 0.05, (n, d)) * sd ** 2, 0.2 * rng.standard_normal((n, d)) * sd)
    Xd, Cd = torch.from_numpy(X).to(DEV), torch.from_numpy(C).to(DEV)
    with gpz_amd.Predictor(model, tile_rows=128) as p:
        report(f"{tag} predict", p, p.predict_psi_cube_missing_dev(Xd, Cd))
        report(f"{tag} draws gamma 16", p, p.draws_psi_cube_missing_dev(Xd, Cd, 16, seed=11, return_gamma=True))


def main():
    for method in ("VD", "VC"):
        for k in (1, 3):
            for force in (False, True):
                run(method, k, force)
    run("VD", 3, False, M=128)
    for method, widths in (("GC", (1, 7, 8, 9, 10)), ("VC", (1, 7, 8, 9, 10)), ("VD", (1, 20))):
        for d in widths:
            run_edges(method, d, 20, 1)
            run_edges(method, d, 91, 3)
    for method in ("GC", "VC"):
        for d in (1, 6, 7, 9, 10):
            run_cube(method, d, 20, 1)
            run_cube(method, d, 91, 3)
    for method in ("GC", "VC"):
        for d in (5, 10, 2):
            for m, k in ((7, 1), (17, 2), (7, 2), (17, 1)):              # both KM instantiations of the pair kernel at both m
                run_cube_missing(method, d, m, k)
        run_cube_missing_slabs(method)


if __name__ == "__main__":
    main()
