"""SHA-256 of everything the streaming predictor returns, for comparing two builds of the library bit for bit
(profiles/r11_predictor_refactor.txt: the host code of gpz_predictor.hip before and after it was folded onto one pipeline).

    python tools/predictor_digest.py > digest.txt        # in each tree, on the same machine; then diff the two files

Seeded models of both kinds (VD, VC) on both routes (fused, force_tiles) with k = 1 and 3, d = 5, m = 50; 2500 rows in 1024-row tiles
(the last one partial).  Every entry of the handle is called: predict with and without PHI and with Psi, draws by seed and by an
explicit Z and with Psi, stack with and without draws, groups and weights, and the device entries on float64, float32 and strided
rows.  After each call one line: the call, the digest of each array it returned, and the handle's route and info."""
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


def run(method, k, force):
    tag = f"{method} k={k} {'tiles' if force else 'fused'}"
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
    with gpz_amd.Predictor(model, tile_rows=TILE, force_tiles=force) as p:   # a handle that meets the stack first, then PHI
        report(f"{tag} second handle stack_dev", p, tuple(p.stack_dev(Xd, edges, n_draws=2, seed=3)))
        report(f"{tag} second handle stack", p, tuple(p.stack(X, edges, n_draws=DRAWS, seed=3)))
        report(f"{tag} second handle predict_dev phi", p, p.predict_dev(Xd, return_phi=True))
        report(f"{tag} second handle predict phi", p, p.predict(X, return_phi=True))


def main():
    for method in ("VD", "VC"):
        for k in (1, 3):
            for force in (False, True):
                run(method, k, force)


if __name__ == "__main__":
    main()
