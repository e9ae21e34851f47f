"""Generates tests/golden/ica.npz from scikit-learn and the REAL reference (imported through oracle/ref_harness.py, dev
container only; never imported by a test; needs numpy and scikit-learn there):

    python tools/make_ica_golden.py

The inputs are not stored: tests/_ica_checks.py rebuilds them from seeds (``fit_input``; ``_nmf_checks.cube``) and the
sub-image stacks come from tests/golden/stat.npz.

Before anything is written this script ASSERTS that the numpy rule of tests/_ica_checks.py (``fit_rule``: whitening through
the Gram matrix of the smaller side plus eigh, the parallel fixed point, the finish) reproduces the library on every case
with EQUAL n_iter, and records per case the library's result, ``n_iter_`` and the rule-versus-library distance (max abs
difference over max abs value, the largest over the five outputs).  The tests take 1000 x that distance as their
tolerance.  A case is refused unless
  * 1000 x distance <= 1e-9: a wrong update cannot hide behind a loose bound;
  * |u[0, j]| >= 0.01 max|u| for every kept component: the sign rule u *= sign(u[0]) is not a coin toss;
  * sigma_k / sigma_1 >= 0.01: the Gram route of the whitening loses at most 2^-52 1e4;
  * |lim - tol| >= 1e-3 tol at the stopping iteration and at the one before it: n_iter equality may be demanded.

  fit|<name>|components, |sources, |mixing, |whitening, |mean, |n_iter, |dist
        sklearn.decomposition.FastICA(k, random_state=7, tol=1e-4, max_iter=200, **the case's arguments) on
        ``fit_input(name)`` in float64;  the same keys with the suffix 32: on ``X.astype(float32).astype(float64)``
  stat|<case>|k<k>|components, |X_vec_t, |dist (+ suffix 32), stat|<case>|com_frames
        the reference's imlocal.ica(k) on the stat.npz case, frames in float64 / in float32 converted back to float64
        (imblock_ica returns the same arrays and the first two coordinate columns: asserted)
  cube|<tag>|components, |maps, |n_iter, |dist
        the reference's SpectralUnmixer('ica', 3) on the 6 x 7 x 20 cube after np.random.seed(11): plain, normalize=True
TEST INFRASTRUCTURE ONLY.
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness  # noqa: E402
import _ica_checks as C  # noqa: E402
import _nmf_checks as N  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
REFUSE = 1e-9 / 1000.0


def accept(name, rule, lib, n_iter, tol=1e-4):
    """The four conditions; ``lib``: the library's FIELDS that are compared (a dict).  Returns the distance."""
    d = max(C.rel(rule[f], lib[f]) for f in lib)
    u, sigma, lims = rule["u"], rule["sigma"], rule["lims"]
    print(f"{name}: rule vs library {d:.2e}, n_iter {rule['n_iter']} / {n_iter}, sigma_k/sigma_1 {sigma[-1] / sigma[0]:.3f}, "
          f"min |u0|/max|u| {np.abs(u[0]).min() / np.abs(u).max():.3f}, last lims {lims[-2:]}")
    assert rule["n_iter"] == n_iter, f"{name}: n_iter {rule['n_iter']} != {n_iter}"
    assert d <= REFUSE, f"{name}: the rule is {d:.2e} from the library: its tolerance would exceed 1e-9"
    assert (np.abs(u[0]) >= 0.01 * np.abs(u).max()).all(), f"{name}: the sign of a component is a coin toss"
    assert sigma[-1] / sigma[0] >= 0.01, f"{name}: ill-conditioned whitening"
    assert all(abs(lim - tol) >= 1e-3 * tol for lim in lims[-2:]), f"{name}: lim too close to tol"
    assert lims[-1] < tol, f"{name}: did not converge"
    return d


def sk_fit(X, k, **kw):
    from sklearn.decomposition import FastICA
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # no ConvergenceWarning: every case converges
        m = FastICA(n_components=k, **kw)
        S = m.fit_transform(X)
    return dict(components=m.components_, sources=S, mixing=m.mixing_, whitening=m.whitening_, mean=m.mean_), m.n_iter_


def fits(out):
    for name, (n, d, k, _) in C.FITS.items():
        kw = C.fit_kwargs(name)
        for tag, X in (("", C.fit_input(name)), ("32", C.fit_input(name).astype(np.float32).astype(np.float64))):
            lib, n_iter = sk_fit(X, k, **kw)
            rule = C.fit_rule(X, k, **kw)
            for f in C.FIELDS:
                out[f"fit|{name}|{f}{tag}"] = lib[f]
            out[f"fit|{name}|n_iter{tag}"] = n_iter
            out[f"fit|{name}|dist{tag}"] = accept(f"fit {name} {tag}", rule, lib, n_iter)


def stats(out):
    import _stat_checks as S
    from atomai.stat import multivar as ref
    for name in C.STAT_CASES:
        frames, coords, r, _ = S.case(name)
        for tag, fr in (("", frames.astype(np.float64)), ("32", frames.astype(np.float32).astype(np.float64))):
            for k in C.STAT_KS:
                s = ref.imlocal(fr, coords, r, 0)
                with warnings.catch_warnings():
                    warnings.simplefilter("error")
                    comp, xt, cf = s.ica(k)
                    comp2, xt2, centres = s.imblock_ica(k)
                assert np.array_equal(comp, comp2) and np.array_equal(xt, xt2) and np.array_equal(centres, cf[:, :2])
                X = s.imgstack.reshape(s.d0, -1)
                assert X.dtype == np.float64
                rule = C.fit_rule(X, k, random_state=1)
                prefix = f"stat|{name}|k{k}"
                out[f"{prefix}|components{tag}"], out[f"{prefix}|X_vec_t{tag}"] = comp, xt
                out[f"{prefix}|dist{tag}"] = accept(f"{prefix} {tag} {X.shape}", rule,
                                                    dict(components=comp.reshape(k, -1), sources=xt), rule["n_iter"])
                out[f"stat|{name}|com_frames"] = cf.astype(np.float64)


def cubes(out):
    from atomai.stat.unmixer import SpectralUnmixer
    for tag, normalize in (("plain", False), ("norm", True)):
        data = N.cube()
        u = SpectralUnmixer("ica", 3, normalize=normalize)
        np.random.seed(C.CUBE_SEED)
        with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter("error")
            comp, maps = u.fit(data)
        X = data.reshape(-1, data.shape[-1])
        norms = X.sum(1, keepdims=True) if normalize else 1.0
        np.random.seed(C.CUBE_SEED)
        rule = C.fit_rule(X / norms, 3, random_state=None)
        rule["sources"] = rule["sources"] * norms
        out[f"cube|{tag}|components"], out[f"cube|{tag}|maps"], out[f"cube|{tag}|n_iter"] = comp, maps, u.model.n_iter_
        out[f"cube|{tag}|dist"] = accept(f"cube {tag}", rule, dict(components=comp, sources=maps.reshape(-1, 3)),
                                         u.model.n_iter_)


def main():
    ref_harness.import_reference()
    out = {}
    fits(out)
    stats(out)
    cubes(out)
    path = os.path.join(GOLD, "ica.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
