"""Generates tests/golden/nmf.npz from scikit-learn, scipy and the REAL reference (imported through
oracle/ref_harness.py, dev container only; never imported by a test; needs numpy, scipy and scikit-learn there):

    python tools/make_nmf_golden.py

The inputs are not stored: tests/_nmf_checks.py rebuilds them from seeds (``fit_input``, ``fft_windows``, ``image``,
``cube``) and the sub-image stacks come from tests/golden/stat.npz.  skimage is absent, so ``view_as_windows`` in the
imported atomai.stat.fft_nmf is replaced by ``sliding_window_view(image, size)[::sx, ::sy]``, restated from its
documentation (not pinned to skimage itself).

Before anything is written this script ASSERTS that the numpy rule of tests/_nmf_checks.py (``fit_rule``: the sweep and
the initialisations, NNDSVD from the exact SVD; ``fft_rule``: direct DFT at the cropped frequencies and the separable
linear zoom) reproduces the library on every case, and records per case the library's result, ``n_iter_`` and the
rule-versus-library distance (max abs difference over max abs value).  The tests take 1000 x that distance as their
tolerance, so a case whose tolerance would exceed 1e-9 is refused here: a wrong update cannot hide behind a loose bound.

  fit|<name>|W, |H, |n_iter, |dist   sklearn.decomposition.NMF(k, init, solver='cd', random_state=42, tol=1e-4,
                                     max_iter=1000).fit_transform on the float64 input
  fit|<name>|sure                    the rule stopped at the same n_iter, with its violation ratio <= tol (1 - 1e-6) at the
                                     stop and >= tol (1 + 1e-6) one iteration earlier: n_iter equality may be demanded
  fit|<name>|W32, |H32, |n_iter32    the same on the float32 copy of the input;  |dist32: its distance to the float64 run
  fft|<name>|out, |dist              the reference's SlidingFFTNMF.process_fft on ``fft_windows(name)``
  img|pos_vec, |fft, |fft_dist       make_windows / process_fft of the 40 x 52 image, window 16, steps (8, 12)
  img|components, |abundances, |dist analyze_image of it with 3 components;  img2|...: the two-window image
  stat|<case>|raw_raises             the reference's imlocal.nmf(k) on the stat.npz case as it is: its frames have a few
                                     pixels below 0, which scikit-learn refuses with a ValueError (True where it did)
  stat|<case>|converged, |converged32   whether scikit-learn stopped before max_iter = 1000 (else it warned)
  stat|<case>|k, |components, |X_vec_t, |com_frames, |dist (+ components32, X_vec_t32, dist32)
                                     the reference's imlocal.nmf(k) on the case's frames clipped at 0, float64 and float32
                                     (imblock_nmf returns the same arrays and the first two coordinate columns: asserted)
  cube|<tag>|components, |maps, |dist   the reference's SpectralUnmixer('nmf', 3, init='nndsvda', max_iter=1000, tol=1e-4)
                                     on the 6 x 7 x 20 cube: plain, normalize=True, and shifted to negative values
TEST INFRASTRUCTURE ONLY.
"""
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness  # noqa: E402
import _nmf_checks as C  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
REFUSE = 1e-9 / 1000.0


def dist(rule, lib):
    return max(C.rel(a, b) for a, b in zip(rule, lib))


def accept(name, d):
    print(f"{name}: rule vs library {d:.2e}")
    assert d <= REFUSE, f"{name}: the rule is {d:.2e} from the library: its tolerance would exceed 1e-9"
    return d


def sk_fit(X, k, init, **kw):
    from sklearn.decomposition import NMF
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # no ConvergenceWarning: every case converges
        m = NMF(n_components=k, init=init, solver="cd", **kw)
        W = m.fit_transform(X)
    return W, m.components_, m.n_iter_


def rule_against(name, X, k, init, lib, **kw):
    """Distance of the rule to the library's (W, H, n_iter) on X and whether n_iter is decidable."""
    W, H, n_iter, ratios = C.fit_rule(X, k, init, **kw)
    tol = kw["tol"]
    assert n_iter == lib[2], (name, n_iter, lib[2])
    sure = ratios[-1] <= tol * (1 - 1e-6) and (len(ratios) < 2 or ratios[-2] >= tol * (1 + 1e-6))
    return accept(name, dist((W, H), lib[:2])), sure


def fits(out):
    for name, (n, d, k, init) in C.FITS.items():
        X = C.fit_input(name)
        lib = sk_fit(X, k, init, **C.FIT_KW)
        out[f"fit|{name}|W"], out[f"fit|{name}|H"], out[f"fit|{name}|n_iter"] = lib
        out[f"fit|{name}|dist"], out[f"fit|{name}|sure"] = rule_against(f"fit {name}", X, k, init, lib, **C.FIT_KW)
        lib32 = sk_fit(X.astype(np.float32), k, init, **C.FIT_KW)
        assert lib32[0].dtype == np.float32
        out[f"fit|{name}|W32"], out[f"fit|{name}|H32"], out[f"fit|{name}|n_iter32"] = lib32
        out[f"fit|{name}|dist32"] = dist(lib32[:2], lib[:2])
        print(f"  n_iter {lib[2]} (float32: {lib32[2]}), sure {out[f'fit|{name}|sure']}, float32 run "
              f"{out[f'fit|{name}|dist32']:.2e} from the float64 run")


def reference_sliding(mod, wx, wy, sx=None, sy=None, factor=2, zoom=2, ham=True, components=4):
    s = mod.SlidingFFTNMF(wx, wy, sx, sy, interpolation_factor=factor, zoom_factor=zoom, hamming_filter=ham,
                          components=components)
    if wx == wy:
        s._calculate_window_params((wx, wy))
    else:                      # its Hamming table cannot be built for a non-square window: set what process_fft reads
        assert not ham
        s.window_size_x, s.window_size_y = wx, wy
    return s


def ffts(out, mod):
    for name, (wx, wy, n, ham, zoom, factor) in C.FFTS.items():
        windows = C.fft_windows(name)
        lib = reference_sliding(mod, wx, wy, factor=factor, zoom=zoom, ham=ham).process_fft(windows)
        rule = C.fft_rule(windows, ham, zoom, factor)
        assert rule.shape == lib.shape, (name, rule.shape, lib.shape)
        out[f"fft|{name}|out"] = lib
        out[f"fft|{name}|dist"] = accept(f"fft {name} {lib.shape}", C.rel(rule, lib))


def images(out, mod):
    for tag, spec in (("img", C.IMAGE), ("img2", C.IMAGE2)):
        img = C.image(spec)
        s = reference_sliding(mod, spec["window"], spec["window"], *spec["steps"], components=spec["components"])
        with tempfile.TemporaryDirectory() as tmp:
            comp, ab = s.analyze_image(img, os.path.join(tmp, "run"))
        windows = s.make_windows(img)
        fft = s.process_fft(windows)
        rule = C.fft_rule(windows, True, 2, 2)
        d_fft = accept(f"{tag} process_fft {fft.shape}", C.rel(rule, fft))
        flat = rule.reshape(len(rule), -1)
        lib = (ab.transpose(1, 2, 0).reshape(len(rule), -1), comp.reshape(len(comp), -1), None)
        W, H, n_iter, _ = C.fit_rule(flat, s.components, "random", 42, 1e-4, 1000)
        out[f"{tag}|components"], out[f"{tag}|abundances"] = comp, ab
        out[f"{tag}|dist"] = accept(f"{tag} analyze_image, {s.components} components, n_iter {n_iter}",
                                    dist((W, H), lib[:2]))
        if tag == "img":
            out["img|pos_vec"], out["img|fft"], out["img|fft_dist"] = s.pos_vec, fft, d_fft
        else:
            assert s.components == 2


def stats(out):
    import _stat_checks as S
    from atomai.stat import multivar as ref
    for name in C.STAT_CASES:
        frames, coords, r, K = S.case(name)
        k = K                                 # the planted classes (1 for r7c1_k1)
        out[f"stat|{name}|k"] = k
        try:                                  # the planted frames have a few pixels below 0: scikit-learn refuses them
            ref.imlocal(frames, coords, r, 0).nmf(k)
            raw_raises = False
        except ValueError as e:
            assert "Negative values" in str(e)
            raw_raises = True
        out[f"stat|{name}|raw_raises"] = raw_raises
        assert raw_raises == bool((ref.imlocal(frames, coords, r, 0).imgstack < 0).any())
        frames = np.maximum(frames, 0)
        for dtype, tag in ((np.float64, ""), (np.float32, "32")):
            s = ref.imlocal(frames.astype(dtype), coords, r, 0)
            with warnings.catch_warnings(record=True) as caught:   # (r7c1_k1 starts at its optimum: the violation cannot
                warnings.simplefilter("always")                    # fall by 1e4 and scikit-learn runs out of iterations)
                comp, xt, cf = s.nmf(k)
                comp2, xt2, centres = s.imblock_nmf(k)
            out[f"stat|{name}|converged{tag}"] = not any("Maximum number of iterations" in str(w.message) for w in caught)
            assert np.array_equal(comp, comp2) and np.array_equal(xt, xt2) and np.array_equal(centres, cf[:, :2])
            out[f"stat|{name}|components{tag}"], out[f"stat|{name}|X_vec_t{tag}"] = comp, xt
            if dtype == np.float64:
                X = s.imgstack.reshape(s.d0, -1)
                W, H, n_iter, _ = C.fit_rule(X, k, None, 1, 1e-4, 1000)
                assert (n_iter < 1000) == bool(out[f"stat|{name}|converged"])
                out[f"stat|{name}|com_frames"] = cf
                out[f"stat|{name}|dist"] = accept(f"stat {name} k={k} n_iter {n_iter}",
                                                  dist((W, H), (xt, comp.reshape(k, -1))))
                lib64 = (xt, comp)
            else:
                assert comp.dtype == np.float32
                out[f"stat|{name}|dist32"] = dist((xt, comp), lib64)
                print(f"  float32 run {out[f'stat|{name}|dist32']:.2e} from the float64 run")


def cubes(out):
    from atomai.stat.unmixer import SpectralUnmixer
    kw = dict(init="nndsvda", max_iter=1000, tol=1e-4)
    for tag, normalize, negative in (("plain", False, False), ("norm", True, False), ("neg", False, True)):
        data = C.cube(negative)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)                      # its own "Shifting data" warning
            comp, maps = SpectralUnmixer("nmf", 3, normalize=normalize, **kw).fit(data)
        X = data.reshape(-1, data.shape[-1])
        norms = X.sum(1, keepdims=True) if normalize else 1.0
        X = X / norms
        X = X - min(X.min(), 0.0)
        W, H, n_iter, _ = C.fit_rule(X, 3, **kw)
        out[f"cube|{tag}|components"], out[f"cube|{tag}|maps"] = comp, maps
        out[f"cube|{tag}|dist"] = accept(f"cube {tag} n_iter {n_iter}", dist((W * norms, H), (maps.reshape(-1, 3), comp)))


def main():
    ref_harness.import_reference()
    try:
        import atomai.stat.fft_nmf as mod
    except Exception as e:                                        # noqa: BLE001
        raise SystemExit(f"atomai.stat.fft_nmf does not import under the harness: {e!r}")
    mod.view_as_windows = lambda image, size, step: np.lib.stride_tricks.sliding_window_view(image, size)[::step[0], ::step[1]]
    out = {}
    fits(out)
    ffts(out, mod)
    images(out, mod)
    stats(out)
    cubes(out)
    path = os.path.join(GOLD, "nmf.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
