"""Shared bodies of the NMF tests (emulator tier on CPU, gpu tier on the MI355X): csrc/nmf.hip and csrc/fftwin.hip through
atomai_amd.stat._nmf, and the public functions and classes built on them, against the numpy rule below and against
tests/golden/nmf.npz, which tools/make_nmf_golden.py records from scikit-learn, scipy and the reference (and where it
asserts that the numpy rule reproduces them on every case).  Neither scikit-learn, scipy nor the reference is imported here.

Bounds.  One half-step against the fp64 rule: |dT| <= 1e-11 max|T| (an fp64 dot product of d <= 1024 non-negative terms
is off by at most d 2^-53 ~ 1e-13 of its value; this leaves 100 x over that); the violation and the Gram matrices are
held to the same relative bound.  Everything compared with the golden file: the device differs from the library exactly
as the numpy rule does, in summation order only, so the tolerance of a case is 1000 x the rule-versus-library distance
(max abs difference over max abs value) that the generator recorded for it, with a floor of 2^-52 under the distance: a
distance of values in fp64 cannot be resolved below their spacing.  The generator refuses a case whose tolerance would
exceed 1e-9.  For float32 input the device (fp64 arithmetic on the float32 values) must be within twice the recorded
distance between scikit-learn's float32 and float64 runs of scikit-learn's float32 run.  ``n_iter`` equality is demanded
only where the generator has checked the rule's violation ratio on both sides of the stop (key ``|sure``)."""
import os
import warnings

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_gold = None
_cache = {}

HALF_SHAPES = [(1, 9, 1), (5, 700, 2), (700, 5, 2), (70, 45, 3), (37, 19, 5), (257, 130, 32)]
HALF_VARIANTS = [((70, 45, 3), "zerocol"), ((37, 19, 5), "zeros"), ((257, 130, 32), "zeros"), ((257, 130, 32), "zerocol")]
# name: (n, d, k, init)  --  rank-k matrices plus 1 % noise, fit_input(name)
FITS = {
    "random_70x45_k3": (70, 45, 3, "random"),
    "random_37x19_k5": (37, 19, 5, "random"),
    "random_300x256_k4": (300, 256, 4, "random"),
    "nndsvda_60x100_k5": (60, 100, 5, "nndsvda"),
    "nndsvd_60x100_k5": (60, 100, 5, "nndsvd"),
    "nndsvda_200x768_k3": (200, 768, 3, "nndsvda"),
    "nndsvd_200x768_k3": (200, 768, 3, "nndsvd"),
}
FIT_KW = dict(random_state=42, tol=1e-4, max_iter=1000)
# name: (wx, wy, n windows, hamming, zoom_factor, interpolation_factor)
FFTS = {
    "w8_z4": (8, 8, 3, True, 4, 2),
    "w15": (15, 15, 3, True, 2, 2),
    "w16_z1_f3": (16, 16, 3, True, 1, 3),
    "w24": (24, 24, 2, True, 2, 2),
    "w30_f15": (30, 30, 2, True, 2, 1.5),
    "w20x28_nh_z3_f1": (20, 28, 2, False, 3, 1),
    "w128": (128, 128, 2, True, 2, 2),
}
IMAGE = dict(shape=(40, 52), window=16, steps=(8, 12), components=3)
IMAGE2 = dict(shape=(16, 24), window=16, steps=(8, 8), components=4)         # two windows: components drop to 2
STAT_CASES = ["r5c3", "r8c1", "r7c1_k1"]
CUBE = (6, 7, 20)


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLD, "nmf.npz")) as g:
            _gold = {k: g[k] for k in g.files}
    return _gold


def tol_of(key):
    """1000 x the recorded rule-versus-library distance (floored at 2^-52)."""
    return 1000.0 * max(float(gold()[key]), 2.0 ** -52)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), np.finfo(np.float64).tiny))


# ------------------------------------------------------------------------------------------------ inputs
def low_rank(n, d, k, seed, noise=0.01):
    """A non-negative rank-k matrix plus 1 % noise: the product of two factors with about half their entries zero (the
    coordinate descent then settles in tens of iterations, which keeps the tests quick) plus uniform noise of
    ``noise`` times the mean."""
    rs = np.random.RandomState(seed)
    A = rs.rand(n, k) * (rs.rand(n, k) < 0.5)
    B = rs.rand(k, d) * (rs.rand(k, d) < 0.5)
    X = A @ B
    return X + noise * X.mean() * rs.rand(n, d)


def fit_input(name):
    n, d, k, _ = FITS[name]
    return low_rank(n, d, k, 1000 + n + d + k)


def fft_windows(name):
    wx, wy, n = FFTS[name][:3]
    return np.random.RandomState(wx * 131 + wy).rand(n, wx, wy)


def image(spec):
    """Two textures side by side on a 0 .. 255 scale, so that the windows differ."""
    h, w = spec["shape"]
    rs = np.random.RandomState(h * 1000 + w)
    yy, xx = np.mgrid[:h, :w]
    img = np.where(xx < w // 2, np.sin(2 * np.pi * xx / 4.0), np.sin(2 * np.pi * yy / 3.0)) + 0.3 * rs.rand(h, w)
    return 100.0 + 50.0 * img


def cube(negative=False):
    rs = np.random.RandomState(77)
    h, w, e = CUBE
    c = low_rank(h * w, e, 3, 78).reshape(h, w, e)
    return c - 0.25 if negative else c


# ------------------------------------------------------------------------------------------------ the numpy rule
def half_step_rule(X, T, F):
    """One half-step of scikit-learn's coordinate descent in fp64: T (R, k) is updated in place with F (L, k) fixed, X
    is (R, L).  Returns the violation."""
    XF, FF = X @ F, F.T @ F
    violation = 0.0
    for t in range(T.shape[1]):
        grad = -XF[:, t] + T @ FF[t]
        pg = np.where(T[:, t] == 0, np.minimum(0.0, grad), grad)
        violation += np.abs(pg).sum()
        if FF[t, t] != 0:
            T[:, t] = np.maximum(T[:, t] - grad / FF[t, t], 0.0)
    return violation


def init_rule(X, k, init, random_state):
    """scikit-learn's initial factors in fp64 (W (n, k), H (k, d)); NNDSVD from the exact SVD."""
    n, d = X.shape
    if init is None:
        init = "nndsvda" if k <= min(n, d) else "random"
    if init == "random":
        avg = np.sqrt(X.mean() / k)
        rng = np.random.RandomState(random_state)
        H = np.abs(avg * rng.standard_normal((k, d)))
        W = np.abs(avg * rng.standard_normal((n, k)))
        return W, H
    U, S, V = np.linalg.svd(X, full_matrices=False)
    W, H = np.zeros((n, k)), np.zeros((k, d))
    W[:, 0], H[0] = np.sqrt(S[0]) * np.abs(U[:, 0]), np.sqrt(S[0]) * np.abs(V[0])
    for j in range(1, k):
        x, y = U[:, j], V[j]
        xp, yp, xn, yn = np.maximum(x, 0), np.maximum(y, 0), np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        mp, mn = np.linalg.norm(xp) * np.linalg.norm(yp), np.linalg.norm(xn) * np.linalg.norm(yn)
        if mp > mn:
            u, v, sigma = xp / np.linalg.norm(xp), yp / np.linalg.norm(yp), mp
        else:
            u, v, sigma = xn / np.linalg.norm(xn), yn / np.linalg.norm(yn), mn
        W[:, j], H[j] = np.sqrt(S[j] * sigma) * u, np.sqrt(S[j] * sigma) * v
    W[W < 1e-6], H[H < 1e-6] = 0, 0
    if init == "nndsvda":
        W[W == 0], H[H == 0] = X.mean(), X.mean()
    return W, H


def fit_rule(X, k, init=None, random_state=None, tol=1e-4, max_iter=200):
    """The whole fit in fp64: (W, H, n_iter, ratios), ratios[i] = violation / first violation of iteration i + 1."""
    X = np.asarray(X, dtype=np.float64)
    W, H = init_rule(X, k, init, random_state)
    Ht = np.ascontiguousarray(H.T)
    ratios, first = [], None
    for n_iter in range(1, max_iter + 1):
        violation = half_step_rule(X, W, Ht) + half_step_rule(X.T, Ht, W)
        if n_iter == 1:
            first = violation
        if first == 0:
            break
        ratios.append(violation / first)
        if ratios[-1] <= tol:
            break
    return W, Ht.T.copy(), n_iter, ratios


def zoom_rule(a, factor):
    """scipy.ndimage.zoom(a, factor, order=1) of a 2D array."""
    if factor <= 1:
        return a
    out_shape = [int(round(s * factor)) for s in a.shape]
    tabs = []
    for n_in, n_out in zip(a.shape, out_shape):
        src = np.arange(n_out) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 1.0)
        i0 = np.floor(src).astype(int)
        t = src - i0
        ok = src <= n_in - 1
        tabs.append((np.where(ok, i0, 0), np.where(ok, np.minimum(i0 + 1, n_in - 1), 0), np.where(ok, 1 - t, 0.0),
                     np.where(ok, t, 0.0)))
    (i0, i1, xa, xb), (j0, j1, ya, yb) = tabs
    out = a[np.ix_(i0, j0)] * xa[:, None] * ya[None, :]
    out = out + a[np.ix_(i0, j1)] * xa[:, None] * yb[None, :]
    out = out + a[np.ix_(i1, j0)] * xb[:, None] * ya[None, :]
    return out + a[np.ix_(i1, j1)] * xb[:, None] * yb[None, :]


def hamming_table(wx, wy):
    bw2d = np.outer(np.hamming(wx), np.ones(wy))
    return np.sqrt(bw2d * bw2d.T)


def fft_rule(windows, hamming, zoom_factor, factor):
    """process_fft as a direct DFT at the cropped frequencies only: shifted index s is frequency (s - N // 2) mod N."""
    n, wx, wy = windows.shape
    zs = max(1, wx // (2 * zoom_factor))
    x0, x1, y0, y1 = max(0, wx // 2 - zs), min(wx, wx // 2 + zs), max(0, wy // 2 - zs), min(wy, wy // 2 + zs)
    fx, fy = (np.arange(x0, x1) - wx // 2) % wx, (np.arange(y0, y1) - wy // 2) % wy
    Ex = np.exp(-2j * np.pi * ((fx[:, None] * np.arange(wx)[None, :]) % wx) / wx)
    Ey = np.exp(-2j * np.pi * ((fy[:, None] * np.arange(wy)[None, :]) % wy) / wy)
    out = []
    for w in windows:
        a = w * hamming_table(wx, wy) if hamming else w
        out.append(zoom_rule(np.log1p(np.abs(Ex @ a @ Ey.T)), factor))
    return np.array(out)


# ------------------------------------------------------------------------------------------------ 1. one half-step
def half_inputs(n, d, k, trans, variant):
    """X (n, d), T and F for one half-step.  variant 'zerocol': an all-zero column of the fixed factor (the Hessian
    entry is 0: no update); 'zeros': exact zeros in the updated factor (the projected-gradient branch)."""
    key = (n, d, k, trans, variant)
    if key not in _cache:
        rs = np.random.RandomState(n * 7919 + d * 31 + k + 5 * trans)
        X = rs.rand(n, d)
        R, L = (d, n) if trans else (n, d)
        T, F = np.abs(rs.standard_normal((R, k))), np.abs(rs.standard_normal((L, k)))
        if variant == "zerocol":
            F[:, k // 2] = 0.0
        if variant == "zeros":
            T[rs.rand(R, k) < 0.4] = 0.0
        out = {}
        for dt in (np.float64, np.float32):
            Xd = X.astype(dt)
            Xr = Xd.astype(np.float64)
            Tn = T.copy()
            viol = half_step_rule(Xr.T if trans else Xr, Tn, F)
            out[dt] = (Xd, Tn, viol)
        _cache[key] = (T, F, out)
    return _cache[key]


def check_half_step(shape, trans, dtype, device, variant="plain"):
    from atomai_amd.stat import _nmf
    n, d, k = shape
    T, F, out = half_inputs(n, d, k, trans, variant)
    Xd, Tn, viol = out[dtype]
    got_T, got_v, gram_T, gram_F = _nmf.nmf_half_step(torch.from_numpy(Xd).to(device), torch.from_numpy(T),
                                                      torch.from_numpy(F), trans)
    got_T = got_T.cpu().numpy()
    if variant == "zeros":
        assert (T == 0).any() and np.array_equal(got_T == 0, Tn == 0)
    if variant == "zerocol":
        assert np.array_equal(got_T[:, k // 2], T[:, k // 2])              # untouched: its Hessian entry is 0
    err = dict(T=rel(got_T, Tn), viol=abs(float(got_v) - viol) / viol, gram_T=rel(gram_T.cpu().numpy(), Tn.T @ Tn),
               gram_F=rel(gram_F.cpu().numpy(), F.T @ F))
    print(shape, trans, np.dtype(dtype).name, variant, err)
    assert max(err.values()) <= 1e-11, err


def check_splits():
    """The number of splits is a function of the shape; the SlidingFFTNMF shape gets enough workgroups for the chip."""
    from atomai_amd.stat import _nmf
    for n, d, k in HALF_SHAPES + [(841, 4096, 4)]:
        for trans in (0, 1):
            s = _nmf.splits(n, d, k, trans)
            assert 1 <= s <= 32 and s == _nmf.splits(n, d, k, trans)
    assert _nmf.splits(841, 4096, 4, 0) * -(-841 // 32) >= 256 and _nmf.splits(841, 4096, 4, 1) * (4096 // 256) >= 256


# ------------------------------------------------------------------------------------------------ 2. full fits
def check_fit(name, device, dtype=np.float64):
    from atomai_amd.stat import _nmf
    g = gold()
    n, d, k, init = FITS[name]
    X = fit_input(name).astype(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = _nmf.fit_nmf(torch.from_numpy(X).to(device), k, init=init, **FIT_KW)
    W, H = res["W"].cpu().numpy(), res["H"].cpu().numpy()
    if dtype == np.float64:
        tol = tol_of(f"fit|{name}|dist")
        err = max(rel(W, g[f"fit|{name}|W"]), rel(H, g[f"fit|{name}|H"]))
        print(name, "n_iter", res["n_iter"], int(g[f"fit|{name}|n_iter"]), "err", err, "tol", tol)
        assert err <= tol, (err, tol)
        if bool(g[f"fit|{name}|sure"]):
            assert res["n_iter"] == int(g[f"fit|{name}|n_iter"])
    else:
        tol = 2.0 * float(g[f"fit|{name}|dist32"])
        err = max(rel(W, g[f"fit|{name}|W32"]), rel(H, g[f"fit|{name}|H32"]))
        print(name, "float32 n_iter", res["n_iter"], int(g[f"fit|{name}|n_iter32"]), "err", err, "tol", tol)
        assert err <= tol, (err, tol)
    assert res["converged"] and W.dtype == np.float64 and W.shape == (n, k) and H.shape == (k, d)


def check_determinism(device):
    from atomai_amd.stat import _nmf
    X = torch.from_numpy(fit_input("random_37x19_k5").astype(np.float32)).to(device)
    runs = [_nmf.fit_nmf(X, 5, init="random", random_state=3, tol=1e-3, max_iter=60) for _ in range(2)]
    assert runs[0]["n_iter"] == runs[1]["n_iter"]
    assert torch.equal(runs[0]["W"], runs[1]["W"]) and torch.equal(runs[0]["H"], runs[1]["H"])


# ------------------------------------------------------------------------------------------------ 3. the FFT front end
def _sliding(name):
    from atomai_amd.stat.fft_nmf import SlidingFFTNMF
    wx, wy, n, ham, zf, f = FFTS[name]
    s = SlidingFFTNMF(wx, wy, interpolation_factor=f, zoom_factor=zf, hamming_filter=ham)
    s._calculate_window_params((wx, wy))
    return s


def check_fft(name):
    g = gold()
    got = _sliding(name).process_fft(fft_windows(name))
    want, tol = g[f"fft|{name}|out"], tol_of(f"fft|{name}|dist")
    err = rel(got, want)
    print(name, got.shape, "err", err, "tol", tol)
    assert got.dtype == np.float64 and err <= tol, (err, tol)


def _image_sliding(spec):
    from atomai_amd.stat.fft_nmf import SlidingFFTNMF
    return SlidingFFTNMF(spec["window"], spec["window"], *spec["steps"], components=spec["components"])


def check_in_place_equals_stack():
    """The same kernel reads the overlapping windows from the image and from the materialised stack: equal bits; and
    both match the reference's process_fft."""
    from atomai_amd.stat import _nmf
    g = gold()
    s = _image_sliding(IMAGE)
    windows = s.make_windows(image(IMAGE))
    assert windows.shape == (16, 16, 16) and s.windows_shape == (4, 4) and np.array_equal(s.pos_vec, g["img|pos_vec"])
    stack = s.process_fft(windows)
    norm = s._normalised(image(IMAGE))
    feats, size = _nmf.fft_features(norm, (16, 16), s.windows_shape, IMAGE["steps"], s.hamming_window)
    assert size == (16, 16) and np.array_equal(feats.cpu().numpy().reshape(stack.shape), stack)
    assert rel(stack, g["img|fft"]) <= tol_of("img|fft_dist")


def check_analyze_image(tmp_path):
    g = gold()
    s = _image_sliding(IMAGE)
    comp, ab = s.analyze_image(image(IMAGE), str(tmp_path / "run"))
    tol = tol_of("img|dist")
    err = max(rel(comp, g["img|components"]), rel(ab, g["img|abundances"]))
    print("analyze_image err", err, "tol", tol)
    assert comp.shape == (3, 16, 16) and ab.shape == (3, 4, 4) and err <= tol, (err, tol)
    assert np.array_equal(np.load(tmp_path / "run_components.npy"), comp)
    assert np.array_equal(np.load(tmp_path / "run_abundances.npy"), ab)
    rgb = np.stack([image(IMAGE)] * 3 + [np.zeros(IMAGE["shape"])], axis=-1)       # RGBA: the weights sum to 1
    assert np.allclose(_image_sliding(IMAGE).make_windows(rgb), _image_sliding(IMAGE).make_windows(image(IMAGE)),
                       rtol=0, atol=1e-12)


def check_two_windows(tmp_path):
    g = gold()
    s = _image_sliding(IMAGE2)
    comp, ab = s.analyze_image(image(IMAGE2), str(tmp_path / "two"))
    assert s.components == 2 and comp.shape == (2, 16, 16) and ab.shape == (2, 1, 2)
    tol = tol_of("img2|dist")
    assert max(rel(comp, g["img2|components"]), rel(ab, g["img2|abundances"])) <= tol


# ------------------------------------------------------------------------------------------------ 4. imlocal, unmixer
def check_imlocal(name):
    import _stat_checks as S
    import atomai_amd as aoi
    from atomai_amd.stat import nmf
    from atomai_amd.stat._gmm import ConvergenceWarning
    g = gold()
    k = int(g[f"stat|{name}|k"])
    frames, coords, r, _ = S.case(name)
    if bool(g[f"stat|{name}|raw_raises"]):       # a few pixels of the planted frames are below 0: a ValueError, as there
        with pytest.raises(ValueError, match="non-negative"):
            nmf.imlocal_nmf(S.stat_of(name)[0], k)
    frames = np.maximum(frames, 0)
    for dtype, tag in ((np.float64, ""), (np.float32, "32")):
        stack = aoi.stat.imlocal(frames.astype(dtype), coords, r, 0)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            comp, xt, cf = nmf.imlocal_nmf(stack, k)
        if dtype == np.float64:                   # (r7c1_k1 starts at its optimum and runs out of iterations, as there)
            assert bool(g[f"stat|{name}|converged"]) != any(w.category is ConvergenceWarning for w in caught)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", ConvergenceWarning)
                comp2, xt2, centres = nmf.imblock_nmf(stack, k)
            assert np.array_equal(comp, comp2) and np.array_equal(xt, xt2) and np.array_equal(centres, cf[:, :2])
        tol = tol_of(f"stat|{name}|dist") if dtype == np.float64 else 2.0 * float(g[f"stat|{name}|dist32"])
        err = max(rel(comp, g[f"stat|{name}|components{tag}"]), rel(xt, g[f"stat|{name}|X_vec_t{tag}"]))
        print(name, np.dtype(dtype).name, "err", err, "tol", tol)
        assert err <= tol, (err, tol)
        assert comp.shape == (k, stack.d1, stack.d2, stack.d3) and np.array_equal(cf, g[f"stat|{name}|com_frames"])


def check_unmixer():
    from atomai_amd.stat.unmixer import SpectralUnmixer
    g = gold()
    for tag, normalize, negative in (("plain", False, False), ("norm", True, False), ("neg", False, True)):
        u = SpectralUnmixer("nmf", 3, normalize=normalize, init="nndsvda", max_iter=1000, tol=1e-4)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            comp, maps = u.fit(cube(negative))
        assert negative == any("Shifting" in str(w.message) for w in caught)
        tol = tol_of(f"cube|{tag}|dist")
        err = max(rel(comp, g[f"cube|{tag}|components"]), rel(maps, g[f"cube|{tag}|maps"]))
        print("unmixer", tag, "err", err, "tol", tol)
        assert comp.shape == (3, 20) and maps.shape == (6, 7, 3) and err <= tol, (err, tol)
    for method in ("pca", "ica", "gmm"):
        with pytest.raises(NotImplementedError, match="nmf"):
            SpectralUnmixer(method)
    with pytest.raises(ValueError):
        SpectralUnmixer("svd")
    with pytest.raises(ValueError, match="3D"):
        SpectralUnmixer().fit(np.ones((4, 5)))


# ------------------------------------------------------------------------------------------------ 5. errors
def check_errors(device):
    from atomai_amd.stat import _gmm, _nmf
    from atomai_amd.stat.fft_nmf import SlidingFFTNMF
    X = torch.from_numpy(low_rank(12, 9, 2, 5)).to(device)
    bad = X.clone()
    bad[3, 4] = -1e-3
    with pytest.raises(ValueError, match="non-negative"):
        _nmf.fit_nmf(bad, 2)
    bad[3, 4] = float("nan")
    with pytest.raises(ValueError, match="non-negative"):
        _nmf.fit_nmf(bad, 2)
    with pytest.raises(ValueError, match="32"):
        _nmf.fit_nmf(X, 33, init="random")
    with pytest.raises(ValueError, match="n_components <= min"):
        _nmf.fit_nmf(X, 10, init="nndsvd")
    with pytest.raises(ValueError, match="init"):
        _nmf.fit_nmf(X, 2, init="nndsvdar")
    with pytest.warns(_gmm.ConvergenceWarning):
        res = _nmf.fit_nmf(X, 2, init="random", random_state=0, max_iter=2)
    assert res["n_iter"] == 2 and not res["converged"]
    res = _nmf.fit_nmf(X, 10, random_state=0, max_iter=3, tol=0)            # init=None beyond min(n, d): 'random'
    assert res["W"].shape == (12, 10)
    with pytest.raises(ValueError, match="128"):
        SlidingFFTNMF(129, 129).make_windows(np.ones((200, 200)))
    with pytest.raises(ValueError, match="128"):
        _nmf.fft_features(np.ones((1, 129, 8)), (129, 8))
    with pytest.raises(NotImplementedError, match="array"):
        SlidingFFTNMF().analyze_image("image.png")
    with pytest.raises(ValueError, match="square"):
        SlidingFFTNMF(16, 20).make_windows(np.ones((40, 40)))
    with pytest.raises(ValueError, match="Invalid data"):                    # an all-zero image: every spectrum is log1p(0)
        SlidingFFTNMF(16, 16).analyze_image(np.zeros((32, 32)))


def check_module_paths():
    """The working classes live at the reference's module paths; the package-level names still raise."""
    import atomai_amd as aoi
    assert aoi.stat.fft_nmf.SlidingFFTNMF is not aoi.stat.SlidingFFTNMF
    assert aoi.stat.nmf.fit_nmf is aoi.stat._nmf.fit_nmf
    for cls in (aoi.stat.SlidingFFTNMF, aoi.stat.SpectralUnmixer):
        with pytest.raises(NotImplementedError, match="atomai_amd.stat"):
            cls()
    assert aoi.stat.fft_nmf.SlidingFFTNMF().components == 4 and aoi.stat.unmixer.SpectralUnmixer().method == "nmf"
