"""Shared bodies of the FastICA tests (emulator tier on CPU, gpu tier on the MI355X): csrc/ica.hip through
atomai_amd.stat._ica, and the public functions and classes built on it, against the numpy rule below and against
tests/golden/ica.npz, which tools/make_ica_golden.py records from scikit-learn and the reference (and where it asserts that
the numpy rule reproduces them on every case).  Neither scikit-learn nor the reference is imported here.

Bounds.  Step + reduce and the projection against the fp64 rule: 1e-11 x the largest entry of the same expression
evaluated on absolute values (mean(|g| |x|^T) + |h| |W|, resp. scale |M| |X - mean|^T).  For n, d <= 4097 terms at 2^-53
each the summation error is at most 5e-13 of that, and tanh / exp are within a few ulp: about 20 x is left.  The column
standard deviations (sums of at most 700 non-negative terms, 8e-14 relative) are held to 1e-12 relative.  Everything
compared with the golden file: the device differs from the library as the numpy rule does (summation order, the Gram route
of the whitening), so the tolerance of a case is 1000 x the rule-versus-library distance (max abs difference over max abs
value) that the generator recorded for it, floored at 2^-52.  The generator refuses a case whose tolerance would exceed
1e-9, whose sign rule or whitening is ill-conditioned, or whose ``lim`` is within 1e-3 tol of ``tol`` at the stop or one
iteration earlier, so ``n_iter`` equality is demanded everywhere.  For float32 input the device does fp64 arithmetic on the
float32 values: it is compared, at the same tolerance, with the library run on ``X.astype(float32).astype(float64)``."""
import os
import warnings

import numpy as np
import pytest
import torch

import _nmf_checks as N

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_gold = None
_cache = {}

FUN_NAMES = ("logcosh", "exp", "cube")
STEP_SHAPES = [(1, 1), (2, 63), (2, 64), (3, 65), (5, 700), (8, 257), (16, 1000), (32, 4097)]       # (k, n)
PROJ_SHAPES = [(2, 3, 1), (700, 5, 2), (70, 45, 3), (45, 200, 3), (257, 130, 32)]                   # (n, d, k)
# name: (n, d, k, keyword arguments of the fit); inputs: fit_input(name)
FITS = {
    "60x9_k2": (60, 9, 2, {}),
    "45x200_k3": (45, 200, 3, {}),
    "45x200_k3_exp": (45, 200, 3, dict(fun="exp")),
    "45x200_k3_cube": (45, 200, 3, dict(fun="cube")),
    "300x40_k3": (300, 40, 3, {}),
    "300x40_k3_exp": (300, 40, 3, dict(fun="exp")),
    "300x40_k3_cube": (300, 40, 3, dict(fun="cube")),
    "300x40_k3_alpha": (300, 40, 3, dict(fun_args={"alpha": 1.5})),
    "300x40_k3_arbitrary": (300, 40, 3, dict(whiten="arbitrary-variance")),
    "257x130_k8_winit": (257, 130, 8, dict(w_init="given")),
    "1000x48_k16": (1000, 48, 16, {}),
}
FIT_KW = dict(random_state=7, tol=1e-4, max_iter=200)
# Seed of a shape's input where the default (2000 + n + d + k) gives a case that the generator refuses: a first row of u
# near zero at 45 x 200, a fixed point that amplifies the rule-versus-library distance beyond 1e-12 at 1000 x 48.
INPUT_SEED = {(45, 200, 3): 2249, (1000, 48, 16): 3065}
FIELDS = ("components", "sources", "mixing", "whitening", "mean")
STAT_CASES = ["r5c3", "r8c1", "r7c1_k1"]
STAT_KS = (2, 3)
CUBE_SEED = 11


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLD, "ica.npz")) as g:
            _gold = {k: g[k] for k in g.files}
    return _gold


def tol_of(key):
    """1000 x the recorded rule-versus-library distance (floored at 2^-52)."""
    return 1000.0 * max(float(gold()[key]), 2.0 ** -52)


rel = N.rel


# ------------------------------------------------------------------------------------------------ inputs
def mixture(n, d, k, seed, noise=0.02):
    """k independent sources (Laplace and uniform in turn) through a random (k, d) matrix, plus 2 % noise."""
    rs = np.random.RandomState(seed)
    S = np.empty((n, k))
    for j in range(k):
        S[:, j] = rs.laplace(size=n) if j % 2 == 0 else rs.uniform(-np.sqrt(3.0), np.sqrt(3.0), n)
    X = S @ rs.standard_normal((k, d)) + 1.0 + rs.rand(d)
    return X + noise * X.std() * rs.standard_normal((n, d))


def fit_input(name):
    n, d, k, _ = FITS[name]
    return mixture(n, d, k, INPUT_SEED.get((n, d, k), 2000 + n + d + k))


def fit_kwargs(name):
    k, kw = FITS[name][2], dict(FITS[name][3])
    if kw.get("w_init") == "given":
        kw["w_init"] = np.random.RandomState(99).uniform(-1, 1, (k, k)) + 2.0 * np.eye(k)
    return {**FIT_KW, **kw}


# ------------------------------------------------------------------------------------------------ the numpy rule
def contrast(Y, fun, alpha=1.0):
    if fun == "logcosh":
        g = np.tanh(alpha * Y)
        return g, alpha * (1.0 - g ** 2)
    if fun == "exp":
        e = np.exp(-(Y ** 2) / 2.0)
        return Y * e, (1.0 - Y ** 2) * e
    return Y ** 3, 3.0 * Y ** 2


def step_rule(X1, W, fun, alpha=1.0):
    """A = g(W X1) X1^T / n - diag(mean g'(W X1)) W and the same expression on absolute values (the bound's scale)."""
    n = X1.shape[1]
    g, gp = contrast(W @ X1, fun, alpha)
    h = gp.mean(1)
    return g @ X1.T / n - h[:, None] * W, np.abs(g) @ np.abs(X1).T / n + np.abs(h)[:, None] * np.abs(W)


def symdec(W):
    s, u = np.linalg.eigh(W @ W.T)
    s = np.clip(s, np.finfo(np.float64).tiny, None)
    return (u * (1.0 / np.sqrt(s))) @ u.T @ W


def fit_rule(X, k, fun="logcosh", fun_args=None, whiten="unit-variance", max_iter=200, tol=1e-4, random_state=None,
             w_init=None):
    """The whole fit in fp64, whitening through the Gram matrix of the smaller side.  Returns a dict with the five
    FIELDS, ``n_iter``, ``lims`` (lim of every iteration), ``u`` (d, k) and ``sigma`` (k,)."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    k = min(k, n, d)
    alpha = (fun_args or {}).get("alpha", 1.0)
    mean = X.mean(0)
    Xc = X - mean
    lam, vec = np.linalg.eigh(Xc.T @ Xc if d <= n else Xc @ Xc.T)
    lam, vec = lam[::-1][:k], vec[:, ::-1][:, :k]
    sigma = np.sqrt(lam)
    u = vec if d <= n else Xc.T @ vec / sigma
    u = u * np.sign(u[0])
    K = (u / sigma).T
    X1 = np.sqrt(n) * (K @ Xc.T)
    if w_init is None:
        rng = np.random.mtrand._rand if random_state is None else np.random.RandomState(random_state)
        w_init = rng.normal(size=(k, k))
    W = symdec(np.asarray(w_init, dtype=np.float64))
    lims = []
    for n_iter in range(1, max_iter + 1):
        W1 = symdec(step_rule(X1, W, fun, alpha)[0])
        lims.append(np.abs(np.abs((W1 * W).sum(1)) - 1.0).max())
        W = W1
        if lims[-1] < tol:
            break
    S = (W @ K @ Xc.T).T
    if whiten == "unit-variance":
        sd = S.std(0)
        S, W = S / sd, W / sd[:, None]
    C = W @ K
    return dict(components=C, sources=S, mixing=np.linalg.pinv(C), whitening=K, mean=mean, n_iter=n_iter, lims=lims, u=u,
                sigma=sigma)


# ------------------------------------------------------------------------------------------------ 1. the kernels
def step_inputs(k, n):
    """X1 (k, n) with unit-variance rows (n = 1: as drawn) and an orthogonal W, and the rule's output per contrast."""
    if (k, n) not in _cache:
        rs = np.random.RandomState(k * 10007 + n)
        X1 = rs.standard_normal((k, n)) + 0.3 * rs.laplace(size=(k, n))
        if n > 1:
            X1 = (X1 - X1.mean(1, keepdims=True)) / X1.std(1, keepdims=True)
        W = np.linalg.qr(rs.standard_normal((k, k)))[0]
        _cache[(k, n)] = (X1, W, {(f, a): step_rule(X1, W, f, a) for f in FUN_NAMES for a in (1.0,)},
                          step_rule(X1, W, "logcosh", 1.7))
    return _cache[(k, n)]


def check_step(shape, fun, device):
    from atomai_amd.stat import _ica
    k, n = shape
    X1, W, rules, rule_alpha = step_inputs(k, n)
    cases = [(1.0, rules[(fun, 1.0)])] + ([(1.7, rule_alpha)] if fun == "logcosh" else [])
    for alpha, (want, scale) in cases:
        got = _ica.ica_step(torch.from_numpy(X1).to(device), torch.from_numpy(W).to(device), fun, alpha).cpu().numpy()
        err, bound = float(np.abs(got - want).max()), 1e-11 * float(scale.max())
        print("step", shape, fun, alpha, "blocks", _ica.blocks(n, k), "err", err, "bound", bound)
        assert got.shape == (k, k) and got.dtype == np.float64 and err <= bound, (err, bound)


def check_project(shape, dtype, device):
    from atomai_amd.stat import _ica
    n, d, k = shape
    rs = np.random.RandomState(n * 131 + d * 7 + k)
    X = (rs.rand(n, d) + 0.5).astype(dtype)
    X64 = X.astype(np.float64)
    M, mean, scale = rs.standard_normal((k, d)), X64.mean(0), np.sqrt(n)
    want, mag = scale * (M @ (X64 - mean).T), scale * (np.abs(M) @ np.abs(X64 - mean).T)
    got = _ica.project(torch.from_numpy(X).to(device), torch.from_numpy(mean).to(device),
                       torch.from_numpy(M).to(device), scale).cpu().numpy()
    err, bound = float(np.abs(got - want).max()), 1e-11 * float(mag.max())
    print("project", shape, np.dtype(dtype).name, "err", err, "bound", bound)
    assert got.shape == (k, n) and got.dtype == np.float64 and err <= bound, (err, bound)
    if n > 1:                                                        # the column standard deviations of step 5
        sd = _ica.row_std(torch.from_numpy(want).to(device)).cpu().numpy()
        assert rel(sd, want.std(1)) <= 1e-12


def check_blocks():
    """The grid of the step is a function of (k, n) only: of n, in fact."""
    from atomai_amd.stat import _ica
    for k, n in STEP_SHAPES + [(10, 20000), (32, 10 ** 6)]:
        b = _ica.blocks(n, k)
        assert 1 <= b <= 256 and b == _ica.blocks(n, k) == _ica.blocks(n, 1) == _ica.blocks(n, 32)
    assert [_ica.blocks(n, 3) for n in (1, 64, 65, 4097, 20000)] == [1, 1, 2, 65, 157]
    assert _ica.blocks(0, 3) == 0 and _ica.blocks(100, 33) == 0


# ------------------------------------------------------------------------------------------------ 2. full fits
def _compare(res, prefix, tag, tol):
    g = gold()
    err = {f: rel(res[f], g[f"{prefix}|{f}{tag}"]) for f in FIELDS}
    print(prefix, tag or "f64", "n_iter", res["n_iter"], int(g[f"{prefix}|n_iter{tag}"]), "err", err, "tol", tol)
    assert max(err.values()) <= tol, (err, tol)
    assert res["n_iter"] == int(g[f"{prefix}|n_iter{tag}"])


def check_fit(name, device, dtype=np.float64):
    from atomai_amd.stat import _ica
    n, d, k, _ = FITS[name]
    X = fit_input(name).astype(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = _ica.fit_ica(torch.from_numpy(X).to(device), k, **fit_kwargs(name))
    assert res["converged"] and all(res[f].dtype == torch.float64 for f in FIELDS)
    assert res["components"].shape == (k, d) and res["sources"].shape == (n, k) and res["mixing"].shape == (d, k)
    assert res["whitening"].shape == (k, d) and res["mean"].shape == (d,)
    out = {f: res[f].cpu().numpy() for f in FIELDS}
    out["n_iter"] = res["n_iter"]
    tag = "" if dtype == np.float64 else "32"
    _compare(out, f"fit|{name}", tag, tol_of(f"fit|{name}|dist{tag}"))


def check_determinism(device):
    from atomai_amd.stat import _ica
    X = torch.from_numpy(fit_input("300x40_k3").astype(np.float32)).to(device)
    runs = [_ica.fit_ica(X, 3, **FIT_KW) for _ in range(2)]
    assert runs[0]["n_iter"] == runs[1]["n_iter"]
    assert all(torch.equal(runs[0][f], runs[1][f]) for f in FIELDS)


# ------------------------------------------------------------------------------------------------ 3. imlocal, unmixer
def check_imlocal(name):
    import _stat_checks as S
    import atomai_amd as aoi
    from atomai_amd.stat import ica
    g = gold()
    frames, coords, r, _ = S.case(name)
    for dtype, tag in ((np.float64, ""), (np.float32, "32")):
        stack = aoi.stat.imlocal(frames.astype(dtype), coords, r, 0)
        for k in STAT_KS:
            prefix = f"stat|{name}|k{k}"
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                comp, xt, cf = ica.imlocal_ica(stack, k)
            tol = tol_of(f"{prefix}|dist{tag}")
            err = max(rel(comp, g[f"{prefix}|components{tag}"]), rel(xt, g[f"{prefix}|X_vec_t{tag}"]))
            print(name, k, np.dtype(dtype).name, "err", err, "tol", tol)
            assert err <= tol, (err, tol)
            assert comp.shape == (k, stack.d1, stack.d2, stack.d3) and comp.dtype == np.float64
            assert np.array_equal(cf, g[f"stat|{name}|com_frames"])
            if dtype == np.float64 and k == STAT_KS[0]:
                comp2, xt2, centres = ica.imblock_ica(stack, k, marker_size=10)
                assert np.array_equal(comp, comp2) and np.array_equal(xt, xt2) and np.array_equal(centres, cf[:, :2])


def check_unmixer():
    from atomai_amd.stat.ica import ICAUnmixer
    g = gold()
    for tag, normalize in (("plain", False), ("norm", True)):
        u = ICAUnmixer(3, normalize=normalize)
        np.random.seed(CUBE_SEED)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            comp, maps = u.fit(N.cube())
        tol = tol_of(f"cube|{tag}|dist")
        err = max(rel(comp, g[f"cube|{tag}|components"]), rel(maps, g[f"cube|{tag}|maps"]))
        print("ICAUnmixer", tag, "n_iter", u.n_iter_, "err", err, "tol", tol)
        assert comp.shape == (3, 20) and maps.shape == (6, 7, 3) and u.image_shape_ == (6, 7) and err <= tol, (err, tol)
        assert u.n_iter_ == int(g[f"cube|{tag}|n_iter"])
        assert u.components_ is comp and u.abundance_maps_ is maps
    with pytest.raises(ValueError, match="3D"):
        ICAUnmixer().fit(np.ones((4, 5)))


# ------------------------------------------------------------------------------------------------ 4. errors
def check_errors(device):
    from atomai_amd.stat import _gmm, _ica
    X = torch.from_numpy(mixture(40, 36, 3, 5)).to(device)
    with pytest.raises(ValueError, match="32"):
        _ica.fit_ica(X, 33)
    with pytest.raises(NotImplementedError, match="whiten=False"):
        _ica.fit_ica(X, 2, whiten=False)
    with pytest.raises(ValueError, match="whiten"):
        _ica.fit_ica(X, 2, whiten="unit")
    with pytest.raises(NotImplementedError, match="deflation"):
        _ica.fit_ica(X, 2, algorithm="deflation")
    with pytest.raises(NotImplementedError, match="callable"):
        _ica.fit_ica(X, 2, fun=lambda y: (y, np.ones(len(y))))
    with pytest.raises(ValueError, match="fun"):
        _ica.fit_ica(X, 2, fun="tanh")
    with pytest.raises(ValueError, match="alpha"):
        _ica.fit_ica(X, 2, fun_args={"alpha": 3.0})
    with pytest.raises(ValueError, match="w_init"):
        _ica.fit_ica(X, 2, w_init=np.eye(3))
    small = X[:9, :5].contiguous()
    with pytest.warns(UserWarning, match="n_components is too large"):
        res = _ica.fit_ica(small, 7, random_state=0, max_iter=3, tol=1.0)
    assert res["components"].shape == (5, 5) and res["sources"].shape == (9, 5)
    with pytest.warns(_gmm.ConvergenceWarning):
        res = _ica.fit_ica(X, 3, random_state=0, max_iter=1)
    assert res["n_iter"] == 1 and not res["converged"]
    flat = X.clone()
    flat[:, 1:] = flat[:, :1] * 1e-7 * torch.arange(1, 36, device=X.device, dtype=X.dtype)     # sigma_2 / sigma_1 ~ 0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _ica.fit_ica(flat + 1e-9 * X, 2, random_state=0, max_iter=2)
    assert any("sigma_1 / sigma_k" in str(w.message) for w in caught)


def check_module_paths():
    """The working code lives in atomai_amd.stat.ica; the reference's own entry points still raise and name it."""
    import _stat_checks as S
    import atomai_amd as aoi
    assert aoi.stat.ica.fit_ica is aoi.stat._ica.fit_ica
    s, _ = S.stat_of("r5c3")
    for fn in (s.ica, s.imblock_ica):
        with pytest.raises(NotImplementedError, match="atomai_amd.stat.ica"):
            fn(2)
    with pytest.raises(NotImplementedError, match="atomai_amd.stat.ica"):
        aoi.stat.unmixer.SpectralUnmixer("ica")
    u = aoi.stat.ica.ICAUnmixer()
    assert u.n_components == 4 and u.method == "ica" and u.components_ is None
