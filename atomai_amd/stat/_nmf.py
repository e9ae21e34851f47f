"""Non-negative matrix factorisation on the device (csrc/nmf.hip, csrc/fftwin.hip): thin wrappers over the C ABI and the
driver that mirrors ``sklearn.decomposition.NMF(solver='cd').fit_transform``.

X stays on the device in the dtype it was given (float32 or float64); every product, sum and update is fp64.  The driver
reads back ONE pair of numbers per iteration (the two half-steps' violations).  Initial factors: ``'random'`` draws from
``numpy.random.RandomState(random_state)`` on the host exactly as scikit-learn does; ``'nndsvd'`` / ``'nndsvda'`` apply
scikit-learn's rule to the exact top singular triplets (scikit-learn takes them from a randomised SVD; NNDSVD does not
depend on the sign convention).
"""
import math
import warnings

import numpy as np
import torch

from .. import _lib as L
from ._gmm import ConvergenceWarning, _check_k

INITS = (None, "random", "nndsvd", "nndsvda")
FFT_WINDOW_MAX = 128


def _device():
    return torch.device("cpu") if L.is_test_backend() and not torch.cuda.is_available() else torch.device("cuda")


def _as_x(X):
    """A contiguous (n, d) float32 / float64 tensor on the device, from a tensor or an array (other dtypes -> float64)."""
    if not isinstance(X, torch.Tensor):
        X = np.asarray(X)
        if X.dtype not in (np.float32, np.float64):
            X = X.astype(np.float64)
        X = torch.from_numpy(np.ascontiguousarray(X))
    elif X.dtype not in (torch.float32, torch.float64):
        X = X.to(torch.float64)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"X must be a non-empty (n_samples, n_features) matrix, got {tuple(X.shape)}")
    return X.to(_device()).contiguous()


def splits(n, d, k, trans):
    return int(L.load().amx_nmf_splits(int(n), int(d), int(k), int(trans)))


class _Half:
    """Buffers of one half-step: the factor T (R, k) it updates, its partial products and per-workgroup partials."""

    def __init__(self, X, k, trans, T):
        n, d = X.shape
        f64 = dict(dtype=torch.float64, device=X.device)
        self.X, self.k, self.trans, self.T = X, k, int(trans), T
        self.R = d if trans else n
        self.S = splits(n, d, k, trans)
        self.G = -(-self.R // int(L.load().amx_nmf_rows()))
        self.P = torch.empty(self.S, self.R, k, **f64)
        self.Pv, self.Pg = torch.empty(self.G, **f64), torch.empty(self.G, k, k, **f64)
        self.gram = torch.empty(k, k, **f64)                      # T^T T, what the OTHER half-step reads

    def gram_only(self):
        sp = L.stream_ptr(self.T)
        L.call("amx_nmf_cd", None, 0, self.R, self.k, None, L.ptr(self.T), 1, L.ptr(self.Pv), L.ptr(self.Pg), sp)
        L.call("amx_nmf_reduce", L.ptr(self.Pv), L.ptr(self.Pg), self.G, self.k, None, L.ptr(self.gram), sp)

    def step(self, F, FF, viol):
        """T <- one sweep with F (L, k) fixed and FF = F^T F; ``viol``: the 0-d slot that receives the violation."""
        n, d = self.X.shape
        sp = L.stream_ptr(self.T)
        L.call("amx_nmf_xf", L.ptr(self.X), int(self.X.dtype == torch.float64), n, d, self.trans, L.ptr(F), self.k,
               L.ptr(self.P), sp)
        L.call("amx_nmf_cd", L.ptr(self.P), self.S, self.R, self.k, L.ptr(FF), L.ptr(self.T), 0, L.ptr(self.Pv),
               L.ptr(self.Pg), sp)
        L.call("amx_nmf_reduce", L.ptr(self.Pv), L.ptr(self.Pg), self.G, self.k, L.ptr(viol), L.ptr(self.gram), sp)


# ------------------------------------------------------------------------------------------------ what the tests call
def nmf_half_step(X, T, F, trans):
    """One half-step on copies: X (n, d), T the factor to update ((n, k), or (d, k) with ``trans``), F the fixed one.
    Returns the new T, the violation (0-d tensor), the Gram matrix of the new T and that of F (all float64)."""
    X = _as_x(X)
    k = T.shape[1]
    _check_k(k)
    R, Lr = (X.shape[1], X.shape[0]) if trans else X.shape
    if tuple(T.shape) != (R, k) or tuple(F.shape) != (Lr, k):
        raise ValueError(f"T must be {(R, k)} and F {(Lr, k)}, got {tuple(T.shape)} and {tuple(F.shape)}")
    T = T.to(X.device, torch.float64).contiguous().clone()
    F = F.to(X.device, torch.float64).contiguous().clone()
    fixed = _Half(X, k, not trans, F)
    fixed.gram_only()
    half = _Half(X, k, trans, T)
    viol = torch.zeros(2, dtype=torch.float64, device=X.device)
    half.step(F, fixed.gram, viol[0])
    return T, viol[0], half.gram, fixed.gram


def _x_mean(X):
    return X.sum(dtype=torch.float64) / X.numel()


def _nndsvd(X, k, fill):
    """scikit-learn's NNDSVD on the exact top-k singular triplets, from the fp64 Gram matrix of the smaller side.
    ``fill``: what replaces the zeros (None: 'nndsvd', the mean of X: 'nndsvda')."""
    n, d = X.shape
    X64 = X.to(torch.float64)
    small = X64.T @ X64 if d <= n else X64 @ X64.T
    lam, vec = torch.linalg.eigh((small + small.T) * 0.5)
    lam, vec = lam.flip(0)[:k].clamp_(min=0.0), vec.flip(1)[:, :k]
    S = lam.sqrt()
    other = (X64 @ vec if d <= n else X64.T @ vec) / S.clamp(min=torch.finfo(torch.float64).tiny)
    U, V = (other, vec) if d <= n else (vec, other)            # (n, k), (d, k)
    W, Ht = torch.zeros_like(U), torch.zeros_like(V)
    W[:, 0], Ht[:, 0] = S[0].sqrt() * U[:, 0].abs(), S[0].sqrt() * V[:, 0].abs()
    for j in range(1, k):
        x, y = U[:, j], V[:, j]
        xp, yp, xn, yn = x.clamp(min=0), y.clamp(min=0), x.clamp(max=0).abs(), y.clamp(max=0).abs()
        mp, mn = torch.linalg.norm(xp) * torch.linalg.norm(yp), torch.linalg.norm(xn) * torch.linalg.norm(yn)
        if float(mp) > float(mn):
            u, v, sigma = xp / torch.linalg.norm(xp), yp / torch.linalg.norm(yp), mp
        else:
            u, v, sigma = xn / torch.linalg.norm(xn), yn / torch.linalg.norm(yn), mn
        lbd = (S[j] * sigma).sqrt()
        W[:, j], Ht[:, j] = lbd * u, lbd * v
    for M in (W, Ht):
        M[M < 1e-6] = 0.0                                       # (scikit-learn's eps)
        if fill is not None:
            M[M == 0] = fill
    return W.contiguous(), Ht.contiguous()


def _initial(X, k, init, random_state):
    n, d = X.shape
    if init not in INITS:
        raise ValueError(f"init must be one of {INITS}, got {init!r}")
    if init in ("nndsvd", "nndsvda") and k > min(n, d):
        raise ValueError(f"init = '{init}' can only be used when n_components <= min(n_samples, n_features)")
    if init is None:
        init = "nndsvda" if k <= min(n, d) else "random"
    mean = _x_mean(X)
    if init == "random":
        avg = math.sqrt(float(mean) / k)
        rng = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
        H = np.abs(avg * rng.standard_normal(size=(k, d)))      # H first, then W: scikit-learn's order of the draws
        W = np.abs(avg * rng.standard_normal(size=(n, k)))
        return (torch.from_numpy(W).to(X.device).contiguous(),
                torch.from_numpy(np.ascontiguousarray(H.T)).to(X.device).contiguous())
    return _nndsvd(X, k, mean if init == "nndsvda" else None)


def fit_nmf(X, n_components, init=None, random_state=None, tol=1e-4, max_iter=200):
    """Factorises the non-negative (n, d) matrix ``X`` (tensor or array, float32 or float64) as W H with
    ``n_components`` <= 32 components, as ``sklearn.decomposition.NMF(solver='cd', init=init, random_state=...,
    tol=tol, max_iter=max_iter).fit_transform`` does.  Returns a dict with ``W`` (n, k) and ``H`` (k, d) float64 device
    tensors, ``n_iter`` and ``converged``.  ``init``: None ('nndsvda' if k <= min(n, d), else 'random'), 'nndsvda',
    'nndsvd' or 'random'."""
    X = _as_x(X)
    k = int(n_components)
    _check_k(k)
    if max_iter < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter}")
    if not bool((torch.isfinite(X).all() & (X >= 0).all()).item()):
        raise ValueError("NMF needs finite, non-negative data: X has negative, NaN or infinite entries")
    W, Ht = _initial(X, k, init, random_state)
    hw, hh = _Half(X, k, 0, W), _Half(X, k, 1, Ht)
    viol = torch.zeros(2, dtype=torch.float64, device=X.device)
    hh.gram_only()                                               # the first H H^T
    first, converged, n_iter = None, False, 0
    for n_iter in range(1, max_iter + 1):
        hw.step(Ht, hh.gram, viol[0])
        hh.step(W, hw.gram, viol[1])
        v = viol.cpu()
        violation = float(v[0]) + float(v[1])
        if n_iter == 1:
            first = violation
        if first == 0 or violation / first <= tol:
            converged = True
            break
    if not converged and tol > 0:
        warnings.warn(f"fit_nmf reached max_iter={max_iter} before the projected gradient fell below tol={tol}: raise "
                      "max_iter or tol", ConvergenceWarning)
    return {"W": W, "H": Ht.T.contiguous(), "n_iter": n_iter, "converged": converged}


# ------------------------------------------------------------------------------------------------ sliding-window FFT
def crop_limits(wx, wy, zoom_factor):
    """The reference's centre crop of the shifted spectrum (it uses window_size_x for both axes' zoom_size)."""
    zoom_size = max(1, int(wx // (2 * zoom_factor)))
    cx, cy = wx // 2, wy // 2
    return max(0, cx - zoom_size), min(wx, cx + zoom_size), max(0, cy - zoom_size), min(wy, cy + zoom_size)


def zoom_table(n_in, factor):
    """scipy.ndimage.zoom(order=1, mode='constant') along one axis: (i0, i1, w0, w1) per output sample; a source
    coordinate beyond the last input sample gives (-1, -1, 0, 0), scipy's zero."""
    if factor <= 1:
        idx = np.arange(n_in, dtype=np.int32)
        return idx, idx.copy(), np.ones(n_in), np.zeros(n_in)
    n_out = int(round(n_in * factor))
    ratio = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    src = np.arange(n_out, dtype=np.float64) * ratio
    i0 = np.floor(src)
    t = src - i0
    i1 = np.minimum(i0 + 1, n_in - 1)
    outside = src > n_in - 1
    i0[outside], i1[outside], t[outside] = -1, -1, 0.0
    w0 = np.where(outside, 0.0, 1.0 - t)
    return i0.astype(np.int32), i1.astype(np.int32), w0, t


def _twiddles(N, dev):
    m = np.arange(N, dtype=np.float64)
    a = 2.0 * np.pi * m / N
    return torch.from_numpy(np.cos(a)).to(dev), torch.from_numpy(np.sin(a)).to(dev)


def fft_features(data, window, grid=None, steps=None, hamming=None, zoom_factor=2, interpolation_factor=2):
    """The feature matrix of SlidingFFTNMF.process_fft, on the device.  ``data``: the (H, W) float64 image together with
    ``grid`` = (windows down, windows across) and ``steps``, read in place, or an (n, wx, wy) stack (``grid`` None).
    ``hamming``: the (wx, wy) table or None.  Returns (features (n, fx * fy) float64 device tensor, (fx, fy)); raises
    ValueError for windows above 128 pixels and for an all-zero or non-finite result."""
    wx, wy = int(window[0]), int(window[1])
    if wx > FFT_WINDOW_MAX or wy > FFT_WINDOW_MAX:
        raise ValueError(f"windows above {FFT_WINDOW_MAX} x {FFT_WINDOW_MAX} pixels are not supported on the device, "
                         f"got {wx} x {wy}")
    dev = _device()
    if not isinstance(data, torch.Tensor):
        data = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float64))
    data = data.to(dev, torch.float64).contiguous()
    if grid is None:
        if data.dim() != 3 or tuple(data.shape[1:]) != (wx, wy):
            raise ValueError(f"a window stack must be (n, {wx}, {wy}), got {tuple(data.shape)}")
        nw0, nw1, strides, step = data.shape[0], 1, (wy, 1), (wx, 0)
    else:
        if data.dim() != 2:
            raise ValueError(f"an image read in place must be 2D, got {tuple(data.shape)}")
        nw0, nw1, strides, step = int(grid[0]), int(grid[1]), (data.shape[1], 1), (int(steps[0]), int(steps[1]))
        if (nw0 - 1) * step[0] + wx > data.shape[0] or (nw1 - 1) * step[1] + wy > data.shape[1]:
            raise ValueError("the window grid leaves the image")
    x0, x1, y0, y1 = crop_limits(wx, wy, zoom_factor)
    zx, zy = zoom_table(x1 - x0, interpolation_factor), zoom_table(y1 - y0, interpolation_factor)
    nox, noy = len(zx[0]), len(zy[0])
    up = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in zx + zy]
    cx, sx = _twiddles(wx, dev)
    cy, sy = _twiddles(wy, dev)
    ham = None if hamming is None else torch.from_numpy(np.ascontiguousarray(hamming, dtype=np.float64)).to(dev)
    if ham is not None and tuple(ham.shape) != (wx, wy):
        raise ValueError(f"the Hamming table must be ({wx}, {wy}), got {tuple(ham.shape)}")
    n = nw0 * nw1
    out = torch.empty(n, nox * noy, dtype=torch.float64, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    L.call("amx_fftwin", L.ptr(data), data.numel(), 0, strides[0], strides[1], step[0], step[1], nw0, nw1, wx, wy,
           L.ptr(ham), L.ptr(cx), L.ptr(sx), L.ptr(cy), L.ptr(sy), x0, x1 - x0, y0, y1 - y0, L.ptr(up[0]), L.ptr(up[1]),
           L.ptr(up[2]), L.ptr(up[3]), nox, L.ptr(up[4]), L.ptr(up[5]), L.ptr(up[6]), L.ptr(up[7]), noy, L.ptr(out),
           L.ptr(flags), L.stream_ptr(out))
    seen = int(((flags & 1).max() | (flags & 2).max()).item())    # one read-back: the OR of the windows' flag words
    if not seen & 1 or seen & 2:
        raise ValueError("Invalid data for NMF: contains zeros, NaNs or Infs")
    return out, (nox, noy)
