"""FastICA on the device (csrc/ica.hip): thin wrappers over the C ABI and the driver that mirrors
``sklearn.decomposition.FastICA(algorithm='parallel').fit_transform``.

X stays on the device in the dtype it was given (float32 or float64); every product, sum and update is fp64, so a float32
stack gives what scikit-learn gives on ``X.astype(float64)``, NOT what its float32 arithmetic gives.  The whitening takes
the top singular triplets of the centred matrix from the fp64 Gram matrix of its smaller side plus ``torch.linalg.eigh``
(dense fp64 GEMMs go to the BLAS library); the Gram matrix is accumulated over chunks of the reduction axis (rows when
d <= n, columns otherwise) in a fixed order, each chunk centred and converted in a workspace of at most
``GRAM_CHUNK_BYTES`` (64 MiB): no second full-size copy of X exists at any time.  The Gram route squares the condition
number: the k-th singular value is lost at about 2^-52 (sigma_1 / sigma_k)^2 relative, and ``fit_ica`` warns (it does not
raise) where that exceeds 1e-9, i.e. beyond sigma_1 / sigma_k ~ 2000.

One iteration is two launches of csrc/ica.hip (step, reduce), the k x k symmetric decorrelation through
``torch.linalg.eigh`` on the device, and ONE scalar (``lim``) read back.
"""
import math
import warnings

import numpy as np
import torch

from .. import _lib as L
from ._gmm import ConvergenceWarning, _check_k
from ._nmf import _as_x

FUNS = {"logcosh": 0, "exp": 1, "cube": 2}
WHITEN = ("unit-variance", "arbitrary-variance")
GRAM_CHUNK_BYTES = 64 * 1024 * 1024          # fp64 workspace of one centred chunk of X
GRAM_LOSS_WARN = 1e-9                        # warn where 2^-52 (sigma_1 / sigma_k)^2 exceeds this


def blocks(n, k):
    """Workgroups of one step: a function of n only."""
    return int(L.load().amx_ica_blocks(int(n), int(k)))


def project(X, mean, M, scale=1.0):
    """(k, n) float64: ``scale * M (X - mean)^T`` with X (n, d) float32 / float64 read in place."""
    n, d = X.shape
    k = M.shape[0]
    out = torch.empty(k, n, dtype=torch.float64, device=X.device)
    L.call("amx_ica_project", L.ptr(X), int(X.dtype == torch.float64), n, d, L.ptr(mean), L.ptr(M), k, float(scale),
           L.ptr(out), L.stream_ptr(out))
    return out


class _Step:
    """Buffers of the fixed-point step on X1 (k, n): per-workgroup partials and the matrix the decorrelation reads."""

    def __init__(self, X1, fun, alpha):
        self.X1, self.fun, self.alpha = X1, int(fun), float(alpha)
        self.k, self.n = X1.shape
        self.G = blocks(self.n, self.k)
        f64 = dict(dtype=torch.float64, device=X1.device)
        self.Pg, self.Ph = torch.empty(self.G, self.k, self.k, **f64), torch.empty(self.G, self.k, **f64)
        self.A = torch.empty(self.k, self.k, **f64)

    def run(self, W):
        """A = g(W X1) X1^T / n - diag(mean g'(W X1)) W."""
        sp = L.stream_ptr(self.A)
        L.call("amx_ica_step", L.ptr(self.X1), self.n, self.k, self.fun, self.alpha, L.ptr(W), L.ptr(self.Pg),
               L.ptr(self.Ph), sp)
        L.call("amx_ica_reduce", L.ptr(self.Pg), L.ptr(self.Ph), self.G, self.k, self.n, L.ptr(W), L.ptr(self.A), sp)
        return self.A


def _check_fun(fun, fun_args):
    if callable(fun):
        raise NotImplementedError("a callable contrast function cannot run on the device: fun must be one of "
                                  f"{tuple(FUNS)}")
    if fun not in FUNS:
        raise ValueError(f"fun must be one of {tuple(FUNS)}, got {fun!r}")
    alpha = float((fun_args or {}).get("alpha", 1.0))
    if not 1 <= alpha <= 2:
        raise ValueError("alpha must be in [1,2]")
    return FUNS[fun], alpha


def ica_step(X1, W, fun="logcosh", alpha=1.0):
    """What the tests call: one step + reduce on copies.  X1 (k, n), W (k, k); returns A (k, k) float64."""
    code, alpha = _check_fun(fun, {"alpha": alpha})
    X1 = X1.to(torch.float64).contiguous()
    _check_k(X1.shape[0])
    W = W.to(X1.device, torch.float64).contiguous()
    return _Step(X1, code, alpha).run(W).clone()


def row_std(S):
    """numpy.std of every row of S (k, n), float64."""
    sd = torch.empty(S.shape[0], dtype=torch.float64, device=S.device)
    L.call("amx_ica_rowstd", L.ptr(S), S.shape[0], S.shape[1], L.ptr(sd), L.stream_ptr(sd))
    return sd


def sym_decorrelation(W):
    """(W W^T)^(-1/2) W through eigh of W W^T, eigenvalues clipped at the smallest normal number, as scikit-learn."""
    s, u = torch.linalg.eigh(W @ W.T)
    s = s.clamp(min=torch.finfo(torch.float64).tiny)
    return ((u * (1.0 / s.sqrt())) @ u.T @ W).contiguous()


def _centred_chunks(X, mean, axis):
    """The centred float64 chunks of X along ``axis``, in order, each at most GRAM_CHUNK_BYTES."""
    n, d = X.shape
    other = d if axis == 0 else n
    step = max(1, GRAM_CHUNK_BYTES // (8 * other))
    for a in range(0, X.shape[axis], step):
        if axis == 0:
            yield a, X[a:a + step].to(torch.float64) - mean
        else:
            yield a, X[:, a:a + step].to(torch.float64) - mean[a:a + step]


def _whitening(X, k):
    """mean (d,), the whitening matrix K (k, d), u (d, k) and sigma (k,) of the centred X, scikit-learn's sign rule."""
    n, d = X.shape
    mean = X.sum(0, dtype=torch.float64) / n
    axis = 0 if d <= n else 1
    m = min(n, d)
    gram = torch.zeros(m, m, dtype=torch.float64, device=X.device)
    for _, C in _centred_chunks(X, mean, axis):
        gram += C.T @ C if axis == 0 else C @ C.T
    lam, vec = torch.linalg.eigh((gram + gram.T) * 0.5)
    lam, vec = lam.flip(0)[:k], vec.flip(1)[:, :k].contiguous()
    top, last = float(lam[0]), float(lam[-1])
    loss = 2.0 ** -52 * (top / last) if last > 0 else math.inf          # (lam = sigma^2)
    if loss > GRAM_LOSS_WARN:
        ratio = math.sqrt(top / last) if last > 0 else math.inf
        warnings.warn(f"fit_ica whitens through the Gram matrix, which loses the smallest kept singular value at about "
                      f"2^-52 (sigma_1 / sigma_k)^2 = {loss:.1e} relative (sigma_1 / sigma_k = {ratio:.3g}): the "
                      "components are less accurate than scikit-learn's SVD route; ask for fewer components")
    sigma = lam.clamp(min=torch.finfo(torch.float64).tiny).sqrt()
    if axis == 0:
        u = vec
    else:
        u = torch.empty(d, k, dtype=torch.float64, device=X.device)
        for a, C in _centred_chunks(X, mean, 1):
            u[a:a + C.shape[1]] = C.T @ vec / sigma
    u = u * torch.sign(u[0])
    return mean, (u / sigma).T.contiguous(), u, sigma


def _w_init(k, random_state, w_init):
    if w_init is not None:
        w_init = np.asarray(w_init, dtype=np.float64)
        if w_init.shape != (k, k):
            raise ValueError(f"w_init has invalid shape -- should be {(k, k)}")
        return w_init
    if random_state is None:
        rng = np.random.mtrand._rand                  # numpy's global state, as scikit-learn's check_random_state(None)
    elif isinstance(random_state, np.random.RandomState):
        rng = random_state
    else:
        rng = np.random.RandomState(random_state)
    return rng.normal(size=(k, k))


def fit_ica(X, n_components, fun="logcosh", fun_args=None, whiten="unit-variance", max_iter=200, tol=1e-4,
            random_state=None, w_init=None, algorithm="parallel"):
    """Independent components of the (n, d) matrix ``X`` (tensor or array, float32 or float64, kept as given) as
    ``sklearn.decomposition.FastICA(n_components, algorithm='parallel', whiten=whiten, fun=fun, fun_args=fun_args,
    max_iter=max_iter, tol=tol, w_init=w_init, random_state=random_state).fit_transform`` computes them, with at most 32
    components.  Returns a dict of float64 device tensors ``components`` (k, d), ``sources`` (n, k), ``mixing`` (d, k),
    ``mean`` (d,) and ``whitening`` (k, d), plus ``n_iter`` and ``converged``.

    ``fun``: 'logcosh' (``fun_args={'alpha': a}``, 1 <= a <= 2), 'exp' or 'cube'.  ``random_state=None`` draws the
    initial matrix from numpy's global state.  The arithmetic is fp64 on the values of X whatever its dtype.  The whitening
    goes through the Gram matrix of the smaller side (chunk workspace: ``GRAM_CHUNK_BYTES`` = 64 MiB); a warning is
    given where 2^-52 (sigma_1 / sigma_k)^2 exceeds 1e-9.  ``mixing`` is the pseudo-inverse of ``components`` formed as
    u diag(sigma) W^-1 from the whitening's factors."""
    if algorithm != "parallel":
        raise NotImplementedError(f"algorithm={algorithm!r} is not implemented: only the parallel (symmetric) FastICA "
                                  "runs on the device ('deflation' extracts one component at a time)")
    if whiten not in WHITEN:
        if whiten is False:
            raise NotImplementedError("whiten=False is not implemented: the device solver whitens the data itself "
                                      f"(whiten must be one of {WHITEN})")
        raise ValueError(f"whiten must be one of {WHITEN}, got {whiten!r}")
    code, alpha = _check_fun(fun, fun_args)
    if max_iter < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter}")
    X = _as_x(X)
    n, d = X.shape
    if n < 2:
        raise ValueError(f"fit_ica needs at least 2 samples, got {n}")
    k = int(n_components)
    if k > min(n, d):
        k = min(n, d)
        warnings.warn(f"n_components is too large: it will be set to {k}")
    _check_k(k)
    mean, K, u, sigma = _whitening(X, k)
    W = sym_decorrelation(torch.from_numpy(_w_init(k, random_state, w_init)).to(X.device))
    step = _Step(project(X, mean, K, math.sqrt(n)), code, alpha)
    converged, n_iter = False, 0
    for n_iter in range(1, max_iter + 1):
        W1 = sym_decorrelation(step.run(W))
        lim = float(((W1 * W).sum(1).abs() - 1.0).abs().max())           # the one read-back of the iteration
        W = W1
        if lim < tol:
            converged = True
            break
    if not converged:
        warnings.warn("FastICA did not converge. Consider increasing tolerance or the maximum number of iterations.",
                      ConvergenceWarning)
    St = project(X, mean, (W @ K).contiguous(), 1.0)                      # (k, n)
    if whiten == "unit-variance":
        sd = row_std(St)
        St = St / sd[:, None]
        W = W / sd[:, None]
    return {"components": (W @ K).contiguous(), "sources": St.T.contiguous(),
            "mixing": ((u * sigma) @ torch.linalg.inv(W)).contiguous(), "mean": mean, "whitening": K,
            "n_iter": n_iter, "converged": converged}
