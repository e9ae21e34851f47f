"""Gaussian-mixture EM on the device (csrc/stat.hip): thin wrappers over the C ABI and the driver that mirrors
``sklearn.mixture.GaussianMixture(init_params='kmeans').fit_predict`` for 'diag' and 'spherical' covariances.

Everything stays on the device; the driver reads back ONE scalar per iteration (the changed-label count of a Lloyd
iteration, the lower bound of an EM iteration).  Random numbers are drawn on the host from
``numpy.random.default_rng(random_state)``: the component numbering therefore is NOT sklearn's.
"""
import math
import warnings

import numpy as np
import torch

from .. import _lib as L

K_MAX = 32
COVARIANCES = ("diag", "spherical")


class ConvergenceWarning(UserWarning):
    """The EM loop reached ``max_iter`` before the lower bound settled (sklearn.exceptions.ConvergenceWarning's role)."""


def _check_k(K):
    if not 1 <= int(K) <= K_MAX:
        raise ValueError(f"n_components must be between 1 and {K_MAX} (the limit of the device kernel), got {K}")


def _as_x(X):
    if X.dtype != torch.float32 or X.dim() != 2 or not X.is_contiguous():
        raise ValueError("X must be a contiguous (N, D) float32 tensor")
    if X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"X must have at least one row and one column, got {tuple(X.shape)}")
    return X


class _Work:
    """Partial rows of one pass and their fp64 sums, allocated once per (N, D, K)."""

    def __init__(self, X, K, sums=True):
        N, D = X.shape
        dev = X.device
        self.N, self.D, self.K = N, D, K
        self.G = -(-N // int(L.load().amx_gmm_rows()))
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        self.P1 = torch.empty(self.G, K, D, **f32) if sums else None
        self.P2 = torch.empty(self.G, K, D, **f32) if sums else None
        self.Pn = torch.empty(self.G, K, **f64)
        self.Pl = torch.empty(self.G, **f64)
        self.Pc = torch.empty(self.G, dtype=torch.int32, device=dev)
        self.S1 = torch.empty(K, D, **f64) if sums else None
        self.S2 = torch.empty(K, D, **f64) if sums else None
        self.nk = torch.empty(K, **f64)
        self.lse = torch.empty((), **f64)
        self.changed = torch.empty((), dtype=torch.int64, device=dev)


pass_timings = None      # benchmarks: set to a list and every pass on a GPU appends (kind, K, start event, end event)


def _launch_pass(X, w, mean32, prec32, cst, shift, hard=False, prev=None, label=None, logp=None, sums=True):
    sp = L.stream_ptr(X)
    timed = pass_timings is not None and X.is_cuda
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    L.call("amx_gmm_pass", L.ptr(X), w.N, w.D, w.K, L.ptr(mean32), L.ptr(prec32), L.ptr(cst), L.ptr(shift), int(hard),
           L.ptr(prev), L.ptr(w.P1 if sums else None), L.ptr(w.P2 if sums else None), L.ptr(w.Pn), L.ptr(w.Pl),
           L.ptr(w.Pc), L.ptr(logp), L.ptr(label), sp)
    if timed:
        e1.record()
        pass_timings.append(("lloyd" if hard else "em" if sums else "labels", w.K, e0, e1))
    L.call("amx_gmm_reduce", L.ptr(w.P1 if sums else None), L.ptr(w.P2 if sums else None), L.ptr(w.Pn), L.ptr(w.Pl),
           L.ptr(w.Pc), w.G, w.K, w.D, L.ptr(w.S1 if sums else None), L.ptr(w.S2 if sums else None), L.ptr(w.nk),
           L.ptr(w.lse), L.ptr(w.changed), sp)


class _Params:
    def __init__(self, K, D, dev):
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        self.mean, self.var, self.prec = (torch.empty(K, D, **f64) for _ in range(3))
        self.mean32, self.prec32 = torch.empty(K, D, **f32), torch.empty(K, D, **f32)
        self.weights, self.cst = torch.empty(K, **f64), torch.empty(K, **f64)


def _launch_finalize(w, shift, N, covariance, reg_covar, out):
    L.call("amx_gmm_finalize", L.ptr(w.nk), L.ptr(w.S1), L.ptr(w.S2), L.ptr(shift), w.K, w.D, float(N), float(reg_covar),
           int(covariance == "spherical"), L.ptr(out.mean), L.ptr(out.var), L.ptr(out.prec), L.ptr(out.mean32),
           L.ptr(out.prec32), L.ptr(out.weights), L.ptr(out.cst), L.stream_ptr(w.nk))


# ------------------------------------------------------------------------------------------------ what the tests call
def gmm_pass(X, mean, prec, logw, shift, hard=False, want_logp=False):
    """One E step plus the sums of the M step.  ``mean``, ``prec`` (K, D) float32, ``logw`` (K,) log weights, ``shift``
    (D,) float32.  Returns ``label`` (N,) int32, ``lb`` = mean of the rows' log-sum-exp (0-d float64 tensor), ``nk``
    (K,), ``S1`` = r^T (X - shift), ``S2`` = r^T (X - shift)^2 (K, D) float64, ``logp`` (N, K) float64 or None."""
    X = _as_x(X)
    K, D = mean.shape
    _check_k(K)
    mean = mean.to(torch.float32).contiguous()
    prec = prec.to(torch.float32).contiguous()
    shift = shift.to(torch.float32).contiguous()
    cst = (logw.to(torch.float64) + 0.5 * torch.log(prec.to(torch.float64)).sum(1)
           - 0.5 * D * math.log(2.0 * math.pi)).contiguous()
    w = _Work(X, K)
    label = torch.empty(X.shape[0], dtype=torch.int32, device=X.device)
    logp = torch.empty(X.shape[0], K, dtype=torch.float64, device=X.device) if want_logp else None
    _launch_pass(X, w, mean, prec, cst, shift, hard=hard, label=label, logp=logp)
    return {"label": label, "lb": w.lse / X.shape[0], "nk": w.nk, "S1": w.S1, "S2": w.S2, "logp": logp}


def gmm_update(nk, S1, S2, shift, N, covariance, reg_covar=1e-6):
    """The M step from the sums of ``gmm_pass``: returns ``mean, var, prec, weights`` (float64)."""
    if covariance not in COVARIANCES:
        raise NotImplementedError(f"covariance '{covariance}' is not on the device; choose from {COVARIANCES}")
    K, D = S1.shape
    _check_k(K)
    w = _Work.__new__(_Work)
    w.K, w.D = K, D
    w.nk, w.S1, w.S2 = (t.to(torch.float64).contiguous() for t in (nk, S1, S2))
    out = _Params(K, D, S1.device)
    _launch_finalize(w, shift.to(torch.float32).contiguous(), N, covariance, reg_covar, out)
    return out.mean, out.var, out.prec, out.weights


def column_mean(X):
    """Column mean of X as a K = 1 pass (every responsibility is 1): (D,) float64."""
    X = _as_x(X)
    D = X.shape[1]
    w = _Work(X, 1)
    zero = torch.zeros(1, D, dtype=torch.float32, device=X.device)
    _launch_pass(X, w, zero, zero, torch.zeros(1, dtype=torch.float64, device=X.device), zero.view(D))
    return w.S1.view(D) / X.shape[0]


def _sq_distances(X, centres):
    """(N, C) float64 squared distances to the rows of ``centres``: -2 logp of unit precisions and zero constants."""
    C, D = centres.shape
    w = _Work(X, C, sums=False)
    logp = torch.empty(X.shape[0], C, dtype=torch.float64, device=X.device)
    _launch_pass(X, w, centres, torch.ones_like(centres), torch.zeros(C, dtype=torch.float64, device=X.device), None,
                 logp=logp, sums=False)
    return logp.mul_(-2.0)


def _seed(X, K, rng):
    """Greedy k-means++ (sklearn.cluster._kmeans._kmeans_plusplus): 2 + floor(ln K) candidates per centre, the random
    numbers from the host generator, everything else on the device without a read-back."""
    N = X.shape[0]
    n_local = 2 + int(math.log(K))
    first = torch.tensor([int(rng.integers(N))], device=X.device)
    centres = [X.index_select(0, first)]
    closest = _sq_distances(X, centres[0]).view(N)
    for _ in range(1, K):
        u = torch.from_numpy(rng.uniform(size=n_local)).to(X.device)
        cum = torch.cumsum(closest, 0)
        ids = torch.searchsorted(cum, u * cum[-1]).clamp_(max=N - 1)
        cand = X.index_select(0, ids)
        d2 = torch.minimum(_sq_distances(X, cand), closest[:, None])
        best = torch.argmin(d2.sum(0)).view(1)
        closest = d2.index_select(1, best).view(N).contiguous()
        centres.append(cand.index_select(0, best))
    return torch.cat(centres, 0).contiguous()


def fit_gmm(X, n_components, covariance="diag", random_state=1, tol=1e-3, max_iter=100, reg_covar=1e-6):
    """Fits the mixture to the (N, D) float32 device tensor ``X`` and returns a dict with ``labels`` (N,) int64,
    ``means``, ``variances`` (K, D) and ``weights`` (K,) float64, ``lower_bound`` (float), ``n_iter``, ``converged``.

    Two departures from sklearn, besides the random stream.  A cluster that a Lloyd iteration leaves EMPTY is not moved
    to the point farthest from its centre, as sklearn's KMeans does: its sums are zero, so its next centre is the
    column mean of the data, from where it either picks up points or stays empty (its component then has weight
    10 eps / N and the labels use fewer than K classes).  The weights are n_k / N with n_k + 10 eps, and are not
    renormalised to sum to one as current sklearn does: they sum to 1 + 10 K eps / N."""
    X = _as_x(X)
    K = int(n_components)
    _check_k(K)
    if covariance not in COVARIANCES:
        raise NotImplementedError(f"covariance '{covariance}' is not on the device; choose from {COVARIANCES}")
    N, D = X.shape
    if N < K:
        raise ValueError(f"n_components={K} needs at least as many samples, got {N}")
    dev = X.device
    rng = np.random.default_rng(random_state)
    shift = column_mean(X).to(torch.float32).contiguous()
    w, par = _Work(X, K), _Params(K, D, dev)
    # ---- k-means: greedy k-means++ seeds, then Lloyd iterations through the same kernel with one-hot responsibilities
    centres = _seed(X, K, rng)
    ones = torch.ones(K, D, dtype=torch.float32, device=dev)
    zeros = torch.zeros(K, dtype=torch.float64, device=dev)
    labels = [torch.full((N,), -1, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)]
    for it in range(300):
        _launch_pass(X, w, centres, ones, zeros, shift, hard=True, prev=labels[it % 2], label=labels[(it + 1) % 2])
        _launch_finalize(w, shift, N, covariance, reg_covar, par)      # = the M step from the hard labels when they stand
        if int(w.changed.item()) == 0:
            break
        centres = par.mean32
    # ---- EM
    lower, prev, converged, n_iter = -math.inf, -math.inf, False, 0
    for n_iter in range(1, max_iter + 1):
        _launch_pass(X, w, par.mean32, par.prec32, par.cst, shift)
        _launch_finalize(w, shift, N, covariance, reg_covar, par)
        lower = float(w.lse.item()) / N
        if abs(lower - prev) < tol:
            converged = True
            break
        prev = lower
    if not converged:
        warnings.warn(f"fit_gmm did not converge in {max_iter} iterations (tol={tol}): try a different random_state, "
                      "or raise max_iter or tol", ConvergenceWarning)
    label = torch.empty(N, dtype=torch.int32, device=dev)
    _launch_pass(X, w, par.mean32, par.prec32, par.cst, None, label=label, sums=False)
    return {"labels": label.to(torch.int64), "means": par.mean, "variances": par.var, "weights": par.weights,
            "lower_bound": lower, "n_iter": n_iter, "converged": converged}
