"""One-dimensional clustering of atom intensities on the device (csrc/intensity.hip): thin wrappers over the C ABI.

The column is float64 on the device; the kernels that search it take it SORTED ascending (``torch.sort`` is the caller's
job), ``assign`` takes it as it is.  Nothing here reads a value back."""
import numpy as np
import torch

from .. import _lib as L


def device():
    return torch.device("cpu") if L.is_test_backend() and not torch.cuda.is_available() else torch.device("cuda")


def column(x):
    """``x`` (array or tensor of any shape, float32 / float64 / integer) as a contiguous 1-D float64 device tensor."""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float64))
    x = x.reshape(-1).to(torch.float64)
    if not x.is_cuda:
        x = x.to(device())
    return x.contiguous()


def kth_gap(xs, K):
    """(gap (n,), mean ()): the distance of every row of the sorted column to its K-th nearest value, and their mean."""
    n = xs.shape[0]
    gap = torch.empty(n, dtype=torch.float64, device=xs.device)
    partial = torch.empty(int(L.load().amx_kth_gap_blocks(n)), dtype=torch.float64, device=xs.device)
    mean = torch.empty((), dtype=torch.float64, device=xs.device)
    L.call("amx_kth_gap_1d", L.ptr(xs), n, int(K), L.ptr(gap), L.ptr(partial), L.ptr(mean), L.stream_ptr(xs))
    return gap, mean


def meanshift(xs, seeds, bw, max_iter):
    """(centre (S,) float64, count (S,) int64, iters (S,) int64) of every seed, one workgroup each."""
    S = seeds.shape[0]
    centre = torch.empty(S, dtype=torch.float64, device=xs.device)
    count = torch.empty(S, dtype=torch.int64, device=xs.device)
    iters = torch.empty(S, dtype=torch.int64, device=xs.device)
    L.call("amx_meanshift_1d", L.ptr(xs), xs.shape[0], L.ptr(seeds), S, float(bw), int(max_iter), L.ptr(centre),
           L.ptr(count), L.ptr(iters), L.stream_ptr(xs))
    return centre, count, iters


def lloyd(xs, centres, tol, max_iter):
    """(centres (k,) float64 in the order given, n_iter () int64) of the Lloyd fit from ``centres``."""
    k = centres.shape[0]
    out = torch.empty(k, dtype=torch.float64, device=xs.device)
    n_iter = torch.empty((), dtype=torch.int64, device=xs.device)
    L.call("amx_lloyd_1d", L.ptr(xs), xs.shape[0], L.ptr(centres), k, float(tol), int(max_iter), L.ptr(out),
           L.ptr(n_iter), L.stream_ptr(xs))
    return out, n_iter


def assign(x, centres):
    """(n,) int64: index of the nearest centre of every row of the unsorted column, the first of equally near ones."""
    label = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    L.call("amx_assign_1d", L.ptr(x), x.shape[0], L.ptr(centres), centres.shape[0], L.ptr(label), L.stream_ptr(x))
    return label
