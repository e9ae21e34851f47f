"""Density clustering on the device (csrc/cluster.hip): thin wrappers over the C ABI.

``dbscan`` is the segmented DBSCAN of a flat 2-column table (one pass for any number of frames, scikit-learn's labels),
``cluster_stats`` the per-cluster count, mean and population variance with the member rows in table order.  Inputs and
outputs are device tensors; segment offsets are HOST sequences, as in ``_knn``.  The sorts, prefix sums and gathers
between the kernels are torch calls on the same device; the only read-backs are one scalar per round of the
connected-components loop and the cluster counts that size the ragged output of ``cluster_stats``.
"""
import math

import numpy as np
import torch

from .. import _lib as L
from ._knn import _offsets

H_MARGIN = 2.0 ** -16     # cell edge >= eps * (1 + H_MARGIN): the derivation is in csrc/cluster.hip
N_MAX = 2 ** 31 - 1


def _check(pts, eps, min_samples, seg):
    if not isinstance(pts, torch.Tensor) or pts.dtype != torch.float64 or pts.dim() != 2 or pts.shape[1] != 2 \
            or not pts.is_contiguous():
        raise ValueError("pts must be a contiguous (N, 2) float64 tensor")
    if not (isinstance(eps, (int, float, np.integer, np.floating)) and 0.0 < float(eps) < math.inf):
        raise ValueError(f"eps must be a positive finite number, got {eps!r}")
    if int(min_samples) != min_samples or int(min_samples) < 1:
        raise ValueError(f"min_samples must be an integer >= 1, got {min_samples!r}")
    if len(pts) >= N_MAX:
        raise ValueError("the device clustering handles fewer than 2^31 rows")
    return _offsets(seg, len(pts), "seg")


def _run(pts, eps, min_samples, seg):
    """The kernels of cluster.hip in order.  Returns a dict of device tensors in ORIGINAL row order (labels int64, core
    bool, sid int32 = segment of every row, rank (N + 1,) int64 = clusters that start before a row) and the host
    integers rounds and cells (reserved), and gdim (S, 2) the grids."""
    seg = _check(pts, eps, min_samples, seg)
    eps, min_samples = float(eps), int(min_samples)
    N, S, dev = len(pts), len(seg) - 1, pts.device
    sizes = np.diff(seg)
    if N == 0:
        empty = lambda dt: torch.empty(0, dtype=dt, device=dev)                         # noqa: E731
        return {"labels": empty(torch.int64), "core": empty(torch.bool), "sid": empty(torch.int32),
                "rank": torch.zeros(1, dtype=torch.int64, device=dev), "seg": seg, "rounds": 0, "cells": 0,
                "gdim": torch.ones((S, 2), dtype=torch.int64, device=dev)}
    sp = L.stream_ptr(pts)
    # 3 n + 1 cells bound the grid of a segment of n rows (cluster.hip, "Cell count"): reserved from the host's sizes
    cbase = np.concatenate(([0], np.cumsum(np.where(sizes > 0, 3 * sizes + 1, 0)))).astype(np.int64)
    C = int(cbase[-1])
    seg_d, cbase_d = torch.from_numpy(seg).to(dev), torch.from_numpy(cbase).to(dev)
    grid = torch.empty((S, 3), dtype=torch.float64, device=dev)
    gdim = torch.empty((S, 2), dtype=torch.int64, device=dev)
    key = torch.empty(N, dtype=torch.int64, device=dev)
    sid = torch.empty(N, dtype=torch.int32, device=dev)
    L.call("amx_cluster_grid", L.ptr(pts), N, L.ptr(seg_d), S, L.ptr(cbase_d), eps * (1.0 + H_MARGIN), L.ptr(grid),
           L.ptr(gdim), sp)
    L.call("amx_cluster_keys", L.ptr(pts), N, L.ptr(seg_d), S, L.ptr(cbase_d), L.ptr(grid), L.ptr(gdim), L.ptr(key),
           L.ptr(sid), sp)
    # rows by cell: a stable sort, so the order inside a cell is the table's and nothing depends on a scatter order
    skey, orig = torch.sort(key, stable=True)
    spts, ssid = pts[orig].contiguous(), sid[orig].contiguous()
    cstart = torch.searchsorted(skey, torch.arange(C + 1, dtype=torch.int64, device=dev)).contiguous()
    eps2 = eps * eps
    core_s = torch.empty(N, dtype=torch.int32, device=dev)
    geom = (L.ptr(cbase_d), L.ptr(gdim), L.ptr(cstart), C, eps2)
    L.call("amx_cluster_core", L.ptr(spts), N, L.ptr(ssid), L.ptr(skey), S, *geom, min_samples, L.ptr(core_s), sp)
    # connected components: hook (snapshot pa -> copy pb), jump (pb to its roots, mirrored into pa), until nothing hooks
    pa = torch.arange(N, dtype=torch.int32, device=dev)
    pb = pa.clone()
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    rounds, cap = 0, int(sizes.max())
    while True:
        rounds += 1
        if rounds > cap:
            raise RuntimeError(f"connected components did not settle within {cap} rounds, the size of the largest "
                               f"segment")
        changed.zero_()
        L.call("amx_cluster_hook", L.ptr(spts), N, L.ptr(ssid), L.ptr(skey), S, *geom, L.ptr(core_s), L.ptr(orig),
               L.ptr(pa), L.ptr(pb), L.ptr(changed), sp)
        if not int(changed.item()):                  # the one scalar read back per round
            break
        L.call("amx_cluster_jump", L.ptr(pa), L.ptr(pb), N, sp)
    core = torch.empty(N, dtype=torch.bool, device=dev)
    core[orig] = core_s != 0
    root = core & (pa.long() == torch.arange(N, dtype=torch.int64, device=dev))
    rank = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(root.long(), 0))).contiguous()
    labels = torch.empty(N, dtype=torch.int64, device=dev)
    L.call("amx_cluster_label", L.ptr(spts), N, L.ptr(ssid), L.ptr(skey), L.ptr(seg_d), S, *geom, L.ptr(core_s),
           L.ptr(orig), L.ptr(pa), L.ptr(rank), L.ptr(labels), sp)
    return {"labels": labels, "core": core, "sid": sid, "rank": rank, "seg": seg, "rounds": rounds, "cells": C,
            "gdim": gdim}


def dbscan(pts, eps, min_samples, seg=None):
    """DBSCAN of the rows of ``pts`` (N, 2) float64 within segments (no offsets: one segment) with scikit-learn's
    numbering per segment: clusters 0, 1, ... by their smallest core row, a border row takes the smallest label among
    its core neighbours, noise is -1.  Returns ``labels`` (N,) int64, ``core`` (N,) bool and the number of rounds the
    connected-components loop took (the last one, which finds nothing to hook, included)."""
    r = _run(pts, eps, min_samples, seg)
    return r["labels"], r["core"], r["rounds"]


def grid_cells(pts, eps, seg=None):
    """(reserved, used): the cells the wrapper allocates for this table (3 n + 1 per non-empty segment of n rows) and
    the cells the grids of the non-empty segments have.  Neither depends on the extent of the points over ``eps``."""
    r = _run(pts, eps, 1, seg)
    if not len(pts):
        return 0, 0
    live = torch.from_numpy(np.diff(r["seg"]) > 0).to(pts.device)
    return r["cells"], int(r["gdim"].prod(1)[live].sum().item())


def cluster_stats(pts, labels, rank, seg):
    """Statistics of the clusters ``dbscan`` found.  ``rank`` and ``seg`` as ``_run`` returns them.  Returns
    ``kseg`` (S + 1,) host offsets of every segment's clusters in the flat cluster list, and the device tensors
    ``count`` (K,) int64, ``mean`` / ``var`` (K, 2) float64 (population variance), ``members`` (M,) int64 = rows of
    ``pts`` cluster by cluster, each in table order (the noise rows follow), and ``moff`` (K + 1,) int64 their
    offsets."""
    N, dev = len(pts), pts.device
    seg_d = torch.from_numpy(np.asarray(seg, dtype=np.int64)).to(dev)
    kseg_d = rank[seg_d]
    kseg = kseg_d.cpu().numpy()                     # one read-back: it sizes the ragged output
    K = int(kseg[-1])
    count = torch.empty(K, dtype=torch.int64, device=dev)
    mean = torch.empty((K, 2), dtype=torch.float64, device=dev)
    var = torch.empty((K, 2), dtype=torch.float64, device=dev)
    if K == 0:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return kseg, count, mean, var, z, torch.zeros(1, dtype=torch.int64, device=dev)
    # global cluster number of every row (noise: K, sorted to the end); a stable sort keeps table order inside a cluster
    first = kseg_d[torch.repeat_interleave(torch.arange(len(seg) - 1, device=dev), (seg_d[1:] - seg_d[:-1]))]
    g = torch.where(labels >= 0, first + labels, torch.full_like(labels, K))
    gs, rows = torch.sort(g, stable=True)
    moff = torch.searchsorted(gs, torch.arange(K + 1, dtype=torch.int64, device=dev)).contiguous()
    members = rows.contiguous()                     # all N rows: the noise rows lie at and beyond moff[K]
    L.call("amx_cluster_stats", L.ptr(pts), N, L.ptr(members), N, L.ptr(moff), K, L.ptr(count), L.ptr(mean), L.ptr(var),
           L.stream_ptr(pts))
    return kseg, count, mean, var, members, moff
