"""Nearest-neighbour queries on the device (csrc/knn.hip): thin wrappers over the C ABI.

``knn`` is the segmented brute-force k-nearest-neighbour search (one launch for any number of frames), ``radius`` the
fixed-radius query of one set (count, prefix sum, emit, then two stable sorts on the device), ``window_mean`` the mean
intensity in a small window around every atom of a flat table.  Inputs and outputs are device tensors; segment offsets
are HOST sequences (the callers know the table lengths), from which the (segment, first query) tile table is built.
"""
import math

import numpy as np
import torch

from .. import _lib as L

K_MAX = 32        # KNN_KMAX of csrc/knn.hip
DIMS = (2, 3)
TILE = 256        # KNN_T of csrc/knn.hip: queries per workgroup


def _points(t, name):
    if t.dtype != torch.float64 or t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous (N, dim) float64 tensor")
    return t


def _check_dim(dim):
    if dim not in DIMS:
        raise ValueError(f"the device neighbour search handles dim 2 or 3, got {dim}")


def check_k(k):
    if not 1 <= int(k) <= K_MAX:
        raise ValueError(f"the device kernel keeps at most {K_MAX} neighbours per query (the query itself included), "
                         f"got k = {k}")


def _offsets(seg, n, name):
    seg = np.array([0, n] if seg is None else seg, dtype=np.int64)
    if seg.ndim != 1 or len(seg) < 1 or seg[0] != 0 or seg[-1] != n or (np.diff(seg) < 0).any():
        raise ValueError(f"{name} must be non-decreasing offsets from 0 to {n}")
    return seg


def tile_table(qseg):
    """(T, 2) int64 host array of (segment, first query row): every segment's queries in tiles of ``TILE``."""
    qseg = np.asarray(qseg, dtype=np.int64)
    ntiles = -(-np.diff(qseg) // TILE)
    seg = np.repeat(np.arange(len(ntiles), dtype=np.int64), ntiles)
    within = np.arange(len(seg), dtype=np.int64) - np.repeat(np.cumsum(ntiles) - ntiles, ntiles)
    return np.stack((seg, qseg[seg] + TILE * within), axis=1)


def knn(pts, qry, k, bound=math.inf, pseg=None, qseg=None):
    """The ``k`` nearest rows of ``pts`` (P, dim) for every row of ``qry`` (Q, dim), within segments: a query in
    [qseg[s], qseg[s+1]) searches the points in [pseg[s], pseg[s+1]) only (no offsets: one segment).  Returns ``dist``
    (Q, k) float64 ascending and ``idx`` (Q, k) int64 rows of ``pts``; +inf / -1 where there is no neighbour with
    ``dist < bound``.  A query that is one of the points finds itself first."""
    pts, qry = _points(pts, "pts"), _points(qry, "qry")
    dim = qry.shape[1]
    _check_dim(dim)
    if pts.shape[1] != dim:
        raise ValueError(f"pts has {pts.shape[1]} columns, qry {dim}")
    check_k(k)
    P, Q = pts.shape[0], qry.shape[0]
    pseg, qseg = _offsets(pseg, P, "pseg"), _offsets(qseg, Q, "qseg")
    if len(pseg) != len(qseg):
        raise ValueError("pseg and qseg must describe the same number of segments")
    dev = qry.device
    dist = torch.full((Q, int(k)), math.inf, dtype=torch.float64, device=dev)
    idx = torch.full((Q, int(k)), -1, dtype=torch.int64, device=dev)
    tiles = tile_table(qseg)
    if len(tiles):
        t_dev, p_dev, q_dev = (torch.from_numpy(a).to(dev) for a in (tiles, pseg, qseg))
        L.call("amx_knn", L.ptr(pts), P, L.ptr(qry), Q, dim, L.ptr(p_dev), L.ptr(q_dev), len(qseg) - 1, L.ptr(t_dev),
               len(tiles), int(k), float(bound), L.ptr(dist), L.ptr(idx), L.stream_ptr(qry))
    return dist, idx


def radius(pts, qry, rmax):
    """All rows of ``pts`` (P, dim) with ``dist < rmax`` for every row of ``qry`` (Q, dim).  Returns ``count`` (Q,) int64
    and the flat ``idx`` (M,) int64 / ``dist`` (M,) float64, M = count.sum(): query i owns the slice that starts at
    ``count[:i].sum()``, ordered by distance (equal distances by row)."""
    pts, qry = _points(pts, "pts"), _points(qry, "qry")
    dim = qry.shape[1]
    _check_dim(dim)
    if pts.shape[1] != dim:
        raise ValueError(f"pts has {pts.shape[1]} columns, qry {dim}")
    P, Q = pts.shape[0], qry.shape[0]
    dev = qry.device
    sp = L.stream_ptr(qry)
    count = torch.zeros(Q, dtype=torch.int64, device=dev)
    L.call("amx_radius_count", L.ptr(pts), P, L.ptr(qry), Q, dim, float(rmax), L.ptr(count), sp)
    incl = torch.cumsum(count, 0)
    offs = (incl - count).contiguous()
    M = int(incl[-1].item()) if Q else 0
    qid = torch.empty(M, dtype=torch.int64, device=dev)
    idx = torch.empty(M, dtype=torch.int64, device=dev)
    dist = torch.empty(M, dtype=torch.float64, device=dev)
    L.call("amx_radius_emit", L.ptr(pts), P, L.ptr(qry), Q, dim, float(rmax), L.ptr(offs), M, L.ptr(qid), L.ptr(idx),
           L.ptr(dist), sp)
    # per-query order by distance: stable by distance, then stable by query (rows were emitted in row order, so equal
    # distances stay in row order)
    by_dist = torch.sort(dist, stable=True).indices
    perm = by_dist[torch.sort(qid[by_dist], stable=True).indices]
    return count, idx[perm], dist[perm]


def window_mean(frames, coords, meta, r):
    """float64 mean of the (B, H, W) float32 ``frames`` over the r x r window around every atom of the flat table
    ``coords`` (n, 2) float64 / ``meta`` (n, 2) int32 (frame, class), the layout of ``refine_device``."""
    if frames.dim() != 3 or frames.dtype != torch.float32:
        raise ValueError("expected (B, H, W) float32 frames")
    if int(r) != r or not 1 <= int(r) <= 1024:
        raise ValueError(f"the window side must be an integer 1 <= r <= 1024, got {r}")
    coords = _points(coords, "coords")
    if coords.shape[1] != 2 or meta.dtype != torch.int32 or tuple(meta.shape) != (len(coords), 2):
        raise ValueError("expected coords (n, 2) float64 and meta (n, 2) int32")
    frames, meta = frames.contiguous(), meta.contiguous()
    B, H, W = frames.shape
    out = torch.empty(len(coords), dtype=torch.float64, device=frames.device)
    if len(coords):
        L.call("amx_window_mean", L.ptr(frames), B, H, W, L.ptr(coords), L.ptr(meta), len(coords), int(r), L.ptr(out),
               L.stream_ptr(frames))
    return out
