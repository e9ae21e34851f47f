"""Graph analysis of atom tables on the device (csrc/graph.hip): thin wrappers over the C ABI.

``bonds`` builds the bond graph of a flat segmented table as a CSR (count, prefix sum, emit), ``components`` labels the
connected components of a CSR (hooking and pointer jumping), ``rings`` lists its shortest-path rings (count, prefix
sum, emit, then torch sorts).  Inputs and outputs are device tensors; segment offsets are HOST sequences, as in
``_knn``.  Read-backs: one pair of scalars in ``bonds`` (the largest degree's row, the number of CSR entries), one
scalar per round of ``components``, one vector of S + 1 offsets in ``rings``.
"""
import numpy as np
import torch

from .. import _lib as L
from ._knn import _offsets, tile_table

DEG_MAX = 16      # bonds per atom
RING_MAX = 16     # RG_LMAX of csrc/graph.hip: rows per ring
CLASS_MAX = 16    # GR_CMAX of csrc/graph.hip
N_MAX = 2 ** 31 - 1


def check_ring_size(size):
    if int(size) != size or not 3 <= int(size) <= RING_MAX:
        raise ValueError(f"the device ring search handles rings of 3 to {RING_MAX} atoms, got {size!r}")


def _csr(rowptr, col):
    if not isinstance(rowptr, torch.Tensor) or rowptr.dtype != torch.int64 or rowptr.dim() != 1 or len(rowptr) < 1 \
            or not rowptr.is_contiguous():
        raise ValueError("rowptr must be a contiguous (N + 1,) int64 tensor")
    if not isinstance(col, torch.Tensor) or col.dtype != torch.int32 or col.dim() != 1 or not col.is_contiguous():
        raise ValueError("col must be a contiguous (M,) int32 tensor")
    if len(rowptr) - 1 >= N_MAX:
        raise ValueError("the device graph kernels handle fewer than 2^31 rows")
    return len(rowptr) - 1, len(col)


def bonds(pts, cls, cut2, seg=None):
    """The bond graph of the rows of ``pts`` (N, 3) float64 with classes ``cls`` (N,) int32 in [0, C) within segments
    (no offsets: one segment): rows i != j are bonded if ``dx*dx + dy*dy + dz*dz <= cut2[cls[i], cls[j]]`` in float64,
    ``cut2`` (C, C) float64.  Returns the CSR ``rowptr`` (N + 1,) int64 and ``col`` (M,) int32 (rows of the flat table,
    every row's neighbours ascending).  More than 16 bonds at one atom raise ValueError."""
    if not isinstance(pts, torch.Tensor) or pts.dtype != torch.float64 or pts.dim() != 2 or pts.shape[1] != 3 \
            or not pts.is_contiguous():
        raise ValueError("pts must be a contiguous (N, 3) float64 tensor")
    N, dev = len(pts), pts.device
    if N >= N_MAX:
        raise ValueError("the device graph kernels handle fewer than 2^31 rows")
    if not isinstance(cls, torch.Tensor) or cls.dtype != torch.int32 or tuple(cls.shape) != (N,) or not cls.is_contiguous():
        raise ValueError("cls must be a contiguous (N,) int32 tensor")
    if not isinstance(cut2, torch.Tensor) or cut2.dtype != torch.float64 or cut2.dim() != 2 \
            or cut2.shape[0] != cut2.shape[1] or not cut2.is_contiguous():
        raise ValueError("cut2 must be a contiguous (C, C) float64 tensor")
    C = cut2.shape[0]
    if not 1 <= C <= CLASS_MAX:
        raise ValueError(f"the device bond builder handles 1 to {CLASS_MAX} classes, got {C}")
    seg = _offsets(seg, N, "seg")
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if N == 0:
        return rowptr, torch.empty(0, dtype=torch.int32, device=dev)
    sp = L.stream_ptr(pts)
    tiles = tile_table(seg)
    S, T = len(seg) - 1, len(tiles)
    seg_d, tiles_d = torch.from_numpy(seg).to(dev), torch.from_numpy(tiles).to(dev)
    deg = torch.zeros(N, dtype=torch.int64, device=dev)
    L.call("amx_bond_count", L.ptr(pts), L.ptr(cls), N, L.ptr(cut2), C, L.ptr(seg_d), S, L.ptr(tiles_d), T, L.ptr(deg),
           sp)
    torch.cumsum(deg, 0, out=rowptr[1:])
    rows = torch.arange(N, dtype=torch.int64, device=dev)
    first_bad = torch.where(deg > DEG_MAX, rows, torch.full_like(rows, N)).min()
    bad, M = torch.stack((first_bad, rowptr[-1])).tolist()          # the one read-back
    if bad < N:
        frame = int(np.searchsorted(seg, bad, side="right")) - 1
        raise ValueError(f"atom {bad - int(seg[frame])} of frame {frame} (row {bad} of the flat table) has "
                         f"{int(deg[bad].item())} bonds; the graph kernels handle at most {DEG_MAX} per atom (are the "
                         f"coordinates in angstroms, and is px2ang right?)")
    col = torch.empty(M, dtype=torch.int32, device=dev)
    L.call("amx_bond_emit", L.ptr(pts), L.ptr(cls), N, L.ptr(cut2), C, L.ptr(seg_d), S, L.ptr(tiles_d), T, L.ptr(rowptr),
           M, L.ptr(col), sp)
    return rowptr, col


def components(rowptr, col):
    """Connected components of the CSR (every edge present from both ends): ``parent`` (N,) int32, the smallest row of
    every row's component, and the number of hooking rounds (the last one, which hooks nothing, included)."""
    N, M = _csr(rowptr, col)
    dev = rowptr.device
    pa = torch.arange(N, dtype=torch.int32, device=dev)
    if N == 0:
        return pa, 0
    sp = L.stream_ptr(rowptr)
    pb = pa.clone()
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    rounds = 0
    while True:
        rounds += 1
        if rounds > N + 1:
            raise RuntimeError(f"connected components did not settle within {N + 1} rounds")
        changed.zero_()
        L.call("amx_graph_hook", L.ptr(rowptr), L.ptr(col), N, M, L.ptr(pa), L.ptr(pb), L.ptr(changed), sp)
        if not int(changed.item()):                  # the one scalar read back per round
            break
        L.call("amx_cluster_jump", L.ptr(pa), L.ptr(pb), N, sp)
    return pa, rounds


def rings(rowptr, col, seg, size):
    """The rings of 3 to ``size`` rows of the CSR: simple cycles on which no two rows are joined by a path of the whole
    graph that is shorter than the shorter way round.  Returns ``ring`` (R, 16) int32, every ring's rows ascending and
    -1 behind them, ``length`` (R,) int32, and the host offsets ``rseg`` (S + 1,) int64 of every segment's rings; within
    a segment the rings are ordered by (length, rows lexicographic)."""
    N, M = _csr(rowptr, col)
    check_ring_size(size)
    seg = _offsets(seg, N, "seg")
    dev = rowptr.device
    S = len(seg) - 1
    if N == 0:
        return (torch.empty((0, RING_MAX), dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                np.zeros(S + 1, dtype=np.int64))
    sp = L.stream_ptr(rowptr)
    count = torch.zeros(N, dtype=torch.int64, device=dev)
    L.call("amx_ring_count", L.ptr(rowptr), L.ptr(col), N, M, int(size), L.ptr(count), sp)
    offs = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(count, 0, out=offs[1:])
    rseg = offs[torch.from_numpy(seg).to(dev)].cpu().numpy()        # the one read-back: it sizes the ragged output
    R = int(rseg[-1])
    ring = torch.full((R, RING_MAX), -1, dtype=torch.int32, device=dev)
    length = torch.zeros(R, dtype=torch.int32, device=dev)
    if R == 0:
        return ring, length, rseg
    L.call("amx_ring_emit", L.ptr(rowptr), L.ptr(col), N, M, int(size), L.ptr(offs), R, L.ptr(ring), L.ptr(length), sp)
    # (segment, length, rows): stable sorts from the last key to the first.  The rings were emitted root by root, so
    # they are already grouped by segment; the segment of a ring is that of its first row.
    order = torch.arange(R, dtype=torch.int64, device=dev)
    for c in range(int(size) - 1, -1, -1):
        order = order[torch.sort(ring[order, c], stable=True).indices]
    order = order[torch.sort(length[order], stable=True).indices]
    sid = torch.searchsorted(torch.from_numpy(rseg[1:]).to(dev), torch.arange(R, dtype=torch.int64, device=dev), right=True)
    order = order[torch.sort(sid[order], stable=True).indices]
    return ring[order].contiguous(), length[order].contiguous(), rseg
