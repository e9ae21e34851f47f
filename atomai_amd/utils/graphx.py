"""Graph analysis of atom tables (reference: atomai/utils/graphx.py): bonds, rings, ring clusters (topological
defects) and the largest connected subgraph, on the kernels of csrc/graph.hip.

The reference builds one Python ``Node`` per atom, runs a recursive depth-first search from every atom and a second
one for every vertex pair of every cycle it found, and takes connected components from networkx.  Here a table (or a
dictionary of tables, every frame one segment of a single pass) goes through ``_graph.bonds`` (a CSR of the bonds),
``_graph.rings`` and ``_graph.components``.  A ring is a simple cycle of 3 to ``max(cycles)`` atoms on which no two
atoms are joined by a path of the whole graph shorter than the shorter way round: the set that the reference's
``polycount`` + ``remove_filled_polygons`` keep (tools/make_graph_golden.py asserts that on every golden case).

Limits: at most 16 bonds per atom, rings of at most 16 atoms, at most 16 classes in a call.  Covalent radii (pm) come
from the ``radii`` keyword, else from mendeleev if it is installed; no table is built in.  scipy, networkx and
mendeleev are not needed to compute; networkx only by ``Graph.nx_graph`` / ``Graph.rings_to_nx_graph``.
"""
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _graph
from .coords import _device


# ------------------------------------------------------------------------------------------------ radii and cutoffs
def _covalent_radii(elements: Sequence[str], radii: Optional[Dict[str, float]]) -> Dict[str, float]:
    elements = list(dict.fromkeys(elements))
    if radii is not None:
        missing = [e for e in elements if e not in radii]
        if missing:
            raise ValueError(f"no covalent radius for {missing} in the radii keyword (pm, e.g. radii={{'C': 75.0}})")
        return {e: float(radii[e]) for e in elements}
    try:
        from mendeleev import element
    except ImportError:
        raise ValueError(f"no covalent radius for {elements}: mendeleev is not installed and no table is built in; "
                         f"pass them in pm with the radii keyword, e.g. radii={{'C': 75.0}}") from None
    return {e: element(e).covalent_radius for e in elements}


def get_interatomic_r(atoms: Union[Tuple[str, str], List[str]], expand: Optional[float] = None,
                      radii: Optional[Dict[str, float]] = None) -> float:
    """Bond length of two elements in angstroms, ``(R_1 + R_2) / 100`` of their covalent radii in pm, times ``expand``
    if it is given.  ``radii`` maps element names to radii in pm; without it they are taken from mendeleev."""
    a1, a2 = atoms
    r = _covalent_radii([a1, a2], radii)
    r12 = (r[a1] + r[a2]) / 100
    if expand:
        r12 = expand * r12
    return r12


def _element(map_dict, c):
    try:
        return map_dict[c]
    except KeyError:
        raise ValueError(f"class {c!r} of the coordinate table is missing from map_dict {map_dict!r}") from None


# ------------------------------------------------------------------------------------------------ the shared pass
class _Pass:
    """Tables -> one flat segmented table on the device and its bond CSR.  ``scaled`` are the host tables with the
    coordinate columns multiplied by px2ang (the class column last), ``seg`` the host offsets."""

    def __init__(self, tables, map_dict, px2ang, expand, radii):
        px2ang = float(px2ang)
        if not (np.isfinite(px2ang) and px2ang > 0.0):
            raise ValueError(f"px2ang must be a positive finite number, got {px2ang!r}")
        self.px2ang, self.map_dict, self.scaled = px2ang, map_dict, []
        for t in tables:
            t = np.array(t, dtype=np.float64)
            if t.ndim != 2 or t.shape[1] not in (3, 4):
                raise ValueError(f"expected an (N, 3) table [x, y, class] or an (N, 4) table [x, y, z, class], got shape "
                                 f"{t.shape}")
            if not np.isfinite(t).all():
                raise ValueError("the coordinate table holds non-finite values")
            t[:, :-1] = t[:, :-1] * px2ang
            self.scaled.append(t)
        self.seg = np.concatenate(([0], np.cumsum([len(t) for t in self.scaled]))).astype(np.int64)
        self.N = N = int(self.seg[-1])
        dev = _device()
        if N == 0:
            self.rowptr = torch.zeros(1, dtype=torch.int64, device=dev)
            self.col = torch.empty(0, dtype=torch.int32, device=dev)
            return
        pts = np.zeros((N, 3), dtype=np.float64)
        klass = np.empty(N, dtype=np.float64)
        for t, lo, hi in zip(self.scaled, self.seg[:-1], self.seg[1:]):
            pts[lo:hi, :t.shape[1] - 1] = t[:, :-1]
            klass[lo:hi] = t[:, -1]
        uval, idx = np.unique(klass, return_inverse=True)
        if len(uval) > _graph.CLASS_MAX:
            raise ValueError(f"the table holds {len(uval)} classes; the device bond builder handles at most "
                             f"{_graph.CLASS_MAX}")
        names = [_element(map_dict, u) for u in uval]
        known = _covalent_radii(names, radii)
        cut = np.array([[get_interatomic_r([a, b], expand, known) for b in names] for a in names], dtype=np.float64)
        self.names = names
        self.rowptr, self.col = _graph.bonds(torch.from_numpy(pts).to(dev),
                                             torch.from_numpy(idx.reshape(-1).astype(np.int32)).to(dev),
                                             torch.from_numpy(cut * cut).to(dev), self.seg)

    def rings(self, size):
        """The rings of 3 to ``size`` atoms of all frames: ``ring`` (R, 16) int64 host array of FLAT rows (ascending,
        -1 behind them), ``length`` (R,) and the host offsets ``rseg`` of every frame's rings, each frame's ordered by
        (length, rows).  The device copies stay in ``self.ring`` / ``self.length`` for ``cluster_rows``."""
        self.ring, self.length, rseg = _graph.rings(self.rowptr, self.col, self.seg, size)
        return self.ring.cpu().numpy().astype(np.int64), self.length.cpu().numpy(), rseg

    def cluster_rows(self, cycles):
        """Rows (flat, ascending) that rings_to_nx_graph keeps for the ring sizes ``cycles``, and each one's component
        (its smallest row).  Needs ``rings`` first."""
        N, dev = self.N, self.rowptr.device
        sizes = torch.tensor(sorted(set(int(c) for c in cycles)), dtype=torch.int32, device=dev)
        ids = self.ring[torch.isin(self.length, sizes)]
        in_ring = torch.zeros(N, dtype=torch.bool, device=dev)
        in_ring[ids[ids >= 0].long()] = True
        src = torch.repeat_interleave(torch.arange(N, dtype=torch.int64, device=dev), self.rowptr[1:] - self.rowptr[:-1])
        dst = self.col.long()
        # a bond stays if its smaller-numbered end lies on a requested ring
        edge = in_ring[torch.minimum(src, dst)]
        keep = torch.bincount(src[edge], minlength=N) >= 2              # nodes of degree below 2 go, once
        edge = edge & keep[src] & keep[dst]
        rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(src[edge], minlength=N), 0, out=rowptr[1:])
        parent, _ = _graph.components(rowptr, self.col[edge].contiguous())
        rows = torch.nonzero(keep).reshape(-1)
        return rows.cpu().numpy(), parent[rows].cpu().numpy().astype(np.int64)


def _cycles(cycles) -> List[int]:
    cycles = [cycles] if np.isscalar(cycles) else list(cycles)
    if not cycles:
        raise ValueError("no ring size was requested")
    for c in cycles:
        _graph.check_ring_size(c)
    return [int(c) for c in cycles]


def _frames(coordinates):
    if isinstance(coordinates, dict):
        return list(coordinates.keys()), list(coordinates.values()), True
    return [0], [coordinates], False


# ------------------------------------------------------------------------------------------------ Graph
class Graph:
    """Bond graph of one atom table, array-backed.

    ``coordinates`` is an (N, 3) table [x, y, class] or an (N, 4) table [x, y, z, class] in angstroms; ``map_dict``
    maps the classes to element names.  ``find_neighbors`` fills the CSR ``rowptr`` / ``col`` and ``neighbors`` (one
    ascending int array per atom); ``polycount`` fills ``rings`` (ascending int arrays, ordered by length, then ids).
    The shortest-path filter is part of the search, so ``remove_filled_polygons`` has nothing left to do."""

    def __init__(self, coordinates: np.ndarray, map_dict: Dict) -> None:
        coordinates = np.asarray(coordinates, dtype=np.float64)
        if coordinates.ndim != 2 or coordinates.shape[1] not in (3, 4):
            raise ValueError(f"expected an (N, 3) or (N, 4) table, got shape {coordinates.shape}")
        if coordinates.shape[-1] == 3:
            coordinates = np.concatenate((coordinates[:, :2], np.zeros_like(coordinates)[:, 0:1], coordinates[:, 2:3]),
                                         axis=-1)
        self.coordinates = coordinates
        self.map_dict = map_dict
        self.size = len(coordinates)
        self.rings: List[np.ndarray] = []
        self.neighbors: List[np.ndarray] = []
        self.rowptr = self.col = None
        self._pass = None

    def find_neighbors(self, expand: float = 1.2, radii: Optional[Dict[str, float]] = None) -> None:
        self._pass = _Pass([self.coordinates], self.map_dict, 1.0, expand, radii)
        self.rowptr, self.col = self._pass.rowptr.cpu().numpy(), self._pass.col.cpu().numpy()
        self.neighbors = np.split(self.col.astype(np.int64), self.rowptr[1:-1]) if self.size else []
        self.rings = []

    def polycount(self, max_depth: int) -> None:
        _graph.check_ring_size(max_depth)
        if self._pass is None:
            raise RuntimeError("call find_neighbors before polycount")
        ring, length, _ = self._pass.rings(int(max_depth))
        self.rings = [r[:n] for r, n in zip(ring, length)]

    def remove_filled_polygons(self) -> None:
        """Kept for the reference's call sequence: ``polycount`` already returns shortest-path rings only."""

    def _atoms(self):
        return [_element(self.map_dict, c) for c in self.coordinates[:, -1]]

    def nx_graph(self):
        """The whole bond graph as a networkx graph (node attributes ``pos`` and ``atom``, as the reference's)."""
        try:
            import networkx as nx
        except ImportError:
            raise ImportError("Graph.nx_graph needs networkx") from None
        if self.rowptr is None:
            raise RuntimeError("call find_neighbors first")
        g = nx.Graph()
        flat = self.size > 0 and bool(np.all(self.coordinates[0, 2] == self.coordinates[:, 2]))
        for i, (atom, nb) in enumerate(zip(self._atoms(), self.neighbors)):
            g.add_node(i, pos=tuple(self.coordinates[i, :2 if flat else 3].tolist()), atom=atom)
            g.add_edges_from((i, int(j)) for j in nb)
        return g

    def rings_to_nx_graph(self, ring_size: Sequence[int]):
        """The reference's graph of the rings of the sizes ``ring_size``: their atoms, the bonds from each of them to
        its larger-numbered neighbours, minus (once) every node of degree below 2."""
        try:
            import networkx as nx
        except ImportError:
            raise ImportError("Graph.rings_to_nx_graph needs networkx") from None
        ring_size = [ring_size] if isinstance(ring_size, (int, np.integer)) else ring_size
        atoms = self._atoms()
        g = nx.Graph()
        add = lambda i: g.add_node(i, pos=tuple(self.coordinates[i, :3].tolist()), atom=atoms[i])     # noqa: E731
        for ring in self.rings:
            if len(ring) not in ring_size:
                continue
            for v in map(int, ring):
                add(v)
                for w in map(int, self.neighbors[v]):
                    if w > v:
                        add(w)
                        g.add_edge(v, w)
        g.remove_nodes_from([n for n, d in g.degree() if d < 2])
        return g


# ------------------------------------------------------------------------------------------------ rings
def _find_cycles(tables, cycles, map_dict, px2ang, kwargs):
    cycles = _cycles(cycles)
    p = _Pass(tables, map_dict, px2ang, kwargs.get("expand", 1.2), kwargs.get("radii"))
    out = [[] for _ in tables]
    if p.N:
        ring, length, rseg = p.rings(max(cycles))
        for f, (t, lo, a, b) in enumerate(zip(p.scaled, p.seg[:-1], rseg[:-1], rseg[1:])):
            ids = ring[a:b][np.isin(length[a:b], cycles)]
            if len(ids):
                rows = t[ids[ids >= 0] - lo]             # ring after ring, each one's atoms ascending
                rows[:, :-1] = rows[:, :-1] * (1 / p.px2ang)
                out[f] = rows
    return out


def find_cycles(coordinate_data: np.ndarray, cycles: Union[int, List[int]], map_dict: Dict[int, str], px2ang: float,
                **kwargs) -> np.ndarray:
    """Coordinates of the atoms of every ring with one of the sizes ``cycles``: the rows of ``coordinate_data`` at each
    ring's ascending atom numbers, ring after ring ordered by (size, atom numbers), class column kept, the
    coordinates multiplied by ``px2ang`` and by ``1 / px2ang`` as the reference does.  Keywords: ``expand`` (1.2) and
    ``radii``.  Raises ValueError when there is no such ring (the reference's np.concatenate of nothing)."""
    rows = _find_cycles([coordinate_data], cycles, map_dict, px2ang, kwargs)[0]
    if isinstance(rows, list):
        raise ValueError(f"no ring of size {cycles} was found: need at least one array to concatenate")
    return rows


def find_cycles_frames(coord_dict: Dict[int, np.ndarray], cycles: Union[int, List[int]], map_dict: Dict[int, str],
                       px2ang: float, **kwargs) -> Dict[int, np.ndarray]:
    """``find_cycles`` for every frame of the Locator's ``{frame: table}`` dictionary, all frames in one pass of each
    kernel.  A frame without a ring of the requested sizes gets an empty (0, columns) table."""
    keys, tables, _ = _frames(coord_dict)
    res = _find_cycles(tables, cycles, map_dict, px2ang, kwargs)
    return {k: (np.empty((0, np.shape(t)[1])) if isinstance(r, list) else r) for k, t, r in zip(keys, tables, res)}


def find_cycle_clusters(coordinate_data: Union[np.ndarray, Dict[int, np.ndarray]], cycles: Union[int, List[int]],
                        map_dict: Dict[int, str], px2ang: float, **kwargs):
    """Clusters of rings of the sizes ``cycles`` (topological defects): a list of coordinate arrays without the class
    column, one per cluster; for a ``{frame: table}`` dictionary, a dictionary of such lists from one pass.

    The clusters are the reference's: the atoms of the requested rings and the bonds from each of them to its
    larger-numbered neighbours, minus (once) every atom with fewer than two of these bonds, split into connected
    components.  Departure: the rows of a cluster ascend by atom number and the clusters by their smallest atom (the
    reference's order is networkx's insertion order)."""
    cycles = _cycles(cycles)
    keys, tables, many = _frames(coordinate_data)
    p = _Pass(tables, map_dict, px2ang, kwargs.get("expand", 1.2), kwargs.get("radii"))
    out = {k: [] for k in keys}
    if p.N:
        p.rings(max(cycles))
        rows, root = p.cluster_rows(cycles)
        order = np.argsort(root, kind="stable")
        rows, root = rows[order], root[order]
        frame = np.searchsorted(p.seg, root, side="right") - 1
        for part in np.split(np.arange(len(rows)), np.nonzero(np.diff(root))[0] + 1) if len(rows) else []:
            f = frame[part[0]]
            out[keys[f]].append(p.scaled[f][rows[part] - p.seg[f]][:, :-1] * (1 / p.px2ang))
    return out if many else out[keys[0]]


# ------------------------------------------------------------------------------------------------ subgraphs
def filter_subgraphs(coordinates: Union[Dict[int, np.ndarray], np.ndarray], map_dict: Dict[int, str], px2ang: float,
                     **kwargs) -> Dict[int, np.ndarray]:
    """Keeps, per frame, the atoms of the largest connected component of the bond graph (of equal ones, the one with
    the smallest atom number): rows [x, y, class] with x and y as ``(coord * px2ang) / px2ang`` and the class looked up
    through the inverted ``map_dict``, as the reference computes them.  All frames go through one pass.  Departure:
    the rows are in ascending atom order."""
    keys, tables, _ = _frames(coordinates)
    p = _Pass(tables, map_dict, px2ang, kwargs.get("expand", 1.2), kwargs.get("radii"))
    if any(len(t) == 0 for t in p.scaled):
        raise ValueError("attempt to take the largest subgraph of an empty table")
    parent = _graph.components(p.rowptr, p.col)[0].cpu().numpy().astype(np.int64)
    inverse = {v: k for k, v in map_dict.items()}
    out = {}
    for k, t, lo, hi in zip(keys, p.scaled, p.seg[:-1], p.seg[1:]):
        root = parent[lo:hi] - lo
        rows = np.nonzero(root == np.argmax(np.bincount(root)))[0]          # the first maximum: the smallest root
        cls = np.array([inverse[_element(map_dict, c)] for c in t[rows, -1]], dtype=np.float64)
        out[k] = np.stack((t[rows, 0] / p.px2ang, t[rows, 1] / p.px2ang, cls), axis=1)
    return out


def filter_subgraphs_(coordinate_arr: np.ndarray, map_dict: Dict[int, str], px2ang: float, **kwargs) -> np.ndarray:
    """``filter_subgraphs`` of a single table."""
    return filter_subgraphs({0: coordinate_arr}, map_dict, px2ang, **kwargs)[0]
