"""Shared bodies of the graph-analysis tests (emulator tier on CPU, gpu tier on the MI355X): csrc/graph.hip through
atomai_amd.utils._graph and atomai_amd.utils.graphx against a plain numpy / pure-Python restatement of the rules and
against tests/golden/graph.npz, which tools/make_graph_golden.py records from the reference's graphx.py (and where it
asserts that the restatement below reproduces the reference on every case).  Neither the reference nor scipy, networkx
or mendeleev is imported here.

The restatement is the DEFINITION, not a search like the kernel's or the reference's:
  bonds       i != j and dx*dx + dy*dy + dz*dz <= cut2[ci][cj] in float64, cut = expand * ((R_a + R_b) / 100);
  rings       simple cycles of 3 .. L atoms on which every pair's distance in the whole graph (all-pairs breadth-first
              search) equals its distance round the cycle, each once;
  clusters    atoms of the requested rings + their bonds to larger-numbered neighbours, minus (once) the nodes of
              degree below 2, connected components;
  subgraph    the largest connected component, of equal ones the one with the smallest atom.
Everything is compared exactly: integers as integers, coordinates bit for bit."""
import math
import os
import sys

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RADII = {"C": 75.0, "Si": 116.0}          # pm; the table the golden was recorded with (asserted in gold())
_gold = None
_memo = {}


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLD, "graph.npz")) as g:
            _gold = {k: g[k] for k in g.files}
        assert dict(zip(_gold["radii|names"].tolist(), _gold["radii|values"].tolist())) == RADII
    return _gold


def cases():
    return [str(n) for n in gold()["names"]]


def case(name):
    """table (px), map_dict, px2ang, expand, L, cycles of a golden case."""
    g = gold()
    map_dict = {int(k): str(v) for k, v in zip(g[f"{name}|classes"], g[f"{name}|elements"])}
    return (g[f"{name}|table"], map_dict, float(g[f"{name}|px2ang"]), float(g[f"{name}|expand"]), int(g[f"{name}|L"]),
            [int(c) for c in g[f"{name}|cycles"]])


# ------------------------------------------------------------------------------------------------ the restatement
def scale(table, px2ang):
    t = np.array(table, dtype=np.float64)
    t[:, :-1] = t[:, :-1] * px2ang
    return t


def points(scaled):
    """(n, 3) positions (z = 0 for a 3-column table) and the class column."""
    p = np.zeros((len(scaled), 3))
    p[:, :scaled.shape[1] - 1] = scaled[:, :-1]
    return p, scaled[:, -1]


def cut2_table(names, expand, radii=RADII):
    cut = np.array([[expand * ((radii[a] + radii[b]) / 100) for b in names] for a in names], dtype=np.float64)
    return cut * cut


def bonds_rule(scaled, map_dict, expand, radii=RADII):
    """Neighbour lists (ascending int64 arrays) of the scaled table."""
    p, klass = points(scaled)
    if not len(p):
        return []
    uval, idx = np.unique(klass, return_inverse=True)
    idx = idx.reshape(-1)
    cut2 = cut2_table([map_dict[int(u)] for u in uval], expand, radii)
    d = p[None, :, :] - p[:, None, :]
    q = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    adj = q <= cut2[idx[:, None], idx[None, :]]
    np.fill_diagonal(adj, False)
    return [np.nonzero(row)[0].astype(np.int64) for row in adj]


def csr(adj):
    rowptr = np.concatenate(([0], np.cumsum([len(a) for a in adj]))).astype(np.int64)
    col = np.concatenate(adj).astype(np.int32) if len(adj) and rowptr[-1] else np.zeros(0, dtype=np.int32)
    return rowptr, col


def distances(adj):
    """All-pairs graph distances by breadth-first search (n where there is no path)."""
    n = len(adj)
    dist = np.full((n, n), n, dtype=np.int64)
    for s in range(n):
        dist[s, s] = 0
        front, d = [s], 0
        while front:
            d += 1
            nxt = []
            for v in front:
                for w in adj[v]:
                    if dist[s, w] == n:
                        dist[s, w] = d
                        nxt.append(int(w))
            front = nxt
    return dist


def rings_rule(adj, L):
    """Sorted list (by length, then rows) of the rings of 3 .. L atoms as ascending tuples.  Cycles are enumerated from
    their smallest atom in one direction; a prefix is dropped only where the definition already fails for it (the atom
    at position p of a ring of l <= L atoms lies min(p, l - p) bonds from the first)."""
    dist = distances(adj)
    found = []

    def walk(path):
        root, v, p = path[0], path[-1], len(path)
        for w in adj[v]:
            w = int(w)
            if w == root and p >= 3 and path[1] < v:
                if all(dist[path[j], path[k]] == min(k - j, p - (k - j)) for j in range(p) for k in range(j + 1, p)):
                    found.append(tuple(sorted(path)))
            elif w > root and p < L and w not in path and (dist[root, w] == p or dist[root, w] <= L - p):
                walk(path + [w])

    for r in range(len(adj)):
        walk([r])
    assert len(set(found)) == len(found)
    return sorted(found, key=lambda t: (len(t), t))


def components_rule(adj, nodes=None):
    """Smallest atom of every atom's component ({atom: root}), over ``nodes`` (all) and the bonds among them."""
    nodes = set(range(len(adj))) if nodes is None else set(nodes)
    root = {}
    for s in sorted(nodes):
        if s in root:
            continue
        root[s] = s
        stack = [s]
        while stack:
            for w in adj[stack.pop()]:
                w = int(w)
                if w in nodes and w not in root:
                    root[w] = s
                    stack.append(w)
    return root


def clusters_rule(adj, rings, cycles):
    """Sorted list of sorted atom lists: what the reference's rings_to_nx_graph + connected components keep."""
    on_ring = sorted({v for r in rings if len(r) in cycles for v in r})
    edges = {(v, int(w)) for v in on_ring for w in adj[v] if w > v}
    degree = {}
    for a, b in edges:
        degree[a] = degree.get(a, 0) + 1
        degree[b] = degree.get(b, 0) + 1
    keep = {v for v, d in degree.items() if d >= 2}
    sub = [[w for w in adj[v] if (min(v, int(w)), max(v, int(w))) in edges] for v in range(len(adj))]
    root = components_rule(sub, keep)
    out = {}
    for v in sorted(keep):
        out.setdefault(root[v], []).append(v)
    return [out[r] for r in sorted(out)]


def subgraph_rule(adj):
    root = components_rule(adj)
    roots = np.array([root[v] for v in range(len(adj))])
    return np.nonzero(roots == np.argmax(np.bincount(roots)))[0]


def honeycomb(nx, ny, a=1.42):
    """Atoms of nx x ny cells of a honeycomb lattice with bond length ``a`` (angstroms), in raster order."""
    pts = []
    for i in range(nx):
        for j in range(ny):
            ox, oy = 3.0 * a * i, math.sqrt(3.0) * a * j
            for dx, dy in ((0.0, 0.0), (a, 0.0), (1.5 * a, 0.5 * math.sqrt(3.0) * a), (2.5 * a, 0.5 * math.sqrt(3.0) * a)):
                pts.append((ox + dx, oy + dy))
    pts = np.array(pts)
    return pts[np.lexsort((pts[:, 0], pts[:, 1]))]


def memo(key, fn):
    """A reference result computed once and shared among the tests (never modified)."""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def case_rule(name):
    def build():
        table, map_dict, px2ang, expand, L, cycles = case(name)
        adj = bonds_rule(scale(table, px2ang), map_dict, expand)
        rings = rings_rule(adj, L)
        return adj, rings
    return memo(("case", name), build)


def as_tuples(ring_list):
    return [tuple(int(v) for v in r) for r in ring_list]


def gold_rings(name):
    r = gold()[f"{name}|rings"].astype(np.int64)
    return [tuple(int(v) for v in row[row >= 0]) for row in r]


def split(flat, offs):
    return [flat[a:b] for a, b in zip(offs[:-1], offs[1:])]


# ------------------------------------------------------------------------------------------------ 1. golden cases
def check_case(name, device):
    """Bonds, rings and components equal the restatement and the golden exactly; find_cycles equals the golden bit for
    bit; find_cycle_clusters and filter_subgraphs equal it after the stated row and cluster sorting."""
    import atomai_amd as aoi
    from atomai_amd.utils import _graph
    g = gold()
    table, map_dict, px2ang, expand, L, cycles = case(name)
    adj, rings = case_rule(name)
    rowptr, col = csr(adj)
    assert np.array_equal(rowptr, g[f"{name}|rowptr"]) and np.array_equal(col, g[f"{name}|col"])
    assert rings == gold_rings(name)
    # the Graph class
    G = aoi.utils.Graph(scale(table, px2ang), map_dict)
    G.find_neighbors(expand=expand, radii=RADII)
    assert G.rowptr.dtype == np.int64 and G.col.dtype == np.int32 and G.size == len(table)
    assert np.array_equal(G.rowptr, rowptr) and np.array_equal(G.col, col)
    assert len(G.neighbors) == len(adj) and all(np.array_equal(a, b) for a, b in zip(G.neighbors, adj))
    G.polycount(L)
    G.remove_filled_polygons()
    print(f"{name}: {len(table)} atoms, {len(col) // 2} bonds, max degree {int(np.diff(rowptr).max())}, L = {L}: "
          f"{len(rings)} rings of sizes {sorted({len(r) for r in rings})}")
    assert as_tuples(G.rings) == rings
    # components of the whole graph
    rp, cl = torch.from_numpy(rowptr).to(device), torch.from_numpy(col).to(device)
    parent, rounds = _graph.components(rp, cl)
    root = components_rule(adj)
    assert parent.dtype == torch.int32 and parent.cpu().tolist() == [root[v] for v in range(len(adj))]
    # find_cycles
    kw = {"expand": expand, "radii": RADII}
    want = g[f"{name}|find_cycles"]
    got = aoi.utils.find_cycles(table, cycles, map_dict, px2ang, **kw)
    assert got.dtype == np.float64 and got.shape == want.shape and got.tobytes() == want.tobytes()
    sel = [r for r in rings if len(r) in cycles]
    assert np.array_equal(got[:, -1], np.concatenate([table[list(r), -1] for r in sel]))
    # find_cycle_clusters: rows ascending inside a cluster, clusters by their smallest atom
    ids = clusters_rule(adj, rings, cycles)
    assert ids == [c.tolist() for c in split(g[f"{name}|cluster_ids"], g[f"{name}|cluster_off"])]
    want = split(g[f"{name}|cluster_rows"], g[f"{name}|cluster_off"])
    got = aoi.utils.find_cycle_clusters(table, cycles, map_dict, px2ang, **kw)
    assert isinstance(got, list) and len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == np.float64 and a.shape == b.shape and a.tobytes() == b.tobytes()
    # filter_subgraphs: rows in ascending atom order
    rows = subgraph_rule(adj)
    assert np.array_equal(rows, g[f"{name}|filtered_ids"])
    want = g[f"{name}|filtered"]
    for got in (aoi.utils.filter_subgraphs_(table, map_dict, px2ang, **kw),
                aoi.utils.filter_subgraphs(table, map_dict, px2ang, **kw)[0]):
        assert got.dtype == np.float64 and got.shape == want.shape and got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ 2. tiny tables
def tiny_tables():
    a = 1.42
    hexagon = [(a * math.cos(math.pi / 3 * k), a * math.sin(math.pi / 3 * k)) for k in range(6)]
    rad = 0.5 * a / math.sin(math.pi / 16)
    circle = [(rad * math.cos(math.pi / 8 * k), rad * math.sin(math.pi / 8 * k)) for k in range(16)]
    flat = lambda xy: np.array([(x, y, 0.0) for x, y in xy]).reshape(-1, 3)                    # noqa: E731
    cube = np.array([(a * i, a * j, a * k, 0.0) for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    return {
        "none": (np.empty((0, 3)), 6), "one": (flat([(0.5, 0.25)]), 6), "two": (flat([(0.0, 0.0), (a, 0.0)]), 6),
        "triangle": (flat([(0.0, 0.0), (a, 0.0), (0.5 * a, 0.8 * a)]), 6),
        # a square of side 1.7: its diagonal (2.40) is no bond; of side 1.2: both diagonals (1.70) are
        "square": (flat([(0.0, 0.0), (1.7, 0.0), (1.7, 1.7), (0.0, 1.7)]), 6),
        # a rhombus with ONE short diagonal: the chorded 4-cycle must go and two 3-rings stay
        "rhombus": (flat([(0.0, 0.0), (1.5, 0.0), (0.75, 1.3), (2.25, 1.3)]), 6),
        "hexagon": (flat(hexagon), 6),
        "fused": (flat(naphthalene(a)), 10),
        "cube": (cube, 4),
        # 16 atoms on a circle: the longest ring the kernel handles, and its deepest shortest-path test (7 bonds)
        "ring16": (flat(circle), 16), "ring16_L15": (flat(circle), 15),
    }


def naphthalene(a):
    """Two fused hexagons, 10 atoms: its 10-atom perimeter is a cycle but no ring (the shared bond is a chord)."""
    s = math.sqrt(3.0) * a
    left = [(a * math.cos(math.pi / 3 * k + math.pi / 6), a * math.sin(math.pi / 3 * k + math.pi / 6)) for k in range(6)]
    right = [(x + s, y) for x, y in left]
    every = []
    for p in left + right:
        if not any(math.hypot(p[0] - q[0], p[1] - q[1]) < 1e-6 for q in every):
            every.append(p)
    assert len(every) == 10
    return every


def check_tiny(device):
    import atomai_amd as aoi
    map_dict = {0: "C"}
    expect = {"none": [], "one": [], "two": [], "triangle": [3], "square": [4], "rhombus": [3, 3], "hexagon": [6],
              "fused": [6, 6], "cube": [4] * 6, "ring16": [16], "ring16_L15": []}
    for name, (table, L) in tiny_tables().items():
        adj = bonds_rule(table, map_dict, 1.2)
        rings = rings_rule(adj, L)
        assert [len(r) for r in rings] == expect[name], (name, rings)
        G = aoi.utils.Graph(table, map_dict)
        assert G.coordinates.shape == (len(table), 4) and G.size == len(table)
        G.find_neighbors(expand=1.2, radii=RADII)
        G.polycount(L)
        G.remove_filled_polygons()
        rowptr, col = csr(adj)
        assert np.array_equal(G.rowptr, rowptr) and np.array_equal(G.col, col), name
        assert as_tuples(G.rings) == rings, (name, G.rings)
        if rings:
            got = aoi.utils.find_cycles(table, sorted({len(r) for r in rings} | {L}), map_dict, 1.0, radii=RADII)
            assert got.tobytes() == np.concatenate([table[list(r)] for r in rings]).tobytes(), name
        if len(table):
            got = aoi.utils.filter_subgraphs_(table, map_dict, 1.0, radii=RADII)
            assert got.tobytes() == table[subgraph_rule(adj)][:, [0, 1, -1]].tobytes(), name
    assert len(bonds_rule(tiny_tables()["rhombus"][0], map_dict, 1.2)[1]) == 3          # the chord is there
    assert sorted(len(a) for a in bonds_rule(tiny_tables()["fused"][0], map_dict, 1.2)) == [2] * 8 + [3] * 2


def check_dense(device):
    """17 atoms on one spot, 16 bonds each, are a complete graph: 16!/2 simple cycles of 17 rows pass through every
    atom, and every cycle of more than three has a chord, so the rings are the 680 triangles, at any L.  The search
    must come back at once at L = 16 (it drops a path at its first chord)."""
    import itertools
    import atomai_amd as aoi
    pile = np.tile([[1.0, 2.0, 0.0]], (17, 1))
    want = sorted(itertools.combinations(range(17), 3))
    assert rings_rule(bonds_rule(pile, {0: "C"}, 1.2), 4) == want
    for L in (3, 4, 16):
        G = aoi.utils.Graph(pile, {0: "C"})
        G.find_neighbors(radii=RADII)
        assert [len(a) for a in G.neighbors] == [16] * 17
        G.polycount(L)
        assert as_tuples(G.rings) == want, L
    got = aoi.utils.find_cycle_clusters(pile, [3, 16], {0: "C"}, 1.0, radii=RADII)
    assert len(got) == 1 and got[0].tobytes() == pile[:, :2].tobytes()


# ------------------------------------------------------------------------------------------------ 3. frames
def frames_tables():
    """Three frames of 255, 256 and 257 atoms, one row either side of the 256-row tile: the SAME jittered honeycomb cut
    after that many atoms (rows at identical positions in different frames), with three atoms of a second class."""
    def build():
        rng = np.random.default_rng(31)
        xy = honeycomb(6, 12)
        assert len(xy) >= 255
        xy = xy[:255] + rng.uniform(-0.08, 0.08, (255, 2))
        for at in (200, 100):                             # an atom on the middle of a bond: 3-rings
            other = np.argsort(((xy - xy[at]) ** 2).sum(1))[1]
            xy = np.insert(xy, at, 0.5 * (xy[at] + xy[other]), axis=0)
        cls = np.zeros(257)
        cls[[40, 130, 254]] = 1.0
        table = np.concatenate((xy / 0.104, cls[:, None]), axis=1)
        return {7: table[:255].copy(), 3: table[:256].copy(), 5: table.copy()}
    return memo("frames", build)


def check_frames(device):
    """Frames do not link, and every frame's results equal its single-frame run and the restatement."""
    import atomai_amd as aoi
    frames = frames_tables()
    map_dict, px2ang, kw = {0: "C", 1: "Si"}, 0.104, {"expand": 1.2, "radii": RADII}
    cycles = [3, 4, 5, 7, 8]
    every = aoi.utils.find_cycles_frames(frames, cycles, map_dict, px2ang, **kw)
    clusters = aoi.utils.find_cycle_clusters(frames, cycles, map_dict, px2ang, **kw)
    filtered = aoi.utils.filter_subgraphs(frames, map_dict, px2ang, **kw)
    assert list(every) == list(clusters) == list(filtered) == [7, 3, 5]
    for k, table in frames.items():
        def build(table=table):
            adj = bonds_rule(scale(table, px2ang), map_dict, 1.2)
            return adj, rings_rule(adj, 8)
        adj, rings = memo(("frames", k), build)
        sel = [r for r in rings if len(r) in cycles]
        assert len(sel) >= 2 and max(len(a) for a in adj) <= 6
        one = aoi.utils.find_cycles(table, cycles, map_dict, px2ang, **kw)
        assert every[k].tobytes() == one.tobytes() and len(one) == sum(len(r) for r in sel)
        assert np.array_equal(one[:, -1], np.concatenate([table[list(r), -1] for r in sel]))
        one = aoi.utils.find_cycle_clusters(table, cycles, map_dict, px2ang, **kw)
        ids = clusters_rule(adj, rings, cycles)
        assert len(ids) >= 1 and [len(c) for c in clusters[k]] == [len(c) for c in one] == [len(c) for c in ids]
        for a, b, c in zip(clusters[k], one, ids):
            assert a.tobytes() == b.tobytes() == (scale(table, px2ang)[c][:, :-1] * (1 / px2ang)).tobytes()
        one = aoi.utils.filter_subgraphs_(table, map_dict, px2ang, **kw)
        assert filtered[k].tobytes() == one.tobytes() and len(one) == len(subgraph_rule(adj))
    # the flat table itself: the CSR of the three frames is the three CSRs, shifted
    from atomai_amd.utils import graphx
    p = graphx._Pass(list(frames.values()), map_dict, px2ang, 1.2, RADII)
    rowptr, col = p.rowptr.cpu().numpy(), p.col.cpu().numpy()
    for k, lo, hi in zip(frames, p.seg[:-1], p.seg[1:]):
        r1, c1 = csr(_memo[("frames", k)][0])
        assert np.array_equal(rowptr[lo:hi + 1] - rowptr[lo], r1) and np.array_equal(col[rowptr[lo]:rowptr[hi]] - lo, c1)


# ------------------------------------------------------------------------------------------------ 4. the cutoff
def cutoff_pairs(ca, cb):
    """Pairs (atom of class ca at the origin, atom of class cb at (dx, dy, dz)), one frame each, whose sum of squares
    lies exactly at, or one step of a coordinate either side of, cut2[ca][cb]: (pts, cls, seg, cut2, expected)."""
    names = ["C"] if ca == cb == 0 else ["C", "Si"]
    cut2 = cut2_table(names, 1.2)
    r = 1.2 * ((RADII[names[ca]] + RADII[names[cb]]) / 100)
    assert r * r == cut2[ca, cb]
    offsets = [(r, 0.0, 0.0), (np.nextafter(r, 0.0), 0.0, 0.0), (np.nextafter(r, np.inf), 0.0, 0.0), (0.0, 0.0, r),
               (0.0, -np.nextafter(r, np.inf), 0.0)]
    rng = np.random.default_rng(17 + ca + 2 * cb)
    for _ in range(12):                                   # a general direction, its largest component first
        u = rng.normal(size=3)
        d = r * u / np.sqrt((u * u).sum())
        d = d[np.argsort(-np.abs(d))]
        q = lambda x: x * x + d[1] * d[1] + d[2] * d[2]   # noqa: E731
        x = math.sqrt(cut2[ca, cb] - d[1] * d[1] - d[2] * d[2])
        toward = np.inf if q(x) <= cut2[ca, cb] else 0.0  # walk x to the step where the test flips
        for _ in range(64):
            nxt = np.nextafter(x, toward)
            if (q(nxt) <= cut2[ca, cb]) != (q(x) <= cut2[ca, cb]):
                break
            x = nxt
        inside, outside = (x, nxt) if q(x) <= cut2[ca, cb] else (nxt, x)
        assert q(inside) <= cut2[ca, cb] < q(outside) and outside == np.nextafter(inside, np.inf)
        offsets += [(inside, d[1], d[2]), (outside, d[1], d[2]), (-inside, d[1], d[2]), (-outside, d[1], d[2])]
    pts = np.zeros((2 * len(offsets), 3))
    pts[1::2] = offsets
    cls = np.tile(np.array([ca, cb], dtype=np.int32), len(offsets))
    seg = 2 * np.arange(len(offsets) + 1, dtype=np.int64)
    d = pts[1::2]
    expected = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] <= cut2[ca, cb]
    assert expected[:5].tolist() == [True, True, False, True, False] and expected.sum() >= 20 and (~expected).sum() >= 20
    return pts, cls, seg, cut2, expected


def check_cutoff(device):
    """Pairs exactly at the cutoff by the fp64 rule and one step either side, in a one-class and a two-class table."""
    import atomai_amd as aoi
    from atomai_amd.utils import _graph
    for ca, cb in ((0, 0), (0, 1), (1, 1)):
        pts, cls, seg, cut2, expected = cutoff_pairs(ca, cb)
        rowptr, col = _graph.bonds(torch.from_numpy(pts).to(device), torch.from_numpy(cls).to(device),
                                   torch.from_numpy(cut2).to(device), seg)
        deg = np.diff(rowptr.cpu().numpy())
        assert np.array_equal(deg[0::2], expected.astype(np.int64)) and np.array_equal(deg[1::2], deg[0::2]), (ca, cb)
        partner = np.arange(len(pts)) ^ 1
        assert np.array_equal(col.cpu().numpy(), partner[deg > 0].astype(np.int32))
    # through the public class, one class and two: at the cutoff bonded, one step beyond not
    for names, cols in ((("C", "C"), (0.0, 0.0)), (("C", "Si"), (0.0, 1.0))):
        r = aoi.utils.get_interatomic_r(names, 1.2, radii=RADII)
        assert r == 1.2 * ((RADII[names[0]] + RADII[names[1]]) / 100)
        for x, bonded in ((r, True), (np.nextafter(r, np.inf), False), (np.nextafter(r, 0.0), True)):
            G = aoi.utils.Graph(np.array([[0.0, 0.0, cols[0]], [0.0, x, cols[1]]]), {0: "C", 1: "Si"})
            G.find_neighbors(expand=1.2, radii=RADII)
            assert [a.tolist() for a in G.neighbors] == ([[1], [0]] if bonded else [[], []]), (names, x)


# ------------------------------------------------------------------------------------------------ 5. determinism
def check_determinism(device):
    """Two runs give identical tensors: CSR, rings and components."""
    from atomai_amd.utils import _graph
    table, map_dict, px2ang, expand, L, _ = case("big2_L8")
    frames = [table, table[:50], table[::-1].copy()]
    p, klass = points(np.concatenate([scale(t, px2ang) for t in frames]))
    uval, idx = np.unique(klass, return_inverse=True)
    cut2 = cut2_table([map_dict[int(u)] for u in uval], expand)
    seg = np.concatenate(([0], np.cumsum([len(t) for t in frames])))
    outs = []
    for _ in range(2):
        rowptr, col = _graph.bonds(torch.from_numpy(p).to(device), torch.from_numpy(idx.reshape(-1).astype(np.int32)).to(device),
                                   torch.from_numpy(cut2).to(device), seg)
        ring, length, rseg = _graph.rings(rowptr, col, seg, L)
        parent, rounds = _graph.components(rowptr, col)
        outs.append([rowptr, col, ring, length, torch.from_numpy(rseg), parent, torch.tensor([rounds])])
    assert len(outs[0][2]) > 100
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ 6. validation
def check_validation(device):
    """What the public functions refuse, each before or without a launch that could fault."""
    import atomai_amd as aoi
    from atomai_amd.utils import _graph
    U = aoi.utils
    md, kw = {0: "C", 1: "Si"}, {"radii": RADII}
    hexagon = tiny_tables()["hexagon"][0]
    # degree above 16: 18 atoms on one spot in the second frame
    pile = np.tile([[1.0, 2.0, 0.0]], (18, 1))
    with pytest.raises(ValueError, match=r"atom 0 of frame 1 .* 17 bonds"):
        U.filter_subgraphs({0: hexagon, 1: pile}, md, 1.0, **kw)
    with pytest.raises(ValueError, match="17 bonds"):
        U.find_cycles(pile, 6, md, 1.0, **kw)
    ok = np.tile([[1.0, 2.0, 0.0]], (17, 1))                      # 16 bonds each are fine
    assert len(U.filter_subgraphs_(ok, md, 1.0, **kw)) == 17
    # ring sizes
    for bad in (2, 17, 0, -1, [5, 17], [2, 6], [], 6.5):
        with pytest.raises(ValueError):
            U.find_cycles(hexagon, bad, md, 1.0, **kw)
        with pytest.raises(ValueError):
            U.find_cycle_clusters(hexagon, bad, md, 1.0, **kw)
    G = U.Graph(hexagon, md)
    G.find_neighbors(radii=RADII)
    for bad in (2, 17):
        with pytest.raises(ValueError):
            G.polycount(bad)
    rp, cl = (torch.from_numpy(a).to(device) for a in (G.rowptr, G.col))
    for bad in (2, 17):
        with pytest.raises(ValueError):
            _graph.rings(rp, cl, None, bad)
    assert len(_graph.rings(rp, cl, None, 16)[0]) == 1 and len(_graph.rings(rp, cl, None, 3)[0]) == 0
    # classes
    many = np.array([[3.0 * i, 0.0, float(i)] for i in range(17)])
    with pytest.raises(ValueError, match="17 classes"):
        U.find_cycles(many, 6, {i: "C" for i in range(17)}, 1.0, **kw)
    with pytest.raises(ValueError, match="16 classes"):
        _graph.bonds(torch.zeros((4, 3), dtype=torch.float64, device=device), torch.zeros(4, dtype=torch.int32, device=device),
                     torch.ones((17, 17), dtype=torch.float64, device=device))
    two = hexagon.copy()
    two[2, -1] = 1.0
    with pytest.raises(ValueError, match="missing from map_dict"):
        U.find_cycles(two, 6, {0: "C"}, 1.0, **kw)
    with pytest.raises(ValueError, match="missing from map_dict"):
        U.Graph(two, {0: "C"}).find_neighbors(radii=RADII)
    # coordinates
    for v in (np.nan, np.inf, -np.inf):
        bad = hexagon.copy()
        bad[3, 1] = v
        for fn in (lambda: U.find_cycles(bad, 6, md, 1.0, **kw), lambda: U.find_cycle_clusters(bad, 6, md, 1.0, **kw),
                   lambda: U.filter_subgraphs(bad, md, 1.0, **kw), lambda: U.Graph(bad, md).find_neighbors(radii=RADII)):
            with pytest.raises(ValueError, match="non-finite"):
                fn()
    for bad in (np.zeros((4, 2)), np.zeros((4, 5)), np.zeros(4)):
        with pytest.raises(ValueError):
            U.find_cycles(bad, 6, md, 1.0, **kw)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="px2ang"):
            U.find_cycles(hexagon, 6, md, bad, **kw)
    # radii
    with pytest.raises(ValueError, match=r"Si.*radii"):
        U.find_cycles(two, 6, md, 1.0, radii={"C": 75.0})
    with pytest.raises(ValueError, match=r"Si.*radii"):
        U.get_interatomic_r(["C", "Si"], 1.2, radii={"C": 75.0})
    try:
        import mendeleev  # noqa: F401
    except ImportError:
        with pytest.raises(ValueError, match=r"mendeleev.*radii"):
            U.find_cycles(hexagon, 6, md, 1.0)
        with pytest.raises(ValueError, match=r"mendeleev.*radii"):
            U.get_interatomic_r(["C", "C"])
    assert U.get_interatomic_r(["C", "Si"], radii=RADII) == (75.0 + 116.0) / 100
    # no ring of the requested size: the reference's np.concatenate([]) is a ValueError
    with pytest.raises(ValueError, match="concatenate"):
        U.find_cycles(hexagon, 5, md, 1.0, **kw)
    with pytest.raises(ValueError, match="concatenate"):
        U.find_cycles(np.empty((0, 3)), 6, md, 1.0, **kw)
    assert U.find_cycle_clusters(hexagon, 5, md, 1.0, **kw) == []
    empty = U.find_cycles_frames({4: hexagon, 9: np.empty((0, 3))}, 5, md, 1.0, **kw)
    assert list(empty) == [4, 9] and empty[4].shape == empty[9].shape == (0, 3)
    with pytest.raises(ValueError):
        U.filter_subgraphs_(np.empty((0, 3)), md, 1.0, **kw)
    # malformed CSR tensors
    for args in ((rp.int(), cl), (rp, cl.long()), (rp[None], cl), (rp[::2], cl)):
        with pytest.raises(ValueError):
            _graph.components(*args)


# ------------------------------------------------------------------------------------------------ 7. imports
def check_no_host_libraries(monkeypatch):
    """The computing path imports none of scipy, networkx and mendeleev: with all three made unimportable every public
    function still runs, and the two modules import them nowhere at module level.  The networkx exports say so."""
    import re
    import atomai_amd as aoi
    root = os.path.dirname(os.path.abspath(aoi.utils.__file__))
    for f in ("graphx.py", "_graph.py"):
        text = open(os.path.join(root, f)).read()
        assert not re.search(r"^(from|import)\s+(scipy|networkx|mendeleev)\b", text, flags=re.M), f
    for name in list(sys.modules):
        if name.split(".")[0] in ("scipy", "networkx", "mendeleev"):
            monkeypatch.delitem(sys.modules, name)
    for name in ("scipy", "networkx", "mendeleev"):
        monkeypatch.setitem(sys.modules, name, None)                # "import name" now raises ImportError
    table, L = tiny_tables()["fused"]
    md, kw = {0: "C"}, {"radii": RADII}
    assert len(aoi.utils.find_cycles(table, 6, md, 1.0, **kw)) == 12
    assert len(aoi.utils.find_cycles_frames({0: table, 1: table}, 6, md, 1.0, **kw)[1]) == 12
    assert [len(c) for c in aoi.utils.find_cycle_clusters(table, 6, md, 1.0, **kw)] == [10]
    assert len(aoi.utils.filter_subgraphs(table, md, 1.0, **kw)[0]) == 10
    G = aoi.utils.Graph(table, md)
    G.find_neighbors(radii=RADII)
    G.polycount(L)
    assert [len(r) for r in G.rings] == [6, 6]
    with pytest.raises(ImportError, match="networkx"):
        G.nx_graph()
    with pytest.raises(ImportError, match="networkx"):
        G.rings_to_nx_graph([6])


def check_exports():
    import atomai_amd as aoi
    for name in ("Graph", "find_cycles", "find_cycles_frames", "find_cycle_clusters", "filter_subgraphs",
                 "filter_subgraphs_", "get_interatomic_r"):
        assert name in aoi.utils.__all__ and callable(getattr(aoi.utils, name)), name
    assert not hasattr(aoi.utils.Graph, "find_rings") and not hasattr(aoi.utils.Graph, "shortest_path")
