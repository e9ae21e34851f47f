"""Generates tests/golden/graph.npz from the REAL reference's atomai/utils/graphx.py (loaded from its path under
oracle/ref_harness.REFERENCE_ROOT; dev container only; never imported by a test; needs numpy, scipy, networkx and
matplotlib there):

    python tools/make_graph_golden.py

The reference takes covalent radii from mendeleev, which the dev container does not have.  A stand-in module of this
tool's own is put in sys.modules first: its ``element()`` returns objects whose ``covalent_radius`` comes from RADII
below (pm), which is recorded in the golden (radii|names, radii|values).  The values only have to be the same on both
sides; the tests pass them through the ``radii`` keyword.

``names`` lists the cases; case c holds
  c|table (n, 3) float64 in pixels, c|px2ang, c|expand, c|L, c|cycles (max = L), c|classes + c|elements (map_dict);
  c|rowptr int64, c|col int32      the reference's neighbour lists after Graph.find_neighbors, ascending, as a CSR;
  c|rings (R, 16) int16            polycount(L) + remove_filled_polygons(): ascending ids, -1 behind them, ordered by
                                   (length, ids);
  c|find_cycles                    what find_cycles(table, cycles, map_dict, px2ang, expand=...) returned;
  c|cluster_rows, c|cluster_ids, c|cluster_off
                                   find_cycle_clusters' arrays with the rows of every cluster in ascending atom order
                                   and the clusters by their smallest atom (the atom of a returned row is found by
                                   comparing bits; the rows of a table are distinct), concatenated, with offsets;
  c|filtered, c|filtered_ids       filter_subgraphs_' table with its rows in ascending atom order.

Before anything is written this script ASSERTS on every case that the restatement of tests/_graph_checks.py equals
the reference: bonds as sets, rings as a sorted list without duplicates, cluster member sets, the filtered table after
row sorting; that no pair of atoms lies within 1e-9 (relative, in the squared distance) of its cutoff; and that no two
rings tie on the reference's sort key (length, first three ids).

Cases (angstrom geometry divided by px2ang = 0.104; C-C bonds 1.42, cutoffs 1.2 (R_a + R_b) / 100):
  hcA_L6, hcA_L8     80-atom jittered honeycomb, 4 vacancies, one class
  hcB_L6, hcB_L8     the same lattice, 5 vacancies, 3 added atoms (bond centres and a hexagon centre: degree up to 6),
                     two classes
  hcC_L6             2 added atoms, one class, no vacancy
  square_L4/6/8      5 x 4 square lattice of spacing 1.5
  vac_L9, vac_L12    honeycomb with one vacancy in its middle: the 12-ring round it appears at L = 12 only (asserted)
  tri_L3, tri_L6     5 x 5 triangular lattice of spacing 1.5
  big2_L6, big2_L8   320-atom jittered honeycomb, a fifth of the atoms of the second class (Si - Si second neighbours
                     bond), 4 vacancies, 4 added atoms
TEST INFRASTRUCTURE ONLY.
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness  # noqa: E402
import _graph_checks as K  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
RADII = {"C": 75.0, "Si": 116.0}
PX2ANG, EXPAND = 0.104, 1.2


def load_reference():
    class _Element:
        def __init__(self, name):
            self.covalent_radius = RADII[name]

    def element(ids):
        return _Element(ids) if isinstance(ids, str) else [_Element(i) for i in ids]

    stand_in = types.ModuleType("mendeleev")
    stand_in.element = element
    sys.modules["mendeleev"] = stand_in
    import matplotlib
    matplotlib.use("Agg")
    path = os.path.join(ref_harness.REFERENCE_ROOT, "atomai", "utils", "graphx.py")
    spec = importlib.util.spec_from_file_location("reference_graphx", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def with_class(xy, cls=0.0):
    cls = np.broadcast_to(np.asarray(cls, dtype=np.float64), (len(xy),))
    return np.concatenate((np.asarray(xy) / PX2ANG, cls[:, None]), axis=1)


def tables():
    rng = np.random.default_rng(2025)
    out = {}
    hc = K.honeycomb(4, 5)
    assert len(hc) == 80
    interior = [i for i in range(80) if (((hc - hc[i]) ** 2).sum(1) < 1.5 ** 2).sum() == 4]
    jit = hc + rng.uniform(-0.07, 0.07, hc.shape)

    def centre_of_bond(p, i):
        j = np.argsort(((p - p[i]) ** 2).sum(1))[1]
        return 0.5 * (p[i] + p[j])

    def centre_of_hexagon(p, i):
        near = np.argsort(((p - p[i]) ** 2).sum(1))[:4]                  # i and its three neighbours
        a, b = p[near[1]] - p[i], p[near[2]] - p[i]
        return p[i] + a + b                                                 # across the hexagon that a and b span

    gone = rng.choice(interior, 5, replace=False)
    a = np.delete(jit, gone[:4], axis=0)
    out["hcA"] = (with_class(a), {0: "C"}, (6, 8))
    extra = np.array([centre_of_bond(jit, interior[3]), centre_of_bond(jit, interior[11]),
                      centre_of_hexagon(hc, interior[7])])
    b = np.concatenate((np.delete(jit, gone, axis=0), extra))
    b = b[rng.permutation(len(b))]
    out["hcB"] = (with_class(b, rng.random(len(b)) < 0.25), {0: "C", 1: "Si"}, (6, 8))
    c = np.concatenate((jit, extra[[0, 2]]))
    out["hcC"] = (with_class(c[np.lexsort((c[:, 0], c[:, 1]))]), {0: "C"}, (6,))
    ij = np.stack(np.meshgrid(np.arange(5.0), np.arange(4.0), indexing="ij"), -1).reshape(-1, 2)
    out["square"] = (with_class(1.5 * ij), {0: "C"}, (4, 6, 8))
    middle = int(np.argmin(((hc - hc.mean(0)) ** 2).sum(1)))                # far enough from the edge for the 12-ring
    out["vac"] = (with_class(np.delete(jit, middle, axis=0)), {0: "C"}, (9, 12))
    ij = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 2)
    out["tri"] = (with_class(1.5 * np.stack((ij[:, 0] + 0.5 * ij[:, 1], 0.5 * np.sqrt(3.0) * ij[:, 1]), 1)), {0: "C"},
                  (3, 6))
    big = K.honeycomb(8, 10)
    assert len(big) == 320
    inner = [i for i in range(320) if (((big - big[i]) ** 2).sum(1) < 1.5 ** 2).sum() == 4]
    jb = big + rng.uniform(-0.07, 0.07, big.shape)
    pick = rng.choice(inner, 8, replace=False)
    extra = np.array([centre_of_bond(jb, pick[4]), centre_of_bond(jb, pick[5]), centre_of_hexagon(big, pick[6]),
                      centre_of_hexagon(big, pick[7])])
    t = np.concatenate((np.delete(jb, pick[:4], axis=0), extra))
    t = t[np.lexsort((t[:, 0], t[:, 1]))]
    out["big2"] = (with_class(t, rng.random(len(t)) < 0.2), {0: "C", 1: "Si"}, (6, 8))
    return out


def reference_case(ref, table, map_dict, L, cycles):
    scaled = K.scale(table, PX2ANG)
    G = ref.Graph(scaled.copy(), map_dict)
    G.find_neighbors(expand=EXPAND)
    adj = [np.array(sorted(n.id for n in v.neighbors), dtype=np.int64) for v in G.vertices]
    assert all(len(set(a.tolist())) == len(a) for a in adj)
    G.polycount(max_depth=L)
    raw = len(G.rings)
    G.remove_filled_polygons()
    rings = [tuple(sorted(int(v.id) for v in r)) for r in G.rings]
    assert len(set(rings)) == len(rings), "the reference lists a ring twice"
    keys = [(len(r), r[0], r[1], r[2]) for r in rings]
    assert len(set(keys)) == len(keys), "two rings tie on the reference's sort key"
    rings = sorted(rings, key=lambda r: (len(r), r))
    try:
        fc = ref.find_cycles(table.copy(), list(cycles), map_dict, PX2ANG, expand=EXPAND)
    except ValueError:
        fc = None
    clusters = ref.find_cycle_clusters(table.copy(), list(cycles), map_dict, PX2ANG, expand=EXPAND)
    filtered = ref.filter_subgraphs_(table.copy(), map_dict, PX2ANG, expand=EXPAND)
    return scaled, adj, raw, rings, fc, clusters, filtered


def ids_of(rows, every):
    """The atom of every row of ``rows``: the row of ``every`` with the same bits."""
    assert len({r.tobytes() for r in every}) == len(every)
    where = {r.tobytes(): i for i, r in enumerate(np.ascontiguousarray(every))}
    return np.array([where[np.ascontiguousarray(r).tobytes()] for r in rows], dtype=np.int64)


def main():
    ref = load_reference()
    gold = {"radii|names": np.array(list(RADII)), "radii|values": np.array(list(RADII.values()))}
    names = []
    for base, (table, map_dict, depths) in tables().items():
        for L in depths:
            name = f"{base}_L{L}"
            cycles = [s for s in range(3, L + 1) if s != 6 or L == 6]
            scaled, adj, raw, rings, fc, clusters, filtered = reference_case(ref, table, map_dict, L, cycles)
            if fc is None:                      # nothing but hexagons: ask for them too
                cycles = list(range(3, L + 1))
                scaled, adj, raw, rings, fc, clusters, filtered = reference_case(ref, table, map_dict, L, cycles)
            assert fc is not None, name
            # no pair near its cutoff
            p, klass = K.points(scaled)
            uval, idx = np.unique(klass, return_inverse=True)
            cut2 = K.cut2_table([map_dict[int(u)] for u in uval], EXPAND, RADII)[idx.reshape(-1)[:, None], idx.reshape(-1)[None, :]]
            d = p[None] - p[:, None]
            q = (d * d).sum(-1)
            off = ~np.eye(len(p), dtype=bool)
            assert (np.abs(q / cut2 - 1.0)[off] > 1e-9).all(), name
            # the restatement equals the reference
            r_adj = K.bonds_rule(scaled, map_dict, EXPAND, RADII)
            assert all(set(a.tolist()) == set(b.tolist()) for a, b in zip(adj, r_adj)) and len(adj) == len(r_adj), name
            assert max(len(a) for a in adj) <= 16
            r_rings = K.rings_rule(r_adj, L)
            assert r_rings == rings, (name, len(r_rings), len(rings))
            want = [scaled[list(r)] for r in rings if len(r) in cycles]
            want = np.concatenate(want)
            want[:, :-1] = want[:, :-1] * (1 / PX2ANG)
            assert fc.tobytes() == want.tobytes(), name
            every = scaled[:, :-1] * (1 / PX2ANG)
            cl_ids = [np.sort(ids_of(c, every)) for c in clusters]
            cl_ids.sort(key=lambda c: c[0])
            assert [c.tolist() for c in cl_ids] == K.clusters_rule(r_adj, r_rings, cycles), name
            xy = np.stack((scaled[:, 0] / PX2ANG, scaled[:, 1] / PX2ANG), 1)
            f_ids = ids_of(filtered[:, :2], xy)
            order = np.argsort(f_ids)
            assert np.array_equal(f_ids[order], K.subgraph_rule(r_adj)), name
            assert np.array_equal(filtered[order][:, 2], table[f_ids[order], -1])
            if base == "vac":
                assert [len(r) for r in rings].count(12) == (L == 12), name
            names.append(name)
            rowptr, col = K.csr(adj)
            ring_arr = np.full((len(rings), 16), -1, dtype=np.int16)
            for i, r in enumerate(rings):
                ring_arr[i, :len(r)] = r
            gold.update({
                f"{name}|table": table, f"{name}|px2ang": np.float64(PX2ANG), f"{name}|expand": np.float64(EXPAND),
                f"{name}|L": np.int64(L), f"{name}|cycles": np.array(cycles, dtype=np.int64),
                f"{name}|classes": np.array(list(map_dict), dtype=np.int64), f"{name}|elements": np.array(list(map_dict.values())),
                f"{name}|rowptr": rowptr, f"{name}|col": col, f"{name}|rings": ring_arr, f"{name}|find_cycles": fc,
                f"{name}|cluster_ids": np.concatenate(cl_ids) if cl_ids else np.zeros(0, dtype=np.int64),
                f"{name}|cluster_rows": np.concatenate([every[c] for c in cl_ids]) if cl_ids else np.zeros((0, 2)),
                f"{name}|cluster_off": np.concatenate(([0], np.cumsum([len(c) for c in cl_ids]))).astype(np.int64),
                f"{name}|filtered": filtered[order], f"{name}|filtered_ids": f_ids[order]})
            sizes = np.bincount([len(r) for r in rings], minlength=L + 1)[3:]
            print(f"{name}: {len(table)} atoms, max degree {max(len(a) for a in adj)}, {raw} cycles searched, {len(rings)} "
                  f"rings (sizes 3..{L}: {sizes.tolist()}), cycles {cycles}: {len(fc)} rows, {len(cl_ids)} clusters "
                  f"{[len(c) for c in cl_ids]}, largest subgraph {len(f_ids)}")
    gold["names"] = np.array(names)
    path = os.path.join(GOLD, "graph.npz")
    np.savez_compressed(path, **gold)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
