"""Generates tests/golden/coords.npz from the REAL reference (imported through oracle/ref_harness.py, dev container only;
never imported by a test; needs numpy and scipy there):

    python tools/make_coords_golden.py

Inputs are jittered square lattices: site (7 i, 7 j) + U(-0.8, 0.8) per coordinate, drawn from ``default_rng``; the
class column alternates 0 / 1 at random.  The file holds the inputs and what the reference's atomai.utils.coords
functions return for them.

Keys
  nn|sizes (10,)                 atoms per frame of ONE dictionary (keys 0 .. 9): 0, 1, 2, 3, 7, 17, 255, 256, 257, 600
  nn|coords|f (n, 3) float64     its tables
  nn|nns                         the nn values 1, 2, 6, 15, 31
  nn|ub|nn, nn|ub|bound          the get_nn_distances(nn, upper_bound) case (some rows drop, some stay)
  nn|idx|f (n, nn_f + 1) int16   the reference's neighbour rows of frame f, column 0 the atom itself, from the call with
                                 nn_f = the largest nn of nn|nns that frame f is long enough for (frames 0, 1: none)
  nn|sha|<nn> (2,) str           sha256 of the bytes of np.concatenate of the reference's get_nn_distances(dict, nn)
                                 distance list, and of its coordinate list
  nn|ub|keep|f (n,) bool, nn|ub|idx|f (kept, nn + 1) int16, nn|ub|sha (2,)   the same for the upper-bound case
The reference returns float64 distances and GATHERED coordinate rows.  Storing them as such would take 0.6 MB for these
sizes, so they are stored losslessly as row indices plus digests: this script ASSERTS that every table has distinct rows
(so the indices are recovered from the returned coordinates without ambiguity), that the outputs for a smaller nn are
the leading columns of the outputs for the largest one, and that the reference's distances equal
sqrt(dx * dx + dy * dy) evaluated in numpy float64 at those indices BIT FOR BIT; the test rebuilds both arrays from the
indices, checks them against the digests — after which it holds the reference's output exactly — and compares.

  cmp|c1, cmp|c2 (n, 3), cmp|d_max; cmp|o1, cmp|o2, cmp|dr         compare_coordinates(c1, c2, d_max)
  edge|dim (h, w), edge|dist; edge|out                              remove_edge_coord(cmp|c2, dim, dist)
  fcc|f (n, 3) f = 0, 1, 2 (the movie), fcc|first (n, 3), fcc|rmax; fcc|means, fcc|stds (n, 2), fcc|counts (n,),
      fcc|members (sum counts, 3)                                  find_coord_clusters({0: first}, movie, rmax)
  int|frames (3, H, W) float32, int|keys (3,), int|coords|k (n, 3), int|rs; int|out|r|k (n,) float64
      get_intensities(dict, float64 copy of the frames, r): the windows' means in float64 on float32-representable
      pixels.  Atoms at both edges (a negative start gives NaN in the reference: an empty slice), a planted x.5 pair.

Preconditions ASSERTED here in fp64 brute force (so the tests may compare every row): consecutive sorted squared
distances, up to one past the last one used, differ by more than 1e-9 relative; no distance lies within 1e-9 relative of
a bound; no coordinate that is rounded lies within 1e-9 of a half-integer other than the planted exact ones.
TEST INFRASTRUCTURE ONLY.
"""
import hashlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SIZES = [0, 1, 2, 3, 7, 17, 255, 256, 257, 600]
NNS = [1, 2, 6, 15, 31]
UB_NN, UB_BOUND = 4, 7.6
REL = 1e-9


def lattice(n, rng, origin=(0.0, 0.0)):
    side = int(np.ceil(np.sqrt(max(n, 1))))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n]
    xy = 7.0 * ij + np.asarray(origin) + rng.uniform(-0.8, 0.8, (n, 2))
    return np.concatenate((xy, rng.integers(0, 2, (n, 1)).astype(np.float64)), axis=1)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sq_dists(q, p):
    """Brute-force squared distances (len(q), len(p)) in float64, one rounded operation per ufunc call."""
    acc = np.zeros((len(q), len(p)))
    for c in range(q.shape[1]):
        t = p[None, :, c] - q[:, None, c]
        acc = acc + t * t
    return acc


def assert_gaps(q2, used, bounds=(), what=""):
    """Rows of q2: squared distances.  Sorted, the first used + 1 must be separated; none may sit on a bound."""
    s = np.sort(q2, axis=1)[:, :used + 1]
    s = s[:, np.isfinite(s).all(0)] if s.size else s
    if s.shape[1] >= 2:
        gap = (s[:, 1:] - s[:, :-1]) / np.maximum(s[:, 1:], 1e-300)
        assert gap.min() > REL, (what, float(gap.min()))
        worst = float(gap.min())
    else:
        worst = np.inf
    for b in bounds:
        d = np.sqrt(q2)
        assert (np.abs(d - b) > REL * b).all(), (what, b)
    return worst


def row_index(table, rows):
    """Rows of ``table`` that the gathered ``rows`` (..., C) came from (tables have distinct rows: asserted)."""
    assert len(np.unique(table, axis=0)) == len(table)
    flat = rows.reshape(-1, table.shape[1])
    hit = (flat[:, None, :] == table[None, :, :]).all(-1)
    assert (hit.sum(1) == 1).all()
    return hit.argmax(1).reshape(rows.shape[:-1])


def rebuilt_distances(table, idx):
    p = table[idx]                                          # (m, k, C)
    dx, dy = p[:, 1:, 0] - p[:, :1, 0], p[:, 1:, 1] - p[:, :1, 1]
    return np.sqrt(dx * dx + dy * dy)


def main():
    ref_harness.import_reference()
    from atomai.utils import coords as ref
    from scipy import spatial
    out = {}
    worst = np.inf

    # ------------------------------------------------------------------------------------------ get_nn_distances
    rng = np.random.default_rng(0)
    frames = {f: lattice(n, rng) for f, n in enumerate(SIZES)}
    out["nn|sizes"], out["nn|nns"] = np.array(SIZES), np.array(NNS)
    for f, t in frames.items():
        out[f"nn|coords|{f}"] = t
        if len(t) >= 2:
            q2 = sq_dists(t[:, :2], t[:, :2])
            worst = min(worst, assert_gaps(q2, min(len(t), 32), (UB_BOUND,), f"nn frame {f}"))
    idx_of = {}
    for nn in NNS:
        d_all, p_all = ref.get_nn_distances(frames, nn)
        assert len(d_all) == len(p_all) == len(SIZES)
        for f, (d, p) in enumerate(zip(d_all, p_all)):
            t = frames[f]
            n = len(t)
            if n < nn + 1:
                assert d.shape == (0, nn) and p.shape == (0, nn + 1, 3), (f, nn, d.shape, p.shape)
                continue
            assert d.shape == (n, nn) and p.shape == (n, nn + 1, 3) and d.dtype == p.dtype == np.float64
            ix = row_index(t, p)
            assert np.array_equal(ix[:, 0], np.arange(n))
            assert rebuilt_distances(t, ix).tobytes() == d.tobytes(), (f, nn, "reference != fp64 brute force")
            # scipy's tree against brute force with a stable argsort
            order = np.argsort(sq_dists(t[:, :2], t[:, :2]), axis=1, kind="stable")[:, :nn + 1]
            assert np.array_equal(order, ix), (f, nn)
            if f in idx_of:                                 # nested: a smaller nn is the leading columns
                assert np.array_equal(idx_of[f], ix[:, :idx_of[f].shape[1]]), (f, nn)
            idx_of[f] = ix
        out[f"nn|sha|{nn}"] = np.array([sha(np.concatenate(d_all)), sha(np.concatenate(p_all))])
    for f, ix in idx_of.items():
        out[f"nn|idx|{f}"] = ix.astype(np.int16)
    d_all, p_all = ref.get_nn_distances(frames, UB_NN, UB_BOUND)
    out["nn|ub|nn"], out["nn|ub|bound"] = UB_NN, UB_BOUND
    kept_total = 0
    for f, (d, p) in enumerate(zip(d_all, p_all)):
        t = frames[f]
        ix = row_index(t, p) if len(p) else np.empty((0, UB_NN + 1), dtype=np.int64)
        keep = np.zeros(len(t), dtype=bool)
        keep[ix[:, 0]] = True
        assert np.array_equal(np.nonzero(keep)[0], ix[:, 0]) and d.shape == (len(ix), UB_NN)
        assert (d < UB_BOUND).all() and rebuilt_distances(t, ix).tobytes() == d.tobytes()
        if len(t) >= 255:
            assert 0 < keep.sum() < len(t), (f, keep.sum())     # some rows drop and some stay
        kept_total += int(keep.sum())
        out[f"nn|ub|keep|{f}"], out[f"nn|ub|idx|{f}"] = keep, ix.astype(np.int16)
    out["nn|ub|sha"] = np.array([sha(np.concatenate(d_all)), sha(np.concatenate(p_all))])
    print(f"get_nn_distances: upper bound {UB_BOUND} keeps {kept_total} of {sum(SIZES)} rows")

    # ------------------------------------------------------------------------------------------ compare_coordinates
    rng = np.random.default_rng(1)
    c2 = lattice(120, rng)
    pick = rng.permutation(120)[:90]
    c1 = c2[pick].copy()
    c1[:, :2] += rng.normal(0, 0.45, (90, 2))
    flip = rng.uniform(size=90) < 0.15
    c1[flip, 2] = 1 - c1[flip, 2]                           # the class column takes part in the reference's distance
    c1 = np.concatenate((c1, np.array([[200.0, 200.0, 0.0], [-30.0, 4.0, 1.0]])))
    d_max = 1.0
    q2 = sq_dists(c1, c2)
    worst = min(worst, assert_gaps(q2, 1, (d_max,), "compare_coordinates"))
    o1, o2, dr = ref.compare_coordinates(c1, c2, d_max)
    assert 0 < len(dr) < len(c1) and o1.shape == o2.shape == (len(dr), 3)
    assert np.array_equal(dr, np.sqrt(q2.min(1))[np.sqrt(q2.min(1)) < d_max])
    out.update({"cmp|c1": c1, "cmp|c2": c2, "cmp|d_max": d_max, "cmp|o1": o1, "cmp|o2": o2, "cmp|dr": dr})
    print(f"compare_coordinates: {len(dr)} of {len(c1)} matched within {d_max}")
    # remove_edge_coord on the same lattice (rows 0 .. 77, columns 0 .. 77): h != w shows which column meets which
    edge_dim, edge_dist = (60, 75), 9
    kept = ref.remove_edge_coord(c2, edge_dim, edge_dist)
    assert 0 < len(kept) < len(c2) and not np.array_equal(kept, ref.remove_edge_coord(c2, edge_dim[::-1], edge_dist))
    out.update({"edge|dim": np.array(edge_dim), "edge|dist": edge_dist, "edge|out": kept})

    # ------------------------------------------------------------------------------------------ find_coord_clusters
    base = lattice(40, rng)
    movie = {}
    for f in range(3):
        t = base.copy()
        t[:, :2] += rng.normal(0, 0.5, (40, 2))
        movie[f] = t[rng.permutation(40)[:40 - 3 * f]]      # later frames lose atoms
    first = np.concatenate((movie[0], np.array([[300.0, 300.0, 0.0]])))      # the last atom has no neighbour
    rmax = 2.0
    every = np.concatenate([movie[f] for f in range(3)])
    q2 = sq_dists(first[:, :2], every[:, :2])
    worst = min(worst, assert_gaps(q2, 6, (rmax,), "find_coord_clusters"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        means, stds, clusters = ref.find_coord_clusters({0: first}, movie, rmax)
    counts = np.array([len(c) for c in clusters])
    assert counts.max() >= 3 and counts.min() == 0 and np.isnan(means[-1]).all() and np.isnan(stds[-1]).all()
    for f, t in movie.items():
        out[f"fcc|{f}"] = t
    out.update({"fcc|first": first, "fcc|rmax": rmax, "fcc|means": means, "fcc|stds": stds, "fcc|counts": counts,
                "fcc|members": np.concatenate(clusters)})
    print(f"find_coord_clusters: cluster sizes {np.bincount(counts).tolist()} (count of sizes 0, 1, ...)")

    # ------------------------------------------------------------------------------------------ get_intensities
    H, W = 30, 34
    img = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    keys = [2, 0, 1]                                        # the frame is picked by KEY, not by position
    tables = {}
    for k in keys:
        t = lattice(16, rng, origin=(4.0, 5.0))
        edge = np.array([[0.2, 5.3, 0.0], [6.1, 0.3, 0.0], [0.4, 0.4, 1.0], [1.3, 1.2, 0.0], [29.4, 33.6, 1.0],
                         [29.6, 12.2, 0.0], [28.2, 32.7, 0.0], [15.5, 10.0, 0.0], [14.5, 11.5, 1.0]])
        tables[k] = np.concatenate((t, edge))
        frac = np.abs(tables[k][:-2, :2] % 1.0 - 0.5)
        assert (frac > REL).all()
    out["int|frames"], out["int|keys"], out["int|rs"] = img, np.array(keys), np.array([2, 3, 4])
    for k in keys:
        out[f"int|coords|{k}"] = tables[k]
    for r in (2, 3, 4):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = ref.get_intensities(tables, img.astype(np.float64)[..., None], r)
        for k, v in zip(keys, res):
            assert v.dtype == np.float64 and v.shape == (len(tables[k]),)
            assert np.isnan(v[16:20]).sum() >= 3 and np.isfinite(v[:16]).all() and np.isfinite(v[20:]).all(), (r, k, v)
            out[f"int|out|{r}|{k}"] = v
    # the tree itself against brute force on one large frame (scipy's own agreement, recorded in the log)
    t = frames[9]
    d, i = spatial.cKDTree(t[:, :2]).query(t[:, :2], k=32)
    assert np.array_equal(i, np.argsort(sq_dists(t[:, :2], t[:, :2]), axis=1, kind="stable")[:, :32])
    print(f"smallest relative gap between consecutive squared distances that a comparison relies on: {worst:.3e}")
    path = os.path.join(GOLD, "coords.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; stat.npz has", os.path.getsize(os.path.join(GOLD, "stat.npz")))
    assert os.path.getsize(path) < os.path.getsize(os.path.join(GOLD, "stat.npz"))


if __name__ == "__main__":
    main()
