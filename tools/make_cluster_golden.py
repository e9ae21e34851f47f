"""Generates tests/golden/cluster.npz from scikit-learn and from the REAL reference (imported through
oracle/ref_harness.py, dev container only; never imported by a test; needs numpy, scipy and scikit-learn there):

    python tools/make_cluster_golden.py

Part 1: DBSCAN tables.  ``names`` lists the cases; case c holds
  c|pts (n, 2) float64, c|seg (S + 1,) int64 segment offsets, c|runs (R, 2) float64 = (eps, min_samples) per run,
  c|labels (R, n) int16 and c|core (R, n) bool: sklearn.cluster.DBSCAN(eps, min_samples).fit(segment), segment by segment.
Before anything is written this script ASSERTS that the O(n^2) numpy rule of tests/_cluster_checks.py (``rule``: fp64
dx*dx + dy*dy <= eps*eps, core = count >= min_samples, components numbered by their smallest core row, a border row takes
the smallest label among its core neighbours) reproduces scikit-learn's labels and core flags on every run of every case.
The case ``lattice01`` (the integer lattice scaled by 0.1, eps = 0.1: its ties are no longer exact in binary) is kept
only if that assertion holds for it; otherwise it is dropped with a message.

  single      one point, min_samples 1 (cluster 0) and 2 (noise)
  same50      50 identical points, min_samples 10
  lattice     12 x 12 integer lattice + 20 duplicated rows, shuffled; eps 1, nextafter(1, 0), sqrt 2; min_samples 1, 2, 5
  lattice01   the same scaled by 0.1, eps 0.1
  uniform257  257 uniform points in [0, 20)^2: eps 1.7, min_samples 3, and eps 1.0, min_samples 4.  The seed is the first
              for which at least 5 border rows have core neighbours in two different clusters in the second run
              (asserted).  In the first run no row can: below min_samples = 3 a row has one neighbour at most.
  chains      two chains of 300 and 40 points, spacing 0.9 eps, laid as snakes (runs 2.7 eps apart, so only consecutive
              points are neighbours), rows shuffled, min_samples 2
  segments    segments of 0, 1, 37, 300 and 64 rows; the rows of the smaller segments repeat positions of the 300
  far         two blobs of 30 points around (-1e3, -1e3) and (1e6, 1e6), eps 1e-3

Part 2: the reference's atomai.utils.cluster_coord.  cc|<case>|f (n, 3) f = 0, 1, 2 the frames, cc|<case>|eps,
cc|<case>|ms; cc|<case>|clusters (K, m, 3), cc|<case>|mean, cc|<case>|var (K, 2) what it returned.
  noisy   three frames of jittered positions plus detections that appear in one frame only: noise points
  clean   three frames of well separated positions, no noise: np.unique(labels)[1:] drops cluster 0 there
The reference builds np.array(list of clusters), which numpy >= 1.24 refuses for clusters of different sizes, so both
cases are built to give three members per cluster (asserted).
TEST INFRASTRUCTURE ONLY.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness  # noqa: E402
import _cluster_checks as K  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def sk_dbscan(pts, seg, eps, ms):
    from sklearn.cluster import DBSCAN
    labels, core = np.full(len(pts), -1, dtype=np.int64), np.zeros(len(pts), dtype=bool)
    for lo, hi in zip(seg[:-1], seg[1:]):
        if hi > lo:
            fit = DBSCAN(eps=eps, min_samples=int(ms)).fit(pts[lo:hi])
            labels[lo:hi] = fit.labels_
            core[lo + fit.core_sample_indices_] = True
    return labels, core


def two_cluster_borders(pts, eps, ms):
    labels, core = K.rule(pts, eps, ms)
    adj = K.neighbours(pts, eps)
    n = 0
    for i in np.nonzero(~core & (labels >= 0))[0]:
        n += len(np.unique(labels[adj[i] & core])) >= 2
    return n


def snake(n, step, run, origin):
    """n points of a path that goes ``run`` steps right, 3 up, ``run`` left, 3 up, ...: only consecutive points lie
    within step / 0.9 of each other."""
    out, pos, d, left = [], np.array(origin, dtype=np.float64), 1.0, run
    up = 0
    for _ in range(n):
        out.append(pos.copy())
        if up:
            pos = pos + (0.0, step)
            up -= 1
        elif left:
            pos = pos + (d * step, 0.0)
            left -= 1
            if not left:
                up, d, left = 3, -d, run
    return np.array(out)


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    one = lambda n: np.array([0, n], dtype=np.int64)                                      # noqa: E731
    out["single"] = (np.array([[3.5, -2.0]]), one(1), [(1.0, 1), (1.0, 2)])
    out["same50"] = (np.tile([[7.25, -3.125]], (50, 1)), one(50), [(0.5, 10)])
    ij = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0), indexing="ij"), -1).reshape(-1, 2)
    lat = np.concatenate((ij, ij[rng.choice(144, 20, replace=False)]))
    lat = lat[rng.permutation(len(lat))]
    runs = [(e, m) for e in (1.0, np.nextafter(1.0, 0.0), np.sqrt(2.0)) for m in (1, 2, 5)]
    out["lattice"] = (lat, one(len(lat)), runs)
    out["lattice01"] = (0.1 * lat, one(len(lat)), [(0.1, m) for m in (1, 2, 5)])
    # A row that is not core at min_samples = 3 has at most ONE neighbour besides itself, so it cannot touch two
    # clusters: the run (1.7, 3) crosses the 256-row tile, and the border rule is exercised by a second run on the same
    # table, (1.0, 4), for which the seed is chosen.
    for seed in range(2000):
        u = np.random.default_rng(seed).uniform(0.0, 20.0, (257, 2))
        if two_cluster_borders(u, 1.0, 4) >= 5:
            break
    assert two_cluster_borders(u, 1.0, 4) >= 5 and two_cluster_borders(u, 1.7, 3) == 0
    print(f"uniform257: seed {seed}, {two_cluster_borders(u, 1.0, 4)} border rows between two clusters at (1.0, 4)")
    out["uniform257"] = (u, one(257), [(1.7, 3), (1.0, 4)])
    ch = np.concatenate((snake(300, 0.9, 25, (0.0, 0.0)), snake(40, 0.9, 6, (40.0, 5.0))))
    out["chains"] = (ch[rng.permutation(len(ch))], one(len(ch)), [(1.0, 2)])
    big = rng.uniform(0.0, 12.0, (300, 2))
    sizes = [0, 1, 37, 300, 64]
    pts = np.concatenate((big[5:6], big[100:137], big, big[:64]))
    out["segments"] = (pts, np.concatenate(([0], np.cumsum(sizes))).astype(np.int64), [(1.0, 3)])
    far = np.concatenate((-1e3 + rng.normal(0.0, 3e-4, (30, 2)), 1e6 + rng.normal(0.0, 3e-4, (30, 2))))
    out["far"] = (far[rng.permutation(60)], one(60), [(1e-3, 3)])
    return out


def main():
    gold = {}
    names = []
    for name, (pts, seg, runs) in cases().items():
        labels, core, ok = [], [], True
        for eps, ms in runs:
            sl, sc = sk_dbscan(pts, seg, eps, ms)
            rl, rc = K.rule_segments(pts, seg, eps, ms)
            same = np.array_equal(sl, rl) and np.array_equal(sc, rc)
            if not same and name == "lattice01":
                ok = False
                print(f"lattice01 DROPPED: the numpy rule and scikit-learn disagree at eps = {eps}, min_samples = {ms} "
                      f"({(sl != rl).sum()} labels)")
                break
            assert same, (name, eps, ms)
            labels.append(sl)
            core.append(sc)
        if not ok:
            continue
        names.append(name)
        gold[f"{name}|pts"], gold[f"{name}|seg"] = pts, seg
        gold[f"{name}|runs"] = np.array(runs, dtype=np.float64)
        gold[f"{name}|labels"] = np.array(labels).astype(np.int16)
        gold[f"{name}|core"] = np.array(core)
        print(f"{name}: n = {len(pts)}, runs = {len(runs)}, clusters = {[int(x.max()) + 1 for x in labels]}, "
              f"noise = {[int((x < 0).sum()) for x in labels]}")
    gold["names"] = np.array(names)

    ref_harness.import_reference()
    from atomai.utils import cluster_coord
    rng = np.random.default_rng(7)
    ij = np.stack(np.meshgrid(np.arange(6.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 2)
    base = 8.0 * ij + 4.0 + rng.uniform(-1.0, 1.0, ij.shape)
    cls = rng.integers(0, 2, (len(base), 1)).astype(np.float64)
    for case, extra in (("noisy", 4), ("clean", 0)):
        frames = {}
        for f in range(3):
            xy = base + rng.uniform(-0.15, 0.15, base.shape)
            stray = np.concatenate((rng.uniform(0.0, 48.0, (extra, 2)), np.ones((extra, 1))), axis=1)
            frames[f] = np.concatenate((np.concatenate((xy, cls), axis=1), stray))[rng.permutation(len(xy) + extra)]
        eps, ms = 0.5, 3
        clusters, mean, var = cluster_coord(frames, eps, ms)
        every = np.concatenate([frames[f] for f in range(3)])
        labels, _ = K.rule(every[:, :2], eps, ms)
        assert ((labels < 0).sum() > 0) == (case == "noisy") and (labels < 0).sum() == 3 * extra
        want = len(base) - (case == "clean")
        assert clusters.dtype == np.float64 and clusters.shape == (want, 3, 3) and mean.shape == var.shape == (want, 2)
        for f in range(3):
            gold[f"cc|{case}|{f}"] = frames[f]
        gold[f"cc|{case}|eps"], gold[f"cc|{case}|ms"] = np.float64(eps), np.int64(ms)
        gold[f"cc|{case}|clusters"], gold[f"cc|{case}|mean"], gold[f"cc|{case}|var"] = clusters, mean, var
        print(f"cluster_coord {case}: {len(every)} rows, {int((labels < 0).sum())} noise, {len(mean)} clusters returned")
    path = os.path.join(GOLD, "cluster.npz")
    np.savez_compressed(path, **gold)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
