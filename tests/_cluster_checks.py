"""Shared bodies of the density-clustering tests (emulator tier on CPU, gpu tier on the MI355X): csrc/cluster.hip through
atomai_amd.utils._cluster against the O(n^2) numpy form of the DBSCAN rule and against tests/golden/cluster.npz, which
tools/make_cluster_golden.py records from scikit-learn and from the reference's cluster_coord (and where it asserts that
the numpy rule reproduces scikit-learn on every case).  Neither scikit-learn nor the reference is imported here.

Labels and core flags are compared exactly, every row.  Means and variances are compared with the worst-case bound of
a sum of m terms in fp64, (m + 8) * 2^-53 * sum |terms|: the terms of a mean are the x_i / m, those of a variance the
(x_i - mean)^2 / m.  The numpy model (``stats_model``) is the two-pass form of np.mean / np.var with the members added
in table order."""
import math
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
_gold = None
_rule = {}


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLD, "cluster.npz")) as g:
            _gold = {k: g[k] for k in g.files}
    return _gold


def cases():
    """The DBSCAN tables of the golden but the one-row table of check_tiny (the generator lists what it kept)."""
    return [str(n) for n in gold()["names"] if n != "single"]


def case(name):
    g = gold()
    return g[f"{name}|pts"], g[f"{name}|seg"], g[f"{name}|runs"], g[f"{name}|labels"], g[f"{name}|core"]


# ------------------------------------------------------------------------------------------------ the numpy oracle
def neighbours(p, eps):
    """(n, n) bool: dx*dx + dy*dy <= eps*eps in float64, one rounding per operation."""
    dx, dy = p[None, :, 0] - p[:, None, 0], p[None, :, 1] - p[:, None, 1]
    return dx * dx + dy * dy <= eps * eps


def rule(p, eps, ms):
    """DBSCAN labels with scikit-learn's numbering, O(n^2): components of the core-core graph numbered by ascending
    smallest core row; a border row takes the smallest label among its core neighbours; the rest is -1."""
    n = len(p)
    labels = np.full(n, -1, dtype=np.int64)
    if n == 0:
        return labels, np.zeros(0, dtype=bool)
    adj = neighbours(p, eps)
    core = adj.sum(1) >= ms
    k = 0
    for i in range(n):
        if core[i] and labels[i] < 0:
            labels[i] = k
            stack = [i]
            while stack:
                nb = np.nonzero(adj[stack.pop()] & core & (labels < 0))[0]
                labels[nb] = k
                stack.extend(nb.tolist())
            k += 1
    for i in np.nonzero(~core)[0]:
        nb = labels[adj[i] & core]
        if len(nb):
            labels[i] = nb.min()
    return labels, core


def rule_segments(pts, seg, eps, ms):
    parts = [rule(pts[lo:hi], eps, ms) for lo, hi in zip(seg[:-1], seg[1:])]
    if not parts:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    return np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])


def rule_cached(name, r):
    """The rule's answer for run r of a golden case, computed once and shared (never modified)."""
    if (name, r) not in _rule:
        pts, seg, runs = case(name)[:3]
        _rule[(name, r)] = rule_segments(pts, seg, runs[r, 0], int(runs[r, 1]))
    return _rule[(name, r)]


def stats_model(xy):
    """mean, var, bound of the mean, bound of the variance of the (m, 2) rows: two passes, rows added in order."""
    m = len(xy)
    s = np.zeros(2)
    for row in xy:
        s = s + row
    mean = s / m
    v = np.zeros(2)
    for row in xy:
        d = row - mean
        v = v + d * d
    return mean, v / m, (m + 8) * U * np.abs(xy).sum(0) / m, (m + 8) * U * v / m


def dev_pts(p, device):
    return torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64)).to(device)


# ------------------------------------------------------------------------------------------------ 1. dbscan
def check_case(name, device):
    """Cases 2-8 of the golden: labels and core flags of every run equal the rule's and scikit-learn's, every row; the
    cluster statistics agree with the numpy model; the member rows are the rows of each label in table order."""
    from atomai_amd.utils import _cluster
    pts, seg, runs, glabels, gcore = case(name)
    x = dev_pts(pts, device)
    for r, (eps, ms) in enumerate(runs):
        ms = int(ms)
        labels, core, rounds = _cluster.dbscan(x, eps, ms, seg)
        assert labels.dtype == torch.int64 and core.dtype == torch.bool and labels.shape == core.shape == (len(pts),)
        labels, core = labels.cpu().numpy(), core.cpu().numpy()
        rl, rc = rule_cached(name, r)
        print(f"{name}: eps = {eps!r}, min_samples = {ms}: {int(labels.max(initial=-1)) + 1} clusters, "
              f"{int((labels < 0).sum())} noise, {rounds} rounds")
        assert np.array_equal(core, rc) and np.array_equal(core, gcore[r]), (name, eps, ms)
        assert np.array_equal(labels, rl) and np.array_equal(labels, glabels[r].astype(np.int64)), (name, eps, ms)
        if name == "chains":
            # two clusters, the chains, numbered by their smallest row.  On a path the roots that survive a round are
            # the local minima of the current roots along the path, at most every second one: 300 -> 150 -> 75 -> 38 ->
            # 19 -> 10 -> 5 -> 3 -> 2 -> 1 is 9 rounds, and one more finds nothing to hook.  One-hop propagation
            # would need about as many rounds as the chain has points.
            assert labels.max() == 1 and (labels >= 0).all() and sorted(np.bincount(labels)) == [40, 300]
            assert labels[0] == 0 and rounds <= 10, rounds
        check_stats(x, pts, seg, eps, ms, rl)


def check_stats(x, pts, seg, eps, ms, labels):
    from atomai_amd.utils import _cluster
    r = _cluster._run(x, eps, ms, seg)
    kseg, count, mean, var, rows, moff = _cluster.cluster_stats(x, r["labels"], r["rank"], r["seg"])
    count, mean, var, rows, moff = (a.cpu().numpy() for a in (count, mean, var, rows, moff))
    assert mean.dtype == var.dtype == np.float64 and count.dtype == rows.dtype == moff.dtype == np.int64
    k = 0
    for s, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        nk = int(labels[lo:hi].max(initial=-1)) + 1
        assert kseg[s] == k and kseg[s + 1] == k + nk
        for c in range(nk):
            want = lo + np.nonzero(labels[lo:hi] == c)[0]
            assert np.array_equal(rows[moff[k]:moff[k + 1]], want) and count[k] == len(want)
            m, v, bm, bv = stats_model(pts[want])
            assert (np.abs(mean[k] - m) <= bm).all() and (np.abs(var[k] - v) <= bv).all(), (s, c, mean[k] - m, var[k] - v)
            k += 1
    assert k == len(count) == len(mean) == len(var) == len(moff) - 1


def check_tiny(device):
    """Case 1: no rows at all (with and without empty segments), and one row as its own cluster or as noise."""
    from atomai_amd.utils import _cluster
    for seg in (None, [0, 0, 0]):
        labels, core, rounds = _cluster.dbscan(torch.empty((0, 2), dtype=torch.float64, device=device), 1.0, 1, seg)
        assert labels.shape == core.shape == (0,) and labels.dtype == torch.int64 and core.dtype == torch.bool
        assert rounds == 0
    pts, seg, runs, glabels, gcore = case("single")
    for r, want in enumerate((0, -1)):
        labels, core, rounds = _cluster.dbscan(dev_pts(pts, device), runs[r, 0], int(runs[r, 1]))
        assert labels.tolist() == [want] == glabels[r].tolist() and core.tolist() == [want == 0] == gcore[r].tolist()
        assert rounds == 1


def check_segments(device):
    """Case 7: rows of different segments at identical positions do not link, and the segmented call equals one call
    per segment."""
    from atomai_amd.utils import _cluster
    pts, seg, runs = case("segments")[:3]
    eps, ms = runs[0, 0], int(runs[0, 1])
    assert np.array_equal(pts[seg[4]:seg[5]], pts[seg[3]:seg[3] + 64])              # identical positions
    labels, core, _ = _cluster.dbscan(dev_pts(pts, device), eps, ms, seg)
    for lo, hi in zip(seg[:-1], seg[1:]):
        l1, c1, _ = _cluster.dbscan(dev_pts(pts[lo:hi], device), eps, ms)
        assert torch.equal(labels[lo:hi], l1) and torch.equal(core[lo:hi], c1)
    # the 64 rows alone are sparser than among the 300: linking across segments would change their core flags
    assert not np.array_equal(core[seg[4]:seg[5]].cpu().numpy(), core[seg[3]:seg[3] + 64].cpu().numpy())


def check_far_cells(device):
    """Case 8: extent / eps is 1e9 per axis; the grid is sized by the number of rows."""
    from atomai_amd.utils import _cluster
    pts, seg, runs = case("far")[:3]
    assert (pts.max(0) - pts.min(0)).min() / runs[0, 0] > 1e8
    reserved, used = _cluster.grid_cells(dev_pts(pts, device), runs[0, 0], seg)
    print(f"far: {len(pts)} rows, {reserved} cells reserved, {used} used")
    assert 1 <= used <= reserved <= 4 * len(pts)


def check_determinism(device):
    """Case 9: two runs give the same bits in every output."""
    from atomai_amd.utils import _cluster
    pts, seg, runs = case("uniform257")[:3]
    x = dev_pts(pts, device)
    outs = []
    for _ in range(2):
        r = _cluster._run(x, runs[0, 0], int(runs[0, 1]), seg)
        st = _cluster.cluster_stats(x, r["labels"], r["rank"], r["seg"])
        outs.append([r["labels"], r["core"], r["rank"]] + list(st[1:]) + [torch.tensor([r["rounds"]]), torch.from_numpy(st[0])])
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def check_validation(device):
    """Case 12: what dbscan refuses."""
    from atomai_amd.utils import _cluster
    x = torch.zeros((6, 2), dtype=torch.float64, device=device)
    bad = [((x.float(), 1.0, 1), {}), ((torch.zeros((6, 3), dtype=torch.float64, device=device), 1.0, 1), {}),
           ((torch.zeros(6, dtype=torch.float64, device=device), 1.0, 1), {}),
           ((torch.zeros((2, 6), dtype=torch.float64, device=device).t(), 1.0, 1), {}),
           ((x, 0.0, 1), {}), ((x, -1.0, 1), {}), ((x, math.nan, 1), {}), ((x, math.inf, 1), {}),
           ((x, 1.0, 0), {}), ((x, 1.0, 1.5), {}),
           ((x, 1.0, 1), {"seg": [0, 4, 3, 6]}), ((x, 1.0, 1), {"seg": [0, 5]}), ((x, 1.0, 1), {"seg": [1, 6]})]
    for args, kw in bad:
        with pytest.raises(ValueError):
            _cluster.dbscan(*args, **kw)
    labels, core, _ = _cluster.dbscan(x, 1.0, 6, seg=[0, 0, 6, 6])
    assert labels.tolist() == [0] * 6 and core.all()


# ------------------------------------------------------------------------------------------------ 2. public surface
def check_cluster_coord():
    """Case 10: aoi.utils.cluster_coord against what the reference returned: a dictionary with noise points, and one
    without, where np.unique(labels)[1:] drops cluster 0.  The reference returned a float64 (K, 3, 3) array of
    clusters (all of three members; it cannot return clusters of different sizes under numpy >= 1.24); this package
    returns the same rows in an object array, as predictors.epredictor.cluster_coord always has."""
    import atomai_amd as aoi
    g = gold()
    for name in ("noisy", "clean"):
        frames = {f: g[f"cc|{name}|{f}"] for f in range(3)}
        eps, ms = float(g[f"cc|{name}|eps"]), int(g[f"cc|{name}|ms"])
        rc, rm, rv = g[f"cc|{name}|clusters"], g[f"cc|{name}|mean"], g[f"cc|{name}|var"]
        for arg in (frames, [frames[0], frames[1], frames[2]]):
            clusters, mean, var = aoi.utils.cluster_coord(arg, eps, ms)
            assert isinstance(clusters, np.ndarray) and clusters.dtype == object and clusters.shape == rc.shape
            assert np.array_equal(clusters.astype(np.float64), rc)
            assert mean.dtype == var.dtype == np.float64 and mean.shape == rm.shape and var.shape == rv.shape
            for k in range(len(rc)):
                _, _, bm, bv = stats_model(rc[k][:, :2])
                assert (np.abs(mean[k] - rm[k]) <= bm).all() and (np.abs(var[k] - rv[k]) <= bv).all(), (name, k)
        every = np.concatenate([frames[f] for f in range(3)])
        labels, _ = rule(every[:, :2], eps, ms)
        assert len(rc) == labels.max() + 1 - (name == "clean") and ((labels < 0).any() == (name == "noisy"))
    # clusters of different sizes (the reference cannot return these): against the rule and the numpy model
    rng = np.random.default_rng(5)
    tables = [np.concatenate((rng.uniform(0, 9, (n, 2)), rng.integers(0, 2, (n, 1))), axis=1) for n in (40, 0, 55)]
    clusters, mean, var = aoi.utils.cluster_coord(tables, 0.9, 3)
    every = np.concatenate(tables)
    labels, _ = rule(every[:, :2], 0.9, 3)
    ids = np.unique(labels)[1:]
    assert clusters.dtype == object and len(clusters) == len(ids) >= 3 and len({len(c) for c in clusters}) > 1
    for k, lab in enumerate(ids):
        assert np.array_equal(clusters[k], every[labels == lab])
        m, v, bm, bv = stats_model(every[labels == lab][:, :2])
        assert (np.abs(mean[k] - m) <= bm).all() and (np.abs(var[k] - v) <= bv).all()
    assert aoi.predictors.epredictor.cluster_coord(tables, 0.9, 3)[1].tobytes() == mean.tobytes()
    # nothing to cluster: the reference's np.array([]) of shape (0,)
    for arg in ({}, {0: np.empty((0, 3))}, {0: np.array([[1.0, 2.0, 0.0]])}):
        clusters, mean, var = aoi.utils.cluster_coord(arg, 0.5, 3)
        assert clusters.shape == mean.shape == var.shape == (0,)


def check_no_sklearn():
    """The analysis path (predictors, utils) imports scikit-learn nowhere.  (The trainers still take their batch schedule
    and their train / test split from it.)"""
    import re
    import atomai_amd
    root = os.path.dirname(os.path.abspath(atomai_amd.__file__))
    offenders = []
    for sub in ("predictors", "utils"):
        for d, _, files in os.walk(os.path.join(root, sub)):
            for f in files:
                text = open(os.path.join(d, f)).read() if f.endswith(".py") else ""
                if re.search(r"^\s*(from|import)\s+sklearn\b", text, flags=re.M):
                    offenders.append(os.path.relpath(os.path.join(d, f), root))
    assert not offenders, offenders


def check_ensemble_locate():
    """Case 11: 12 members x 3 frames of 48 x 48, four members rolled by one pixel so that the variances are not zero,
    against the rule applied to the Locator's own tables; the three frames together equal each frame alone."""
    import atomai_amd as aoi
    from oracle import locator_oracle as lo
    rs = np.random.RandomState(11)
    frames = lo.synthetic_maps(rs, 3, 48, 48, 2, n_blobs=8)
    stack = np.stack([np.roll(frames, 1 if m % 3 == 0 else 0, axis=2) for m in range(12)])      # (12, 3, 48, 48, 2)
    eps = 1.5
    cm, cv = aoi.predictors.ensemble_locate(stack, eps=eps, threshold=0.5)
    assert sorted(cm) == sorted(cv) == [0, 1, 2]
    nonzero, noise = 0, []
    for i in range(3):
        tables = aoi.predictors.Locator(0.5).run(np.ascontiguousarray(stack[:, i]))
        every = np.concatenate([tables[m] for m in range(12)])
        labels, _ = rule(every[:, :2], eps, 10)
        ids = np.unique(labels)[1:]
        noise.append(bool((labels < 0).any()))
        assert len(ids) >= 2 and cm[i].shape == cv[i].shape == (len(ids), 2) and cm[i].dtype == cv[i].dtype == np.float64
        for k, lab in enumerate(ids):
            m, v, bm, bv = stats_model(every[labels == lab][:, :2])
            assert (np.abs(cm[i][k] - m) <= bm).all() and (np.abs(cv[i][k] - v) <= bv).all(), (i, k)
        nonzero += int((cv[i] > 0).sum())
        m1, v1 = aoi.predictors.ensemble_locate(stack[:, i:i + 1], eps=eps, threshold=0.5)
        assert sorted(m1) == [0] and m1[0].tobytes() == cm[i].tobytes() and v1[0].tobytes() == cv[i].tobytes()
    assert nonzero > 0 and sorted(set(noise)) == [False, True]      # both branches of np.unique(labels)[1:]
