"""Shared bodies of the nearest-neighbour tests (emulator tier on CPU, gpu tier on the MI355X): csrc/knn.hip through the
C ABI against numpy fp64 brute force, and the public functions of atomai_amd.utils against tests/golden/coords.npz, which
tools/make_coords_golden.py records from the reference.  Neither the reference nor scipy is imported here.

Bounds.  Distances: |ours - oracle| <= 4 * 2^-52 * d — either side forms d from three rounded operations per coordinate
pair and a square root, under 2 ulp each, and may or may not contract them into FMAs.  Indices are exact: every
comparison the order depends on is asserted (here for the random inputs, in the generator for the golden) to be decided by
more than 1e-9 relative, six orders above the rounding.  Window means: |ours - oracle| <= r^2 * 2^-52 * max |frame|
(at most r^2 - 1 additions of fp64 and one division on either side, each within 2^-53 of a partial sum <= r^2 max)."""
import hashlib
import os
import warnings

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -52
SIZES = [0, 1, 2, 3, 7, 17, 255, 256, 257, 600]          # reference points per segment, all in ONE launch
QSIZES = [3, 0, 5, 1, 300, 17, 2, 256, 1, 40]           # two-set mode: queries per segment (segment 0 has no points)
KS = [1, 3, 16, 32]
_gold = None
_oracle = {}


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLD, "coords.npz")) as g:
            _gold = {k: g[k] for k in g.files}
    return _gold


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def lattice(n, dim, rng):
    side = int(np.ceil(np.sqrt(max(n, 1))))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n]
    xy = 7.0 * ij + rng.uniform(-0.8, 0.8, (n, 2))
    return xy if dim == 2 else np.concatenate((xy, rng.uniform(-3.0, 3.0, (n, 1))), axis=1)


def sq_dists(q, p):
    """(len(q), len(p)) squared distances in float64, the coordinates added in order, one rounding per operation."""
    acc = np.zeros((len(q), len(p)))
    for c in range(q.shape[1]):
        t = p[None, :, c] - q[:, None, c]
        acc = acc + t * t
    return acc


def close(ours, ref):
    """|ours - ref| <= 4 * 2^-52 * ref elementwise, with inf == inf."""
    fin = np.isfinite(ref)
    return np.array_equal(np.isfinite(ours), fin) and (np.abs(ours[fin] - ref[fin]) <= 4 * EPS * ref[fin]).all()


# ------------------------------------------------------------------------------------------------ 1. amx_knn
def knn_oracle(dim, mode):
    """Inputs and the brute-force answer for k = 32, computed once per (dim, mode) and shared (never modified)."""
    key = (dim, mode)
    if key in _oracle:
        return _oracle[key]
    rng = np.random.default_rng(10 * dim + (mode == "two"))
    pseg = np.concatenate(([0], np.cumsum(SIZES)))
    pts = np.concatenate([lattice(n, dim, rng) for n in SIZES])
    if mode == "self":
        qseg, qry = pseg, pts
    else:
        qseg = np.concatenate(([0], np.cumsum(QSIZES)))
        qry = np.concatenate([lattice(n, dim, rng) + rng.uniform(-2, 2, dim) for n in QSIZES])
    Q = len(qry)
    dist, idx = np.full((Q, 32), np.inf), np.full((Q, 32), -1, dtype=np.int64)
    worst = np.inf
    for s in range(len(SIZES)):
        p, q = pts[pseg[s]:pseg[s + 1]], qry[qseg[s]:qseg[s + 1]]
        if not len(p) or not len(q):
            continue
        q2 = sq_dists(q, p)
        order = np.argsort(q2, axis=1, kind="stable")[:, :33]
        srt = np.take_along_axis(q2, order, 1)
        if srt.shape[1] >= 2:                                     # every comparison is decided far above the rounding
            worst = min(worst, float(((srt[:, 1:] - srt[:, :-1]) / srt[:, 1:]).min()))
        m = min(32, len(p))
        dist[qseg[s]:qseg[s + 1], :m] = np.sqrt(srt[:, :m])
        idx[qseg[s]:qseg[s + 1], :m] = order[:, :m] + pseg[s]
    assert worst > 1e-9, (key, worst)
    _oracle[key] = dict(pts=pts, qry=qry, pseg=pseg, qseg=qseg, dist=dist, idx=idx, worst=worst)
    return _oracle[key]


def call_knn(pts, qry, pseg, qseg, k, bound, device):
    """amx_knn through the C ABI; every output element starts as a sentinel that the kernel must overwrite."""
    from atomai_amd import _lib as L
    from atomai_amd.utils import _knn
    P, Q, dim = len(pts), len(qry), qry.shape[1]
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(device)
         for a in (pts, qry, np.asarray(pseg, np.int64), np.asarray(qseg, np.int64), _knn.tile_table(qseg))]
    dist = torch.full((Q, k), -7.0, dtype=torch.float64, device=device)
    idx = torch.full((Q, k), -7, dtype=torch.int64, device=device)
    L.call("amx_knn", L.ptr(t[0]), P, L.ptr(t[1]), Q, dim, L.ptr(t[2]), L.ptr(t[3]), len(qseg) - 1, L.ptr(t[4]),
           len(t[4]), k, float(bound), L.ptr(dist), L.ptr(idx), L.stream_ptr(t[1]))
    return dist.cpu().numpy(), idx.cpu().numpy()


def check_knn(dim, k, mode, device):
    o = knn_oracle(dim, mode)
    dist, idx = call_knn(o["pts"], o["qry"], o["pseg"], o["qseg"], k, np.inf, device)
    rd, ri = o["dist"][:, :k], o["idx"][:, :k]
    fin = np.isfinite(rd)
    err = np.abs(dist[fin] - rd[fin]) / np.where(rd[fin] > 0, rd[fin], 1.0)
    print(f"knn dim {dim} k {k} {mode}: {len(rd)} queries, {int((~fin).sum())} empty slots, max relative error "
          f"{err.max() / EPS:.2f} * 2^-52, smallest gap of the inputs {o['worst']:.2e}")
    assert dist.shape == rd.shape and idx.shape == ri.shape
    assert np.array_equal(idx, ri)                                 # empty slots are -1 in both
    assert np.array_equal(np.isinf(dist), ~fin) and (dist[~fin] > 0).all()
    assert close(dist, rd)
    assert (np.diff(dist[:, :][np.isfinite(dist).all(1)], axis=1) >= 0).all()
    if mode == "self":
        assert np.array_equal(idx[fin[:, 0], 0], np.nonzero(fin[:, 0])[0]) and (dist[fin[:, 0], 0] == 0).all()


def check_knn_bound_and_ties(device):
    """Four points at exactly 5 from the first (sums 9 + 16 and 25 + 0 are exact): ordered by row; bound 5.0 excludes
    them (d < bound, strictly), nextafter(5.0) includes them.  A second segment is out of reach of the first."""
    pts = np.array([[0, 0], [3, 4], [5, 0], [0, 5], [-4, 3], [10, 10], [0.5, 0.5], [0, 1]], dtype=np.float64)
    pseg = [0, 6, 8]
    for order in (np.arange(6), np.array([0, 4, 3, 2, 1, 5])):
        p = np.concatenate((pts[order], pts[6:]))
        dist, idx = call_knn(p, p, pseg, pseg, 6, np.inf, device)
        assert np.array_equal(idx[0], [0, 1, 2, 3, 4, 5]) and np.array_equal(dist[0, :5], [0, 5, 5, 5, 5])
        assert np.array_equal(idx[6], [6, 7, -1, -1, -1, -1]) and np.isinf(dist[6, 2:]).all()
        dist, idx = call_knn(p, p[:1], pseg, [0, 1, 1], 5, 5.0, device)
        assert np.array_equal(idx[0], [0, -1, -1, -1, -1]) and np.isinf(dist[0, 1:]).all()
        dist, idx = call_knn(p, p[:1], pseg, [0, 1, 1], 5, np.nextafter(5.0, 6.0), device)
        assert np.array_equal(idx[0], [0, 1, 2, 3, 4]) and np.array_equal(dist[0], [0, 5, 5, 5, 5])
    # 600 points on the integer line: both neighbours of every point are at exactly 1, 2, ... and for rows 255 / 256 /
    # 511 / 512 the two lie in DIFFERENT LDS tiles, whatever order the tiles are visited in
    line = np.stack((np.arange(600.0), np.zeros(600)), 1)
    want = np.argsort(sq_dists(line, line), axis=1, kind="stable")[:, :5]
    assert np.array_equal(want[256], [256, 255, 257, 254, 258])
    dist, idx = call_knn(line, line, [0, 600], [0, 600], 5, np.inf, device)
    assert np.array_equal(idx, want) and np.array_equal(dist[2:-2], np.tile([0.0, 1, 1, 2, 2], (596, 1)))
    o = knn_oracle(2, "self")                                      # a bound inside the neighbour shells
    dist, idx = call_knn(o["pts"], o["qry"], o["pseg"], o["qseg"], 16, 9.0, device)
    rd, ri = o["dist"][:, :16], o["idx"][:, :16]
    assert (np.abs(o["dist"] - 9.0) > 1e-9 * 9.0).all()
    inside = rd < 9.0
    assert 0.1 < inside.mean() < 0.9
    assert np.array_equal(idx, np.where(inside, ri, -1)) and close(dist, np.where(inside, rd, np.inf))


# ------------------------------------------------------------------------------------------------ 2. radius query
def check_radius(dim, device):
    from atomai_amd.utils import _knn
    rng = np.random.default_rng(40 + dim)
    base = lattice(300, dim, rng)
    pts = np.concatenate([base + rng.normal(0, 0.4, base.shape) for _ in range(3)])[rng.permutation(900)[:700]]
    qry = np.concatenate((base, np.full((1, dim), 500.0)))         # 301 queries: two workgroups; the last finds nothing
    rmax = 8.0
    q2 = sq_dists(qry, pts)
    d = np.sqrt(q2)
    assert (np.abs(d - rmax) > 1e-9 * rmax).all()
    order = np.argsort(q2, axis=1, kind="stable")
    srt = np.take_along_axis(q2, order, 1)[:, :40]
    assert ((srt[:, 1:] - srt[:, :-1]) / srt[:, 1:]).min() > 1e-9 and (np.sqrt(srt[:, -1]) > rmax).all()
    want_count = (d < rmax).sum(1)
    want_idx = np.concatenate([order[i, :c] for i, c in enumerate(want_count)])
    want_dist = np.concatenate([d[i, order[i, :c]] for i, c in enumerate(want_count)])
    runs = []
    for _ in range(2):
        got = _knn.radius(*(torch.from_numpy(a).to(device) for a in (pts, qry)), rmax)
        runs.append([g.cpu().numpy() for g in got])
    count, idx, dist = runs[0]
    print(f"radius dim {dim}: {len(qry)} queries, {len(pts)} points, {int(want_count.sum())} pairs, counts "
          f"{want_count.min()} .. {want_count.max()}")
    assert want_count[-1] == 0 and want_count.max() >= 8
    assert count.dtype == np.int64 and np.array_equal(count, want_count)
    assert idx.dtype == np.int64 and np.array_equal(idx, want_idx)          # the sets AND the order by distance
    assert close(dist, want_dist)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------ 3. window mean
def window_model(frames, coords, fidx, r):
    """numpy's slicing on the float64 copy of the frame; a negative start is NaN (there the reference's slice wraps to
    an empty one), as is a frame index out of range."""
    out = np.full(len(coords), np.nan)
    for i, ((row, col), f) in enumerate(zip(coords, fidx)):
        cx, cy, h = int(np.around(row)), int(np.around(col)), r // 2
        if cx - h < 0 or cy - h < 0 or not 0 <= f < len(frames):
            continue
        win = frames[f].astype(np.float64)[cx - h:cx + h + r % 2, cy - h:cy + h + r % 2]
        if win.size:
            out[i] = win.mean()
    return out


def check_window_mean(r, device):
    from atomai_amd.utils import _knn
    rng = np.random.default_rng(7)
    B, H, W = 2, 19, 23
    frames = rng.uniform(-1, 1, (B, H, W)).astype(np.float32)
    inner = np.stack((rng.uniform(-1.4, H + 1.4, 280), rng.uniform(-1.4, W + 1.4, 280)), 1)   # 300 atoms: two workgroups
    assert (np.abs(inner % 1.0 - 0.5) > 1e-9).all()
    planted = np.array([[0.5, 1.5], [2.5, 3.5], [9.5, 10.5], [H - 0.5, W - 0.5], [H - 1.5, W - 2.5], [0.0, 0.0],
                        [H - 1.0, W - 1.0], [float(H), float(W)], [H + 30.0, 4.0], [-0.5, 8.0], [-40.0, -40.0],
                        [np.nan, 3.0], [1e300, 2.0], [5.0, 6.0], [5.0, 6.0], [4.0, np.inf], [7.2, 7.7], [3.3, 1.1],
                        [6.0, 0.49], [0.49, 6.0]])
    coords = np.concatenate((inner, planted))
    fidx = rng.integers(0, B, len(coords))
    fidx[[-7, -6]] = [-1, B]                                       # frame index out of range: NaN
    ok = np.isfinite(coords).all(1) & (np.abs(coords) < 1e9).all(1)
    want = np.full(len(coords), np.nan)
    want[ok] = window_model(frames, coords[ok], fidx[ok], r)
    meta = np.zeros((len(coords), 2), dtype=np.int32)
    meta[:, 0] = fidx
    got = _knn.window_mean(*(torch.from_numpy(a).to(device) for a in (frames, coords, meta)), r).cpu().numpy()
    fin = np.isfinite(want)
    bound = r * r * EPS * float(np.abs(frames).max())
    err = np.abs(got[fin] - want[fin]).max()
    print(f"window mean r {r}: {int(fin.sum())} finite, {int((~fin).sum())} NaN, max error {err:.3e}, bound {bound:.3e}")
    assert got.dtype == np.float64 and 20 < (~fin).sum() < 200
    assert np.array_equal(np.isnan(got), ~fin) and err <= bound


# ------------------------------------------------------------------------------------------------ 4. public functions
def nn_frames():
    g = gold()
    return {f: g[f"nn|coords|{f}"] for f in range(len(g["nn|sizes"]))}


def reference_nn(nn, ub=False):
    """The reference's get_nn_distances output, rebuilt from the stored neighbour rows and VERIFIED against the digests
    of the arrays the reference returned: past the two assertions these lists are the reference's output bit for bit."""
    g = gold()
    ds, ps = [], []
    for f, t in nn_frames().items():
        if ub:
            ix = g[f"nn|ub|idx|{f}"].astype(np.int64)
        elif f"nn|idx|{f}" in g and g[f"nn|idx|{f}"].shape[1] >= nn + 1:
            ix = g[f"nn|idx|{f}"][:, :nn + 1].astype(np.int64)
        else:
            ix = np.empty((0, nn + 1), dtype=np.int64)
        p = t[ix]
        dx, dy = p[:, 1:, 0] - p[:, :1, 0], p[:, 1:, 1] - p[:, :1, 1]
        ds.append(np.sqrt(dx * dx + dy * dy))
        ps.append(p)
    digest = g["nn|ub|sha"] if ub else g[f"nn|sha|{nn}"]
    assert sha(np.concatenate(ds)) == digest[0] and sha(np.concatenate(ps)) == digest[1]
    return ds, ps


def _assert_nn(got, want, what):
    (gd, gp), (wd, wp) = got, want
    assert len(gd) == len(gp) == len(wd)
    for f, (a, b, c, d) in enumerate(zip(gd, wd, gp, wp)):
        assert a.shape == b.shape and a.dtype == np.float64, (what, f, a.shape, b.shape)       # same dropped rows
        assert c.shape == d.shape and c.dtype == d.dtype and np.array_equal(c, d), (what, f)   # gathered: exact
        assert close(a, b), (what, f)


def check_get_nn_distances(nn):
    import atomai_amd as aoi
    frames = nn_frames()
    want = reference_nn(nn)
    got = aoi.utils.get_nn_distances(frames, nn)
    kept = sum(len(d) for d in got[0])
    print(f"get_nn_distances nn {nn}: {kept} rows in {sum(1 for d in got[0] if len(d))} non-empty frames")
    _assert_nn(got, want, f"nn {nn}")
    assert got[0][0].shape == (0, nn) and got[1][0].shape == (0, nn + 1, 3)      # the empty dictionary entry
    f = 5 if nn <= 15 else 6
    _assert_nn(tuple([x] for x in aoi.utils.get_nn_distances_(frames[f], nn)), ([want[0][f]], [want[1][f]]), "single")
    _assert_nn(aoi.utils.get_nn_distances(frames[f], nn), ([want[0][f]], [want[1][f]]), "array")
    bonds = aoi.utils.map_bonds(frames, nn, plot_results=False)
    assert bonds.tobytes() == np.concatenate(got[0]).tobytes()


def check_get_nn_distances_upper_bound():
    import atomai_amd as aoi
    g = gold()
    nn, ub = int(g["nn|ub|nn"]), float(g["nn|ub|bound"])
    frames = nn_frames()
    want = reference_nn(nn, ub=True)
    got = aoi.utils.get_nn_distances(frames, nn, ub)
    _assert_nn(got, want, "upper bound")
    for f, t in frames.items():                                    # the same rows dropped
        assert np.array_equal(got[1][f][:, 0], t[g[f"nn|ub|keep|{f}"]])
    n_big = sum(len(frames[f]) for f in (6, 7, 8, 9))
    assert 0 < sum(len(got[0][f]) for f in (6, 7, 8, 9)) < n_big
    bonds = aoi.utils.map_bonds(frames, nn, ub, plot_results=False)
    assert bonds.tobytes() == np.concatenate(got[0]).tobytes()


def check_compare_coordinates():
    import atomai_amd as aoi
    g = gold()
    o1, o2, dr = aoi.utils.compare_coordinates(g["cmp|c1"], g["cmp|c2"], float(g["cmp|d_max"]))
    print(f"compare_coordinates: {len(dr)} of {len(g['cmp|c1'])} matched")
    assert o1.dtype == o2.dtype == dr.dtype == np.float64 and dr.shape == g["cmp|dr"].shape
    assert np.array_equal(o1, g["cmp|o1"]) and np.array_equal(o2, g["cmp|o2"]) and close(dr, g["cmp|dr"])
    none = aoi.utils.compare_coordinates(g["cmp|c1"], g["cmp|c2"][:0], 1.0)
    assert none[0].shape == none[1].shape == (0, 3) and none[2].shape == (0,)
    kept = aoi.utils.remove_edge_coord(g["cmp|c2"], tuple(g["edge|dim"]), int(g["edge|dist"]))
    assert np.array_equal(kept, g["edge|out"])


def check_find_coord_clusters():
    import atomai_amd as aoi
    g = gold()
    movie = {f: g[f"fcc|{f}"] for f in range(3)}
    scale = max(np.abs(t).max() for t in movie.values())
    for second in (movie, [movie[f] for f in range(3)]):
        means, stds, clusters = aoi.utils.find_coord_clusters({0: g["fcc|first"]}, second, float(g["fcc|rmax"]))
        assert np.array_equal([len(c) for c in clusters], g["fcc|counts"])
        assert np.array_equal(np.concatenate(clusters), g["fcc|members"])        # members AND their order by distance
        for a, b in ((means, g["fcc|means"]), (stds, g["fcc|stds"])):
            assert a.shape == b.shape and a.dtype == np.float64 and np.array_equal(np.isnan(a), np.isnan(b))
            assert (np.abs(a - b)[~np.isnan(b)] <= 4 * EPS * scale).all()
    assert np.isnan(means[-1]).all() and clusters[-1].shape == (0, 3)


def check_get_intensities(r):
    import atomai_amd as aoi
    g = gold()
    frames, keys = g["int|frames"], [int(k) for k in g["int|keys"]]
    tables = {k: g[f"int|coords|{k}"] for k in keys}
    bound = r * r * EPS * float(np.abs(frames).max())
    for stack in (frames, frames[..., None]):
        got = aoi.utils.get_intensities(tables, stack, r)
        assert len(got) == len(keys)
        for k, a in zip(keys, got):
            b = g[f"int|out|{r}|{k}"]
            assert a.shape == b.shape and a.dtype == np.float64 and np.array_equal(np.isnan(a), np.isnan(b)), (r, k)
            assert (np.abs(a - b)[~np.isnan(b)] <= bound).all(), (r, k)
    k = keys[0]
    one = aoi.utils.get_intensities_(tables[k], frames[k][..., None], r)
    assert one.tobytes() == got[0].tobytes()
    print(f"get_intensities r {r}: {sum(int(np.isnan(a).sum()) for a in got)} NaN of {sum(len(a) for a in got)}")


# ------------------------------------------------------------------------------------------------ 5. determinism
def check_determinism(device):
    o = knn_oracle(3, "two")
    a = call_knn(o["pts"], o["qry"], o["pseg"], o["qseg"], 16, 30.0, device)
    b = call_knn(o["pts"], o["qry"], o["pseg"], o["qseg"], 16, 30.0, device)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    import atomai_amd as aoi
    frames = nn_frames()
    x, y = aoi.utils.get_nn_distances(frames, 6), aoi.utils.get_nn_distances(frames, 6)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x[0] + x[1], y[0] + y[1]))


# ------------------------------------------------------------------------------------------------ 6. edges
def check_edges(device):
    import atomai_amd as aoi
    from atomai_amd import _lib as L
    from atomai_amd.utils import _knn
    frames = nn_frames()
    d, p = aoi.utils.get_nn_distances_(frames[3], 6)               # 3 atoms, 7 wanted: every row drops
    assert d.shape == (0, 6) and p.shape == (0, 7, 3) and d.dtype == p.dtype == np.float64
    d, p = aoi.utils.get_nn_distances({4: frames[0], 9: frames[2]}, 1)       # an empty entry, any keys
    assert d[0].shape == (0, 1) and p[0].shape == (0, 2, 3) and d[1].shape == (2, 1) and p[1].shape == (2, 2, 3)
    d, p = aoi.utils.get_nn_distances({0: frames[0]}, 2)           # nothing to launch
    assert d[0].shape == (0, 2) and p[0].shape == (0, 3, 3)
    assert aoi.utils.get_nn_distances_(frames[5], 31)[0].shape == (0, 31)        # nn + 1 = 32 is the last allowed
    with pytest.raises(ValueError, match="32"):
        aoi.utils.get_nn_distances(frames, 32)
    with pytest.raises(ValueError, match="32"):
        aoi.utils.map_bonds(frames, 40, plot_results=False)
    four = np.zeros((5, 4))
    with pytest.raises(ValueError, match="dim 2 or 3"):
        aoi.utils.compare_coordinates(four, four, 1.0)
    t4 = torch.zeros(5, 4, dtype=torch.float64, device=device)
    with pytest.raises(ValueError, match="dim 2 or 3"):
        _knn.knn(t4, t4, 1)
    with pytest.raises(ValueError, match="dim 2 or 3"):
        _knn.radius(t4, t4, 1.0)
    t2 = torch.zeros(5, 2, dtype=torch.float64, device=device)
    with pytest.raises(ValueError, match="32"):
        _knn.knn(t2, t2, 33)
    seg = torch.tensor([0, 5], dtype=torch.int64, device=device)
    tiles = torch.tensor([[0, 0]], dtype=torch.int64, device=device)
    dist = torch.zeros(5, 33, dtype=torch.float64, device=device)
    idx = torch.zeros(5, 33, dtype=torch.int64, device=device)
    for dim, k in ((4, 1), (1, 1), (2, 0), (2, 33)):               # the C ABI refuses them too
        with pytest.raises(L.AmxError, match="bad argument"):
            L.call("amx_knn", L.ptr(t2), 5, L.ptr(t2), 5, dim, L.ptr(seg), L.ptr(seg), 1, L.ptr(tiles), 1, k, np.inf,
                   L.ptr(dist), L.ptr(idx), L.stream_ptr(t2))
    with pytest.raises(L.AmxError, match="bad argument"):
        L.call("amx_knn", L.ptr(t2), -1, L.ptr(t2), 5, 2, L.ptr(seg), L.ptr(seg), 1, L.ptr(tiles), 1, 1, np.inf,
               L.ptr(dist), L.ptr(idx), L.stream_ptr(t2))
    with pytest.raises(L.AmxError, match="bad argument"):
        L.call("amx_knn", L.ptr(t2), 5, L.ptr(t2), 5, 2, None, L.ptr(seg), 1, L.ptr(tiles), 1, 1, np.inf,
               L.ptr(dist), L.ptr(idx), L.stream_ptr(t2))
    L.call("amx_knn", None, 0, None, 0, 2, None, None, 0, None, 0, 1, np.inf, None, None, L.stream_ptr(t2))    # Q == 0
    d0, i0 = _knn.knn(t2[:0], t2, 2)                               # queries but no points: every slot is empty
    assert torch.isinf(d0).all() and (i0 == -1).all() and d0.shape == (5, 2)
    d0, i0 = _knn.knn(t2, t2[:0], 2)
    assert d0.shape == (0, 2) and i0.shape == (0, 2)
    c, i, d = _knn.radius(t2, t2[:0], 1.0)
    assert c.shape == (0,) and i.shape == (0,) and d.shape == (0,)
    frame = np.zeros((8, 9), dtype=np.float32)
    with pytest.raises(ValueError, match="2-D"):
        aoi.utils.get_intensities_(np.array([[3.0, 3.0, 0.0]]), np.zeros((8, 9, 3)), 3)
    with pytest.raises(ValueError):
        aoi.utils.get_intensities_(np.array([[3.0, 3.0, 0.0]]), frame, 0)
    assert aoi.utils.get_intensities_(np.empty((0, 3)), frame, 3).shape == (0,)
    assert aoi.utils.get_intensities({1: np.empty((0, 3))}, {1: frame}, 3)[0].shape == (0,)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m, s, c = aoi.utils.find_coord_clusters({0: np.array([[50.0, 50.0, 0.0]])}, {0: frames[4]}, 1.0)
    assert np.isnan(m).all() and m.shape == s.shape == (1, 2) and c[0].shape == (0, 3)
    for name in ("get_nn_distances", "get_nn_distances_", "map_bonds", "compare_coordinates", "find_coord_clusters",
                 "get_intensities", "get_intensities_", "remove_edge_coord"):
        assert name in aoi.utils.__all__
