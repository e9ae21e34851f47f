"""Shared bodies of the intensity-class tests (emulator tier on CPU, gpu tier on the MI355X): csrc/intensity.hip through
atomai_amd.stat._intensity / atomai_amd.stat.intensity against a plain-numpy restatement of the three rules and against
tests/golden/classes.npz, which tools/make_classes_golden.py records from scikit-learn and from the reference's
update_classes (and where it asserts that the restatement reproduces scikit-learn's labels, centre counts and n_iter_ on
every case).  Neither scikit-learn nor the reference is imported here.

The restatement adds every range sum in the order the kernels document (``range_sum``: 256 strided partials, then
halving), so kernel and restatement are expected to agree to the bit; integers (counts, iterations, labels) and the gap
rows are compared exactly, sums within n * 2^-52 relative, the bound on re-ordering a sum of n same-sign fp64 terms.
Against the golden, bandwidths and centres are compared within max(1000 x the recorded distance between restatement and
scikit-learn, n * 2^-52) relative (the recorded distance is exactly 0 on some cases)."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -52
T = 256
QUANTILES = (0.1, 0.25, 0.5, 1.0)
_gold = None
_memo = {}


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLD, "classes.npz")) as g:
            _gold = {k: g[k] for k in g.files}
    return _gold


def cases():
    return [str(n) for n in gold()["names"]]


def km_cases():
    return [str(n) for n in gold()["km|names"]]


# ------------------------------------------------------------------------------------------------ the numpy restatement
def wg_sum(v):
    """256 values added by halving: p[t] += p[t + w], w = 128 .. 1."""
    p = np.array(v, dtype=np.float64)
    w = T // 2
    while w >= 1:
        p[:w] = p[:w] + p[w:2 * w]
        w //= 2
    return p[0]


def range_sum(xs, lo=0, hi=None):
    """Sum of xs[lo:hi] in the kernels' order: partial t adds rows lo + t, lo + t + 256, ... in turn."""
    v = np.asarray(xs, dtype=np.float64)[lo:hi]
    pad = np.zeros(-(-max(len(v), 1) // T) * T)
    pad[:len(v)] = v
    acc = np.zeros(T)
    for row in pad.reshape(-1, T):
        acc = acc + row
    return wg_sum(acc)


def gap_rule(xs, K):
    """gap[i]: distance from xs[i] to its K-th nearest value of the sorted xs (itself at 0): the minimum over the windows
    [l, l + K - 1] that contain i of the larger distance to a window end."""
    n = len(xs)
    out = np.empty(n)
    for i in range(n):
        l = np.arange(max(0, i - K + 1), min(i, n - K) + 1)
        out[i] = np.min(np.maximum(xs[i] - xs[l], xs[l + K - 1] - xs[i]))
    return out


def gap_mean(gap):
    n = len(gap)
    partial = [range_sum(gap, a, min(a + T, n)) for a in range(0, n, T)]
    return range_sum(partial) / n


def bandwidth_rule(x, quantile):
    x = np.asarray(x, dtype=np.float64)
    return gap_mean(gap_rule(np.sort(x), max(int(len(x) * quantile), 1)))


def seeds_rule(x, bw):
    """MeanShift(bin_seeding=True): the occupied bins of width bw in the order of their first rows, as float32, times bw;
    the data if every row has a bin of its own."""
    bins, first = np.unique(np.round(x / bw), return_index=True)
    return x.copy() if len(bins) == len(x) else bins[np.argsort(first)].astype(np.float32).astype(np.float64) * bw


def seed_rule(xs, m, bw, max_iter):
    """_mean_shift_single_seed on the sorted column: (mean, members of the last range, completed iterations)."""
    it = 0
    while True:
        inside = np.abs(xs - m) <= bw
        cnt = int(inside.sum())
        if cnt == 0:
            break
        lo = int(np.argmax(inside))
        old, m = m, range_sum(xs, lo, lo + cnt) / cnt
        if abs(m - old) <= 1e-3 * bw or it == max_iter:
            break
        it += 1
    return m, cnt, it


def unique_rule(centre, count, bw):
    found = {}
    for c, m in zip(centre, count):
        if m > 0:
            found[float(c)] = int(m)                                       # a later seed overwrites, as in scikit-learn
    c = np.array([v for v, _ in sorted(found.items(), key=lambda t: (t[1], t[0]), reverse=True)])
    keep = np.ones(len(c), dtype=bool)
    for i in range(len(c)):
        if keep[i]:
            keep[np.abs(c - c[i]) <= bw] = False
            keep[i] = True
    return c[keep]


def assign_rule(x, centres):
    return np.argmin(np.abs(np.asarray(x)[:, None] - np.asarray(centres)[None, :]), axis=1)


def ms_rule(x, bw, max_iter=300):
    """(centres, labels, n_iter) of MeanShift(bandwidth=bw, bin_seeding=True)."""
    x = np.asarray(x, dtype=np.float64)
    xs = np.sort(x)
    res = [seed_rule(xs, m, bw, max_iter) for m in seeds_rule(x, bw)]
    centres = unique_rule([r[0] for r in res], [r[1] for r in res], bw)
    return centres, assign_rule(x, centres), max(r[2] for r in res)


def lloyd_rule(xs, centres, tol, max_iter):
    """Lloyd's algorithm on the sorted column, cut at the midpoints of the centres sorted by (value, index); a row on a
    midpoint goes to the lower-numbered centre; an empty range keeps its centre.  Returns (centres, rounds)."""
    c = np.array(centres, dtype=np.float64)
    k, n = len(c), len(xs)
    prev, it = None, 0
    while it < max_iter:
        order = sorted(range(k), key=lambda a: (c[a], a))
        cut = [0]
        for l, u in zip(order[:-1], order[1:]):
            mid = (c[l] + c[u]) * 0.5
            upper = (xs > mid) | ((xs == mid) & (u < l))
            cut.append(max(int(np.argmax(upper)) if upper.any() else n, cut[-1]))
        cut.append(n)
        ranges = {a: (cut[j], cut[j + 1]) for j, a in enumerate(order)}
        new = np.array([range_sum(xs, *ranges[a]) / (ranges[a][1] - ranges[a][0]) if ranges[a][1] > ranges[a][0] else c[a]
                        for a in range(k)])
        shift = 0.0
        for d in new - c:
            shift += d * d
        c, it = new, it + 1
        if ranges == prev or shift <= tol:
            break
        prev = ranges
    return c, it


def spread_start(x, k):
    """k starting centres spread over the sorted column (the tool's and the tests' common start)."""
    xs = np.sort(x)
    return xs[[(2 * j + 1) * len(xs) // (2 * k) for j in range(k)]]


def match_partition(a, b):
    """The bijection that maps labels a onto labels b (asserted to exist)."""
    pairs = set(zip(a.tolist(), b.tolist()))
    assert len(pairs) == len({p for p, _ in pairs}) == len({q for _, q in pairs}), sorted(pairs)
    return dict(pairs)


def rel(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny), initial=0.0))


def memo(key, fn):
    """A reference computed once and shared among the tests (never modified)."""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def dev(a, device, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


def runs(name):
    """(j, quantile, K, golden bandwidth) of every run of a golden case."""
    g = gold()
    n = len(g[f"{name}|x"])
    return [(j, q, max(int(n * q), 1), float(g[f"{name}|{j}|bw"])) for j, q in enumerate(QUANTILES)]


# ------------------------------------------------------------------------------------------------ 1. kernels
def check_gap(name, device):
    """amx_kth_gap_1d on every run of a golden case: the gap row for row (exact) and the mean."""
    from atomai_amd.stat import _intensity as I
    x = gold()[f"{name}|x"]
    xs = np.sort(x)
    n = len(x)
    for j, q, K, gbw in runs(name):
        gap, mean = I.kth_gap(dev(xs, device), K)
        want = memo(("gap", name, K), lambda: gap_rule(xs, K))
        wmean = gap_mean(want)
        err = rel(float(mean), wmean) if wmean else abs(float(mean))
        print(f"gap {name} q {q} K {K}: rows equal {np.array_equal(gap.cpu().numpy(), want)}, mean {float(mean)!r}, "
              f"rel. distance to the restatement {err:.2e}, to scikit-learn {rel(float(mean), gbw) if gbw else 0.0:.2e}")
        assert np.array_equal(gap.cpu().numpy(), want)
        assert err <= n * EPS
        assert (float(mean) == 0.0) == (gbw == 0.0)
    assert K == n                                                          # quantile 1.0: the end of the search range


def check_seeds(name, device):
    """amx_meanshift_1d on the seeds of every run with a bandwidth, plus two seeds far outside the data; max_iter 300, 0
    and 1: centres, member counts and completed iterations."""
    from atomai_amd.stat import _intensity as I
    x = gold()[f"{name}|x"]
    xs = np.sort(x)
    n = len(x)
    for j, q, K, bw in runs(name):
        if bw == 0.0:
            continue
        span = xs[-1] - xs[0] + 10.0 * bw
        seeds = np.concatenate((seeds_rule(x, bw), [xs[0] - span, xs[-1] + span]))
        for max_iter in (300, 0, 1):
            centre, count, iters = (a.cpu().numpy() for a in I.meanshift(dev(xs, device), dev(seeds, device), bw, max_iter))
            want = memo(("seeds", name, j, max_iter), lambda: [seed_rule(xs, m, bw, max_iter) for m in seeds])
            wc, wn, wi = (np.array(col) for col in zip(*want))
            err = rel(centre, wc)
            print(f"meanshift {name} q {q} max_iter {max_iter}: {len(seeds)} seeds, iterations up to {iters.max()}, "
                  f"centres rel. distance to the restatement {err:.2e}")
            assert np.array_equal(count, wn) and np.array_equal(iters, wi)
            assert err <= n * EPS
            assert count[-2:].tolist() == [0, 0] and iters[-2:].tolist() == [0, 0]
            assert np.array_equal(centre[-2:], seeds[-2:]) and iters.max() <= max_iter


def check_lloyd(device):
    """amx_lloyd_1d from given starting centres: the k-means cases of the golden from a spread start, a row exactly on a
    midpoint (both numberings of the two centres), a start that leaves a cluster empty, max_iter 1."""
    from atomai_amd.stat import _intensity as I
    g = gold()

    def both(xs, start, tol, max_iter, what):
        c, it = I.lloyd(dev(xs, device), dev(start, device), tol, max_iter)
        wc, wit = lloyd_rule(xs, start, tol, max_iter)
        err = rel(c.cpu().numpy(), wc)
        print(f"lloyd {what}: {int(it)} rounds, centres rel. distance to the restatement {err:.2e}")
        assert int(it) == wit and err <= len(xs) * EPS
        return c.cpu().numpy(), int(it)

    for name in km_cases():
        x, k = g[f"{name}|x"], int(g[f"km|{name}|k"])
        xs = np.sort(x)
        tol = float(np.var(x)) * 1e-4
        both(xs, spread_start(x, k), tol, 300, f"{name} k {k}")
        both(xs, spread_start(x, k), tol, 1, f"{name} k {k} max_iter 1")
    mid = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    c, it = both(mid, [0.25, 0.75], 0.0, 300, "row on the midpoint")
    assert c.tolist() == [0.25, 0.875] and it == 2                         # 0.5 went to centre 0, the lower one
    c, it = both(mid, [0.75, 0.25], 0.0, 300, "row on the midpoint, centres swapped")
    assert c.tolist() == [0.75, 0.125] and it == 2                         # 0.5 went to centre 0, the upper one
    x = g["three|x"]
    xs = np.sort(x)
    c, it = both(xs, [0.2, 100.0, 0.6], 0.0, 300, "a cluster left empty")
    assert c[1] == 100.0 and it > 2 and 0.0 < c[0] < c[2] < 1.0             # centre 1 never had a row and stayed


def check_assign(device):
    """amx_assign_1d: a tie goes to the first centre; 40 centres; more centres than one LDS chunk holds (1030)."""
    from atomai_amd.stat import _intensity as I
    for centres in ([0.25, 0.75], [0.75, 0.25]):
        lab = I.assign(dev([0.5, 0.25, 0.75, 0.5], device), dev(centres, device)).cpu().numpy()
        assert lab.tolist() == assign_rule([0.5, 0.25, 0.75, 0.5], centres).tolist() and lab[0] == lab[3] == 0
    x = gold()["uniform257|x"]
    x = np.concatenate((x, x[:100] + 1.0))                                 # 357 rows: two workgroups
    for C in (1, 40, 1030):
        centres = np.random.default_rng(C).uniform(-0.2, 2.2, C)
        centres[C // 2] = centres[0]                                       # a repeated centre: the first one wins
        lab = I.assign(dev(x, device), dev(centres, device))
        assert lab.dtype == torch.int64 and np.array_equal(lab.cpu().numpy(), assign_rule(x, centres))
        assert not (lab == C // 2).any() or C == 1


# ------------------------------------------------------------------------------------------------ 2. public functions
def check_public(name, device):
    """estimate_bandwidth and mean_shift on every run of a golden case against scikit-learn's recorded result."""
    from atomai_amd.stat import intensity
    g = gold()
    x = g[f"{name}|x"]
    n = len(x)
    for j, q, K, gbw in runs(name):
        tol = max(1000.0 * float(g[f"{name}|{j}|dist"]), n * EPS)
        bw = intensity.estimate_bandwidth(dev(x, device), q)
        assert isinstance(bw, float)
        if gbw == 0.0:
            assert bw == 0.0
            with pytest.raises(ValueError, match="identical"):
                intensity.mean_shift(x, quantile=q)
            print(f"public {name} q {q}: bandwidth 0, refused")
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                # (seeds = data where every row has its own bin)
            fit = intensity.mean_shift(dev(x, device), quantile=q)
        centres, labels = fit["centres"].cpu().numpy(), fit["labels"].cpu().numpy()
        gc = g[f"{name}|{j}|centres"]
        print(f"public {name} q {q}: bandwidth rel. {rel(bw, gbw):.2e}, {len(centres)} centres rel. "
              f"{rel(centres, gc) if len(centres) == len(gc) else float('nan'):.2e} (bound {tol:.2e}), n_iter {fit['n_iter']}")
        assert rel(bw, gbw) <= tol and fit["bandwidth"] == bw
        assert len(centres) == len(gc) and fit["n_iter"] == int(g[f"{name}|{j}|n_iter"])
        assert labels.dtype == np.int64 and np.array_equal(labels, g[f"{name}|{j}|labels"].astype(np.int64))
        assert rel(centres, gc) <= tol
    if name == "three":
        assert len(g["three|0|centres"]) > 3 and int(g["three|0|n_iter"]) >= 40        # a long run with spurious modes


def check_kmeans(name, device):
    """kmeans against KMeans(k, random_state=42): the partition up to a relabelling, the centres as sorted lists."""
    from atomai_amd.stat import intensity
    g = gold()
    x, k = g[f"{name}|x"], int(g[f"km|{name}|k"])
    tol = max(1000.0 * float(g[f"km|{name}|dist"]), len(x) * EPS)
    fit = intensity.kmeans(dev(x, device), k)
    centres, labels = fit["centres"].cpu().numpy(), fit["labels"].cpu().numpy()
    err = rel(np.sort(centres), np.sort(g[f"km|{name}|centres"]))
    print(f"kmeans {name} k {k}: {fit['n_iter']} rounds, sorted centres rel. {err:.2e} (bound {tol:.2e})")
    perm = match_partition(labels, g[f"km|{name}|labels"].astype(np.int64))
    assert sorted(perm) == sorted(perm.values()) == list(range(k))
    assert err <= tol and np.array_equal(labels, assign_rule(x, centres)) and 1 <= fit["n_iter"] <= 300
    for c, s in perm.items():
        assert rel(centres[c], g[f"km|{name}|centres"][s]) <= tol


def check_degenerate(device):
    """One row, 50 identical rows: scikit-learn's bandwidth is exactly 0 (recorded) and MeanShift refuses it."""
    from atomai_amd.stat import intensity
    g = gold()
    for name in ("one", "same50"):
        x = g[f"deg|{name}|x"]
        assert float(g[f"deg|{name}|bw"]) == 0.0 and intensity.estimate_bandwidth(dev(x, device)) == 0.0
        with pytest.raises(ValueError, match="identical"):
            intensity.mean_shift(dev(x, device))
        fit = intensity.mean_shift(dev(x, device), bandwidth=0.5)           # a given bandwidth still runs
        assert fit["centres"].tolist() == [float(x[0])] and fit["labels"].tolist() == [0] * len(x)
    with pytest.raises(ValueError):
        intensity.mean_shift(dev(g["three|x"], device), bandwidth=0.0)
    with pytest.raises(ValueError, match="row 1"):
        intensity.kmeans(dev([0.5, np.nan, 0.7], device), 2)
    with pytest.raises(ValueError, match="32"):
        intensity.kmeans(dev(g["three|x"], device), 33)


def check_determinism(device):
    """Two runs give identical bits; a float32 column gives what its float64 copy gives."""
    from atomai_amd.stat import _intensity as I, intensity
    x = gold()["big1025|x"]
    outs = []
    for col in (dev(x, device), dev(x, device), dev(x.astype(np.float32), device, np.float32),
                dev(x.astype(np.float32).astype(np.float64), device)):
        xs = torch.sort(I.column(col))[0]
        gap, mean = I.kth_gap(xs, 256)
        ms = intensity.mean_shift(col, quantile=0.25)
        km = intensity.kmeans(col, 3)
        outs.append([gap, mean, ms["centres"], ms["labels"], torch.tensor([ms["n_iter"], km["n_iter"]]),
                     torch.tensor(ms["bandwidth"], dtype=torch.float64), km["centres"], km["labels"]])
    for pair in ((0, 1), (2, 3)):
        for a, b in zip(outs[pair[0]], outs[pair[1]]):
            assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ 3. update_classes
def uc_case():
    g = gold()
    return g["uc|frames"], {0: g["uc|coords|0"], 1: g["uc|coords|1"]}


def check_update_classes():
    """stat.intensity.update_classes against the tables the reference returned: 'threshold' and 'meanshift' exactly,
    'kmeans' up to a bijective relabelling; a single table plus its frame; the caller's dictionary is not modified."""
    from atomai_amd.stat import intensity
    g = gold()
    frames, coords = uc_case()
    before = {k: v.copy() for k, v in coords.items()}
    thresh, k = float(g["uc|thresh"]), int(g["uc|n_components"])
    for stack in (frames, frames[..., None], frames.astype(np.float64)):
        got = intensity.update_classes(coords, stack, method="threshold", thresh=thresh)
        assert sorted(got) == [0, 1]
        for f in (0, 1):
            assert got[f].dtype == np.float64 and np.array_equal(got[f], g[f"uc|threshold|{f}"])
            assert set(got[f][:, 2]) == {0.0, 1.0}
    got = intensity.update_classes(coords, frames, method="meanshift")
    for f in (0, 1):
        assert np.array_equal(got[f], g[f"uc|meanshift|{f}"])
    assert len(np.unique(np.concatenate([got[0][:, 2], got[1][:, 2]]))) >= 2
    got = intensity.update_classes(coords, frames, method="kmeans", n_components=k)
    ours = np.concatenate([got[f][:, 2] for f in (0, 1)]).astype(np.int64)
    ref = np.concatenate([g[f"uc|kmeans|{f}"][:, 2] for f in (0, 1)]).astype(np.int64)
    perm = match_partition(ours, ref)
    assert sorted(perm) == sorted(perm.values()) == list(range(k))
    for f in (0, 1):
        assert np.array_equal(got[f][:, :2], coords[f][:, :2])
    one = intensity.update_classes(coords[1], frames[1], method="threshold", thresh=thresh)      # one table, its frame
    assert sorted(one) == [0] and np.array_equal(one[0], g["uc|threshold|1"])
    for f in (0, 1):
        assert np.array_equal(coords[f], before[f])


def check_errors():
    """Missing thresh / n_components, a NaN intensity, bandwidth 0, an unknown method."""
    from atomai_amd.stat import intensity
    frames, coords = uc_case()
    with pytest.raises(AttributeError, match="thresh=.5"):
        intensity.update_classes(coords, frames)                           # the reference's default method
    with pytest.raises(AttributeError, match="n_components"):
        intensity.update_classes(coords, frames, method="kmeans")
    with pytest.raises(NotImplementedError, match="Choose between 'threshold', 'kmeans', 'meanshift' and 'gmm_local'"):
        intensity.update_classes(coords, frames, method="dbscan")
    edge = {0: coords[0], 1: np.concatenate((coords[1][:3], [[0.0, 20.0, 0.0]], coords[1][3:]))}   # row 0: window from -1
    for method, kw in (("kmeans", {"n_components": 2}), ("meanshift", {})):
        with pytest.raises(ValueError, match="atom 3 of frame 1"):
            intensity.update_classes(edge, frames, method=method, **kw)
    got = intensity.update_classes(edge, frames, method="threshold", thresh=float(gold()["uc|thresh"]))
    assert np.isnan(got[1][3, 2]) and not np.isnan(np.delete(got[1][:, 2], 3)).any()
    flat = {0: coords[0]}
    with pytest.raises(ValueError, match="identical"):
        intensity.update_classes(flat, np.full((1, 64, 64), 0.5, dtype=np.float32), method="meanshift")


def check_package_level():
    """aoi.stat.update_classes runs 'threshold' and 'meanshift'; 'kmeans' still raises and names the working function."""
    import atomai_amd as aoi
    g = gold()
    frames, coords = uc_case()
    assert aoi.stat.intensity.update_classes is not aoi.stat.update_classes
    got = aoi.stat.update_classes(coords, frames, thresh=float(g["uc|thresh"]))
    assert np.array_equal(got[0], g["uc|threshold|0"]) and np.array_equal(got[1], g["uc|threshold|1"])
    got = aoi.stat.update_classes(coords, frames, method="meanshift", quantile=.25)
    assert np.array_equal(got[0], g["uc|meanshift|0"]) and np.array_equal(got[1], g["uc|meanshift|1"])
    with pytest.raises(NotImplementedError, match=re.escape("atomai_amd.stat.intensity.update_classes(..., method='kmeans')")):
        aoi.stat.update_classes(coords, frames, method="kmeans", n_components=2)
    with pytest.raises(AttributeError):
        aoi.stat.update_classes(coords, frames)
    with pytest.raises(NotImplementedError, match="Choose between"):
        aoi.stat.update_classes(coords, frames, method="dbscan")


def check_no_sklearn():
    """No source file under stat/ and utils/ has an import statement for scikit-learn (the pattern of the clustering
    tests: a search of the sources, run in the emulated tier).  It does NOT show that ``sklearn`` stays out of
    ``sys.modules`` while the three methods run."""
    import atomai_amd
    root = os.path.dirname(os.path.abspath(atomai_amd.__file__))
    offenders = []
    for sub in ("stat", "utils"):
        for d, _, files in os.walk(os.path.join(root, sub)):
            for f in files:
                text = open(os.path.join(d, f)).read() if f.endswith(".py") else ""
                if re.search(r"^\s*(from|import)\s+sklearn\b", text, flags=re.M):
                    offenders.append(os.path.relpath(os.path.join(d, f), root))
    assert not offenders, offenders
    assert os.path.exists(os.path.join(root, "stat", "intensity.py"))
