"""Generates tests/golden/classes.npz from scikit-learn and from the REAL reference (imported through
oracle/ref_harness.py, dev container only; never imported by a test; needs numpy, scikit-learn and matplotlib there):

    python tools/make_classes_golden.py

Part 1: one-dimensional mean shift.  ``names`` lists the cases; case c holds c|x (n,) float64 and, for run j of the
quantiles 0.1, 0.25, 0.5, 1.0:
  c|j|bw       sklearn.cluster.estimate_bandwidth(x[:, None], quantile)
  c|j|centres, c|j|labels (int16), c|j|n_iter   MeanShift(bandwidth=bw, bin_seeding=True).fit(x[:, None])
  c|j|dist     the largest relative distance of bandwidth and centres between scikit-learn and the numpy restatement
A run whose bandwidth is exactly 0 (MeanShift refuses it: asserted) holds c|j|bw = 0 and c|j|dist = 0 only.
Before anything is written this script ASSERTS, on every run of every case, that the restatement of
tests/_classes_checks.py (``bandwidth_rule``, ``ms_rule``) gives scikit-learn's labels, its number of centres and its
n_iter_, and a bandwidth that is 0 exactly where scikit-learn's is.

  three        3 x 200 draws from N(0.2 / 0.5 / 0.9, 0.03); quantile 0.1 takes 53 iterations and gives 6 centres
  two_uneven   500 draws from N(0.3, 0.02) plus 37 from N(0.7, 0.05)
  ties         0.1, 0.1, 0.4, 0.4, 0.4, 0.8, each repeated 7 times: exact duplicates; bandwidth 0 at quantile 0.1
  uniform257   257 uniform values in [0, 1)
  big1025      1025 values of the ``three`` kind: more than one workgroup of the gap kernel
deg|one|x, deg|same50|x with deg|*|bw: one row and 50 identical rows, bandwidth exactly 0.

k-means.  km|names; km|c|k, km|c|centres, km|c|labels (int16): KMeans(k, random_state=42).fit(x[:, None]) of three (k 3),
two_uneven (k 2) and ties (k 3); km|c|dist: relative distance of the sorted centres to ``lloyd_rule`` from
``spread_start``.  ASSERTED: scikit-learn's centres are the means of their own labels within 1e-12; ten other
random_states give the same partition (so "equal up to relabelling, centres as sorted lists" is well-posed); the
restatement gives that partition too.  (scikit-learn's threaded KMeans is not bit-reproducible: a second run of this
script moved one centre of ``three`` by one unit in the last place, which the tests' tolerance covers.)

Part 2: the reference's atomai.stat.update_classes on two 64 x 64 frames of about 40 atoms, two intensity levels far
apart: uc|frames (2, 64, 64) float32, uc|coords|f (n, 3), uc|thresh, uc|n_components; uc|threshold|f, uc|kmeans|f,
uc|meanshift|f the tables it returned (window_size 3, quantile .25; it is given the float64 copy of the frames, so its
window means are the float64 means this package forms).
TEST INFRASTRUCTURE ONLY.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness  # noqa: E402
import _classes_checks as K  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def cases():
    rng = np.random.default_rng(2025)
    mix = lambda n, mus, sig: np.concatenate([rng.normal(m, sig, n) for m in mus])          # noqa: E731
    out = {"three": mix(200, (0.2, 0.5, 0.9), 0.03)}
    out["two_uneven"] = np.concatenate((rng.normal(0.3, 0.02, 500), rng.normal(0.7, 0.05, 37)))
    out["ties"] = np.repeat(np.array([0.1, 0.1, 0.4, 0.4, 0.4, 0.8]), 7)
    out["uniform257"] = rng.uniform(0.0, 1.0, 257)
    big = np.concatenate((mix(341, (0.2, 0.5, 0.9), 0.03), rng.normal(0.5, 0.03, 2)))
    out["big1025"] = big[rng.permutation(len(big))]
    for name in ("three", "two_uneven", "ties"):
        out[name] = out[name][rng.permutation(len(out[name]))]
    assert len(out["big1025"]) == 1025 and len(out["ties"]) == 42
    return out


def sk_meanshift(x, bw):
    from sklearn.cluster import MeanShift
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return MeanShift(bandwidth=bw, bin_seeding=True).fit(x[:, None])


def frames_and_tables():
    """Two frames of 3 x 3 flat atoms on a jittered 7 x 6 grid over a dim noisy background; levels near 0.3 (host) and
    0.9 (dopant, about a quarter), each atom with its own small Gaussian offset.  All values are multiples of 2^-12."""
    rng = np.random.default_rng(11)
    frames = np.round(rng.uniform(0.0, 0.05, (2, 64, 64)) * 4096) / 4096
    tables = {}
    for f in range(2):
        ij = np.stack(np.meshgrid(5 + 9 * np.arange(7), 6 + 10 * np.arange(6), indexing="ij"), -1).reshape(-1, 2)
        ij = ij[rng.permutation(len(ij))[:40 - f]] + rng.integers(-1, 2, (40 - f, 2))
        dopant = rng.uniform(size=len(ij)) < 0.27
        level = np.where(dopant, 0.9, 0.3) + rng.normal(0.0, 0.01, len(ij))
        for (r, c), v in zip(ij, level):
            frames[f, r - 1:r + 2, c - 1:c + 2] = np.round(v * 4096) / 4096
        xy = ij + rng.uniform(-0.45, 0.45, ij.shape)
        tables[f] = np.concatenate((xy, rng.integers(0, 3, (len(ij), 1))), axis=1).astype(np.float64)
    return frames.astype(np.float32), tables


def main():
    from sklearn.cluster import KMeans, estimate_bandwidth
    gold = {"names": np.array(list(cases()))}
    worst = {"bw": 0.0, "centres": 0.0}
    for name, x in cases().items():
        gold[f"{name}|x"] = x
        for j, q in enumerate(K.QUANTILES):
            bw = float(estimate_bandwidth(x[:, None], quantile=q))
            rbw = K.bandwidth_rule(x, q)
            assert (bw == 0.0) == (rbw == 0.0), (name, q, bw, rbw)
            gold[f"{name}|{j}|bw"] = np.float64(bw)
            if bw == 0.0:
                try:
                    sk_meanshift(x, bw)
                    raise AssertionError("MeanShift accepted bandwidth 0")
                except ValueError:
                    pass
                gold[f"{name}|{j}|dist"] = np.float64(0.0)
                print(f"{name} q {q}: bandwidth 0, refused by MeanShift")
                continue
            fit = sk_meanshift(x, bw)
            centres, labels, n_iter = K.ms_rule(x, bw)
            sc = fit.cluster_centers_[:, 0]
            assert len(centres) == len(sc) and n_iter == fit.n_iter_, (name, q, len(centres), len(sc), n_iter, fit.n_iter_)
            assert np.array_equal(labels, fit.labels_), (name, q)
            dbw, dc = K.rel(rbw, bw), K.rel(centres, sc)
            worst["bw"], worst["centres"] = max(worst["bw"], dbw), max(worst["centres"], dc)
            gold[f"{name}|{j}|centres"], gold[f"{name}|{j}|labels"] = sc, fit.labels_.astype(np.int16)
            gold[f"{name}|{j}|n_iter"], gold[f"{name}|{j}|dist"] = np.int64(fit.n_iter_), np.float64(max(dbw, dc))
            print(f"{name} q {q}: n = {len(x)}, bandwidth {bw:.6g} (rel. {dbw:.1e}), {len(sc)} centres (rel. {dc:.1e}), "
                  f"n_iter {fit.n_iter_}")
    print(f"largest relative distance restatement - scikit-learn: bandwidth {worst['bw']:.2e}, centres "
          f"{worst['centres']:.2e}")
    for name, x in (("one", np.array([0.5])), ("same50", np.full(50, 0.25))):
        bw = float(estimate_bandwidth(x[:, None], quantile=0.25))
        assert bw == 0.0 and K.bandwidth_rule(x, 0.25) == 0.0
        gold[f"deg|{name}|x"], gold[f"deg|{name}|bw"] = x, np.float64(bw)

    km = (("three", 3), ("two_uneven", 2), ("ties", 3))
    gold["km|names"] = np.array([n for n, _ in km])
    for name, k in km:
        x = cases()[name]
        fit = KMeans(k, random_state=42).fit(x[:, None])
        sc = fit.cluster_centers_[:, 0]
        for c in range(k):
            assert abs(sc[c] - x[fit.labels_ == c].mean()) <= 1e-12, (name, c)
        for rs in range(10):
            K.match_partition(KMeans(k, random_state=rs).fit(x[:, None]).labels_, fit.labels_)
        rc, rit = K.lloyd_rule(np.sort(x), K.spread_start(x, k), float(np.var(x)) * 1e-4, 300)
        K.match_partition(K.assign_rule(x, rc), fit.labels_)
        dist = K.rel(np.sort(rc), np.sort(sc))
        gold[f"km|{name}|k"], gold[f"km|{name}|centres"] = np.int64(k), sc
        gold[f"km|{name}|labels"], gold[f"km|{name}|dist"] = fit.labels_.astype(np.int16), np.float64(dist)
        print(f"kmeans {name} k {k}: n_iter_ {fit.n_iter_} (restatement from the spread start: {rit}), sorted centres rel. "
              f"{dist:.1e}")

    ref_harness.import_reference()
    from atomai.stat import update_classes
    frames, tables = frames_and_tables()
    thresh, k = 0.6, 2
    gold["uc|frames"], gold["uc|thresh"], gold["uc|n_components"] = frames, np.float64(thresh), np.int64(k)
    for f in tables:
        gold[f"uc|coords|{f}"] = tables[f]
    f64 = frames.astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = {"threshold": update_classes(tables, f64, method="threshold", thresh=thresh),
               "kmeans": update_classes(tables, f64, method="kmeans", n_components=k),
               "meanshift": update_classes(tables, f64, method="meanshift")}
    for method, res in out.items():
        every = np.concatenate([res[f][:, 2] for f in sorted(res)])
        # (mean shift at quantile .25 may split a level into several modes: whatever it finds is recorded)
        assert method == "meanshift" or sorted(np.unique(every)) == [0.0, 1.0], (method, np.unique(every))
        assert len(np.unique(every)) >= 2
        for f in res:
            assert res[f].dtype == np.float64 and np.array_equal(res[f][:, :2], tables[f][:, :2])
            gold[f"uc|{method}|{f}"] = res[f]
        print(f"update_classes {method}: {len(every)} atoms, {int(every.sum())} of class 1")
    path = os.path.join(GOLD, "classes.npz")
    np.savez_compressed(path, **gold)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
