"""Generates tests/golden/stat.npz from the REAL reference (imported through oracle/ref_harness.py, dev container only;
never imported by a test; needs numpy, scipy and scikit-learn there):

    python tools/make_stat_golden.py

Planted-class frames.  Per case everything is drawn from ``default_rng(7)`` in this order: K prototypes
uniform(0.1, 0.9, (K, r, r, C)); B frames uniform(0, 0.05, (B, H, W, C)); then per frame and per grid site
i in range(r, H - r, step), j in range(r, W - r, step): the class k (uniform over K), the r x r x C noise N(0, 1) and the
two coordinate offsets U(-0.4, 0.4).  ``proto[k] + noise * N`` is pasted at [i - r//2, i - r//2 + r) along both axes and
the site becomes the coordinate row (i + U, j + U, 0).  Every frame also gets (1, 1, 0) and (H - 1.2, W / 2, 0), whose
windows leave the frame and are dropped, and (H / 2, W / 2, 1), the wrong class.  The frames are cast to float32.

Keys of a case ``<c>`` (r5c3, r8c1, r7c1_k1; K planted classes, window r):
  <c>|frames (B,H,W,C) float32   <c>|coords|f (n,3) float64   <c>|r   <c>|K   <c>|planted (N,) class of every kept window
  <c>|gmm|<cov>|classes (N,)  <c>|gmm|<cov>|cla (max class, r, r, C)  <c>|gmm|<cov>|com_frames (N, 4): the reference's
      imlocal.gmm(K, cov, random_state=1) on the float64 copy of the frames, cov in (diag, spherical)
  <c>|npca  number of PCA components = K - 1 (2 for the K = 1 case)
  <c>|R64|comp, |proj, |ratio   the reference's pca(npca) and pca_scree_plot on the float64 copy; <c>|R32|...: on float32
  <c>|M|comp, |proj, |ratio     numpy.linalg.svd in fp64 of the centred stack, the largest-magnitude entry of every
                                component positive
  <c>|floor32 (3,)              max |R32 - M| for components, projections and explained-variance ratios
  <c>|com_frames (N, 3)         pca's third return value
Host logic (the r8c1 case has three frames):
  ctm|trace, ctm|M; renum|in, renum|out; traj|start, traj|rmax, traj|flow, traj|frames (get_trajectory on r8c1's
  coordinate dictionary); alltraj|n, alltraj|flow|k, alltraj|frames|k (get_all_trajectories(run_gmm=False, rmax) on r8c1);
  sumtr|traj|k, sumtr|trans|k, sumtr|n, sumtr|msize, sumtr|out; upd|n_components, upd|window_size, upd|table|f
  (update_classes(method='gmm_local') on r8c1).
TEST INFRASTRUCTURE ONLY.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CASES = {  # name: (B, H, W, C, r, K, step, noise, N)
    "r5c3": (2, 37, 41, 3, 5, 3, 6, 0.05, 60),
    "r8c1": (3, 50, 50, 1, 8, 4, 9, 0.05, 48),
    "r7c1_k1": (1, 40, 40, 1, 7, 1, 8, 0.05, 16),
}


def planted(B, H, W, C, r, K, step, noise):
    rng = np.random.default_rng(7)
    proto = rng.uniform(0.1, 0.9, (K, r, r, C))
    frames = rng.uniform(0, 0.05, (B, H, W, C))
    coords, classes = {}, []
    for b in range(B):
        rows = []
        for i in range(r, H - r, step):
            for j in range(r, W - r, step):
                k = int(rng.integers(K))
                lo_i, lo_j = i - r // 2, j - r // 2
                frames[b, lo_i:lo_i + r, lo_j:lo_j + r] = proto[k] + noise * rng.normal(size=(r, r, C))
                rows.append((i + rng.uniform(-0.4, 0.4), j + rng.uniform(-0.4, 0.4), 0.0))
                classes.append(k)
        rows += [(1.0, 1.0, 0.0), (H - 1.2, W / 2, 0.0), (H / 2, W / 2, 1.0)]
        coords[b] = np.array(rows, dtype=np.float64)
    return frames.astype(np.float32), coords, np.array(classes)


def exact_pca(stack, n):
    X = stack.reshape(len(stack), -1).astype(np.float64)
    Xc = X - X.mean(0)
    U, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    sign = np.sign(Vt[np.arange(len(Vt)), np.abs(Vt).argmax(1)])
    Vt, U = Vt * sign[:, None], U * sign[None, :]
    ratio = S ** 2 / np.sum(S ** 2)
    return Vt[:n], (U * S)[:, :n], ratio, S


def main():
    aoi = ref_harness.import_reference()
    from atomai.stat import multivar as ref
    out = {}
    for name, (B, H, W, C, r, K, step, noise, N) in CASES.items():
        frames, coords, classes = planted(B, H, W, C, r, K, step, noise)
        out[f"{name}|frames"] = frames
        for f, t in coords.items():
            out[f"{name}|coords|{f}"] = t
        out[f"{name}|r"], out[f"{name}|K"], out[f"{name}|planted"] = r, K, classes
        s64 = ref.imlocal(frames.astype(np.float64), coords, r, 0)
        s32 = ref.imlocal(frames, coords, r, 0)
        assert s64.imgstack.shape == (N, r, r, C) and s32.imgstack.dtype == np.float32, s64.imgstack.shape
        for cov in ("diag", "spherical"):
            for seed in (1, 2, 3):
                for s in (s64, s32):
                    cla, cl_all, cf = s.gmm(K, cov, seed)
                    got = cf[:, 2].astype(int)
                    pairs = set(zip(got.tolist(), classes.tolist()))
                    assert len(pairs) == K == len(set(got.tolist())), (name, cov, seed, "planted partition not recovered")
            cla, cl_all, cf = s64.gmm(K, cov, 1)
            out[f"{name}|gmm|{cov}|classes"] = cf[:, 2].astype(np.int64)
            out[f"{name}|gmm|{cov}|cla"] = cla
            out[f"{name}|gmm|{cov}|com_frames"] = cf
        n = max(K - 1, 2) if K == 1 else K - 1
        out[f"{name}|npca"] = n
        Mc, Mp, Mr, S = exact_pca(s32.imgstack, n)
        print(f"{name}: N = {N}, D = {r * r * C}, leading singular values {np.round(S[:4], 3)}")
        res = {}
        for tag, s in (("R64", s64), ("R32", s32)):
            comp, proj, cf = s.pca(n)
            ratio = s.pca_scree_plot(plot_results=False)
            res[tag] = (comp.reshape(n, -1), proj, ratio)
            out[f"{name}|{tag}|comp"], out[f"{name}|{tag}|proj"], out[f"{name}|{tag}|ratio"] = res[tag]
        out[f"{name}|com_frames"] = cf
        out[f"{name}|M|comp"], out[f"{name}|M|proj"], out[f"{name}|M|ratio"] = Mc, Mp, Mr
        dev64 = [np.abs(a - b).max() for a, b in zip(res["R64"], (Mc, Mp, Mr))]
        floor = np.array([np.abs(np.asarray(a, dtype=np.float64) - b).max() for a, b in zip(res["R32"], (Mc, Mp, Mr))])
        out[f"{name}|floor32"] = floor
        print(f"   max |R64 - M| = {dev64},  floor32 = max |R32 - M| = {floor.tolist()}")
        assert max(dev64) < 1e-12
    # ---- host logic
    trace = np.array([0, 1, 1, 2, 0, 2, 1, 1, 3, 0])
    out["ctm|trace"], out["ctm|M"] = trace, ref.calculate_transition_matrix(trace)
    cls_in = np.array([2., 5., 5., 9., 2., 7.])
    out["renum|in"], out["renum|out"] = cls_in, ref.imlocal.renumerate_classes(cls_in)
    B, H, W, C, r, K, step, noise, N = CASES["r8c1"]
    frames, coords, _ = planted(B, H, W, C, r, K, step, noise)
    start, rmax = coords[0][5, :2], 3
    flow, fr = ref.imlocal.get_trajectory(coords, start, rmax)
    assert len(fr) == B
    out["traj|start"], out["traj|rmax"], out["traj|flow"], out["traj|frames"] = start, rmax, flow, fr
    s = ref.imlocal(frames.astype(np.float64), coords, r, 0)
    d = s.get_all_trajectories(min_length=0, run_gmm=False, rmax=rmax)
    out["alltraj|n"] = len(d["trajectories"])
    for k, (t, f) in enumerate(zip(d["trajectories"], d["frames"])):
        out[f"alltraj|flow|{k}"], out[f"alltraj|frames|{k}"] = t, f
    trajs = [np.array([[1., 2., 1.], [1., 2., 3.], [1., 2., 3.], [1., 2., 1.]]),
             np.array([[5., 5., 2.], [5., 5., 4.], [5., 5., 2.], [5., 5., 2.], [5., 5., 1.]]),
             np.array([[7., 7., 3.], [7., 7., 4.], [7., 7., 1.], [7., 7., 2.]])]
    trans = [ref.calculate_transition_matrix(ref.imlocal.renumerate_classes(t[:, -1])) for t in trajs]
    out["sumtr|n"], out["sumtr|msize"] = len(trajs), 4
    for k, (t, m) in enumerate(zip(trajs, trans)):
        out[f"sumtr|traj|{k}"], out[f"sumtr|trans|{k}"] = t, m
    out["sumtr|out"] = ref.sum_transitions({"trajectories": trajs, "transitions": trans}, 4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        upd = ref.update_classes(coords, frames.astype(np.float64), method="gmm_local", n_components=K, window_size=r)
    out["upd|n_components"], out["upd|window_size"] = K, r
    for f, t in upd.items():
        out[f"upd|table|{f}"] = t
    path = os.path.join(GOLD, "stat.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
