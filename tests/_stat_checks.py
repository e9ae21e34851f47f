"""Shared bodies of the atomai_amd.stat tests (emulator tier on CPU, gpu tier on the MI355X).

Kernel checks compare against an fp64 numpy model with DERIVED bounds: the worst-case summation bound
(n + 8) * 2^-24 * sum |terms| evaluated in the oracle — n = D and the terms of the quadratic form for the
log-probabilities (and the lower bound), n = 1024 (the longest fp32 chain the kernel may form) and the terms of the sum
for n_k, S1 and S2.  The public classes are compared against tests/golden/stat.npz, which tools/make_stat_golden.py records
from the reference (sklearn on the host); PCA bounds are 4 * floor32, floor32 = the reference's own fp32 error against
the exact fp64 SVD on the same data.  Neither the reference nor scikit-learn is imported here."""
import os
import warnings

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["r5c3", "r8c1", "r7c1_k1"]
U = 2.0 ** -24
PASS_SHAPES = [(1, 49, 1), (60, 75, 3), (257, 64, 7), (100, 768, 16), (100, 75, 17), (65, 75, 32),
               (33, 12288, 3)]           # the last: a row longer than any LDS staging (5 s on the emulator)
# Seed of every shape's inputs, and the margin by which the two best components of EVERY oracle row are asserted to lie
# apart, in units of the logp bound, before all N labels are compared (no row is left out).  100 wherever the inputs can
# give it.  At (100, 768, 16) and (33, 12288, 3) they cannot: the worst-case bound grows like D * q while the gap between
# two components of a random row grows like sqrt(D) (these are the best of 40 seeds each: 11 and 2.8 bounds); there the margin is 2, the
# least at which the comparison is decidable — two log-probabilities that are each within the bound cannot swap.
PASS_SEED = {(1, 49, 1): 5, (60, 75, 3): 22, (257, 64, 7): 39, (100, 768, 16): 75, (100, 75, 17): 73, (65, 75, 32): 90,
             (33, 12288, 3): 107}
LABEL_MARGIN = {(100, 768, 16): 2, (33, 12288, 3): 2}
_gold = None
_oracle = {}


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLD, "stat.npz")) as g:
            _gold = {k: g[k] for k in g.files}
    return _gold


def case(name):
    g = gold()
    frames = g[f"{name}|frames"]
    coords = {f: g[f"{name}|coords|{f}"] for f in range(len(frames))}
    return frames, coords, int(g[f"{name}|r"]), int(g[f"{name}|K"])


def stat_of(name, dtype=np.float32):
    import atomai_amd as aoi
    frames, coords, r, K = case(name)
    return aoi.stat.imlocal(frames.astype(dtype), coords, r, 0), K


# ------------------------------------------------------------------------------------------------ 1. the pass kernel
def pass_oracle(N, D, K):
    """Inputs and the fp64 model of one pass, computed once per shape and shared (never modified)."""
    key = (N, D, K)
    if key in _oracle:
        return _oracle[key]
    rs = np.random.RandomState(PASS_SEED[key])
    X = rs.uniform(0, 1, (N, D)).astype(np.float32)
    mean = (X[rs.choice(N, K, replace=False)] + np.float32(0.01)).astype(np.float32)
    prec = (1.0 / rs.uniform(2.5e-3, 0.1, (K, D))).astype(np.float32)
    wts = rs.uniform(0.2, 1.0, K)
    logw = np.log(wts / wts.sum())
    shift = X.astype(np.float64).mean(0).astype(np.float32)
    X64, m64, p64, s64 = (a.astype(np.float64) for a in (X, mean, prec, shift))
    q = np.empty((N, K))
    for k in range(K):
        q[:, k] = (((X64 - m64[k]) ** 2) * p64[k]).sum(1)
    cst = logw + 0.5 * np.log(p64).sum(1) - 0.5 * D * np.log(2 * np.pi)
    logp = cst[None, :] - 0.5 * q
    b_logp = (D + 8) * U * 0.5 * q                         # the terms of logp's sum are the 1/2 (x - mu)^2 prec, all >= 0
    mx = logp.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(logp - mx).sum(1, keepdims=True)))[:, 0]
    resp = np.exp(logp - lse[:, None])
    label = logp.argmax(1)
    o = dict(X=X, mean=mean, prec=prec, logw=logw, shift=shift, logp=logp, b_logp=b_logp, lse=lse, label=label,
             lb=lse.mean(), b_lb=b_logp.max(1).mean())     # log-sum-exp is 1-Lipschitz in the sup norm of its row
    xs = X64 - s64
    for tag, r in (("soft", resp), ("hard", np.eye(K)[label])):
        o[tag] = dict(nk=r.sum(0), S1=r.T @ xs, S2=r.T @ xs ** 2, b_nk=1032 * U * np.abs(r).sum(0),
                      b_S1=1032 * U * (np.abs(r).T @ np.abs(xs)), b_S2=1032 * U * (np.abs(r).T @ xs ** 2))
    _oracle[key] = o
    return o


def check_pass(shape, device):
    from atomai_amd.stat import _gmm
    N, D, K = shape
    o = pass_oracle(N, D, K)
    t = {k: torch.from_numpy(o[k]).to(device) for k in ("X", "mean", "prec", "logw", "shift")}
    if K > 1:                                              # no row is left out of the label comparison
        top = np.sort(o["logp"], axis=1)[:, -2:]
        margin = (top[:, 1] - top[:, 0]) / np.sort(o["b_logp"], axis=1)[:, -1]
        print(f"pass {shape}: the two best components of every row are >= {margin.min():.1f} logp bounds apart")
        assert (margin > LABEL_MARGIN.get(shape, 100)).all(), (shape, float(margin.min()))
    for tag, hard in (("soft", False), ("hard", True)):
        got = _gmm.gmm_pass(t["X"], t["mean"], t["prec"], t["logw"], t["shift"], hard=hard, want_logp=True)
        got = {k: v.cpu().numpy() for k, v in got.items()}
        ref = o[tag]
        e_logp = np.abs(got["logp"] - o["logp"])
        e_lb = abs(float(got["lb"]) - o["lb"])
        print(f"pass {shape} {tag}: logp err/bound {float((e_logp / o['b_logp']).max()):.3e} "
              f"(max err {e_logp.max():.3e}), lb err {e_lb:.3e} bound {o['b_lb']:.3e}", end="")
        assert got["logp"].dtype == np.float64 and got["logp"].shape == (N, K)
        assert (e_logp <= o["b_logp"]).all(), (shape, tag)
        assert e_lb <= o["b_lb"], (shape, tag)
        assert np.array_equal(got["label"], o["label"]), (shape, tag)
        for name in ("nk", "S1", "S2"):
            err, bound = np.abs(got[name] - ref[name]), ref["b_" + name]
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
            print(f", {name} err/bound {float(ratio.max()):.3e} (max err {err.max():.3e})", end="")
            assert got[name].dtype == np.float64 and (err <= bound).all(), (shape, tag, name)
        print()
        if hard:
            assert np.array_equal(got["nk"], np.bincount(o["label"], minlength=K).astype(np.float64)), shape


# ------------------------------------------------------------------------------------------------ 2. the M step
def check_update(device):
    from atomai_amd.stat import _gmm
    rs = np.random.RandomState(5)
    N, D, K = 200, 75, 4
    X = rs.uniform(0, 1, (N, D))
    shift = X.mean(0).astype(np.float32)
    resp = rs.dirichlet(np.ones(K - 1), N)
    resp = np.concatenate((resp, np.zeros((N, 1))), axis=1)           # the last component owns nothing: nk = 0
    xs = X - shift.astype(np.float64)
    nk, S1, S2 = resp.sum(0), resp.T @ xs, resp.T @ xs ** 2
    assert nk[-1] == 0 and not S1[-1].any()
    for cov in ("diag", "spherical"):
        got = _gmm.gmm_update(*(torch.from_numpy(a).to(device) for a in (nk, S1, S2, shift)), N, cov)
        mean, var, prec, weights = (v.cpu().numpy() for v in got)
        n = nk + 10 * np.finfo(np.float64).eps
        m = S1 / n[:, None]
        v = S2 / n[:, None] - m * m + 1e-6
        if cov == "spherical":
            v = np.repeat((S2 / n[:, None] - m * m).mean(1, keepdims=True) + 1e-6, D, axis=1)
        want = (m + shift.astype(np.float64), v, 1.0 / v, n / N)
        for name, a, b in zip(("mean", "var", "prec", "weights"), (mean, var, prec, weights), want):
            rel = np.abs(a - b) / np.abs(b)
            print(f"gmm_update {cov} {name}: max relative error {rel.max():.3e}")
            assert a.dtype == np.float64 and np.isfinite(a).all() and (rel <= 1e-12).all(), (cov, name, rel.max())
        assert 0 < weights[-1] < 1e-15


# ------------------------------------------------------------------------------------------------ 3. determinism
def check_determinism(device):
    from atomai_amd.stat import _gmm
    s, K = stat_of("r5c3")
    X = torch.from_numpy(np.ascontiguousarray(s.imgstack.reshape(s.d0, -1))).to(device)
    X = torch.cat([X, X + 0.001, X - 0.001], 0).contiguous()          # 180 rows: three workgroups
    a = _gmm.fit_gmm(X, K, "diag", 3)
    b = _gmm.fit_gmm(X, K, "diag", 3)
    assert a["labels"].dtype == torch.int64 and a["converged"]
    assert a["labels"].cpu().numpy().tobytes() == b["labels"].cpu().numpy().tobytes()
    assert a["means"].cpu().numpy().tobytes() == b["means"].cpu().numpy().tobytes()
    assert a["lower_bound"] == b["lower_bound"] and a["n_iter"] == b["n_iter"]


def check_no_convergence_warning(device):
    from atomai_amd.stat import _gmm
    s, K = stat_of("r8c1")
    X = torch.from_numpy(np.ascontiguousarray(s.imgstack.reshape(s.d0, -1))).to(device)
    with pytest.warns(_gmm.ConvergenceWarning, match="did not converge"):
        out = _gmm.fit_gmm(X, K, "diag", 1, tol=0.0, max_iter=2)
    assert out["n_iter"] == 2 and not out["converged"]


# ------------------------------------------------------------------------------------------------ 4. imlocal.gmm
def match_classes(ours, ref):
    """The bijection ours -> reference between two labellings of the same partition (asserted)."""
    pairs = sorted(set(zip(ours.tolist(), ref.tolist())))
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}) == len(set(ref.tolist())), pairs
    return dict(pairs)


def check_gmm(name, cov, seed):
    g = gold()
    s, K = stat_of(name)
    cla, cl_all, cf = s.gmm(K, cov, seed)
    rcf, rcla = g[f"{name}|gmm|{cov}|com_frames"], g[f"{name}|gmm|{cov}|cla"]
    assert cf.dtype == np.float64 and cf.shape == rcf.shape and cla.dtype == np.float64 and cla.shape == rcla.shape
    assert np.array_equal(cf[:, [0, 1, 3]], rcf[:, [0, 1, 3]])
    ours, ref = cf[:, 2].astype(np.int64), g[f"{name}|gmm|{cov}|classes"]
    assert np.array_equal(ours, cf[:, 2]) and ours.min() == 1
    m = match_classes(ours, ref)
    assert len(cl_all) == int(ref.max()) == cla.shape[0]
    for a, b in m.items():
        assert cl_all[a - 1].shape == (int((ref == b).sum()),) + cla.shape[1:] and cl_all[a - 1].dtype == np.float32
        err, bound = np.abs(cla[a - 1] - rcla[b - 1]).max(), 8 * U * np.abs(rcla).max()
        assert err <= bound, (name, cov, seed, a, err, bound)
    print(f"gmm {name} {cov} seed {seed}: classes {m}, counts {[len(c) for c in cl_all]}")


# ------------------------------------------------------------------------------------------------ 5. PCA
def _assert_pca(name, what, comp, proj, ratio):
    g = gold()
    floor = g[f"{name}|floor32"]
    for i, (tag, a) in enumerate((("comp", comp), ("proj", proj), ("ratio", ratio))):
        if a is None:
            continue
        M = g[f"{name}|M|{tag}"]
        assert a.dtype == np.float64 and a.shape == M.shape, (name, what, tag, a.shape, M.shape)
        err = np.abs(a - M).max()
        print(f"{what} {name} {tag}: max |ours - M| {err:.3e}, floor32 {floor[i]:.3e}, bound {4 * floor[i]:.3e}")
        assert err <= 4 * floor[i], (name, what, tag, err, floor[i])


def check_pca(name):
    g = gold()
    s, _ = stat_of(name)
    n = int(g[f"{name}|npca"])
    comp, proj, cf = s.pca(n)
    assert comp.shape == (n, s.d1, s.d2, s.d3) and np.array_equal(cf, g[f"{name}|com_frames"])
    _assert_pca(name, "pca", comp.reshape(n, -1), proj, None)
    comp2, proj2, xy = s.imblock_pca(n)
    assert np.array_equal(xy, g[f"{name}|com_frames"][:, :2])
    _assert_pca(name, "imblock_pca", comp2.reshape(n, -1), proj2, None)
    ratio = s.pca_scree_plot(plot_results=False)
    _assert_pca(name, "pca_scree_plot", None, None, ratio)


def check_pca_wide(device):
    """D <= N (the D x D Gram route; every golden case has N < D): 4 x 4 windows of the r8c1 frames against the fp64 SVD.
    Bound: the fp32 Gram matrix is off by at most E = (N + 8) 2^-24 |Xc|^T |Xc| (worst-case summation), which turns an
    eigenvector by at most 2 sqrt(2) ||E||_F / gap (Davis-Kahan in the form of Yu, Wang and Samworth) and moves an eigenvalue by at most ||E||_F."""
    import atomai_amd as aoi
    frames, coords, _, _ = case("r8c1")
    s = aoi.stat.imlocal(frames, coords, 4, 0)
    N, D = s.d0, s.d1 * s.d2 * s.d3
    assert D == 16 and N >= 3 * D
    X = s.imgstack.reshape(N, D).astype(np.float64)
    Xc = X - X.mean(0)
    _, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    Vt = Vt * np.sign(Vt[np.arange(D), np.abs(Vt).argmax(1)])[:, None]
    lam = S ** 2
    E = np.linalg.norm((N + 8) * U * (np.abs(Xc).T @ np.abs(Xc)))
    E += np.linalg.norm(4 * U * (np.abs(Xc).T @ (np.abs(X) + np.abs(X.mean(0)))))   # Xc itself is formed in fp32
    n = 3
    comp, proj, _ = s.pca(n)
    gaps = np.array([min(abs(lam[i] - lam[j]) for j in range(D) if j != i) for i in range(n)])
    b_comp = 2 * np.sqrt(2) * E / gaps + 2 * U * np.sqrt(D)          # 2-norm; + the fp32 copy the projection GEMM reads
    e_comp = np.abs(comp.reshape(n, D) - Vt[:n]).max(1)
    b_proj = np.linalg.norm(Xc, axis=1).max() * b_comp + (D + 8) * U * np.abs(Xc).sum(1).max() + 2 * U * D
    e_proj = np.abs(proj - Xc @ Vt[:n].T).max(0)
    ratio = s.pca_scree_plot(plot_results=False)
    e_ratio, b_ratio = np.abs(ratio - lam / lam.sum()).max(), 2 * D * E / lam.sum()
    print(f"pca D<=N: comp err {e_comp} bound {b_comp}; proj err {e_proj} bound {b_proj}; ratio err {e_ratio:.3e} "
          f"bound {b_ratio:.3e}")
    assert (e_comp <= b_comp).all() and (e_proj <= b_proj).all() and e_ratio <= b_ratio and ratio.shape == (D,)


# ------------------------------------------------------------------------------------------------ 6. pca_gmm
def check_pca_gmm():
    from atomai_amd.stat.multivar import _pca_device
    s, K = stat_of("r8c1")
    ncomp = [2, 1, 3, 2]
    cla, comps, projs, cf = s.pca_gmm(K, ncomp)
    cla0, cl_all, cf0 = s.gmm(K)
    assert np.array_equal(cla, cla0) and np.array_equal(cf, cf0) and len(comps) == len(projs) == K
    dev = s._device_stack().device
    for j, (imgs, n) in enumerate(zip(cl_all, ncomp)):
        assert comps[j].shape == (n, s.d1, s.d2, s.d3) and projs[j].shape == (len(imgs), n)
        X = torch.from_numpy(np.ascontiguousarray(imgs.reshape(len(imgs), -1))).to(dev)
        c, p, _ = _pca_device(X, n)
        assert np.array_equal(c, comps[j].reshape(n, -1)) and np.array_equal(p, projs[j]), j
    cla1, comps1, projs1, _ = s.pca_gmm(K, 2)                         # a plain int: the same count for every class
    assert all(c.shape[0] == 2 for c in comps1) and np.array_equal(comps1[0], comps[0])
    scree = s.pca_gmm_scree_plot(K, plot_results=False)
    assert len(scree) == K
    for imgs, ev in zip(cl_all, scree):
        assert ev.shape == (min(len(imgs), s.d1 * s.d2 * s.d3),) and abs(ev.sum() - 1) < 1e-12 and (ev >= 0).all()


# ------------------------------------------------------------------------------------------------ 7. host logic
def check_host_logic():
    import atomai_amd as aoi
    g = gold()
    st = aoi.stat
    M = st.calculate_transition_matrix(g["ctm|trace"])
    assert M.dtype == np.float64 and np.array_equal(M, g["ctm|M"])
    out = st.imlocal.renumerate_classes(g["renum|in"])
    assert out.dtype == np.int64 and np.array_equal(out, g["renum|out"])
    frames, coords, r, K = case("r8c1")
    flow, fr = st.imlocal.get_trajectory(coords, g["traj|start"], int(g["traj|rmax"]))
    assert np.array_equal(flow, g["traj|flow"]) and np.array_equal(fr, g["traj|frames"])
    flow, fr = st.imlocal.get_trajectory(coords, np.array([-40.0, -40.0]), 3)        # nothing within rmax
    assert flow.shape == (0, 3) and len(fr) == 0
    s, _ = stat_of("r8c1", np.float64)
    d = s.get_all_trajectories(min_length=0, run_gmm=False, rmax=int(g["traj|rmax"]))
    assert sorted(d) == ["frames", "trajectories"] and len(d["trajectories"]) == int(g["alltraj|n"])
    for k, (t, f) in enumerate(zip(d["trajectories"], d["frames"])):
        assert np.array_equal(t, g[f"alltraj|flow|{k}"]) and np.array_equal(f, g[f"alltraj|frames|{k}"]), k
    n = int(g["sumtr|n"])
    td = {"trajectories": [g[f"sumtr|traj|{k}"] for k in range(n)], "transitions": [g[f"sumtr|trans|{k}"] for k in range(n)]}
    assert np.array_equal(st.sum_transitions(td, int(g["sumtr|msize"])), g["sumtr|out"])


def check_transition_matrix():
    s, K = stat_of("r8c1")
    d = s.transition_matrix(K, rmax=3, sum_all_transitions=True)
    assert sorted(d) == ["all_transitions", "frames", "gmm_components", "trajectories", "transitions"]
    assert len(d["trajectories"]) == len(d["transitions"]) == len(d["frames"]) == 16
    assert d["gmm_components"].shape == (K, s.d1, s.d2, s.d3)
    for t, m in zip(d["trajectories"], d["transitions"]):
        assert t.shape == (3, 3) and m.shape[0] == m.shape[1] == len(np.unique(t[:, -1]))
        rows = m.sum(1)
        assert (np.isclose(rows, 1, rtol=0, atol=1e-12) | (rows == 0)).all() and (m >= 0).all()
    assert d["all_transitions"].shape == (K, K)


def check_update_classes():
    import atomai_amd as aoi
    g = gold()
    frames, coords, r, K = case("r8c1")
    with pytest.raises(NotImplementedError):
        aoi.stat.update_classes(coords, frames, method="kmeans", n_components=2)
    with pytest.raises(AttributeError):
        aoi.stat.update_classes(coords, frames, method="gmm_local", n_components=2)
    got = aoi.stat.update_classes(coords, frames.astype(np.float64), method="gmm_local",
                                  n_components=int(g["upd|n_components"]), window_size=int(g["upd|window_size"]))
    assert sorted(got) == list(range(len(frames)))
    ours = np.concatenate([got[f] for f in sorted(got)])
    ref = np.concatenate([g[f"upd|table|{f}"] for f in sorted(got)])
    assert ours.shape == ref.shape and ours.dtype == ref.dtype and np.array_equal(ours[:, :2], ref[:, :2])
    match_classes(ours[:, 2].astype(np.int64), ref[:, 2].astype(np.int64))
    assert ours[:, 2].min() == 0
    assert np.array_equal(coords[0], g["r8c1|coords|0"])                     # the caller's dictionary is not modified


# ------------------------------------------------------------------------------------------------ 8. edges
def check_edges(device):
    import atomai_amd as aoi
    from atomai_amd.stat import _gmm
    s, K = stat_of("r5c3")
    with pytest.raises(ValueError, match="32"):
        s.gmm(33)
    X = torch.zeros(40, 8, dtype=torch.float32, device=device)
    with pytest.raises(ValueError, match="32"):
        _gmm.fit_gmm(X, 33)
    for cov in ("full", "tied"):
        with pytest.raises(NotImplementedError):
            s.gmm(K, covariance=cov)
    for fn in (s.nmf, s.ica, s.imblock_nmf, s.imblock_ica):
        with pytest.raises(NotImplementedError):
            fn(2)
    for cls in (aoi.stat.SlidingFFTNMF, aoi.stat.SpectralUnmixer):
        with pytest.raises(NotImplementedError):
            cls()
    frames, coords, r, _ = case("r5c3")
    with pytest.raises(ValueError, match="no sub-image"):
        aoi.stat.imlocal(frames, {f: t[-3:] for f, t in coords.items()}, r, 0)
    with pytest.raises(ValueError, match="no sub-image"):
        aoi.stat.imlocal(frames, coords, r, 5)
    s64, _ = stat_of("r5c3", np.float64)
    assert s64.imgstack.dtype == np.float64 and s.imgstack.dtype == np.float32
    assert (s64.d0, s64.d1, s64.d2, s64.d3) == (60, 5, 5, 3) and s64.nb_classes == 3 and s64.r == 5
    assert np.array_equal(s64.imgstack, s.imgstack.astype(np.float64))
    cla, cl_all, _ = s64.gmm(K)
    assert cl_all[0].dtype == np.float64 and s64._device_stack().dtype == torch.float32
    assert s64._device_stack() is s64._device_stack()                       # uploaded once and kept
    with pytest.raises(ValueError):
        s.pca(61)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s.pca(2)
