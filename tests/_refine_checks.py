"""Shared bodies of the peak-refinement tests (emulator tier on CPU, gpu tier on the MI355X) against
tests/golden/refine.npz, which tools/make_refine_golden.py records from the reference's peak_refinement.

Bounds.  The golden carries, per atom, the reference's output R (scipy curve_fit, stopped by ftol = xtol = 1.49e-8) and
the converged minimum M of the same least-squares problem (tolerances 1e-15, started at R), and ``floor`` = max |R - M|
over the decided atoms of the file: the reference's own stopping error.  Ours stops by rules at least as tight about
the same minimum, so |ours - M| <= 2 * floor, and by the triangle inequality |ours - R| <= 3 * floor.  Atoms that the
reference keeps because their patch leaves the frame, or because its converged fit lies 3.5 px or more from the patch
centre (0.5 px beyond the gate: both fits end at the same minimum to ~1e-6 px), the class column, the row order and the
dtype are exact."""
import contextlib
import os
import warnings

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["d2", "d4", "d5", "d9", "d8_border", "n1", "n4", "n65", "multi", "half", "d32", "gate"]
_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLD, "refine.npz")) as g:
            _gold = {k: g[k] for k in g.files}
    return _gold


def frames_of(name):
    g = gold()
    n = len([k for k in g if k.startswith(f"{name}|img|")])
    return [{k: g[f"{name}|{k}|{f}"] for k in ("img", "coords", "d", "ref", "M", "kind")} for f in range(n)]


def refine_flat(name, device):
    """All frames of a case in ONE call of the kernel (per-frame d): list of (N, 3) tables, and the status."""
    from atomai_amd.predictors.locator import refine_device
    fr = frames_of(name)
    frames = torch.from_numpy(np.stack([f["img"] for f in fr])).to(device)
    xy = torch.from_numpy(np.concatenate([f["coords"][:, :2] for f in fr])).to(device)
    meta = np.zeros((len(xy), 2), dtype=np.int32)
    meta[:, 0] = np.concatenate([np.full(len(f["coords"]), i) for i, f in enumerate(fr)])
    out, status = refine_device(frames, xy, torch.from_numpy(meta).to(device), [int(f["d"]) for f in fr],
                                return_status=True)
    out, status = out.cpu().numpy(), status.cpu().numpy()
    b = np.searchsorted(meta[:, 0], np.arange(len(fr) + 1))
    return [np.concatenate((out[b[i]:b[i + 1]], f["coords"][:, 2:3]), axis=1) for i, f in enumerate(fr)], \
        [status[b[i]:b[i + 1]] for i in range(len(fr))]


def assert_parity(got, f, label, status=None):
    """One frame's (N, 3) table against its golden record."""
    floor = float(gold()["floor"])
    ref, M, kind, start = f["ref"], f["M"], f["kind"], f["coords"]
    assert got.dtype == np.float64 and got.shape == ref.shape, (label, got.dtype, got.shape)
    assert np.array_equal(got[:, 2], ref[:, 2]), label                       # class column and row order
    fit, kept, und, gated = kind == 0, kind == 1, kind == 2, kind == 3
    if fit.any():
        eM, eR = np.abs(got[fit, :2] - M[fit]).max(), np.abs(got[fit, :2] - ref[fit, :2]).max()
        print(f"{label}: {fit.sum()} fitted atoms, max |ours - M| {eM:.3e} (bound {2 * floor:.3e}), "
              f"max |ours - reference| {eR:.3e} (bound {3 * floor:.3e})")
        assert eM <= 2 * floor, (label, eM, floor)
        assert eR <= 3 * floor, (label, eR, floor)
    assert np.array_equal(got[kept, :2], ref[kept, :2]), label               # patch rule: bit for bit
    assert np.array_equal(got[gated, :2], ref[gated, :2]), label             # gate: the start, bit for bit
    assert np.isfinite(got).all(), label
    for i in np.nonzero(und)[0]:
        assert np.array_equal(got[i, :2], start[i, :2]) or \
            np.hypot(*(got[i, :2] - np.around(start[i, :2]))) < 3, (label, i)
    if status is not None:
        assert (status[fit] == 0).all() and (status[kept] == 1).all() and (status[gated] == 2).all(), (label, status)


def check_parity(name, device):
    tables, status = refine_flat(name, device)
    for i, f in enumerate(frames_of(name)):
        assert_parity(tables[i], f, f"{name}[{i}]", status[i])


def check_peak_refinement(name):
    """The public single-frame entry point."""
    from atomai_amd.utils import peak_refinement
    for i, f in enumerate(frames_of(name)):
        assert_parity(peak_refinement(f["img"], f["coords"], int(f["d"])), f, f"utils {name}[{i}]")


def _half_prob():
    """2 x 2 blobs whose centres of mass are the start coordinates of the 'half' case (all on .5)."""
    f = frames_of("half")[0]
    prob = np.zeros((1,) + f["img"].shape + (2,), dtype=np.float32)
    prob[..., 1] = 1.0
    for r, c in f["coords"][:, :2]:
        prob[0, int(r):int(r) + 2, int(c):int(c) + 2, 0] = 0.9
    return f, prob


def check_locator(device):
    """Locator(refine=True, d).run(prob, img): the 'half' golden through 2 x 2 blobs (centres of mass exactly on .5),
    then two frames at once, channel_first and one frame per chunk, against utils.peak_refinement (pinned above)
    applied to the unrefined centres."""
    from atomai_amd.predictors import Locator
    from atomai_amd.utils import peak_refinement
    f, prob = _half_prob()
    plain = Locator(device=device).run(prob)[0]
    assert np.array_equal(plain, f["coords"])
    got = Locator(refine=True, d=4, device=device).run(prob, f["img"][None, ..., None])
    assert sorted(got) == [0]
    assert_parity(got[0], f, "Locator half")
    fr = frames_of("multi")[1:]
    imgs = np.stack([x["img"] for x in fr])[..., None]
    prob = np.concatenate(((imgs > 0.45).astype(np.float32), (imgs <= 0.45).astype(np.float32)), axis=-1)
    plain = Locator(dist_edge=3, device=device).run(prob)
    assert min(len(v) for v in plain.values()) >= 10
    want = {i: peak_refinement(imgs[i, ..., 0], plain[i], 3) for i in plain}
    assert any(not np.array_equal(want[i], plain[i]) for i in plain)
    pcf = np.ascontiguousarray(np.transpose(prob, (0, 3, 1, 2)))
    for kw, p in ((dict(), prob), (dict(dim_order="channel_first", chunk_bytes=1), pcf)):
        got = Locator(dist_edge=3, refine=True, d=3, device=device, **kw).run(p, imgs)
        assert sorted(got) == sorted(want)
        for i in want:
            assert got[i].dtype == np.float64 and np.array_equal(got[i], want[i]), (kw, i)


def check_default_d(device):
    """amx_nn2_quarter_mean against the reference's int(mean(nn distances) * 0.25): four tables as frames 0, 1, 3, 5 of
    one call, frame 2 empty and frame 4 with two atoms (no two neighbours: 0)."""
    from atomai_amd import _lib as L
    g = gold()
    tabs = [g[f"nn|coords|{k}"] for k in range(len(g["nn|d"]))]
    slots = {0: tabs[0], 1: tabs[1], 3: tabs[2], 4: tabs[3][:2], 5: tabs[3]}
    xy = torch.from_numpy(np.concatenate([np.ascontiguousarray(t[:, :2]) for t in slots.values()])).to(device)
    meta = np.zeros((len(xy), 2), dtype=np.int32)
    meta[:, 0] = np.concatenate([np.full(len(t), f) for f, t in slots.items()])
    meta = torch.from_numpy(meta).to(device)
    d = torch.full((6,), -7, dtype=torch.int32, device=device)
    L.call("amx_nn2_quarter_mean", L.ptr(xy), L.ptr(meta), len(xy), 6, L.ptr(d), L.stream_ptr(xy))
    want = g["nn|d"]
    assert d.cpu().tolist() == [want[0], want[1], 0, want[2], 0, want[3]], (d.cpu().tolist(), want)
    # d=None through the public entry point: the reference's warning, and the same table as the explicit d
    from atomai_amd.utils import peak_refinement
    f = frames_of("d4")[0]                     # lattice spacing 11 +- 1.1 px of jitter: int(mean * 0.25) = 2
    xy = torch.from_numpy(np.ascontiguousarray(f["coords"][:, :2])).to(device)
    meta = torch.zeros((len(xy), 2), dtype=torch.int32, device=device)
    d1 = torch.zeros(1, dtype=torch.int32, device=device)
    L.call("amx_nn2_quarter_mean", L.ptr(xy), L.ptr(meta), len(xy), 1, L.ptr(d1), L.stream_ptr(xy))
    assert int(d1.item()) == 2
    with pytest.warns(UserWarning, match="d-value for bounding box not found"):
        got = peak_refinement(f["img"], f["coords"])
    assert np.array_equal(got, peak_refinement(f["img"], f["coords"], int(d1.item())))
    assert not np.array_equal(got, f["coords"])


def check_determinism(device):
    for name in ("d5",):                       # 24 atoms: six workgroups
        a, sa = refine_flat(name, device)
        b, sb = refine_flat(name, device)
        for x, y, s, t in zip(a, b, sa, sb):
            assert x.tobytes() == y.tobytes() and s.tobytes() == t.tobytes(), name


def check_end_to_end():
    """Segmentor.predict(refine=True, d=4): same maps, same table shapes and classes as refine=False, and the
    coordinates of utils.peak_refinement applied to the preprocessed frames and the unrefined centres."""
    import atomai_amd as aoi
    from atomai_amd.utils import peak_refinement
    rs = np.random.RandomState(4)
    yy, xx = np.mgrid[:32, :48]
    x = np.zeros((2, 32, 48))
    for k in range(2):
        for r in range(6, 30, 7):
            for c in range(6, 46, 7):
                rr, cc = r + rs.uniform(-1, 1), c + rs.uniform(-1, 1)
                x[k] += np.exp(-((yy - rr) ** 2 + (xx - cc) ** 2) / (2 * 1.4 ** 2))
    x = (x + 0.02 * rs.randn(*x.shape)).astype(np.float32)
    m = aoi.models.Segmentor("Unet", nb_classes=3, nb_filters=4)
    THRESH = 0.472          # the untrained net's class-0 probabilities span 0.462 .. 0.474: ~20 blobs per frame
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dec0, c0 = m.predict(x, thresh=THRESH, num_batches=2)
        dec1, c1 = m.predict(x, refine=True, d=4, thresh=THRESH, num_batches=2)
        images, dec2 = m.predict(x, compute_coords=False, return_image=True)
    assert dec1.dtype == dec0.dtype and np.array_equal(dec0, dec1) and np.array_equal(dec0, dec2)
    assert images.shape == (2, 32, 48, 1)
    assert sorted(c0) == sorted(c1) == [0, 1] and sum(len(v) for v in c0.values()) > 0
    moved = 0
    for i in c0:
        assert c1[i].shape == c0[i].shape and c1[i].dtype == np.float64
        assert np.array_equal(c1[i][:, 2], c0[i][:, 2])
        assert np.array_equal(c1[i], peak_refinement(images[i, ..., 0], c0[i], 4)), i
        moved += int((c1[i][:, :2] != c0[i][:, :2]).any(axis=1).sum())
    print(f"end to end: {sum(len(v) for v in c0.values())} atoms, {moved} moved by the fit")
    assert moved > 0


@contextlib.contextmanager
def no_launch():
    """Fails the test if any kernel entry point is called inside."""
    from atomai_amd import _lib as L
    orig = L.call

    def refuse(name, *a):
        raise AssertionError(f"{name} was launched")
    L.call = refuse
    try:
        yield
    finally:
        L.call = orig


def check_edges(device):
    import atomai_amd as aoi
    from atomai_amd.predictors import Locator, SegPredictor
    from atomai_amd.utils import peak_refinement
    f, prob = _half_prob()
    img4 = f["img"][None, ..., None]
    net = aoi.models.Segmentor("Unet", nb_classes=1, nb_filters=4).net
    seg = {d: SegPredictor(net, refine=True, d=d, nb_classes=1, downsampling=8) for d in (1, 4, 33)}
    with no_launch():
        for d in (0, 1, 33, -2):
            with pytest.raises(ValueError):
                peak_refinement(f["img"], f["coords"], d)
            with pytest.raises(ValueError):
                Locator(refine=True, d=d, device=device).run(prob, img4)
        with pytest.raises(AssertionError, match="Pass input image"):
            Locator(refine=True, d=4, device=device).run(prob)
        with pytest.raises(ValueError, match="frame 0"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            peak_refinement(f["img"], f["coords"][:2])
        for d in (1, 33):
            with pytest.raises(ValueError):
                seg[d].run(f["img"][:32, :32])
        with pytest.raises(NotImplementedError):
            seg[4].run(f["img"][:32, :32], distributed=True)
        got = peak_refinement(f["img"], np.empty((0, 3)), 4)
        assert got.shape == (0, 3) and got.dtype == np.float64
    # d=None, two atoms, through the Locator: the reference's warning, then the refusal
    with pytest.raises(ValueError, match="frame 0"), pytest.warns(UserWarning, match="d-value for bounding box"):
        two = np.zeros_like(prob)
        two[..., 1] = 1.0
        two[0, 20:22, 14:16, 0] = two[0, 41:43, 52:54, 0] = 0.9
        Locator(refine=True, device=device).run(two, img4)
    empty = np.zeros((2,) + prob.shape[1:], dtype=np.float32)
    got = Locator(refine=True, d=4, device=device).run(empty, np.concatenate((img4, img4)))
    assert sorted(got) == [0, 1] and all(v.shape == (0, 3) and v.dtype == np.float64 for v in got.values())
    # a row whose frame index is outside the stack is kept and flagged (status 4), its neighbours are fitted
    from atomai_amd.predictors.locator import refine_device
    frames = torch.from_numpy(f["img"][None]).to(device)
    xy = torch.from_numpy(np.ascontiguousarray(f["coords"][:3, :2])).to(device)
    meta = torch.tensor([[0, 0], [1, 0], [-1, 0]], dtype=torch.int32, device=device)
    out, status = refine_device(frames, xy, meta, 4, return_status=True)
    assert status.cpu().tolist() == [0, 4, 4] and np.array_equal(out.cpu().numpy()[1:], f["coords"][1:3, :2])
    # with refine=False nothing changes: images passed along are ignored
    assert np.array_equal(Locator(device=device).run(prob, img4)[0], f["coords"])
