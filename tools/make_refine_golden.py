"""Generates tests/golden/refine.npz from the REAL reference (imported through oracle/ref_harness.py, dev container
only; never imported by a test):

    python tools/make_refine_golden.py

Every case is one call of the reference's ``peak_refinement`` (atomai/utils/coords.py:179-231) per frame on synthetic
64 x 96 frames (non-square: a row / column swap shows) that carry rotated anisotropic Gaussians (sigma_x != sigma_y,
theta in (0, pi): a swapped x / y or theta sign shows) plus additive noise; the start coordinates are off by up to
+-0.7 px.  Keys of a case ``<c>`` with frames f = 0 ..:

  <c>|img|f  (64, 96) float32       <c>|coords|f  (n, 3) float64 start table      <c>|d|f  half-side
  <c>|ref|f  (n, 3)   the reference's peak_refinement(img, coords, d)
  <c>|popt|f (n, 7)   curve_fit(full_output=True)'s popt (NaN rows: patch rule / failure)     <c>|nfev|f  (n,)
  <c>|margin|f (n,)   | ||popt[1:3] - d|| - 3 |, the distance from the acceptance gate
  <c>|M|f    (n, 2)   the converged minimum in frame coordinates: scipy.optimize.least_squares(method="lm",
                      xtol=ftol=gtol=1e-15) started at popt
  <c>|kind|f (n,)     0 = decided, fitted (reference fitted, nfev <= 800 = half of maxfev, margin >= 0.5)
                      1 = decided, kept for the patch rule (compared exactly)
                      2 = undecided (at most 5 % of a case, asserted here)
                      3 = decided, kept by the gate (the reference's fit converged, with nfev <= 800, 3.5 px or more from
                          the patch centre; compared exactly)
  floor               max |reference - M| over all decided fitted atoms of the file: the reference's own stopping error
  nn|coords|k, nn|d   tables for the default half-side int(mean(two nearest-neighbour distances) * 0.25)
                      (coords.py:205-207); mean * 0.25 lies at least 1e-6 from an integer (asserted here)
TEST INFRASTRUCTURE ONLY.
"""
import os
import sys
import warnings

import numpy as np
from scipy import optimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
H, W = 64, 96
NOISE = 0.02


def synth(rs, centres, d):
    """Frame with one rotated anisotropic Gaussian per centre, widths scaled to the half-side d."""
    x, y = np.mgrid[:H, :W]
    img = np.full((H, W), 0.1)
    base = max(0.9, d / 2.8)
    for (r, c) in centres:
        sx, sy = base * rs.uniform(0.8, 0.95), base * rs.uniform(1.05, 1.25)
        if rs.rand() < 0.5:
            sx, sy = sy, sx
        th = rs.uniform(0.15, np.pi - 0.15)
        amp = rs.uniform(0.6, 1.0)
        a = np.cos(th) ** 2 / (2 * sx ** 2) + np.sin(th) ** 2 / (2 * sy ** 2)
        b = -np.sin(2 * th) / (4 * sx ** 2) + np.sin(2 * th) / (4 * sy ** 2)
        cc = np.sin(th) ** 2 / (2 * sx ** 2) + np.cos(th) ** 2 / (2 * sy ** 2)
        img += amp * np.exp(-(a * (x - r) ** 2 + 2 * b * (x - r) * (y - c) + cc * (y - c) ** 2))
    img += NOISE * rs.randn(H, W)
    return img.astype(np.float32)


def lattice(rs, rows, cols, jitter=0.4):
    return [(r + rs.uniform(-jitter, jitter), c + rs.uniform(-jitter, jitter)) for r in rows for c in cols]


def table(rs, centres, off=0.7):
    t = np.array([(r + rs.uniform(-off, off), c + rs.uniform(-off, off), float(rs.randint(0, 2)))
                  for (r, c) in centres], dtype=np.float64)
    return t.reshape(-1, 3)


def window_of(img, start, d):
    """The 2d x 2d window around the rounded start and its corner, or (None, corner) when it leaves the frame."""
    corner = np.rint(start).astype(np.int64) - d             # np.rint rounds half to even, like np.around
    inside = (corner >= 0).all() and corner[0] + 2 * d <= img.shape[0] and corner[1] + 2 * d <= img.shape[1]
    if not inside:
        return None, corner
    return img[corner[0]:corner[0] + 2 * d, corner[1]:corner[1] + 2 * d], corner


def run_frame(aoi, img, coords, d):
    """The reference's output plus what the checks need to know about every atom."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = aoi.utils.peak_refinement(img, coords, d)
    n = len(coords)
    rec = dict(ref=ref, popt=np.full((n, 7), np.nan), nfev=np.zeros(n, dtype=np.int64), margin=np.full(n, np.nan),
               M=np.full((n, 2), np.nan), kind=np.full(n, 2, dtype=np.int64))
    grid = tuple(np.indices((2 * d, 2 * d)))
    model = aoi.utils.gaussian_2d
    for i in range(n):
        win, corner = window_of(img, coords[i, :2], d)
        if win is None:
            rec["kind"][i] = 1
            assert np.array_equal(ref[i, :2], coords[i, :2])     # the reference kept it
            continue
        data = win.ravel().astype(np.float64)
        guess = np.array([win[d, d], d, d, 1.0, 1.0, 0.0, 0.0])
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fit, _, info, _, _ = optimize.curve_fit(model, grid, win.ravel(), p0=guess, full_output=True)
        except RuntimeError:                                     # scipy gave up: the atom stays undecided
            continue
        shift = np.hypot(fit[1] - d, fit[2] - d)
        rec["popt"][i], rec["nfev"][i], rec["margin"][i] = fit, info["nfev"], abs(shift - 3)
        tight = optimize.least_squares(lambda p: model(grid, *p) - data, fit, method="lm", xtol=1e-15, ftol=1e-15,
                                       gtol=1e-15)
        rec["M"][i] = tight.x[1:3] + corner
        clear = info["nfev"] <= 800 and rec["margin"][i] >= 0.5
        if shift < 3:
            assert np.array_equal(ref[i, :2], fit[1:3] + np.around(coords[i, :2]) - d)
            if clear:
                rec["kind"][i] = 0
        else:
            assert np.array_equal(ref[i, :2], coords[i, :2])     # the reference kept it
            if clear:
                rec["kind"][i] = 3
    return rec


def cases(rs):
    """name -> list of (img, coords, d), one entry per frame."""
    out = {}
    for d, rows, cols in ((2, range(8, 60, 8), range(8, 92, 12)), (4, range(10, 56, 11), range(10, 88, 11)),
                          (5, range(10, 56, 14), range(12, 88, 14)), (9, range(16, 50, 24), range(14, 88, 22))):
        cen = lattice(rs, rows, cols)
        out[f"d{d}"] = [(synth(rs, cen, d), table(rs, cen), d)]
    # atoms 6-8 px from each of the four borders: with d = 8 their patches leave the frame (negative starts at the
    # top / left, truncated slices at the bottom / right); the interior atoms of the same frame are fitted
    cen = [(7.0, 30.2), (6.3, 60.1), (H - 6.9, 30.4), (H - 6.4, 70.3), (30.1, 7.1), (33.0, 6.2), (28.3, W - 7.0),
           (36.2, W - 6.1), (32.4, 30.3), (31.7, 62.2)]
    t = table(rs, cen, off=0.2)
    out["d8_border"] = [(synth(rs, cen, 8), t, 8)]
    for n in (1, 4, 65):                                     # 65: more atoms than one workgroup holds
        cen = lattice(rs, range(7, 58, 8), range(7, 90, 8))
        cen = [cen[i] for i in rs.permutation(len(cen))[:n]]
        out[f"n{n}"] = [(synth(rs, cen, 3), table(rs, cen), 3)]
    multi = []                                               # three frames with different d in one call
    for d, rows, cols in ((3, range(8, 58, 10), range(8, 90, 10)), (6, range(12, 54, 16), range(12, 86, 16)),
                          (4, range(10, 56, 12), range(10, 88, 12))):
        cen = lattice(rs, rows, cols)
        multi.append((synth(rs, cen, d), table(rs, cen), d))
    out["multi"] = multi
    # start coordinates exactly on .5, both parities (np.around: 20.5 -> 20, 21.5 -> 22, 2.5 -> 2, 3.5 -> 4)
    cen = lattice(rs, (20.5, 41.5), (14.5, 33.5, 52.5, 71.5), jitter=0.3)
    t = np.array([(r, c, 0.0) for r in (20.5, 41.5) for c in (14.5, 33.5, 52.5, 71.5)])
    out["half"] = [(synth(rs, cen, 4), t, 4)]
    # (cases below draw from their own generator, so that the ones above keep their data)
    rs = np.random.RandomState(21)
    # d = 32: the whole height of the frame is one patch (64 x 64 pixels, 64 per lane, 64 KB of LDS per workgroup); the
    # second row rounds one pixel lower and its patch leaves the frame
    cen = [(32.2, 47.7)]
    out["d32"] = [(synth(rs, cen, 32), np.array([(31.8, 48.3, 0.0), (32.7, 48.3, 1.0)]), 32)]
    # starts 3.6 - 4.5 px away from their atom with d = 7: the fit converges on the atom, 3 px or more from the patch
    # centre, and the reference keeps the start; two ordinary starts in the same frame
    cen = lattice(rs, (14, 46), (14, 36, 58, 80), jitter=0.3)
    t = np.array([(r + dr, c + dc, 0.0) for (r, c), (dr, dc) in
                  zip(cen, [(3.3, 2.4), (-2.8, 3.4), (0.4, -0.3), (4.3, 0.2), (-3.0, -3.1), (0.2, 4.4), (-0.5, 0.6),
                            (2.9, -3.2)])])
    out["gate"] = [(synth(rs, cen, 7), t, 7)]
    return out


def nn_tables(aoi, rs):
    """Tables for the default half-side: 3 atoms (the minimum), a lattice, more atoms than one tile of 256, and one
    with duplicates; drawn until mean * 0.25 is at least 1e-6 from an integer."""
    out, ds = [], []
    for n, scale in ((3, 30.0), (48, 90.0), (300, 400.0), (700, 900.0)):
        while True:
            c = np.concatenate((rs.rand(n, 2) * scale, rs.randint(0, 2, (n, 1)).astype(np.float64)), axis=1)
            if n == 48:
                c[5, :2] = c[6, :2]                          # duplicates: a nearest-neighbour distance of 0
            dist = np.concatenate((aoi.utils.get_nn_distances_(c)[0]))
            v = np.mean(dist) * 0.25
            if abs(v - np.rint(v)) >= 1e-6 and int(v) >= 2:
                break
        out.append(c)
        ds.append(int(v))
    return out, ds


if __name__ == "__main__":
    aoi = ref_harness.import_reference()
    rs = np.random.RandomState(20)
    gold, floor = {}, 0.0
    for name, frames in cases(rs).items():
        kinds = []
        for f, (img, coords, d) in enumerate(frames):
            r = run_frame(aoi, img, coords, d)
            gold[f"{name}|img|{f}"], gold[f"{name}|coords|{f}"], gold[f"{name}|d|{f}"] = img, coords, np.array(d)
            for k, v in r.items():
                gold[f"{name}|{k}|{f}"] = v
            dec = r["kind"] == 0
            if dec.any():
                floor = max(floor, float(np.abs(r["ref"][dec, :2] - r["M"][dec]).max()))
            kinds.append(r["kind"])
            print(f"{name}[{f}] d={d} n={len(coords)} kinds={np.bincount(r['kind'], minlength=4)} "
                  f"nfev max {r['nfev'].max()} margin min {np.nanmin(r['margin']) if dec.any() else None}")
        kinds = np.concatenate(kinds)
        assert (kinds == 2).sum() <= 0.05 * len(kinds), (name, "too many undecided atoms")
    assert (gold["d8_border|kind|0"] == 1).sum() == 8 and (gold["half|kind|0"] == 0).all()
    assert gold["d32|kind|0"].tolist() == [0, 1] and (gold["gate|kind|0"] == 3).sum() >= 4
    tabs, ds = nn_tables(aoi, rs)
    for k, t in enumerate(tabs):
        gold[f"nn|coords|{k}"] = t
    gold["nn|d"] = np.array(ds)
    gold["floor"] = np.array(floor)
    path = os.path.join(GOLD, "refine.npz")
    np.savez_compressed(path, **gold)
    print("floor", floor, "nn d", ds, os.path.getsize(path), "bytes")
