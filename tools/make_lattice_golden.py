"""Generates tests/golden/lattice.npz from the REAL reference and from scikit-learn (dev container only; never imported
by a test; needs numpy and scikit-learn there):

    python tools/make_lattice_golden.py

The reference's atomai/utils/imgen.py is imported BY FILE PATH (its package ``__init__`` pulls in libraries that are
not installed); atomai/utils/img.py comes through oracle/ref_harness.py, which stubs cv2.

Stamps.  s|<scale>|<rmask>|atom, |mask: ``create_atom_mask_pair(scale, rmask, 2)`` for the pairs of
``_lattice_checks.STAMP_PAIRS`` and (8, 5); s|rot|*: ``MakeAtom(7, 5, 1, theta=1, offset=.25)``; s|default|mask.

Masks.  m|names lists the cases; case c holds m|c|kind ('single' = create_lattice_mask, 'multi_' =
create_multiclass_lattice_mask_, 'multi' = create_multiclass_lattice_mask), m|c|hw, m|c|n frames, m|c|t|f the table of
frame f, m|c|scale, m|c|rmask, m|c|custom (0 = default stamps, 1 / 2 = ``custom_stamp`` / ``big_stamp`` of
tests/_lattice_checks.py), m|c|lat_dtype, m|c|err (1: the reference raised ValueError; then m|c|bad = (frame, row) of
the first row the restatement refuses), and the reference's result m|c|out (or m|c|out|f where it returned a list).
Before anything is written this script ASSERTS, on every case, that ``case_rule`` of tests/_lattice_checks.py returns
exactly what the reference returned (values, dtype, shape, array or list), and an error exactly where it raised.

Patches.  p|frames (3, 37, 53) float64, p|mask2 (3, 37, 53) float64, p|mask3 (3, 37, 53, 3) float32; for setting k of
``PATCH_SETTINGS`` = (patch, n, seed): p|k|X, p|k|Y2, p|k|Y3 = scikit-learn's ``extract_patches_2d(frame, patch,
max_patches=n, random_state=seed)`` of every frame, concatenated (what the reference's extract_patches returns).

Random sub-images.  r|frames (2, 48, 40, 1), r|coords|f, r|ws, r|n; after ``np.random.seed(0)`` each: r|px|j =
extract_random_subimages(frames, ws, n), r|xy|j = the same on frames[..., 0] with the coordinates and coord_class=1,
r|randpx|j = imcrop_randpx(frames[0], ws, n), r|randcoord|j = imcrop_randcoord(frames[1, ..., 0], coords[1][:, :2], ws, n)
(ASSERTED: it drops at least one window).
TEST INFRASTRUCTURE ONLY.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness  # noqa: E402
import _lattice_checks as K  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
H, W = 37, 53


def reference_imgen():
    path = os.path.join(ref_harness.REFERENCE_ROOT, "atomai", "utils", "imgen.py")
    spec = importlib.util.spec_from_file_location("reference_imgen", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scatter(rng, n, classes=None, lo=4.6, h=H, w=W):
    """n positions whose stamps of side <= 7 lie inside the frame, many of them overlapping; a class column if asked."""
    xy = np.column_stack((rng.uniform(lo, h - lo + 1, n), rng.uniform(lo, w - lo + 1, n)))
    return xy if classes is None else np.column_stack((xy, rng.choice(classes, n).astype(np.float64)))


def cases():
    rng = np.random.default_rng(2026)
    c = {}

    def add(name, kind, tables, scale=7, rmask=None, custom=0, lat="float64", hw=(H, W)):
        c[name] = {"name": name, "kind": kind, "tables": [np.asarray(t, dtype=np.float64) for t in tables], "hw": hw,
                   "scale": scale, "rmask": (5 if kind == "single" else 7) if rmask is None else rmask, "custom": custom,
                   "lat_dtype": lat}

    t40 = scatter(rng, 40)
    add("single40", "single", [t40])
    add("single_f32", "single", [t40], lat="float32")
    add("single_int", "single", [t40], lat="int32")
    add("single_empty", "single", [np.zeros((0, 2))])
    add("stack3", "multi", [scatter(rng, 40, (0, 1)), np.zeros((0, 3)), [[20.2, 30.7, 2.0]]])
    add("stack_same", "multi", [scatter(rng, 20, (0, 1)), scatter(rng, 20, (0, 1))])
    add("ov_ab", "single", [[(15, 20), (17, 21)]])
    add("ov_ba", "single", [[(17, 21), (15, 20)]])
    add("ov3", "single", [[(15, 20), (17, 21), (16, 18)]])
    add("ov_same", "single", [[(15, 20), (15, 20)]])
    add("ov_channels", "multi_", [[(15, 20, 1), (17, 21, 2), (25, 30, 2), (27, 31, 2), (16, 19, 1)]])
    add("round", "single", [[(10.5, 10.5), (11.5, 20.5), (20.4999999, 30.5000001), (21.5000001, 40.4999999),
                              (28.5, 11.5), (29.4999999, 21.5000001)]])
    add("edge_top", "single", [[(3, 20)]])
    add("edge_bottom", "single", [[(H - 2, 20)]])
    add("edge_left", "single", [[(20, 3)]])
    add("edge_right", "single", [[(20, W - 2)]])
    add("corners", "single", [[(3, 3), (3, W - 2), (H - 2, 3), (H - 2, W - 2)]])
    add("err_top", "single", [[(2, 20)]])
    add("err_bottom", "single", [[(H - 1, 20)]])
    add("err_left", "single", [[(20, 2)]])
    add("err_right", "single", [[(20, W - 1)]])
    add("err_two", "single", [[(H - 1, 20), (20, 2)]])
    add("err_frame1", "multi", [scatter(rng, 3, (1, 2)), [(20, 20, 1), (20, W - 2, 1), (10, 10, 2), (2, 2, 2)]])
    for (sc, rm), side in zip(K.STAMP_PAIRS, (1, 3, 5, 7, 15)):
        lo = side / 2 + 1.1
        add(f"side{side}", "single", [scatter(rng, 8, lo=lo)], scale=sc, rmask=rm)
    add("side63", "single", [[(32, 32), (33, 35)]], custom=2, hw=(64, 66))
    add("cls01", "multi_", [scatter(rng, 12, (0, 1))])
    add("cls25", "multi_", [scatter(rng, 12, (2, 5))])
    add("cls1", "multi_", [scatter(rng, 6, (3,))])
    add("cls_empty", "multi_", [np.zeros((0, 3))])
    add("custom_single", "single", [[(15, 20), (17, 21), (16, 18), (30, 40)]], custom=1)
    pile = [(15 + k % 2, 20 + k // 2, z) for k, z in enumerate((1, 2, 3, 4, 4, 3, 2, 1))]
    add("custom4", "multi_", [pile + scatter(rng, 10, (1, 2, 3, 4)).tolist()], custom=1)
    add("custom_stack", "multi", [[(15, 20, 0), (16, 21, 1), (15, 22, 2)] + scatter(rng, 8, (0, 1, 2)).tolist(),
                                  [(25, 30, 2), (25, 31, 1), (26, 30, 0)] + scatter(rng, 8, (0, 1, 2)).tolist()], custom=1)
    return c


def run_reference(R, case):
    """The reference's function on copies of the inputs: its result, or 'error' if it raised ValueError."""
    h, w = case["hw"]
    args = (K.CUSTOM[case["custom"]],) if case["custom"] else ()
    kw = {"scale": case["scale"], "rmask": case["rmask"]}
    tables = [t.copy() for t in case["tables"]]
    try:
        if case["kind"] == "single":
            return R.create_lattice_mask(np.zeros((h, w), dtype=case["lat_dtype"]), tables[0], *args, **kw)
        if case["kind"] == "multi_":
            return R.create_multiclass_lattice_mask_(np.zeros((h, w)), tables[0], *args, **kw)
        return R.create_multiclass_lattice_mask(np.zeros((len(tables), h, w)), dict(enumerate(tables)), *args, **kw)
    except ValueError:
        return "error"


def main():
    from sklearn.feature_extraction.image import extract_patches_2d
    R = reference_imgen()
    gold = {}
    K._gold = gold                                                          # stamp_rule reads the stamps recorded here
    for sc, rm in K.STAMP_PAIRS + ((8, 5),):
        gold[f"s|{sc}|{rm}|atom"], gold[f"s|{sc}|{rm}|mask"] = R.create_atom_mask_pair(sc, rm, 2)
        print(f"stamp ({sc}, {rm}): side {gold[f's|{sc}|{rm}|mask'].shape[0]}")
    maker = R.MakeAtom(7, 5, 1, theta=1, offset=0.25)
    gold["s|rot|atom"], gold["s|rot|mask"] = maker.atom2dgaussian(), maker.gen_atom_mask()[1]
    gold["s|default|mask"] = R.MakeAtom().gen_atom_mask()[1]
    assert [gold[f"s|{sc}|{rm}|mask"].shape[0] for sc, rm in K.STAMP_PAIRS] == [1, 3, 5, 7, 15]

    all_cases = cases()
    gold["m|names"] = np.array(list(all_cases))
    for name, case in all_cases.items():
        ref, rule = run_reference(R, case), K.case_rule(case)
        p = f"m|{name}|"
        gold[p + "kind"], gold[p + "hw"], gold[p + "n"] = np.array(case["kind"]), np.array(case["hw"]), np.int64(len(case["tables"]))
        gold[p + "scale"], gold[p + "rmask"], gold[p + "custom"] = (np.int64(case[k]) for k in ("scale", "rmask", "custom"))
        gold[p + "lat_dtype"] = np.array(case["lat_dtype"])
        for f, t in enumerate(case["tables"]):
            gold[p + f"t|{f}"] = t
        err = isinstance(ref, str)
        gold[p + "err"] = np.int64(err)
        assert err == (isinstance(rule, tuple) and rule[0] == "error"), name
        if err:
            gold[p + "bad"] = np.array(rule[1])
            print(f"{name}: ValueError, first refused (frame, row) {rule[1]}")
        elif isinstance(ref, list):
            assert isinstance(rule, list) and len(ref) == len(rule) and all(K.same(a, b) for a, b in zip(ref, rule)), name
            for f, a in enumerate(ref):
                gold[p + f"out|{f}"] = a
            print(f"{name}: list of {[a.shape for a in ref]}")
        else:
            assert not isinstance(rule, list) and K.same(ref, rule), name
            gold[p + "out"] = ref
            print(f"{name}: {ref.shape} {ref.dtype}, {int((ref != 0).sum())} non-zero, min {ref.min() if ref.size else 0}")
    assert (gold["m|custom_single|out"] < 0).any()
    swapped = int((gold["m|ov_ab|out"] != gold["m|ov_ba|out"]).sum())
    print(f"two atoms 2 px apart, both table orders: {swapped} pixels differ")
    assert swapped == 2
    assert isinstance(K.case_rule(all_cases["stack3"]), list) and gold["m|stack_same|out"].ndim == 4

    rng = np.random.default_rng(7)
    frames = rng.integers(0, 16, (3, H, W)) / 16.0
    tabs = [scatter(rng, 25, (0, 1)) for _ in range(3)]
    mask2 = np.array([R.create_lattice_mask(np.zeros((H, W)), t[:, :2].copy()) for t in tabs])
    mask3 = R.create_multiclass_lattice_mask(frames, {f: t.copy() for f, t in enumerate(tabs)}).astype(np.float32)
    assert mask3.shape == (3, H, W, 3)
    gold["p|frames"], gold["p|mask2"], gold["p|mask3"] = frames, mask2, mask3
    for k, (ps, n, seed) in enumerate(K.PATCH_SETTINGS):
        for key, stack in (("X", frames), ("Y2", mask2), ("Y3", mask3)):
            gold[f"p|{k}|{key}"] = np.concatenate([extract_patches_2d(a, ps, max_patches=n, random_state=seed) for a in stack])
        print(f"patches {ps} n {n} seed {seed}: {gold[f'p|{k}|X'].shape} {gold[f'p|{k}|Y3'].shape}")

    ref_harness.import_reference()
    from atomai.utils import img as ref_img
    rh, rw, ws, n = 48, 40, 8, 5
    rframes = rng.integers(0, 16, (2, rh, rw, 1)) / 16.0
    coords = {}
    for f in range(2):
        inner = scatter(rng, 16, (0, 1), lo=6.0, h=rh, w=rw)
        rim = np.column_stack((rng.uniform(0, 3, 14), rng.uniform(0, rw - 1, 14), rng.integers(0, 2, 14)))
        coords[f] = np.concatenate((inner, rim))[rng.permutation(30)]
    gold["r|frames"], gold["r|ws"], gold["r|n"] = rframes, np.int64(ws), np.int64(n)
    for f in coords:
        gold[f"r|coords|{f}"] = coords[f]
    runs = {"px": lambda: ref_img.extract_random_subimages(rframes, ws, n),
            "xy": lambda: ref_img.extract_random_subimages(rframes[..., 0], ws, n, coordinates=coords, coord_class=1),
            "randpx": lambda: ref_img.imcrop_randpx(rframes[0], ws, n),
            "randcoord": lambda: ref_img.imcrop_randcoord(rframes[1, ..., 0], coords[1][:, :2], ws, n)}
    for key, fn in runs.items():
        np.random.seed(0)
        out = fn()
        for j, a in enumerate(out):
            gold[f"r|{key}|{j}"] = np.asarray(a)
        print(f"random sub-images {key}: {[np.asarray(a).shape for a in out]}")
    assert 0 < len(gold["r|randcoord|0"]) < n

    path = os.path.join(GOLD, "lattice.npz")
    np.savez_compressed(path, **gold)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
