"""Benchmark of the training-set kernels (csrc/lattice.hip) on the MI355X:

    python tools/bench_lattice.py [--out profiles/lattice_bench.log] [--tests-log profiles/lattice_tests.log]

64 frames of 1024 x 1024 with 4 000 atoms each on a jittered lattice, two classes, default stamps (side 7).  Times, in
one process and one run:
  * ``create_multiclass_lattice_mask`` end to end, host tables in and host array out (median of 3), and the same call
    with ``as_tensor=True`` (no download);
  * amx_lattice_owner, amx_lattice_fill (float64 and float32 output) and amx_crop_windows alone, on buffers allocated
    beforehand: medians of 20 wall-clock measurements around a synchronised call, with the bytes each moves (computed
    from the shapes) and the bandwidth that implies.  The crop gathers 64 x 128 windows of 256 x 256 from the float32
    frames and, if the device has room for the 12.9 GB result, from the float64 3-channel masks;
  * the host path it replaces, written here with one numpy slice assignment per atom (all 64 frames) and scikit-learn's
    ``extract_patches_2d`` (the FIRST ``--host-frames`` frames only), with the results compared for equality.
Prints one JSON line and writes the log.  ``--tests-log`` also runs every check of tests/_lattice_checks.py on the device
and writes their outcome to that file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"                                               # (a rehearsal of the host logic on the emulator sets "cpu")


def sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


def wall(fn, n):
    ts = []
    for _ in range(n):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts, out


def movie(frames, per_frame, size, rng):
    """Locator-style tables of atoms on a lattice of spacing 16 jittered by +-3 px, classes 0 / 1, and float32 frames."""
    side = size // 16
    ij = 16 * np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) + 8
    tables = {}
    for f in range(frames):
        pick = ij[rng.permutation(len(ij))[:per_frame]]
        xy = pick + rng.uniform(-3.0, 3.0, pick.shape)
        tables[f] = np.concatenate((xy, rng.integers(0, 2, (per_frame, 1))), axis=1)
    return rng.uniform(0.0, 1.0, (frames, size, size)).astype(np.float32), tables


def host_masks(shape, tables, stamp):
    """The path the device replaces: one slice assignment per atom per frame, then the background (plain numpy; this is
    NOT the code under test)."""
    m = stamp.shape[0]
    r1, r2 = int(m / 2 + .5), int(m / 2 - .5)
    out = np.zeros(shape + (3,))
    for f, table in tables.items():
        for (x, y), c in zip(np.around(table[:, :2]).astype(int), table[:, 2].astype(int)):   # classes 0, 1 = channels
            out[f, x - r1:x + r2, y - r1:y + r2, c] = stamp
    out[..., 2] = 1 - (out[..., 0] + out[..., 1])
    out[out < 0] = 0
    return out


def write_tests_log(path, device="cuda"):
    """Every check of tests/_lattice_checks.py on the device; a check that fails raises here as it does under pytest."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _lattice_checks as K
    lines = []

    def ran(what, fn, *a):
        fn(*a)
        lines.append(f"{what}: equal to the reference bit for bit")

    ran("MakeAtom / create_atom_mask_pair", K.check_make_atom)
    for name in K.mask_cases():
        ran(f"mask case {name}" + (" (ValueError, first refused row named)" if K.load_case(name)["err"] else ""),
            K.check_mask_case, name)
    ran("class column left unchanged", K.check_input_unchanged)
    ran("amx_lattice_owner guards", K.check_owner_kernel, device)
    ran("amx_lattice_fill float32 / float64 / background", K.check_fill_dtypes, device)
    ran("as_tensor", K.check_as_tensor)
    ran("amx_crop_windows", K.check_crop, device)
    for k in range(len(K.PATCH_SETTINGS)):
        ran(f"extract_patches setting {K.PATCH_SETTINGS[k]}", K.check_patches, k)
    ran("extract_random_subimages", K.check_random_subimages)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("# python tools/bench_lattice.py --tests-log: the checks of tests/_lattice_checks.py on the device "
                 "(csrc/lattice.hip against the numpy restatement and the golden tests/golden/lattice.npz); every "
                 "comparison is exact equality and every check passed\n")
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {path}: {len(lines)} lines")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice_bench.log"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--per-frame", type=int, default=4000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--patch", type=int, default=256)
    ap.add_argument("--patches", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--tests-log", default=None, help="also run the checks on the device and write their outcome here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lattice.py measures on the GPU; none is visible")
    if args.tests_log:
        write_tests_log(args.tests_log)
    run(args)


def run(args):
    from atomai_amd import _lib as L
    from atomai_amd.utils import _lattice as T, img, imgen

    rng = np.random.default_rng(0)
    F, S, N = args.frames, args.size, args.frames * args.per_frame
    frames, tables = movie(F, args.per_frame, S, rng)
    med = lambda ts: float(np.median(ts))                                  # noqa: E731
    span = lambda ts: f"min {min(ts) * 1e3:.3f} max {max(ts) * 1e3:.3f}"    # noqa: E731
    imgen.create_multiclass_lattice_mask(frames[:2], {0: tables[0], 1: tables[1]})      # warm-up: library, allocator
    t_e2e, masks = wall(lambda: imgen.create_multiclass_lattice_mask(frames, tables), 3)
    t_dev, masks_d = wall(lambda: imgen.create_multiclass_lattice_mask(frames, tables, as_tensor=True), 3)
    assert masks.shape == (F, S, S, 3) and np.array_equal(masks_d.cpu().numpy(), masks)

    # the two kernels alone, on the wrapper's own table layout
    stamp = imgen.create_atom_mask_pair(7, 7, 1)[1]
    flat = np.concatenate([tables[f] for f in range(F)])
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)      # noqa: E731
    xy = up(flat[:, :2], np.float64)
    meta = up(np.column_stack((np.repeat(np.arange(F), args.per_frame), flat[:, 2], flat[:, 2])), np.int32)
    sside, soff = up([stamp.shape[0]] * 2, np.int32), up([0, stamp.size], np.int64)
    stamps, nch = up(np.concatenate((stamp.ravel(), stamp.ravel())), np.float64), up([2] * F, np.int32)
    own = torch.zeros((F, S, S, 2), dtype=torch.int32, device=DEV)
    bad = torch.full((), T.INT_MAX, dtype=torch.int32, device=DEV)
    t_zero, _ = wall(lambda: own.zero_(), args.reps)
    t_own, _ = wall(lambda: L.call("amx_lattice_owner", L.ptr(xy), L.ptr(meta), N, L.ptr(sside), 2, F, S, S, 2,
                                   L.ptr(own), L.ptr(bad), L.stream_ptr(own)), args.reps)
    assert int(bad) == T.INT_MAX
    t_fill = {}
    for dtype in (torch.float64, torch.float32):
        out = torch.empty((F, S, S, 3), dtype=dtype, device=DEV)
        t_fill[dtype], _ = wall(lambda: L.call("amx_lattice_fill", L.ptr(own), L.ptr(xy), L.ptr(meta), N, L.ptr(sside),
                                               L.ptr(soff), 2, L.ptr(stamps), stamps.shape[0], L.ptr(nch), F, S, S, 2, 1,
                                               L.ptr(out), int(dtype == torch.float64), L.stream_ptr(own)), args.reps)
        assert np.array_equal(out[:2].cpu().numpy(), masks[:2].astype(out[:2].cpu().numpy().dtype))
    del out
    npix = F * S * S
    b_own = N * (16 + 12) + N * stamp.size * 4
    b_fill = {torch.float64: npix * (2 * 4 + 3 * 8), torch.float32: npix * (2 * 4 + 3 * 4)}

    # the gather: the offsets of extract_patches (the same for every frame), all frames in one launch
    ph, pw, i, j = img._patch_offsets(S, S, args.patch, args.patches, 0)
    win = up(np.column_stack((np.repeat(np.arange(F), len(i)), np.tile(i, F), np.tile(j, F))), np.int32)
    crops = []
    sources = [("float32 frames, 1 channel", torch.from_numpy(frames[..., None]).to(DEV))]
    need = len(win) * ph * pw * 3 * 8
    if DEV != "cuda" or torch.cuda.mem_get_info()[0] > need + (8 << 30):
        sources.append(("float64 masks, 3 channels", masks_d))
    for what, src in sources:
        dst = torch.empty((len(win), ph, pw, src.shape[-1]), dtype=src.dtype, device=DEV)
        flag = torch.empty(len(win), dtype=torch.int32, device=DEV)
        t_crop, _ = wall(lambda: L.call("amx_crop_windows", L.ptr(src), src.element_size(), 1, F, S, S, src.shape[-1],
                                        L.ptr(win), len(win), ph, pw, L.ptr(dst), L.ptr(flag), L.stream_ptr(src)), args.reps)
        assert not flag.any()
        k = len(i) + 1                                                     # (window 1 of frame 1)
        assert torch.equal(dst[k], src[1, int(i[1]):int(i[1]) + ph, int(j[1]):int(j[1]) + pw])
        crops.append((what, t_crop, 2 * dst.numel() * dst.element_size()))
        del dst
    del masks_d

    hf = min(args.host_frames, F)
    t_pub, (X, Y) = wall(lambda: img.extract_patches(frames[:hf], masks[:hf], args.patch, args.patches), 3)

    # the host path
    t0 = time.perf_counter()
    ref = host_masks((F, S, S), tables, stamp)
    t_host = time.perf_counter() - t0
    same_masks = bool(np.array_equal(ref, masks))
    del ref
    try:
        from sklearn.feature_extraction.image import extract_patches_2d
    except ImportError:
        extract_patches_2d = None
    t_sk = same_patches = None
    if extract_patches_2d is not None:
        t0 = time.perf_counter()
        Xs = np.concatenate([extract_patches_2d(a, (ph, pw), max_patches=args.patches, random_state=0) for a in frames[:hf]])
        Ys = np.concatenate([extract_patches_2d(a, (ph, pw), max_patches=args.patches, random_state=0) for a in masks[:hf]])
        t_sk = time.perf_counter() - t0
        same_patches = bool(np.array_equal(Xs, X) and np.array_equal(Ys, Y))

    gbs = lambda b, ts: b / med(ts) / 1e9                                  # noqa: E731
    res = {"metric": f"create_multiclass_lattice_mask, {F} frames of {S}x{S}, {args.per_frame} atoms each, host to host",
           "value": round(med(t_e2e), 4), "unit": "s", "n_gpus": 1, "dtype": "fp64", "reps": args.reps,
           "s_as_tensor": round(med(t_dev), 4), "ms_owner": round(med(t_own) * 1e3, 3),
           "ms_fill_f64": round(med(t_fill[torch.float64]) * 1e3, 3), "ms_fill_f32": round(med(t_fill[torch.float32]) * 1e3, 3),
           "gbs_fill_f64": round(gbs(b_fill[torch.float64], t_fill[torch.float64]), 1),
           "ms_crop": {w: round(med(t) * 1e3, 3) for w, t, _ in crops},
           "gbs_crop": {w: round(gbs(b, t), 1) for w, t, b in crops},
           "s_host_masks": round(t_host, 3), "masks_equal": same_masks,
           "s_sklearn_patches_first_frames": None if t_sk is None else round(t_sk, 3), "patches_equal": same_patches}
    log = [f"# python tools/bench_lattice.py - {F} frames of {S} x {S}, {args.per_frame} atoms each on a jittered lattice, "
           f"two classes, default stamps (side {stamp.shape[0]}); wall clock around a synchronised call",
           f"create_multiclass_lattice_mask, host tables in, host float64 array ({masks.nbytes / 1e9:.2f} GB) out   "
           f"{med(t_e2e):9.4f} s (median of 3)",
           f"the same with as_tensor=True (uploads, both launches, one scalar read back; no download)        "
           f"{med(t_dev):9.4f} s (median of 3): the rest of the end-to-end time is the download of the result",
           f"zeroing owner ({own.numel() * 4 / 1e6:.0f} MB, torch)                       {med(t_zero) * 1e3:9.3f} ms "
           f"(median of {args.reps}, {span(t_zero)})",
           f"amx_lattice_owner alone, {N} rows                      {med(t_own) * 1e3:9.3f} ms (median of {args.reps}, "
           f"{span(t_own)}); {b_own / 1e6:.1f} MB (28 B per row read, one 4-byte atomic per covered pixel) = "
           f"{gbs(b_own, t_own):.1f} GB/s"]
    for dtype, name in ((torch.float64, "float64"), (torch.float32, "float32")):
        log.append(f"amx_lattice_fill alone, {name} output                    {med(t_fill[dtype]) * 1e3:9.3f} ms (median of "
                   f"{args.reps}, {span(t_fill[dtype])}); {b_fill[dtype] / 1e9:.2f} GB (owner read, output written) = "
                   f"{gbs(b_fill[dtype], t_fill[dtype]):.0f} GB/s")
    for what, t, b in crops:
        log.append(f"amx_crop_windows alone, {len(win)} windows of {ph} x {pw}, {what}   {med(t) * 1e3:9.3f} ms (median of "
                   f"{args.reps}, {span(t)}); {b / 1e9:.2f} GB (read + written) = {gbs(b, t):.0f} GB/s")
    if len(crops) == 1:
        log.append("NOT measured: the gather from the float64 3-channel masks (its result did not fit the free memory)")
    log.append(f"extract_patches, the first {hf} frames and their masks, host to host ({X.nbytes / 1e6:.0f} + "
               f"{Y.nbytes / 1e6:.0f} MB out)   {med(t_pub):9.4f} s (median of 3)")
    log.append(f"host path, same run, one measurement: one numpy slice assignment per atom + background, all {F} frames   "
               f"{t_host:9.3f} s; equal to the device result: {same_masks}")
    if t_sk is None:
        log.append("scikit-learn does not import here: its extract_patches_2d was NOT measured")
    else:
        log.append(f"host path: scikit-learn extract_patches_2d on the first {hf} frames and their masks   {t_sk:9.3f} s; "
                   f"equal to extract_patches here: {same_patches}")
    log.append("NOT measured: kernel times from a profiler trace, frames beyond 1024 x 1024, stamps above side 7, more than "
               "two classes")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(log) + "\n")
    print("\n".join(log))
    print(json.dumps(res))
    if not same_masks or same_patches is False:
        raise SystemExit("the host path and the device path disagree")


if __name__ == "__main__":
    main()
