"""Benchmark of the intensity-based classes (csrc/intensity.hip) on the MI355X:

    python tools/bench_classes.py [--out profiles/classes_bench.log] [--tests-log profiles/classes_tests.log]

64 frames x 4 000 atoms = 256 000 intensities from three levels (N(0.2 / 0.5 / 0.9, 0.03)).  Times, as the median of 20
wall-clock measurements around a synchronised call, ``estimate_bandwidth``, ``mean_shift`` and ``kmeans(3)`` on the
device table (sorts and read-backs included), and ``update_classes(method='meanshift')`` from a host dictionary and host
frames to a host dictionary (median of 3).  In the same run scikit-learn's ``estimate_bandwidth`` and ``MeanShift`` are
timed on the host on the FIRST 20 000 values only (their cost grows with n^2), with the results compared.  Prints one
JSON line and writes the log.  ``--tests-log`` also runs the kernel and golden checks of tests/_classes_checks.py on the
device and writes the figures they print (the errors of every test case) to that file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(fn, n):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts, out


def movie(frames, per_frame, rng):
    """Frames of 3 x 3 flat atoms on a lattice of spacing 8 and the Locator-style dictionary of their positions."""
    side = int(np.ceil(np.sqrt(per_frame)))
    ij = 8 * np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:per_frame] + 4
    size = 8 * side
    imgs = np.zeros((frames, size, size), dtype=np.float32)
    tables, levels = {}, []
    for f in range(frames):
        level = rng.normal(rng.choice([0.2, 0.5, 0.9], per_frame), 0.03)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                imgs[f, ij[:, 0] + dr, ij[:, 1] + dc] = level
        tables[f] = np.concatenate((ij + rng.uniform(-0.4, 0.4, ij.shape), np.zeros((per_frame, 1))), axis=1)
        levels.append(level)
    return imgs, tables, np.concatenate(levels)


def write_tests_log(path, device="cuda"):
    """Runs the checks that print figures (gap, mean shift per seed, Lloyd, the public functions against the golden)
    and keeps what they print; a check that fails raises here as it does under pytest."""
    import contextlib
    import io
    import warnings
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _classes_checks as K
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for check in (K.check_gap, K.check_seeds, K.check_public):
            for name in K.cases():
                check(name, device)
        K.check_lloyd(device)
        for name in K.km_cases():
            K.check_kmeans(name, device)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("# python tools/bench_classes.py --tests-log: the figures printed by check_gap, check_seeds, check_public, "
                 "check_lloyd and check_kmeans of tests/_classes_checks.py (csrc/intensity.hip against the numpy "
                 "restatement and the scikit-learn golden tests/golden/classes.npz); every check passed\n")
        fh.write(buf.getvalue())
    print(f"wrote {path}: {len(buf.getvalue().splitlines())} lines")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classes_bench.log"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--per-frame", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-rows", type=int, default=20000)
    ap.add_argument("--tests-log", default=None, help="also run the checks on the device and write their figures here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classes.py measures on the GPU; none is visible")
    if args.tests_log:
        write_tests_log(args.tests_log)
    run(args)


def run(args):
    from atomai_amd.stat import intensity

    rng = np.random.default_rng(0)
    imgs, tables, levels = movie(args.frames, args.per_frame, rng)
    N = len(levels)
    x = torch.from_numpy(levels).cuda()
    intensity.mean_shift(x[:5000].contiguous())                            # warm-up: library load, allocator
    intensity.kmeans(x[:5000].contiguous(), 3)
    t_bw, bw = wall(lambda: intensity.estimate_bandwidth(x), args.reps)
    t_ms, ms = wall(lambda: intensity.mean_shift(x), args.reps)
    t_km, km = wall(lambda: intensity.kmeans(x, 3), args.reps)
    t_uc, out = wall(lambda: intensity.update_classes(tables, imgs, method="meanshift"), 3)
    classes = np.concatenate([out[f][:, 2] for f in sorted(out)])
    med = lambda ts: float(np.median(ts))                                  # noqa: E731
    res = {"metric": f"mean shift of {N} intensities ({args.frames} frames x {args.per_frame} atoms), bandwidth included",
           "value": round(med(t_ms) * 1e3, 3), "unit": "ms", "n_gpus": 1, "dtype": "fp64", "reps": args.reps,
           "ms_estimate_bandwidth": round(med(t_bw) * 1e3, 3), "ms_kmeans3": round(med(t_km) * 1e3, 3),
           "s_update_classes_meanshift": round(med(t_uc), 4), "bandwidth": bw, "centres": len(ms["centres"]),
           "n_iter": ms["n_iter"], "kmeans_n_iter": km["n_iter"]}
    log = [f"# python tools/bench_classes.py - {args.frames} frames x {args.per_frame} atoms = {N} intensities from three "
           "levels (N(0.2 / 0.5 / 0.9, 0.03)), fp64",
           f"estimate_bandwidth(quantile=.25), device table in, one scalar out (sort included)   {med(t_bw) * 1e3:9.3f} ms "
           f"(median of {args.reps}, wall clock around a synchronised call, min {min(t_bw) * 1e3:.3f} max "
           f"{max(t_bw) * 1e3:.3f}); bandwidth {bw:.6g}",
           f"mean_shift (bandwidth, seeds, all iterations, centres, labels)                      {med(t_ms) * 1e3:9.3f} ms "
           f"(median of {args.reps}, min {min(t_ms) * 1e3:.3f} max {max(t_ms) * 1e3:.3f}); {len(ms['centres'])} centres, "
           f"n_iter {ms['n_iter']}",
           f"kmeans(3) (k-means++ seeding, Lloyd fit in one launch, labels)                      {med(t_km) * 1e3:9.3f} ms "
           f"(median of {args.reps}, min {min(t_km) * 1e3:.3f} max {max(t_km) * 1e3:.3f}); {km['n_iter']} rounds",
           f"update_classes(method='meanshift'), host dictionary and {imgs.nbytes / 1e6:.0f} MB of host frames in, host "
           f"dictionary out   {med(t_uc):9.4f} s (median of 3; {len(np.unique(classes))} classes)"]
    n = min(args.host_rows, N)
    try:
        from sklearn.cluster import MeanShift, estimate_bandwidth
    except ImportError:
        estimate_bandwidth = None
    if estimate_bandwidth is None:
        res["cpu_baseline"] = None
        log.append("scikit-learn does not import here: the host path was NOT measured")
    else:
        sub = levels[:n]
        t0 = time.perf_counter()
        hbw = float(estimate_bandwidth(sub[:, None], quantile=.25))
        t1 = time.perf_counter()
        fit = MeanShift(bandwidth=hbw, bin_seeding=True).fit(sub[:, None])
        t2 = time.perf_counter()
        xs = torch.from_numpy(sub).cuda()
        t_sub, dms = wall(lambda: intensity.mean_shift(xs), 5)
        same = bool(np.array_equal(dms["labels"].cpu().numpy(), fit.labels_))
        drel = abs(dms["bandwidth"] - hbw) / hbw
        res["cpu_baseline"] = {"rows": n, "s_estimate_bandwidth": round(t1 - t0, 3), "s_meanshift_fit": round(t2 - t1, 3),
                               "bandwidth_rel_diff": drel, "labels_identical": same,
                               "ms_device_same_rows": round(med(t_sub) * 1e3, 3)}
        log.append(f"host, the FIRST {n} values only (the cost grows with n^2), same run, one measurement: "
                   f"sklearn estimate_bandwidth {t1 - t0:.2f} s, MeanShift(bin_seeding=True).fit {t2 - t1:.2f} s; "
                   f"mean_shift here on the same {n} values {med(t_sub) * 1e3:.3f} ms (median of 5); bandwidth rel. "
                   f"difference {drel:.1e}, labels identical: {same}, n_iter {dms['n_iter']} vs {fit.n_iter_}")
        log.append(f"NOT measured: scikit-learn on all {N} values")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(log) + "\n")
    print("\n".join(log))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
