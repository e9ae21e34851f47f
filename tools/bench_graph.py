"""Benchmark of the graph analysis of atom tables (csrc/graph.hip) on the MI355X:

    python tools/bench_graph.py [--out profiles/graph_bench.log] [--tests-log profiles/graph_tests.log]

64 frames of a 32 x 32-cell jittered honeycomb (4 096 sites) with 1 % vacancies, one class, about 4 055 atoms each.
Times, as the median of 20 wall-clock measurements around a synchronised call, at ring sizes up to L = 8 and L = 10:
``_graph.bonds`` (amx_bond_count + prefix sum + amx_bond_emit, the tile table's upload and the one read-back
included), the ring pair alone (amx_ring_count + prefix sum + amx_ring_emit on a device CSR, the read-back of the
total included), ``_graph.rings`` (the pair and the torch sorts), ``_graph.components`` (all rounds), and
``find_cycles_frames`` from the host dictionary to the host dictionary (median of 3).  In the same run a plain-Python
search written here (depth-first enumeration from every atom, breadth-first distances for the shortest-path test) is
timed on the FIRST frame only, once per L, and its rings are compared with the device's.  Prints one JSON line and
writes the log.  ``--tests-log`` also runs the checks of tests/_graph_checks.py on the device and writes the figures
they print to that file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RADII = {"C": 75.0}
PX2ANG = 0.104


def wall(fn, n):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts, out


def movie(frames, cells, rng):
    import _graph_checks as K
    lattice = K.honeycomb(cells, cells)
    tables = {}
    for f in range(frames):
        keep = rng.random(len(lattice)) >= 0.01
        xy = lattice[keep] + rng.uniform(-0.07, 0.07, (int(keep.sum()), 2))
        tables[f] = np.concatenate((xy / PX2ANG, np.zeros((len(xy), 1))), axis=1)
    return tables


def host_rings(adj, L):
    """Plain Python: every simple cycle of 3 .. L atoms from its smallest atom, in one direction, kept if no pair of
    its atoms is closer in the graph than round the cycle (breadth-first search from each of its atoms, memoised)."""
    memo = {}

    def dist_from(s, depth):
        if s not in memo:
            seen, front, d = {s: 0}, [s], 0
            while front and d < depth:
                d += 1
                nxt = []
                for v in front:
                    for w in adj[v]:
                        if w not in seen:
                            seen[w] = d
                            nxt.append(w)
                front = nxt
            memo[s] = seen
        return memo[s]

    rings, candidates = [], 0
    for root in range(len(adj)):
        stack = [(root, iter(adj[root]))]
        path = [root]
        while stack:
            v, it = stack[-1]
            w = next(it, None)
            if w is None:
                stack.pop()
                path.pop()
                continue
            if w == root:
                l = len(path)
                if l >= 3 and path[1] < v:
                    candidates += 1
                    if all(dist_from(path[j], L // 2).get(path[k], L) >= min(k - j, l - (k - j))
                           for j in range(l) for k in range(j + 2, l)):
                        rings.append(tuple(sorted(path)))
            elif w > root and len(path) < L and w not in path:
                path.append(w)
                stack.append((w, iter(adj[w])))
    return sorted(rings, key=lambda r: (len(r), r)), candidates


def write_tests_log(path, device="cuda"):
    """Runs the checks of tests/_graph_checks.py on the device and keeps what they print; a check that fails raises
    here as it does under pytest."""
    import contextlib
    import io
    import _graph_checks as K
    buf = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        for name in K.cases():
            K.check_case(name, device)
        for check in (K.check_tiny, K.check_dense, K.check_frames, K.check_cutoff, K.check_determinism, K.check_validation):
            check(device)
            print(f"{check.__name__}: passed")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("# python tools/bench_graph.py --tests-log: the figures printed by the checks of tests/_graph_checks.py "
                 "(csrc/graph.hip against the restatement of the rules and the golden tests/golden/graph.npz recorded from "
                 f"the reference); every check passed, {time.perf_counter() - t0:.1f} s in all\n")
        fh.write(buf.getvalue())
    print(f"wrote {path}: {len(buf.getvalue().splitlines())} lines")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_bench.log"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tests-log", default=None, help="also run the checks on the device and write their figures here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph.py measures on the GPU; none is visible")
    if args.tests_log:
        write_tests_log(args.tests_log)
    run(args)


def run(args):
    from atomai_amd import _lib as L
    from atomai_amd.utils import _graph, graphx

    rng = np.random.default_rng(0)
    tables = movie(args.frames, args.cells, rng)
    md, kw = {0: "C"}, {"radii": RADII}
    p = graphx._Pass(list(tables.values()), md, PX2ANG, 1.2, RADII)            # warm-up: library load, allocator
    N, seg = p.N, p.seg
    pts = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    pts[:, :2] = torch.from_numpy(np.concatenate([t[:, :2] for t in p.scaled])).cuda()
    cls = torch.zeros(N, dtype=torch.int32, device="cuda")
    cut2 = torch.tensor([[(1.2 * 1.5) ** 2]], dtype=torch.float64, device="cuda")
    med = lambda ts: float(np.median(ts))                                  # noqa: E731
    fmt = lambda ts: f"{med(ts) * 1e3:9.3f} ms (min {min(ts) * 1e3:.3f} max {max(ts) * 1e3:.3f})"     # noqa: E731
    t_b, (rowptr, col) = wall(lambda: _graph.bonds(pts, cls, cut2, seg), args.reps)
    assert torch.equal(rowptr, p.rowptr) and torch.equal(col, p.col)
    t_c, (parent, rounds) = wall(lambda: _graph.components(rowptr, col), args.reps)
    deg = (rowptr[1:] - rowptr[:-1]).cpu().numpy()
    M = len(col)
    sp = L.stream_ptr(rowptr)

    def ring_pair(size):
        count = torch.zeros(N, dtype=torch.int64, device="cuda")
        L.call("amx_ring_count", L.ptr(rowptr), L.ptr(col), N, M, size, L.ptr(count), sp)
        offs = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(count, 0, out=offs[1:])
        R = int(offs[-1].item())
        ring = torch.empty((R, 16), dtype=torch.int32, device="cuda")
        length = torch.empty(R, dtype=torch.int32, device="cuda")
        L.call("amx_ring_emit", L.ptr(rowptr), L.ptr(col), N, M, size, L.ptr(offs), R, L.ptr(ring), L.ptr(length), sp)
        return R

    res = {"metric": f"find_cycles_frames of {args.frames} frames, {N} atoms, rings up to 10, host to host", "unit": "s",
           "n_gpus": 1, "dtype": "fp64/int", "reps": args.reps, "atoms": N, "bonds": M // 2,
           "ms_bonds": round(med(t_b) * 1e3, 3), "ms_components": round(med(t_c) * 1e3, 3), "component_rounds": rounds}
    log = [f"# python tools/bench_graph.py - {args.frames} frames of a {args.cells} x {args.cells}-cell jittered honeycomb "
           f"with 1 % vacancies, one class: {N} atoms ({int(np.diff(seg).min())} .. {int(np.diff(seg).max())} per frame), "
           f"{M // 2} bonds, degree {int(deg.min())} .. {int(deg.max())}; medians of {args.reps} wall-clock measurements "
           "around a synchronised call",
           f"_graph.bonds (count, prefix sum, emit; tile table upload and one read-back included)   {fmt(t_b)}",
           f"_graph.components of the whole bond graph ({rounds} rounds, one scalar read back each)      {fmt(t_c)}; "
           f"{len(torch.unique(parent))} components"]
    adj0 = [c.tolist() for c in np.split(p.col.cpu().numpy()[:int(p.rowptr[seg[1]])], p.rowptr.cpu().numpy()[1:seg[1]])]
    for size in (8, 10):
        t_p, R = wall(lambda: ring_pair(size), args.reps)
        t_r, (ring, length, rseg) = wall(lambda: _graph.rings(rowptr, col, seg, size), args.reps)
        cycles = list(range(3, size + 1))
        t_f, out = wall(lambda: graphx.find_cycles_frames(tables, cycles, md, PX2ANG, **kw), 3)
        sizes = np.bincount(length.cpu().numpy(), minlength=size + 1)[3:].tolist()
        t0 = time.perf_counter()
        host, candidates = host_rings(adj0, size)
        t_h = time.perf_counter() - t0
        dev0 = [tuple(r[:n].tolist()) for r, n in zip(ring[:rseg[1]].cpu().numpy(), length[:rseg[1]].cpu().numpy())]
        same = host == dev0
        res.update({f"ms_ring_pair_L{size}": round(med(t_p) * 1e3, 3), f"ms_rings_L{size}": round(med(t_r) * 1e3, 3),
                    f"s_find_cycles_frames_L{size}": round(med(t_f), 4), f"rings_L{size}": R,
                    f"s_host_python_first_frame_L{size}": round(t_h, 3), f"host_rings_identical_L{size}": same})
        log += [f"L = {size}: amx_ring_count + prefix sum + amx_ring_emit (read-back of the total included)         {fmt(t_p)}; "
                f"{R} rings, sizes 3..{size}: {sizes}",
                f"L = {size}: _graph.rings (the pair and {size + 2} stable torch sorts)                                  "
                f"{fmt(t_r)}",
                f"L = {size}: find_cycles_frames(cycles={cycles}), host dictionary in, host dictionary out   "
                f"{med(t_f):9.4f} s (median of 3; {sum(len(v) for v in out.values())} rows)",
                f"L = {size}: plain-Python search on the host, FIRST frame only ({len(adj0)} atoms), one measurement: "
                f"{t_h:.2f} s, {candidates} cycles tested, {len(host)} rings; identical to the device's rings of that "
                f"frame: {same}"]
    res["value"] = res["s_find_cycles_frames_L10"]
    log.append("NOT measured: the reference itself (it does not run without mendeleev), a host search on all frames, "
               "hardware counters of the ring kernel (divergence, occupancy, load balance between roots)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(log) + "\n")
    print("\n".join(log))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
