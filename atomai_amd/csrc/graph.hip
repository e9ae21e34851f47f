// graph.hip — graph analysis of atom tables, on the device: bonds, connected components, rings.
//
// Replaces the per-atom Python objects and the recursive searches behind the reference's Graph.find_neighbors,
// polycount + remove_filled_polygons and the networkx components of find_cycle_clusters / filter_subgraphs
// (atomai/utils/graphx.py).  All frames form one flat table with segment offsets (the layout of amx_knn):
//   bond_kernel        one workgroup = one tile of GR_T rows of ONE segment (the tile table of amx_knn), one row per
//                      thread; the segment's points and classes pass through LDS in tiles of GR_T.  First pass: the
//                      degree of every row; second pass, after an exclusive prefix sum: its neighbours in ascending
//                      row order, a CSR.  Brute force per segment.
//   graph_hook_kernel  one hooking round of connected components over a symmetric CSR; alternates with cl_jump_kernel
//                      of cluster.hip (amx_cluster_jump).
//   ring_kernel        one thread per root row: a depth-first enumeration of the simple cycles of 3 .. L rows whose
//                      smallest row is the root, each in one direction only, and on closing a cycle the test below.
//                      First pass: the number of rings per root; second pass: the rings at the root's offset.
// fp64 and integers.  No floating-point atomics; the hooking round applies integer atomicMin to a copy of a snapshot
// (see cluster.hip, "Determinism"); the ring search has no atomics and its order is fixed by the CSR's: two runs give the
// same bits.
//
// Bond rule.  i != j and dx*dx + dy*dy + dz*dz <= cut2[ci][cj], every operation rounded on its own (the library is built
// with -ffp-contract=off), added in that order.  Rows at the same position are bonded.  A comparison with a NaN is false.
//
// Ring rule.  A ring is a simple cycle v_0 .. v_{l-1} of 3 <= l <= L rows such that for every two of its rows no path in
// the WHOLE graph is shorter than the shorter way round the cycle.  Pairs one step apart need no test.  For a pair at
// ring distance d = min(k - j, l - (k - j)) >= 2 the kernel asks whether v_k is reached from v_j by a walk of at most
// d - 1 bonds that never steps straight back (a shortest path does not, and any walk that reaches v_k contains a path
// that is no longer).  d - 1 <= L / 2 - 1 = 7 levels, unrolled by template recursion: the loop state of every level
// lives in registers.  Distances are tested in ascending order, so a chord (d - 1 = 1) rejects a cycle at once.
// The enumeration itself drops a prefix as soon as its new row is bonded to an inner row of the path (a chord of every
// cycle that could follow): the kept set is the same, and the search stays bounded on dense tables, where the number of
// simple paths of 16 rows is astronomical and the number of chordless ones is not.
//
// No scratch.  The path and the neighbour cursors of the enumeration are indexed by the depth, a runtime value; as
// private arrays they would go to scratch memory.  They live in LDS instead, one column per lane ([level][lane]: the
// lanes of a wave touch 64 consecutive words, no bank conflict), 2 x 16 ints per lane.
#include "amx_device.h"

#define GR_T 256                       // rows per workgroup of the bond and hook kernels (= KNN_T: the same tile table)
#define GR_CMAX 16                     // classes
#define RG_T 64                        // roots per workgroup of the ring kernel: one wave, 8 KB of LDS
#define RG_LMAX 16                     // longest ring

__global__ __launch_bounds__(GR_T) void bond_kernel(const double* __restrict__ pts, const int* __restrict__ cls, long N,
                                                    const double* __restrict__ cut2, int C, const long* __restrict__ seg,
                                                    int S, const long* __restrict__ tiles, int emit,
                                                    const long* __restrict__ rowptr, long M, long* __restrict__ deg,
                                                    int* __restrict__ col) {
    __shared__ double s_p[3][GR_T];
    __shared__ int s_c[GR_T];
    __shared__ double s_cut[GR_CMAX * GR_CMAX];
    const int tid = threadIdx.x;
    const long s = tiles[2 * (long)blockIdx.x], q0 = tiles[2 * (long)blockIdx.x + 1];
    if (s < 0 || s >= S) return;                        // (block-uniform: a malformed table reads and writes nothing)
    long lo = seg[s], hi = seg[s + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > N ? N : hi;
    if (q0 < lo || q0 >= hi) return;
    if (tid < C * C) s_cut[tid] = cut2[tid];            // (C <= 16: C * C <= GR_T)
    const long i = q0 + tid;
    const bool live = i < hi;
    const double x = live ? pts[3 * i] : 0.0, y = live ? pts[3 * i + 1] : 0.0, z = live ? pts[3 * i + 2] : 0.0;
    const int ci = live ? cls[i] : -1;
    const bool ok = ci >= 0 && ci < C;                  // a row of no class has no bonds
    const long o = (emit && live) ? rowptr[i] : 0;
    long n = 0;
    for (long tile = lo; tile < hi; tile += GR_T) {     // (block-uniform bounds: every thread reaches the barriers)
        const long j = tile + tid;
        __syncthreads();
        s_p[0][tid] = j < hi ? pts[3 * j] : 0.0;
        s_p[1][tid] = j < hi ? pts[3 * j + 1] : 0.0;
        s_p[2][tid] = j < hi ? pts[3 * j + 2] : 0.0;
        s_c[tid] = j < hi ? cls[j] : -1;
        __syncthreads();
        const int m = (int)(hi - tile < GR_T ? hi - tile : GR_T);
        if (ok) {
            for (int kk = 0; kk < m; ++kk) {
                const int cj = s_c[kk];
                if (cj < 0 || cj >= C || tile + kk == i) continue;
                const double dx = s_p[0][kk] - x, dy = s_p[1][kk] - y, dz = s_p[2][kk] - z;
                if (dx * dx + dy * dy + dz * dz <= s_cut[ci * C + cj]) {
                    if (emit && o >= 0 && o + n < M) col[o + n] = (int)(tile + kk);
                    ++n;
                }
            }
        }
    }
    if (live && !emit) deg[i] = n;
}

__global__ __launch_bounds__(GR_T) void graph_hook_kernel(const long* __restrict__ rowptr, const int* __restrict__ col,
                                                          long N, long M, const int* __restrict__ pin, int* pout,
                                                          int* changed) {
    const long i = (long)blockIdx.x * GR_T + threadIdx.x;
    if (i >= N) return;
    const int ri = pin[i];
    if (ri < 0 || ri >= N) return;
    long b = rowptr[i], e = rowptr[i + 1];
    b = b < 0 ? 0 : b;
    e = e > M ? M : e;
    bool any = false;
    for (long t = b; t < e; ++t) {
        const int j = col[t];
        if (j < 0 || j >= N) continue;
        const int rj = pin[j];
        // the edge is seen from both ends: the end with the larger root hooks that root under the smaller one
        if (rj < ri && rj >= 0) {
            atomicMin(&pout[ri], rj);
            any = true;
        }
    }
    if (any) atomicOr(changed, 1);
}

// Is `target` reached from v by a walk of at most D bonds whose first step does not return to `prev`?
template <int D>
static __device__ __forceinline__ bool rg_reach(const long* __restrict__ rowptr, const int* __restrict__ col, long N,
                                                long M, int v, int prev, int target) {
    long b = rowptr[v], e = rowptr[(long)v + 1];
    b = b < 0 ? 0 : b;
    e = e > M ? M : e;
    for (long t = b; t < e; ++t) {
        const int w = col[t];
        if (w == target) return true;
        if constexpr (D > 1) {
            if (w != prev && w >= 0 && w < N && rg_reach<D - 1>(rowptr, col, N, M, w, v, target)) return true;
        }
    }
    return false;
}

static __device__ __forceinline__ bool rg_within(const long* __restrict__ rowptr, const int* __restrict__ col, long N,
                                                 long M, int a, int b, int depth) {
    switch (depth) {
        case 1: return rg_reach<1>(rowptr, col, N, M, a, -1, b);
        case 2: return rg_reach<2>(rowptr, col, N, M, a, -1, b);
        case 3: return rg_reach<3>(rowptr, col, N, M, a, -1, b);
        case 4: return rg_reach<4>(rowptr, col, N, M, a, -1, b);
        case 5: return rg_reach<5>(rowptr, col, N, M, a, -1, b);
        case 6: return rg_reach<6>(rowptr, col, N, M, a, -1, b);
        default: return rg_reach<7>(rowptr, col, N, M, a, -1, b);      // (depth <= RG_LMAX / 2 - 1 = 7)
    }
}

// emit == 0: count[root] = rings whose smallest row is root.  emit != 0: ring s of the root (in search order) goes to
// slot offs[root] + s: its rows ascending in ring[slot][0 .. l), -1 behind them, len[slot] = l; nothing at or beyond R.
__global__ __launch_bounds__(RG_T) void ring_kernel(const long* __restrict__ rowptr, const int* __restrict__ col, long N,
                                                    long M, int L, int emit, const long* __restrict__ offs, long R,
                                                    long* __restrict__ count, int* __restrict__ ring,
                                                    int* __restrict__ len) {
    __shared__ int s_path[RG_LMAX][RG_T];
    __shared__ int s_cur[RG_LMAX][RG_T];
    const int tid = threadIdx.x;
    const long root = (long)blockIdx.x * RG_T + tid;
    if (root >= N) return;                              // (no barrier in this kernel)
    const long o = emit ? offs[root] : 0;
    long n = 0;
    int top = 0;
    s_path[0][tid] = (int)root;
    s_cur[0][tid] = 0;
    while (top >= 0) {
        const int v = s_path[top][tid], c = s_cur[top][tid];
        long b = rowptr[v], e = rowptr[(long)v + 1];
        b = b < 0 ? 0 : b;
        e = e > M ? M : e;
        if (b + c >= e) { --top; continue; }
        s_cur[top][tid] = c + 1;
        const int w = col[b + c];
        if (w < root || w >= N) continue;               // only rows above the root: the root is the ring's smallest
        if (w == root) {
            // closing bond; one direction only: the second row of the path is below the last
            if (top < 2 || s_path[1][tid] >= v) continue;
            const int l = top + 1;
            bool keep = true;
            for (int d = 2; keep && 2 * d <= l; ++d) {
                const int nj = 2 * d == l ? d : l;       // every pair once: opposite rows of an even cycle pair up
                for (int j = 0; keep && j < nj; ++j) {
                    const int k = j + d < l ? j + d : j + d - l;
                    keep = !rg_within(rowptr, col, N, M, s_path[j][tid], s_path[k][tid], d - 1);
                }
            }
            if (!keep) continue;
            if (emit && o >= 0 && o + n < R) {
                const long slot = o + n;
                int prev = -1;                           // selection: the rows of a path are distinct
                for (int s = 0; s < RG_LMAX; ++s) {
                    int m = -1;
                    if (s < l) {
                        m = 2147483647;
                        for (int p = 0; p < l; ++p) {
                            const int u = s_path[p][tid];
                            m = (u > prev && u < m) ? u : m;
                        }
                        prev = m;
                    }
                    ring[slot * RG_LMAX + s] = m;
                }
                len[slot] = l;
            }
            ++n;
            continue;
        }
        if (top + 1 >= L) continue;
        bool seen = false;
        for (int p = 1; p <= top; ++p) seen = seen || s_path[p][tid] == w;
        if (seen) continue;
        // A bond from w to an inner row of the path (not the last, not the root) is a chord of every cycle through this
        // prefix: the two rows are at least 2 apart round the cycle and 1 apart in the graph.  Dropping the prefix here
        // changes no result and bounds the search on dense tables (a pile of 17 atoms on one spot is a complete graph).
        // The first four neighbours of w are held in registers and share one walk over the path (an atom of a lattice
        // has three or four); any further ones take a walk each.
        if (top >= 2) {
            long wb = rowptr[w], we = rowptr[(long)w + 1];
            wb = wb < 0 ? 0 : wb;
            we = we > M ? M : we;
            const int x0 = wb < we ? col[wb] : -1, x1 = wb + 1 < we ? col[wb + 1] : -1;      // (-1 is no row of a path)
            const int x2 = wb + 2 < we ? col[wb + 2] : -1, x3 = wb + 3 < we ? col[wb + 3] : -1;
            for (int p = 1; p < top; ++p) {
                const int u = s_path[p][tid];
                seen = seen || u == x0 || u == x1 || u == x2 || u == x3;
            }
            for (long t = wb + 4; t < we && !seen; ++t) {
                const int x = col[t];
                for (int p = 1; p < top; ++p) seen = seen || s_path[p][tid] == x;
            }
            if (seen) continue;
        }
        ++top;
        s_path[top][tid] = w;
        s_cur[top][tid] = 0;
    }
    if (!emit) count[root] = n;
}

// ---------------------------------------------------------------------------------------------- C ABI
#define GR_MAXN 2147483647L
static inline dim3 gr_blocks(long n, int t) { return dim3((unsigned)((n + t - 1) / t)); }

static int bond_common(const double* pts, const int* cls, long N, const double* cut2, int C, const long* seg, int S,
                       const long* tiles, long T, int emit, const long* rowptr, long M, long* deg, int* col, void* stream) {
    AMX_LAUNCH(bond_kernel, dim3((unsigned)T), dim3(GR_T), 0, (hipStream_t)stream, pts, cls, N, cut2, C, seg, S, tiles, emit,
               rowptr, M, deg, col);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_bond_count(const double* pts, const int* cls, long N, const double* cut2, int C, const long* seg, int S,
                              const long* tiles, long T, long* deg, void* stream) {
    if (N < 0 || N >= GR_MAXN || S < 0 || T < 0 || T >= GR_MAXN) AMX_BADARG(1);
    if (C < 1 || C > GR_CMAX) AMX_BADARG(2);
    if (N == 0 || S == 0 || T == 0) return 0;
    if (!pts || !cls || !cut2 || !seg || !tiles || !deg) AMX_BADARG(3);
    return bond_common(pts, cls, N, cut2, C, seg, S, tiles, T, 0, nullptr, 0, deg, nullptr, stream);
}

extern "C" int amx_bond_emit(const double* pts, const int* cls, long N, const double* cut2, int C, const long* seg, int S,
                             const long* tiles, long T, const long* rowptr, long M, int* col, void* stream) {
    if (N < 0 || N >= GR_MAXN || S < 0 || T < 0 || T >= GR_MAXN || M < 0) AMX_BADARG(1);
    if (C < 1 || C > GR_CMAX) AMX_BADARG(2);
    if (N == 0 || S == 0 || T == 0 || M == 0) return 0;
    if (!pts || !cls || !cut2 || !seg || !tiles || !rowptr || !col) AMX_BADARG(3);
    return bond_common(pts, cls, N, cut2, C, seg, S, tiles, T, 1, rowptr, M, nullptr, col, stream);
}

extern "C" int amx_graph_hook(const long* rowptr, const int* col, long N, long M, const int* pin, int* pout, int* changed,
                              void* stream) {
    if (N < 0 || N >= GR_MAXN || M < 0) AMX_BADARG(1);
    if (N == 0) return 0;
    if (!rowptr || !pin || !pout || !changed || (M > 0 && !col)) AMX_BADARG(2);
    if (pin == pout) AMX_BADARG(3);
    AMX_LAUNCH(graph_hook_kernel, gr_blocks(N, GR_T), dim3(GR_T), 0, (hipStream_t)stream, rowptr, col, N, M, pin, pout,
               changed);
    AMX_CHECK_LAUNCH();
    return 0;
}

static int ring_common(const long* rowptr, const int* col, long N, long M, int L, int emit, const long* offs, long R,
                       long* count, int* ring, int* len, void* stream) {
    AMX_LAUNCH(ring_kernel, gr_blocks(N, RG_T), dim3(RG_T), 0, (hipStream_t)stream, rowptr, col, N, M, L, emit, offs, R,
               count, ring, len);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_ring_count(const long* rowptr, const int* col, long N, long M, int L, long* count, void* stream) {
    if (N < 0 || N >= GR_MAXN || M < 0) AMX_BADARG(1);
    if (L < 3 || L > RG_LMAX) AMX_BADARG(2);
    if (N == 0) return 0;
    if (!rowptr || !count || (M > 0 && !col)) AMX_BADARG(3);
    return ring_common(rowptr, col, N, M, L, 0, nullptr, 0, count, nullptr, nullptr, stream);
}

extern "C" int amx_ring_emit(const long* rowptr, const int* col, long N, long M, int L, const long* offs, long R,
                             int* ring, int* len, void* stream) {
    if (N < 0 || N >= GR_MAXN || M < 0 || R < 0) AMX_BADARG(1);
    if (L < 3 || L > RG_LMAX) AMX_BADARG(2);
    if (N == 0 || R == 0) return 0;
    if (!rowptr || !offs || !ring || !len || (M > 0 && !col)) AMX_BADARG(3);
    return ring_common(rowptr, col, N, M, L, 1, offs, R, nullptr, ring, len, stream);
}
