// cluster.hip — density clustering (DBSCAN) of atom tables, on the device.
//
// Replaces sklearn.cluster.DBSCAN behind the reference's cluster_coord (atomai/utils/coords.py:304-347) and the per-frame
// loop of ensemble_locate (atomai/predictors/epredictor.py:297-330).  All frames form one flat table with segment offsets
// (the layout of amx_knn) and go through in one pass:
//   cl_grid_kernel    one workgroup per segment: bounding box, cell edge h, grid dimensions.
//   cl_key_kernel     one thread per row: its segment (binary search of the offsets) and its cell key.  The caller sorts
//                     the rows by key (a stable device sort) and derives the first sorted position of every cell.
//   cl_core_kernel    one thread per sorted row streams the rows of the 3 x 3 surrounding cells — the three cells of
//                     one grid row are one contiguous range of the sorted table — and counts its neighbours.
//   cl_hook_kernel / cl_jump_kernel   connected components of the core-core graph: hooking of the larger root under
//                     the smaller one with an integer atomic minimum, then pointer jumping to the root.
//   cl_label_kernel   scikit-learn's numbering, border rows, noise.
//   cl_stats_kernel   count, mean and population variance per cluster, two passes, one thread per cluster.
// Everything is fp64 and small integers; the search is bound by the latency of the cell lookups, not by arithmetic.
//
// Neighbour test.  dx*dx + dy*dy <= eps2 with eps2 = eps*eps formed once by the caller, every operation rounded on its
// own (the library is built with -ffp-contract=off): the quantity scikit-learn's KD-tree compares, so points at exactly
// eps agree.
//
// Cell edge.  Row i of a segment lies in cell cx = floor(fl(fl(x - xmin) / h)), clamped to [0, nx).  Two neighbours must
// never lie two cells apart.  Let u = 2^-53.  A pair that passes the test has |dx| <= eps (1 + 4u): fl(dx*dx) <= fl(eps2)
// bounds dx^2 by eps^2 (1 + u)^2 / (1 - u), and fl(dx) is within u of dx.  For a = x1 - xmin <= b = x2 - xmin the computed
// quotients are A = a (1 + t1) / h and B = b (1 + t2) / h with |t| <= 2u + u^2 (one subtraction, one division), and the
// cells are two apart only if B - A > 1.  But
//     B - A <= (b - a) / h + (|t1| a + |t2| b) / h <= eps (1 + 4u) / h + 4.1 u (b / h),
// and b / h < nx + 1 <= 2^31 because a segment has fewer than 2^31 rows and at most n + 1 cells along an axis (below).
// So 4.1 u (b / h) < 2^-19.9, and with h >= heps = eps (1 + 2^-16):
//     B - A < (1 + 2^-51) (1 - 2^-16 + 2^-32) + 2^-19.9 < 1.
// With h == eps the first term alone can reach 1 and the rounding of the quotients can push two points at distance eps
// across two cell borders.  The clamp to [0, nx) only moves cells closer together.
//
// Cell count.  h >= max(W / n, H / n, sqrt(W H / n)) for a W x H box of n rows gives W/h <= n, H/h <= n and
// (W/h)(H/h) <= n, so nx ny = (floor(W/h) + 1)(floor(H/h) + 1) <= 3 n + 1: the grid is sized by the number of rows, never
// by extent / eps.  The caller reserves 3 n + 1 cells per segment without a read-back; a grid that would not fit (which
// the bound excludes) degrades to a single cell, which is slower and still correct.
//
// Determinism.  No floating-point atomics.  The hooking round reads a snapshot of the parents (pin) and applies
// atomicMin to a copy (pout): the result is the minimum over a fixed set of proposals, whatever the order.  Pointer
// jumping writes the root of every row, which is a function of the forest alone.  The changed flag is an atomicOr.
#include "amx_device.h"

#define CL_T 256

// cell coordinate of offset d >= 0 along an axis with n cells of edge h; NaN and negative quotients land in cell 0
static __device__ __forceinline__ long cl_cell(double d, double h, long n) {
    const double t = d / h;
    return t >= 1.0 ? (t < (double)n ? (long)t : n - 1) : 0;
}

__global__ __launch_bounds__(CL_T) void cl_grid_kernel(const double* __restrict__ pts, long N, const long* __restrict__ seg,
                                                       const long* __restrict__ cbase, double heps,
                                                       double* __restrict__ grid, long* __restrict__ gdim) {
    __shared__ double s_m[4][CL_T];
    const int tid = threadIdx.x;
    const long s = blockIdx.x;
    long lo = seg[s], hi = seg[s + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > N ? N : hi;
    double xlo = INFINITY, ylo = INFINITY, xhi = -INFINITY, yhi = -INFINITY;
    for (long i = lo + tid; i < hi; i += CL_T) {          // (a NaN is never selected)
        const double x = pts[2 * i], y = pts[2 * i + 1];
        xlo = x < xlo ? x : xlo;
        xhi = x > xhi ? x : xhi;
        ylo = y < ylo ? y : ylo;
        yhi = y > yhi ? y : yhi;
    }
    s_m[0][tid] = xlo; s_m[1][tid] = ylo; s_m[2][tid] = -xhi; s_m[3][tid] = -yhi;     // four minima
    __syncthreads();
    for (int w = CL_T / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            #pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double a = s_m[c][tid], b = s_m[c][tid + w];
                s_m[c][tid] = b < a ? b : a;
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    xlo = s_m[0][0]; ylo = s_m[1][0]; xhi = -s_m[2][0]; yhi = -s_m[3][0];
    const long n = hi - lo, cap = cbase[s + 1] - cbase[s];
    double h = heps;
    long nx = 1, ny = 1;
    if (n > 0 && xlo <= xhi && ylo <= yhi) {
        const double W = xhi - xlo, H = yhi - ylo, dn = (double)n;
        const double h1 = W / dn, h2 = H / dn, h3 = sqrt(W / dn) * sqrt(H);
        h = h1 > h ? h1 : h;
        h = h2 > h ? h2 : h;
        h = h3 > h ? h3 : h;
        const double a = floor(W / h), b = floor(H / h);
        if (a >= 0.0 && a <= dn && b >= 0.0 && b <= dn) {   // (false for NaN / inf: one cell)
            nx = (long)a + 1;
            ny = (long)b + 1;
        }
        if (nx * ny > cap) nx = ny = 1;                    // (nx, ny <= 2^31: the product cannot overflow)
    } else {
        xlo = ylo = 0.0;
    }
    grid[3 * s] = xlo; grid[3 * s + 1] = ylo; grid[3 * s + 2] = h;
    gdim[2 * s] = nx; gdim[2 * s + 1] = ny;
}

__global__ __launch_bounds__(CL_T) void cl_key_kernel(const double* __restrict__ pts, long N, const long* __restrict__ seg,
                                                      int S, const long* __restrict__ cbase,
                                                      const double* __restrict__ grid, const long* __restrict__ gdim,
                                                      long* __restrict__ key, int* __restrict__ sid) {
    const long i = (long)blockIdx.x * CL_T + threadIdx.x;
    if (i >= N) return;
    int lo = 0, hi = S;                                    // first segment with seg[s + 1] > i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid + 1] <= i) lo = mid + 1; else hi = mid;
    }
    if (lo >= S || seg[lo] > i) {                          // offsets that do not cover row i
        key[i] = cbase[S];
        sid[i] = -1;
        return;
    }
    const long nx = gdim[2 * lo], ny = gdim[2 * lo + 1];
    const double h = grid[3 * lo + 2];
    const long cx = cl_cell(pts[2 * i] - grid[3 * lo], h, nx), cy = cl_cell(pts[2 * i + 1] - grid[3 * lo + 1], h, ny);
    key[i] = cbase[lo] + cy * nx + cx;
    sid[i] = lo;
}

// The grid of sorted row p: false if the row belongs to no segment or its tables are inconsistent (nothing is read
// outside cstart [C + 1] then).
struct ClCell {
    long base, nx, ny, cx, cy;
};
static __device__ __forceinline__ bool cl_locate(long p, const int* __restrict__ ssid, const long* __restrict__ skey, int S,
                                                 const long* __restrict__ cbase, const long* __restrict__ gdim, long C,
                                                 ClCell& g) {
    const int s = ssid[p];
    if (s < 0 || s >= S) return false;
    g.base = cbase[s];
    g.nx = gdim[2 * s];
    g.ny = gdim[2 * s + 1];
    if (g.nx < 1 || g.ny < 1 || g.nx > 2147483647L || g.ny > 2147483647L) return false;
    const long cell = skey[p] - g.base;
    if (g.base < 0 || g.base + g.nx * g.ny > C || cell < 0 || cell >= g.nx * g.ny) return false;
    g.cy = cell / g.nx;
    g.cx = cell - g.cy * g.nx;
    return true;
}

// f(q) for every sorted row q of the 3 x 3 cells around g with dx*dx + dy*dy <= eps2 (row p itself included)
template <class F>
static __device__ __forceinline__ void cl_visit(const double* __restrict__ spts, long N, const long* __restrict__ cstart,
                                                const ClCell& g, double x, double y, double eps2, F&& f) {
    const long x0 = g.cx > 0 ? g.cx - 1 : 0, x1 = g.cx + 1 < g.nx ? g.cx + 1 : g.nx - 1;
    const long y0 = g.cy > 0 ? g.cy - 1 : 0, y1 = g.cy + 1 < g.ny ? g.cy + 1 : g.ny - 1;
    for (long yy = y0; yy <= y1; ++yy) {
        long b = cstart[g.base + yy * g.nx + x0], e = cstart[g.base + yy * g.nx + x1 + 1];
        b = b < 0 ? 0 : b;
        e = e > N ? N : e;
        for (long q = b; q < e; ++q) {
            const double dx = spts[2 * q] - x, dy = spts[2 * q + 1] - y;
            if (dx * dx + dy * dy <= eps2) f(q);
        }
    }
}

__global__ __launch_bounds__(CL_T) void cl_core_kernel(const double* __restrict__ spts, long N, const int* __restrict__ ssid,
                                                       const long* __restrict__ skey, int S, const long* __restrict__ cbase,
                                                       const long* __restrict__ gdim, const long* __restrict__ cstart, long C,
                                                       double eps2, long min_samples, int* __restrict__ core) {
    const long p = (long)blockIdx.x * CL_T + threadIdx.x;
    if (p >= N) return;
    ClCell g;
    long n = 0;
    if (cl_locate(p, ssid, skey, S, cbase, gdim, C, g))
        cl_visit(spts, N, cstart, g, spts[2 * p], spts[2 * p + 1], eps2, [&](long) { ++n; });
    core[p] = n >= min_samples ? 1 : 0;
}

__global__ __launch_bounds__(CL_T) void cl_hook_kernel(const double* __restrict__ spts, long N, const int* __restrict__ ssid,
                                                       const long* __restrict__ skey, int S, const long* __restrict__ cbase,
                                                       const long* __restrict__ gdim, const long* __restrict__ cstart, long C,
                                                       double eps2, const int* __restrict__ core,
                                                       const long* __restrict__ orig, const int* __restrict__ pin,
                                                       int* pout, int* changed) {
    const long p = (long)blockIdx.x * CL_T + threadIdx.x;
    if (p >= N || !core[p]) return;
    ClCell g;
    if (!cl_locate(p, ssid, skey, S, cbase, gdim, C, g)) return;
    const long i = orig[p];
    if (i < 0 || i >= N) return;
    const int ri = pin[i];
    bool any = false;
    cl_visit(spts, N, cstart, g, spts[2 * p], spts[2 * p + 1], eps2, [&](long q) {
        if (!core[q]) return;
        const long j = orig[q];
        if (j < 0 || j >= N) return;
        const int rj = pin[j];
        // the edge is seen from both ends: the end with the larger root hooks that root under the smaller one
        if (rj < ri && rj >= 0 && ri < N) {
            atomicMin(&pout[ri], rj);
            any = true;
        }
    });
    if (any) atomicOr(changed, 1);
}

// pb is a forest with pb[i] <= i.  Concurrent writers only replace a parent by an ancestor, so every chain still ends
// at the same root; the bound on the walk guards against a table that is no forest.
__global__ __launch_bounds__(CL_T) void cl_jump_kernel(int* pa, int* pb, long N) {
    const long i = (long)blockIdx.x * CL_T + threadIdx.x;
    if (i >= N) return;
    int r = pb[i];
    for (long step = 0; step < N; ++step) {
        if (r < 0 || r >= N) { r = (int)i; break; }
        const int up = pb[r];
        if (up == r) break;
        r = up;
    }
    pa[i] = r;
    pb[i] = r;
}

__global__ __launch_bounds__(CL_T) void cl_label_kernel(const double* __restrict__ spts, long N, const int* __restrict__ ssid,
                                                        const long* __restrict__ skey, const long* __restrict__ seg, int S,
                                                        const long* __restrict__ cbase, const long* __restrict__ gdim,
                                                        const long* __restrict__ cstart, long C, double eps2,
                                                        const int* __restrict__ core, const long* __restrict__ orig,
                                                        const int* __restrict__ parent, const long* __restrict__ rank,
                                                        long* __restrict__ label) {
    const long p = (long)blockIdx.x * CL_T + threadIdx.x;
    if (p >= N) return;
    const long i = orig[p];
    if (i < 0 || i >= N) return;
    ClCell g;
    long root = -1;
    if (cl_locate(p, ssid, skey, S, cbase, gdim, C, g)) {
        if (core[p]) {
            root = parent[i];
        } else {                                            // border row: the smallest root among its core neighbours,
            cl_visit(spts, N, cstart, g, spts[2 * p], spts[2 * p + 1], eps2, [&](long q) {   // = their smallest label
                if (!core[q]) return;
                const long j = orig[q];
                if (j < 0 || j >= N) return;
                const long r = parent[j];
                if (root < 0 || r < root) root = r;
            });
        }
    }
    long first = root >= 0 ? seg[ssid[p]] : 0;
    first = first < 0 ? 0 : (first > N ? N : first);
    label[i] = (root >= 0 && root < N) ? rank[root] - rank[first] : -1;
}

__global__ __launch_bounds__(CL_T) void cl_stats_kernel(const double* __restrict__ pts, long N, const long* __restrict__ members,
                                                        long M, const long* __restrict__ moff, long K,
                                                        long* __restrict__ count, double* __restrict__ mean,
                                                        double* __restrict__ var) {
    const long k = (long)blockIdx.x * CL_T + threadIdx.x;
    if (k >= K) return;
    long b = moff[k], e = moff[k + 1];
    b = b < 0 ? 0 : b;
    e = e > M ? M : e;
    long m = 0;
    double sx = 0.0, sy = 0.0;
    for (long t = b; t < e; ++t) {
        const long i = members[t];
        if (i < 0 || i >= N) continue;
        sx += pts[2 * i];
        sy += pts[2 * i + 1];
        ++m;
    }
    const double mx = sx / (double)m, my = sy / (double)m;    // (0 / 0 = NaN for an empty cluster)
    double vx = 0.0, vy = 0.0;
    for (long t = b; t < e; ++t) {
        const long i = members[t];
        if (i < 0 || i >= N) continue;
        const double dx = pts[2 * i] - mx, dy = pts[2 * i + 1] - my;
        vx += dx * dx;
        vy += dy * dy;
    }
    count[k] = m;
    mean[2 * k] = mx; mean[2 * k + 1] = my;
    var[2 * k] = vx / (double)m; var[2 * k + 1] = vy / (double)m;
}

// ---------------------------------------------------------------------------------------------- C ABI
#define CL_MAXN 2147483647L
static inline dim3 cl_blocks(long n) { return dim3((unsigned)((n + CL_T - 1) / CL_T)); }

extern "C" int amx_cluster_grid(const double* pts, long N, const long* seg, int S, const long* cbase, double heps,
                                double* grid, long* gdim, void* stream) {
    if (N < 0 || N >= CL_MAXN || S < 0) AMX_BADARG(1);
    if (!(heps > 0.0) || !(heps < INFINITY)) AMX_BADARG(2);
    if (S == 0) return 0;
    if (!seg || !cbase || !grid || !gdim || (N > 0 && !pts)) AMX_BADARG(3);
    AMX_LAUNCH(cl_grid_kernel, dim3((unsigned)S), dim3(CL_T), 0, (hipStream_t)stream, pts, N, seg, cbase, heps, grid, gdim);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_cluster_keys(const double* pts, long N, const long* seg, int S, const long* cbase, const double* grid,
                                const long* gdim, long* key, int* sid, void* stream) {
    if (N < 0 || N >= CL_MAXN || S < 0) AMX_BADARG(1);
    if (N == 0) return 0;
    if (!pts || !seg || !cbase || !grid || !gdim || !key || !sid) AMX_BADARG(2);
    AMX_LAUNCH(cl_key_kernel, cl_blocks(N), dim3(CL_T), 0, (hipStream_t)stream, pts, N, seg, S, cbase, grid, gdim, key, sid);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_cluster_core(const double* spts, long N, const int* ssid, const long* skey, int S, const long* cbase,
                                const long* gdim, const long* cstart, long C, double eps2, long min_samples, int* core,
                                void* stream) {
    if (N < 0 || N >= CL_MAXN || S < 0 || C < 0) AMX_BADARG(1);
    if (min_samples < 1 || !(eps2 >= 0.0)) AMX_BADARG(2);
    if (N == 0) return 0;
    if (!spts || !ssid || !skey || !cbase || !gdim || !cstart || !core) AMX_BADARG(3);
    AMX_LAUNCH(cl_core_kernel, cl_blocks(N), dim3(CL_T), 0, (hipStream_t)stream, spts, N, ssid, skey, S, cbase, gdim, cstart,
               C, eps2, min_samples, core);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_cluster_hook(const double* spts, long N, const int* ssid, const long* skey, int S, const long* cbase,
                                const long* gdim, const long* cstart, long C, double eps2, const int* core, const long* orig,
                                const int* pin, int* pout, int* changed, void* stream) {
    if (N < 0 || N >= CL_MAXN || S < 0 || C < 0) AMX_BADARG(1);
    if (!(eps2 >= 0.0)) AMX_BADARG(2);
    if (N == 0) return 0;
    if (!spts || !ssid || !skey || !cbase || !gdim || !cstart || !core || !orig || !pin || !pout || !changed) AMX_BADARG(3);
    if (pin == pout) AMX_BADARG(4);
    AMX_LAUNCH(cl_hook_kernel, cl_blocks(N), dim3(CL_T), 0, (hipStream_t)stream, spts, N, ssid, skey, S, cbase, gdim, cstart,
               C, eps2, core, orig, pin, pout, changed);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_cluster_jump(int* pa, int* pb, long N, void* stream) {
    if (N < 0 || N >= CL_MAXN) AMX_BADARG(1);
    if (N == 0) return 0;
    if (!pa || !pb) AMX_BADARG(2);
    AMX_LAUNCH(cl_jump_kernel, cl_blocks(N), dim3(CL_T), 0, (hipStream_t)stream, pa, pb, N);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_cluster_label(const double* spts, long N, const int* ssid, const long* skey, const long* seg, int S,
                                 const long* cbase, const long* gdim, const long* cstart, long C, double eps2,
                                 const int* core, const long* orig, const int* parent, const long* rank, long* label,
                                 void* stream) {
    if (N < 0 || N >= CL_MAXN || S < 0 || C < 0) AMX_BADARG(1);
    if (!(eps2 >= 0.0)) AMX_BADARG(2);
    if (N == 0) return 0;
    if (!spts || !ssid || !skey || !seg || !cbase || !gdim || !cstart || !core || !orig || !parent || !rank || !label)
        AMX_BADARG(3);
    AMX_LAUNCH(cl_label_kernel, cl_blocks(N), dim3(CL_T), 0, (hipStream_t)stream, spts, N, ssid, skey, seg, S, cbase, gdim,
               cstart, C, eps2, core, orig, parent, rank, label);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_cluster_stats(const double* pts, long N, const long* members, long M, const long* moff, long K,
                                 long* count, double* mean, double* var, void* stream) {
    if (N < 0 || N >= CL_MAXN || M < 0 || K < 0 || K >= CL_MAXN * CL_T) AMX_BADARG(1);
    if (K == 0) return 0;
    if (!moff || !count || !mean || !var || (M > 0 && (!pts || !members))) AMX_BADARG(2);
    AMX_LAUNCH(cl_stats_kernel, cl_blocks(K), dim3(CL_T), 0, (hipStream_t)stream, pts, N, members, M, moff, K, count, mean,
               var);
    AMX_CHECK_LAUNCH();
    return 0;
}
