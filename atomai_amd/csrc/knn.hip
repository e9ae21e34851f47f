// knn.hip — nearest-neighbour analysis of atom tables, on the device.
//
// Replaces the scipy.spatial.cKDTree queries behind the reference's get_nn_distances, compare_coordinates and
// find_coord_clusters (atomai/utils/coords.py:86-149, 266-301, 350-400) and the per-atom Python loop of get_intensities_
// (coords.py:234-252):
//   knn_kernel<KC, DIM>   segmented k nearest neighbours, brute force.  One workgroup = one tile of KNN_T queries of ONE
//                         segment, one query per thread; the grid runs over a (segment, first query) tile table, so a
//                         single large frame fills the device as well as many small ones.  The segment's reference
//                         points pass through LDS in tiles of KNN_T (as nn2_kernel of refine.hip does); every thread
//                         keeps its KC best candidates sorted in registers (fully unrolled insertion: static indices
//                         only, no scratch).  KC in {4, 8, 16, 32} is the smallest ceiling that holds k.
//   radius_kernel         one set: per query the number of points with d < rmax, or (second pass, after an exclusive
//                         prefix sum of the counts) their rows and distances in row order.
//   window_mean_kernel    fp64 mean of the fp32 frame over the reference's r x r window around the rounded atom.
// Everything is fp64, there are no atomics and every output element has exactly one writer: two runs give the same bits.
//
// Ordering.  Candidates are ranked by the fp64 SUM OF SQUARES q = dx*dx + dy*dy (+ dz*dz), added in that order; among equal
// q the smaller row wins (the insertion compares (q, row) pairs, so the order in which the tiles are visited does not
// matter).  The distance written is sqrt(q).  A candidate counts only if sqrt(q) < bound, strictly (cKDTree's
// distance_upper_bound); q < bound2 with bound2 slightly above bound^2 is a cheap superset test in front of the sqrt.
#include "amx_device.h"

#define KNN_T 256
#define KNN_KMAX 32
#define KNN_U 4                        // candidates per trip of the inner loop

// (q, j) sorts in front of the entry (d, id): smaller sum of squares, equal sums by the smaller row.  An empty slot is
// (+inf, -1) and every candidate has a finite q.
static __device__ __forceinline__ bool knn_before(double q, int j, double d, int id) {
    return q < d || (q == d && j < id);
}

template <int KC>
static __device__ __forceinline__ void knn_insert(double (&d)[KC], int (&id)[KC], double q, int j) {
    #pragma unroll
    for (int s = KC - 1; s >= 1; --s) {                 // downwards: entry s - 1 is still the old one when slot s is written
        const bool up = knn_before(q, j, d[s - 1], id[s - 1]), here = knn_before(q, j, d[s], id[s]);
        d[s] = up ? d[s - 1] : (here ? q : d[s]);
        id[s] = up ? id[s - 1] : (here ? j : id[s]);
    }
    if (knn_before(q, j, d[0], id[0])) { d[0] = q; id[0] = j; }
}

template <int KC>
static __device__ __forceinline__ void knn_consider(double (&d)[KC], int (&id)[KC], double q, int j, double bound,
                                                    double bound2) {
    if (q <= d[KC - 1] && q < bound2) {                 // (<=: an equal sum with a smaller row still moves in)
        if (sqrt(q) < bound) knn_insert<KC>(d, id, q, j);
    }
}

template <int DIM>
static __device__ __forceinline__ double knn_q(const double (&s_p)[DIM][KNN_T], int kk, const double (&x)[DIM]) {
    double q = 0.0;
    #pragma unroll
    for (int c = 0; c < DIM; ++c) {
        const double t = s_p[c][kk] - x[c];
        q += t * t;
    }
    return q;
}

template <int KC, int DIM>
__global__ __launch_bounds__(KNN_T) void knn_kernel(const double* __restrict__ pts, long P, const double* __restrict__ qry,
                                                    long Q, const long* __restrict__ pseg, const long* __restrict__ qseg,
                                                    int S, const long* __restrict__ tiles, int k, double bound,
                                                    double bound2, double* __restrict__ dist, long* __restrict__ idx) {
    __shared__ double s_p[DIM][KNN_T];
    const int tid = threadIdx.x;
    const long seg = tiles[2 * (long)blockIdx.x], q0 = tiles[2 * (long)blockIdx.x + 1];
    if (seg < 0 || seg >= S) return;                    // (block-uniform: a malformed table reads and writes nothing)
    long plo = pseg[seg], phi = pseg[seg + 1], qlo = qseg[seg], qhi = qseg[seg + 1];
    plo = plo < 0 ? 0 : plo;
    phi = phi > P ? P : phi;
    qlo = qlo < 0 ? 0 : qlo;
    qhi = qhi > Q ? Q : qhi;
    if (q0 < qlo || q0 >= qhi || phi - plo > 2147483647L - KNN_T) return;
    const long i = q0 + tid;
    const bool live = i < qhi;
    double x[DIM];
    #pragma unroll
    for (int c = 0; c < DIM; ++c) x[c] = live ? qry[i * DIM + c] : 0.0;
    double d[KC];
    int id[KC];
    #pragma unroll
    for (int s = 0; s < KC; ++s) { d[s] = INFINITY; id[s] = -1; }
    // Tile order: start at the tile that lies as far into the points as this workgroup's queries lie into theirs, then
    // alternate outwards.  Atom tables come in raster order, so for self queries (and for two tables of the same scene)
    // the true neighbours are met in the first few tiles and the k-th best distance, which gates the insertion, is
    // tight from then on; scanning from the start it shrinks row by row and some lane of the wave inserts at almost
    // every candidate.  The result does not depend on the order: (sum of squares, row) is a total order.
    const long nt = phi > plo ? (phi - plo + KNN_T - 1) / KNN_T : 0, nq = qhi - qlo;
    const long mid = q0 - qlo + KNN_T / 2 < nq ? q0 - qlo + KNN_T / 2 : nq - 1;
    long t_up = mid * nt / nq, t_dn = t_up - 1;          // 0 <= t_up < nt (mid < nq); both factors are below 2^31
    for (long step = 0; step < nt; ++step) {            // (block-uniform bounds: every thread reaches the barriers)
        const bool take_up = t_up < nt && (t_dn < 0 || (step & 1) == 0);
        const long tile = plo + KNN_T * (take_up ? t_up++ : t_dn--);
        const long j = tile + tid;
        __syncthreads();
        #pragma unroll
        for (int c = 0; c < DIM; ++c) s_p[c][tid] = j < phi ? pts[j * DIM + c] : 0.0;
        __syncthreads();
        const int m = (int)(phi - tile < KNN_T ? phi - tile : KNN_T), base = (int)(tile - plo);
        if (live) {
            int kk = 0;
            for (; kk + KNN_U <= m; kk += KNN_U) {       // KNN_U independent candidates per trip: their LDS reads and
                double q[KNN_U];                         // fp64 chains overlap, and one test skips all of them
                #pragma unroll
                for (int u = 0; u < KNN_U; ++u) q[u] = knn_q<DIM>(s_p, kk + u, x);
                double qmin = q[0];
                #pragma unroll
                for (int u = 1; u < KNN_U; ++u) qmin = q[u] < qmin ? q[u] : qmin;
                if (qmin <= d[KC - 1] && qmin < bound2) {
                    #pragma unroll
                    for (int u = 0; u < KNN_U; ++u) knn_consider<KC>(d, id, q[u], base + kk + u, bound, bound2);
                }
            }
            for (; kk < m; ++kk) knn_consider<KC>(d, id, knn_q<DIM>(s_p, kk, x), base + kk, bound, bound2);
        }
    }
    if (live) {
        #pragma unroll
        for (int s = 0; s < KC; ++s) {
            if (s < k) {
                dist[i * k + s] = sqrt(d[s]);           // sqrt(+inf) = +inf: an empty slot
                idx[i * k + s] = id[s] < 0 ? -1L : plo + id[s];
            }
        }
    }
}

// emit == 0: count[i] = number of points with sqrt(q) < rmax.  emit != 0: their rows, distances and the query's own row
// go to [offs[i], offs[i] + count) of idx / dist / qid, in row order; nothing is written at or beyond M.
__global__ __launch_bounds__(KNN_T) void radius_kernel(const double* __restrict__ pts, long P, const double* __restrict__ qry,
                                                       long Q, int dim, double rmax, double rmax2, int emit,
                                                       const long* __restrict__ offs, long M, long* __restrict__ count,
                                                       long* __restrict__ qid, long* __restrict__ idx,
                                                       double* __restrict__ dist) {
    __shared__ double s_p[3][KNN_T];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * KNN_T + tid;
    const bool live = i < Q;
    double x[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < dim; ++c) x[c] = live ? qry[i * dim + c] : 0.0;
    long n = 0;
    const long o = (emit && live) ? offs[i] : 0;
    for (long tile = 0; tile < P; tile += KNN_T) {
        const long j = tile + tid;
        __syncthreads();
        for (int c = 0; c < 3; ++c) s_p[c][tid] = (c < dim && j < P) ? pts[j * dim + c] : 0.0;
        __syncthreads();
        const int m = (int)(P - tile < KNN_T ? P - tile : KNN_T);
        if (live) {
            for (int kk = 0; kk < m; ++kk) {
                const double tx = s_p[0][kk] - x[0], ty = s_p[1][kk] - x[1], tz = s_p[2][kk] - x[2];
                double q = tx * tx + ty * ty;
                if (dim == 3) q += tz * tz;
                if (q < rmax2) {
                    const double r = sqrt(q);
                    if (r < rmax) {
                        if (emit && o >= 0 && o + n < M) {
                            qid[o + n] = i;
                            idx[o + n] = tile + kk;
                            dist[o + n] = r;
                        }
                        ++n;
                    }
                }
            }
        }
    }
    if (live && !emit) count[i] = n;
}

__global__ __launch_bounds__(KNN_T) void window_mean_kernel(const float* __restrict__ frames, int B, int H, int W,
                                                            const double* __restrict__ coords, const int* __restrict__ meta,
                                                            long n, int r, double* __restrict__ out) {
    const long i = (long)blockIdx.x * KNN_T + threadIdx.x;
    if (i >= n) return;
    const double row = coords[2 * i], col = coords[2 * i + 1];
    const int fr = meta[2 * i];
    double v = NAN;
    if (fabs(row) < 1e9 && fabs(col) < 1e9 && fr >= 0 && fr < B) {         // (the comparisons are false for NaN)
        const long cx = (long)rint(row), cy = (long)rint(col);           // round half to even, as np.around
        const long h = r / 2, r0 = cx - h, c0 = cy - h;
        long r1 = cx + h + (r & 1), c1 = cy + h + (r & 1);
        r1 = r1 > H ? H : r1;
        c1 = c1 > W ? W : c1;
        if (r0 >= 0 && c0 >= 0 && r1 > r0 && c1 > c0) {                   // a negative start is an empty slice: NaN
            const float* f = frames + (long)fr * H * W;
            double s = 0.0;
            for (long a = r0; a < r1; ++a)
                for (long b = c0; b < c1; ++b) s += (double)f[a * W + b];
            v = s / (double)((r1 - r0) * (c1 - c0));
        }
    }
    out[i] = v;
}

// ---------------------------------------------------------------------------------------------- C ABI
// Superset threshold for "sqrt(q) < b": a little above b^2, never zero for a positive b whose square underflows.
static double knn_bound2(double b) {
    if (!(b > 0.0)) return 0.0;
    const double b2 = b * b * (1.0 + 8.0 * 2.220446049250313e-16);
    return b2 >= 1e-290 ? b2 : 1e-290;
}

template <int DIM>
static int knn_launch(const double* pts, long P, const double* qry, long Q, const long* pseg, const long* qseg, int S,
                      const long* tiles, long T, int k, double bound, double* dist, long* idx, hipStream_t st) {
    const dim3 grid((unsigned)T), block(KNN_T);
    const double b2 = knn_bound2(bound);
    if (k <= 4)
        AMX_LAUNCH((knn_kernel<4, DIM>), grid, block, 0, st, pts, P, qry, Q, pseg, qseg, S, tiles, k, bound, b2, dist, idx);
    else if (k <= 8)
        AMX_LAUNCH((knn_kernel<8, DIM>), grid, block, 0, st, pts, P, qry, Q, pseg, qseg, S, tiles, k, bound, b2, dist, idx);
    else if (k <= 16)
        AMX_LAUNCH((knn_kernel<16, DIM>), grid, block, 0, st, pts, P, qry, Q, pseg, qseg, S, tiles, k, bound, b2, dist, idx);
    else
        AMX_LAUNCH((knn_kernel<32, DIM>), grid, block, 0, st, pts, P, qry, Q, pseg, qseg, S, tiles, k, bound, b2, dist, idx);
    return 0;
}

extern "C" int amx_knn(const double* pts, long P, const double* qry, long Q, int dim, const long* pseg, const long* qseg,
                       int S, const long* tiles, long T, int k, double bound, double* dist, long* idx, void* stream) {
    if (dim != 2 && dim != 3) AMX_BADARG(1);
    if (k < 1 || k > KNN_KMAX) AMX_BADARG(2);
    if (P < 0 || Q < 0 || S < 0 || T < 0 || P >= 2147483647L || Q >= 2147483647L || T >= 2147483647L) AMX_BADARG(3);
    if (Q == 0 || S == 0 || T == 0) return 0;
    if (!qry || !pseg || !qseg || !tiles || !dist || !idx || (P > 0 && !pts)) AMX_BADARG(4);
    if (dim == 2) knn_launch<2>(pts, P, qry, Q, pseg, qseg, S, tiles, T, k, bound, dist, idx, (hipStream_t)stream);
    else knn_launch<3>(pts, P, qry, Q, pseg, qseg, S, tiles, T, k, bound, dist, idx, (hipStream_t)stream);
    AMX_CHECK_LAUNCH();
    return 0;
}

static int radius_common(const double* pts, long P, const double* qry, long Q, int dim, double rmax, int emit,
                         const long* offs, long M, long* count, long* qid, long* idx, double* dist, void* stream) {
    const long blocks = (Q + KNN_T - 1) / KNN_T;
    AMX_LAUNCH(radius_kernel, dim3((unsigned)blocks), dim3(KNN_T), 0, (hipStream_t)stream, pts, P, qry, Q, dim, rmax,
               knn_bound2(rmax), emit, offs, M, count, qid, idx, dist);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_radius_count(const double* pts, long P, const double* qry, long Q, int dim, double rmax, long* count,
                                void* stream) {
    if (dim != 2 && dim != 3) AMX_BADARG(1);
    if (P < 0 || Q < 0 || Q >= 2147483647L * KNN_T) AMX_BADARG(2);
    if (Q == 0) return 0;
    if (!qry || !count || (P > 0 && !pts)) AMX_BADARG(3);
    return radius_common(pts, P, qry, Q, dim, rmax, 0, nullptr, 0, count, nullptr, nullptr, nullptr, stream);
}

extern "C" int amx_radius_emit(const double* pts, long P, const double* qry, long Q, int dim, double rmax, const long* offs,
                               long M, long* qid, long* idx, double* dist, void* stream) {
    if (dim != 2 && dim != 3) AMX_BADARG(1);
    if (P < 0 || Q < 0 || M < 0 || Q >= 2147483647L * KNN_T) AMX_BADARG(2);
    if (Q == 0 || M == 0) return 0;
    if (!qry || !offs || !qid || !idx || !dist || (P > 0 && !pts)) AMX_BADARG(3);
    return radius_common(pts, P, qry, Q, dim, rmax, 1, offs, M, nullptr, qid, idx, dist, stream);
}

extern "C" int amx_window_mean(const float* frames, int B, int H, int W, const double* coords, const int* meta, long n,
                               int r, double* out, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || n < 0) AMX_BADARG(1);
    if (r < 1 || r > 1024) AMX_BADARG(2);
    if (n == 0) return 0;
    if (!frames || !coords || !meta || !out) AMX_BADARG(3);
    const long blocks = (n + KNN_T - 1) / KNN_T;
    if (blocks >= 2147483647L) AMX_BADARG(4);
    AMX_LAUNCH(window_mean_kernel, dim3((unsigned)blocks), dim3(KNN_T), 0, (hipStream_t)stream, frames, B, H, W, coords, meta,
               n, r, out);
    AMX_CHECK_LAUNCH();
    return 0;
}
