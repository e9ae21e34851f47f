// intensity.hip — one-dimensional clustering of atom intensities, on the device.
//
// Replaces sklearn.cluster.estimate_bandwidth, MeanShift(bin_seeding=True) and KMeans behind the reference's
// update_classes (atomai/stat/multivar.py:816-916) for a single column of values.  In one dimension the neighbours of a
// value in the SORTED column are a contiguous range, so every neighbour query is a binary search and every cluster sum
// is a range sum:
//   in_gap_kernel        one thread per row: distance to its K-th nearest value (itself at distance 0), and the sum of
//                        the workgroup's rows;  in_mean_kernel adds those partials and divides by n.
//   in_meanshift_kernel  one workgroup per seed, all iterations of _mean_shift_single_seed inside the launch.
//   in_lloyd_kernel      one workgroup, the whole Lloyd fit of at most 32 centres inside the launch.
//   in_assign_kernel     one thread per row of the UNSORTED column: index of the nearest centre, the first on ties.
// Everything is fp64; the kernels are bound by the latency of the searches and the barriers, not by arithmetic.
//
// Determinism.  No floating-point atomics.  Every sum over rows is in_range_sum: thread t adds the rows lo + t,
// lo + t + 256, ... in that order, then the 256 partials are added by halving through LDS (in_wg_sum).  The library is
// built with -ffp-contract=off, so two runs give the same bits, and numpy can restate the order exactly.
//
// Uniform control flow.  The loops of the mean shift and of the Lloyd fit contain barriers, so every thread must leave
// them on the same iteration: the decision is computed by thread 0 and read by all from one LDS word.
#include "amx_device.h"

#define IN_T 256
#define IN_KMAX 32
#define IN_CHUNK 1024                                       // centres held in LDS at a time by in_assign_kernel

// v added over the workgroup by halving; every thread gets the sum, and s_red is free again on return
static __device__ __forceinline__ double in_wg_sum(double v, double* s_red) {
    const int tid = threadIdx.x;
    s_red[tid] = v;
    __syncthreads();
    for (int w = IN_T / 2; w >= 1; w >>= 1) {
        if (tid < w) s_red[tid] = s_red[tid] + s_red[tid + w];
        __syncthreads();
    }
    const double r = s_red[0];
    __syncthreads();
    return r;
}

// sum of xs[lo, hi) (lo, hi uniform over the workgroup)
static __device__ __forceinline__ double in_range_sum(const double* __restrict__ xs, long lo, long hi, double* s_red) {
    double a = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += IN_T) a += xs[i];
    return in_wg_sum(a, s_red);
}

// The K nearest values of xs[i] are a window [l, l + K - 1] that contains i, l in [max(0, i - K + 1), min(i, n - K)]
// (not empty for 1 <= K <= n).  xs[i] - xs[l] falls with l and xs[l + K - 1] - xs[i] rises: with p the first l where
// the second is at least the first, the minimum of their maximum is the second term at p or the first at p - 1.
__global__ __launch_bounds__(IN_T) void in_gap_kernel(const double* __restrict__ xs, long n, long K,
                                                      double* __restrict__ gap, double* __restrict__ partial) {
    __shared__ double s_red[IN_T];
    const long i = (long)blockIdx.x * IN_T + threadIdx.x;
    double g = 0.0;
    if (i < n) {
        const double x = xs[i];
        const long lo = i - K + 1 > 0 ? i - K + 1 : 0, hi = i < n - K ? i : n - K;
        long a = lo, b = hi + 1;
        while (a < b) {
            const long mid = (a + b) >> 1;                  // lo <= mid <= hi, so mid + K - 1 <= n - 1
            if (xs[mid + K - 1] - x >= x - xs[mid]) b = mid; else a = mid + 1;
        }
        g = INFINITY;
        if (a <= hi) g = xs[a + K - 1] - x;
        if (a > lo) {
            const double f = x - xs[a - 1];
            g = f < g ? f : g;
        }
        gap[i] = g;
    }
    const double sum = in_wg_sum(g, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(IN_T) void in_mean_kernel(const double* __restrict__ partial, long G, long n,
                                                       double* __restrict__ mean_out) {
    __shared__ double s_red[IN_T];
    const double sum = in_range_sum(partial, 0, G, s_red);
    if (threadIdx.x == 0) *mean_out = sum / (double)n;
}

// sklearn.cluster._mean_shift._mean_shift_single_seed on a sorted column.  The members of mean m are the rows with
// fabs(x - m) <= bw.  Subtraction rounds monotonically, so "below m and outside" holds on a prefix of the column and
// "above m and outside" on a suffix: both ends come from a binary search on the membership test itself, never on
// m - bw or m + bw, whose rounding would disagree with it for rows at the edge.
__global__ __launch_bounds__(IN_T) void in_meanshift_kernel(const double* __restrict__ xs, long n,
                                                            const double* __restrict__ seeds, double bw, long max_iter,
                                                            double* __restrict__ centre, long* __restrict__ count,
                                                            long* __restrict__ iters) {
    __shared__ double s_red[IN_T];
    __shared__ double s_m;
    __shared__ long s_lo, s_hi;
    __shared__ int s_stop;
    const int tid = threadIdx.x;
    const long s = blockIdx.x;
    const double thr = 1e-3 * bw;
    double m = seeds[s];
    long it = 0, cnt = 0;
    while (true) {
        if (tid == 0) {                                     // first row that is not below the range
            long a = 0, b = n;
            while (a < b) {
                const long mid = (a + b) >> 1;
                const double x = xs[mid];
                if (x < m && fabs(x - m) > bw) a = mid + 1; else b = mid;
            }
            s_lo = a;
        }
        if (tid == AMX_WAVE) {                              // first row above the range (another wave searches it)
            long a = 0, b = n;
            while (a < b) {
                const long mid = (a + b) >> 1;
                const double x = xs[mid];
                if (x > m && fabs(x - m) > bw) b = mid; else a = mid + 1;
            }
            s_hi = a;
        }
        __syncthreads();
        const long lo = s_lo, hi = s_hi;
        cnt = hi > lo ? hi - lo : 0;
        if (cnt == 0) break;                                // (lo, hi come from LDS: the same for every thread)
        const double sum = in_range_sum(xs, lo, hi, s_red);
        if (tid == 0) {
            const double nm = sum / (double)cnt;
            s_stop = (fabs(nm - m) <= thr || it >= max_iter) ? 1 : 0;
            s_m = nm;
        }
        __syncthreads();
        m = s_m;
        const int stop = s_stop;
        __syncthreads();                                    // s_lo, s_hi, s_m, s_stop are rewritten in the next round
        if (stop) break;
        ++it;
    }
    if (tid == 0) {
        centre[s] = m;
        count[s] = cnt;
        iters[s] = it;
    }
}

// Lloyd's algorithm on a sorted column.  Centres sorted by (value, index) cut the column at their midpoints
// (a + b) * 0.5: the rows above a midpoint go to the upper centre, a row exactly on it to the lower-numbered one.  One
// round: the k ranges, their sums and counts, centre = sum / count (an EMPTY range keeps its centre; scikit-learn moves
// it to the row farthest from its centre).  Stops when no range changed since the round before, when the sum of squared
// centre shifts is <= tol, or after max_iter rounds (scikit-learn's order of those tests).
__global__ __launch_bounds__(IN_T) void in_lloyd_kernel(const double* __restrict__ xs, long n,
                                                        const double* __restrict__ cin, int k, double tol, long max_iter,
                                                        double* __restrict__ cout, long* __restrict__ n_iter) {
    __shared__ double s_red[IN_T];
    __shared__ double s_c[IN_KMAX], s_new[IN_KMAX];
    __shared__ long s_cut[IN_KMAX + 1], s_st[IN_KMAX], s_en[IN_KMAX];
    __shared__ int s_ord[IN_KMAX];
    __shared__ int s_stop;
    const int tid = threadIdx.x;
    if (tid < k) {
        s_c[tid] = cin[tid];
        s_st[tid] = -1;
        s_en[tid] = -1;
    }
    __syncthreads();
    long it = 0;
    while (it < max_iter) {
        if (tid == 0) {                                     // stable insertion sort: equal centres stay in index order
            for (int a = 0; a < k; ++a) {
                int j = a;
                while (j > 0 && s_c[s_ord[j - 1]] > s_c[a]) {
                    s_ord[j] = s_ord[j - 1];
                    --j;
                }
                s_ord[j] = a;
            }
        }
        __syncthreads();
        if (tid <= k) {                                     // cut j: first row of the j-th sorted centre
            long cut = tid == 0 ? 0 : n;
            if (tid > 0 && tid < k) {
                const int l = s_ord[tid - 1], u = s_ord[tid];
                const double mid = (s_c[l] + s_c[u]) * 0.5;
                long a = 0, b = n;
                while (a < b) {
                    const long h = (a + b) >> 1;
                    const double x = xs[h];
                    if (x > mid || (x == mid && u < l)) b = h; else a = h + 1;
                }
                cut = a;
            }
            s_cut[tid] = cut;
        }
        __syncthreads();
        if (tid == 0) {
            int same = 1;
            for (int j = 0; j < k; ++j) {
                if (s_cut[j + 1] < s_cut[j]) s_cut[j + 1] = s_cut[j];      // (midpoints that round to the same value)
                const int c = s_ord[j];
                if (s_st[c] != s_cut[j] || s_en[c] != s_cut[j + 1]) same = 0;
                s_st[c] = s_cut[j];
                s_en[c] = s_cut[j + 1];
            }
            s_stop = same;
        }
        __syncthreads();
        for (int c = 0; c < k; ++c) {
            const long lo = s_st[c], hi = s_en[c];
            const double sum = in_range_sum(xs, lo, hi, s_red);
            if (tid == 0) s_new[c] = hi > lo ? sum / (double)(hi - lo) : s_c[c];
        }
        if (tid == 0) {
            double shift = 0.0;
            for (int c = 0; c < k; ++c) {
                const double d = s_new[c] - s_c[c];
                shift += d * d;
                s_c[c] = s_new[c];
            }
            if (shift <= tol) s_stop = 1;
        }
        ++it;
        __syncthreads();
        if (s_stop) break;                                  // (the next write of s_stop lies behind two barriers)
    }
    if (tid < k) cout[tid] = s_c[tid];
    if (tid == 0) *n_iter = it;
}

__global__ __launch_bounds__(IN_T) void in_assign_kernel(const double* __restrict__ x, long n,
                                                         const double* __restrict__ centres, long C,
                                                         long* __restrict__ label) {
    __shared__ double s_c[IN_CHUNK];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * IN_T + tid;
    const double v = i < n ? x[i] : 0.0;
    double best = INFINITY;
    long arg = 0;
    for (long c0 = 0; c0 < C; c0 += IN_CHUNK) {             // (no thread leaves before the last barrier)
        const int m = C - c0 < IN_CHUNK ? (int)(C - c0) : IN_CHUNK;
        for (int j = tid; j < m; j += IN_T) s_c[j] = centres[c0 + j];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            const double d = fabs(v - s_c[j]);
            if (d < best) {                                 // strict: the first of equally near centres is kept
                best = d;
                arg = c0 + j;
            }
        }
        __syncthreads();
    }
    if (i < n) label[i] = arg;
}

// ---------------------------------------------------------------------------------------------- C ABI
#define IN_MAXN 2147483647L
#define IN_MAXIT 1000000000L

extern "C" long amx_kth_gap_blocks(long n) { return n < 1 || n >= IN_MAXN ? 0 : (n + IN_T - 1) / IN_T; }

extern "C" int amx_kth_gap_1d(const double* xs, long n, long K, double* gap, double* partial, double* mean_out,
                              void* stream) {
    if (n < 1 || n >= IN_MAXN || K < 1 || K > n) AMX_BADARG(1);
    if (!xs || !gap || !partial || !mean_out) AMX_BADARG(2);
    const long G = amx_kth_gap_blocks(n);
    AMX_LAUNCH(in_gap_kernel, dim3((unsigned)G), dim3(IN_T), 0, (hipStream_t)stream, xs, n, K, gap, partial);
    AMX_CHECK_LAUNCH();
    AMX_LAUNCH(in_mean_kernel, dim3(1), dim3(IN_T), 0, (hipStream_t)stream, (const double*)partial, G, n, mean_out);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_meanshift_1d(const double* xs, long n, const double* seeds, long S, double bw, long max_iter,
                                double* centre, long* count, long* iters, void* stream) {
    if (n < 1 || n >= IN_MAXN || S < 0 || S >= IN_MAXN) AMX_BADARG(1);
    if (!(bw > 0.0) || !(bw < INFINITY) || max_iter < 0 || max_iter > IN_MAXIT) AMX_BADARG(2);
    if (S == 0) return 0;
    if (!xs || !seeds || !centre || !count || !iters) AMX_BADARG(3);
    AMX_LAUNCH(in_meanshift_kernel, dim3((unsigned)S), dim3(IN_T), 0, (hipStream_t)stream, xs, n, seeds, bw, max_iter,
               centre, count, iters);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_lloyd_1d(const double* xs, long n, const double* centres_in, int k, double tol, long max_iter,
                            double* centres_out, long* n_iter, void* stream) {
    if (n < 1 || n >= IN_MAXN || k < 1 || k > IN_KMAX) AMX_BADARG(1);
    if (!(tol >= 0.0) || max_iter < 0 || max_iter > IN_MAXIT) AMX_BADARG(2);
    if (!xs || !centres_in || !centres_out || !n_iter) AMX_BADARG(3);
    AMX_LAUNCH(in_lloyd_kernel, dim3(1), dim3(IN_T), 0, (hipStream_t)stream, xs, n, centres_in, k, tol, max_iter,
               centres_out, n_iter);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_assign_1d(const double* x, long n, const double* centres, long C, long* label, void* stream) {
    if (n < 0 || n >= IN_MAXN || C < 1 || C >= IN_MAXN) AMX_BADARG(1);
    if (n == 0) return 0;
    if (!x || !centres || !label) AMX_BADARG(2);
    AMX_LAUNCH(in_assign_kernel, dim3((unsigned)((n + IN_T - 1) / IN_T)), dim3(IN_T), 0, (hipStream_t)stream, x, n,
               centres, C, label);
    AMX_CHECK_LAUNCH();
    return 0;
}
