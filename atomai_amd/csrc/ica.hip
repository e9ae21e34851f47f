// ica.hip — the FastICA-specific passes (sklearn.decomposition.FastICA, algorithm='parallel'), on the device.
//
// Replaces the host solver behind the reference's imlocal.ica / imblock_ica (atomai/stat/multivar.py:211-246, 445-484) and
// SpectralUnmixer(method='ica') (atomai/stat/unmixer.py).  The driver (stat/_ica.py) whitens through the fp64 Gram matrix of
// the smaller side and torch.linalg.eigh (dense fp64 GEMMs go to the BLAS library); what is ICA's own is here:
//   ica_project<TX, KC>   out[t][r] = scale * sum_j M[t][j] (X[r][j] - mean[j]):  X1 = sqrt(n) K (X - mean)^T before the
//                         iteration and S^T = (W K) (X - mean)^T after it.  X (float32 or float64) is read in place, the
//                         mean is subtracted on load; a wave owns 32 / KC rows, its lanes run along j (coalesced) and a
//                         __shfl_xor butterfly adds the lanes.  (amx_nmf_xf is NOT reused: it cannot subtract the mean
//                         on load, and subtracting K mean afterwards cancels.)
//   ica_step<FUN, KC>     one fixed-point step reads X1 [k][n] exactly once.  A workgroup owns a slice of samples and walks
//                         it in trips of 64: the trip's k x 64 tile of X1 goes to LDS (coalesced), wave q forms
//                         y_i = sum_t W[i][t] x_t for the components i = q, q + 4, ... (W in LDS, the same address for the
//                         whole wave), g = G(y) goes to LDS, G'(y) is added into a register; then every thread owns up to
//                         four entries (i, t) of g X1^T and adds the trip's 64 products in sample order.  The workgroup
//                         writes its partial g X1^T [k][k] and sum G' [k]; no k x n intermediate reaches memory.
//   ica_reduce            adds the partials in a fixed order (a wave per entry: lane l takes the workgroups l, l + 64, ...
//                         in ascending order, a butterfly adds the lanes) and writes g X1^T / n - diag(h) W, h = sum G' / n.
//   ica_rowstd            np.std of every row of S^T [k][n] (two passes, per-thread strided sums added in thread order).
// The k x k symmetric decorrelation (W W^T)^(-1/2) W and lim are torch.linalg.eigh and a handful of k x k torch operations
// on the device (stat/_ica.py); the driver reads back ONE scalar per iteration.  Every sum has a fixed order and there are no
// atomics: two runs give the same bits.  The slice length is a function of n only (ica_chunk), so the grid is too.
//
// Where the time goes.  One step moves 8 k n bytes for 2 k^2 n flops, k / 4 flop per byte: below the fp64 vector balance of
// ~10 flop/byte for every k <= 32, and at the shapes this package meets (n of 1e3 - 1e5, k <= 16: X1 of 0.1 - 10 MB, resident
// in the last-level cache) a step is a few microseconds of work behind the latency of its launches.  What the kernel buys is
// two launches and no temporaries against about ten launches of the same step written as torch operations; the fit as a
// whole is dominated by the Gram matrix of the whitening (2 n d min(n, d) flops, BLAS).  LDS: W (KC^2) and two tiles of
// KC x 65 doubles (rows padded by one double: the column reads of phase C land on distinct banks), 41 KB at KC = 32.
// Registers at KC = 32: 4 accumulators of g X1^T and 8 of sum G' per thread, no per-thread k x k array.
#include "amx_device.h"
#include <cmath>

#define ICA_KMAX 32
#define ICA_T 256                      // threads of every workgroup here
#define ICA_TS 64                      // samples of one trip of ica_step (one per lane of a wave)
#define ICA_MAX_BLOCKS 256             // (one per compute unit; a constant, so that the grid depends on n only)
#define ICA_WAVES (ICA_T / AMX_WAVE)

enum { ICA_LOGCOSH = 0, ICA_EXP = 1, ICA_CUBE = 2 };

static inline int ica_kc(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }

// samples per workgroup of ica_step: whole trips, at most ICA_MAX_BLOCKS workgroups
static long ica_chunk(long n) {
    const long c = (n + ICA_MAX_BLOCKS - 1) / ICA_MAX_BLOCKS;
    return (c + ICA_TS - 1) / ICA_TS * ICA_TS;
}

template <typename TX, int KC>
__global__ __launch_bounds__(ICA_T) void ica_project(const TX* __restrict__ X, long n, long d,
                                                     const double* __restrict__ mean, const double* __restrict__ M, int k,
                                                     double scale, double* __restrict__ out) {
    constexpr int RPT = 32 / KC;
    const int lane = threadIdx.x & (AMX_WAVE - 1), wave = threadIdx.x / AMX_WAVE;
    const long r0 = ((long)blockIdx.x * ICA_WAVES + wave) * RPT;
    double acc[RPT][KC];
    #pragma unroll
    for (int i = 0; i < RPT; ++i)
        #pragma unroll
        for (int t = 0; t < KC; ++t) acc[i][t] = 0.0;
    for (long j = lane; j < d; j += AMX_WAVE) {
        const double mu = mean[j];
        double f[KC];
        #pragma unroll
        for (int t = 0; t < KC; ++t) f[t] = t < k ? M[t * d + j] : 0.0;
        #pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const double x = r0 + i < n ? (double)X[(r0 + i) * d + j] - mu : 0.0;
            #pragma unroll
            for (int t = 0; t < KC; ++t) acc[i][t] += x * f[t];
        }
    }
    #pragma unroll
    for (int i = 0; i < RPT; ++i) {
        #pragma unroll
        for (int t = 0; t < KC; ++t) {
            if (t < k) {                                             // (uniform)
                double v = acc[i][t];
                #pragma unroll
                for (int m = AMX_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
                if (lane == 0 && r0 + i < n) out[(long)t * n + r0 + i] = scale * v;
            }
        }
    }
}

template <int FUN>
static __device__ __forceinline__ void ica_contrast(double y, double alpha, double& g, double& gp) {
    if (FUN == ICA_LOGCOSH) {
        g = tanh(alpha * y);
        gp = alpha * (1.0 - g * g);
    } else if (FUN == ICA_EXP) {
        const double e = exp(-(y * y) / 2.0);
        g = y * e;
        gp = (1.0 - y * y) * e;
    } else {
        g = y * y * y;
        gp = 3.0 * (y * y);
    }
}

template <int FUN, int KC>
__global__ __launch_bounds__(ICA_T) void ica_step(const double* __restrict__ X1, long n, int k,
                                                  const double* __restrict__ W, double alpha, long chunk,
                                                  double* __restrict__ Pg, double* __restrict__ Ph) {
    constexpr int NACC = KC * KC > ICA_T ? KC * KC / ICA_T : 1;     // entries of g X1^T per thread
    constexpr int NH = KC > ICA_WAVES ? KC / ICA_WAVES : 1;         // components per wave
    __shared__ double s_w[KC * KC];
    __shared__ double s_x[KC][ICA_TS + 1];
    __shared__ double s_g[KC][ICA_TS + 1];
    const int tid = threadIdx.x, lane = tid & (AMX_WAVE - 1), wave = tid / AMX_WAVE;
    const long lo = (long)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    for (int e = tid; e < KC * KC; e += ICA_T) {
        const int i = e / KC, t = e % KC;
        s_w[e] = (i < k && t < k) ? W[i * k + t] : 0.0;
    }
    double acc[NACC], hacc[NH];
    #pragma unroll
    for (int c = 0; c < NACC; ++c) acc[c] = 0.0;
    #pragma unroll
    for (int c = 0; c < NH; ++c) hacc[c] = 0.0;
    for (long j0 = lo; j0 < hi; j0 += ICA_TS) {
        __syncthreads();                                             // the last trip's readers are done (first trip: s_w)
        for (int e = tid; e < KC * ICA_TS; e += ICA_T) {
            const int t = e / ICA_TS, m = e % ICA_TS;
            s_x[t][m] = (t < k && j0 + m < hi) ? X1[(long)t * n + j0 + m] : 0.0;
        }
        __syncthreads();
        const bool live = j0 + lane < hi;                            // a sample beyond the slice has x = 0: y = 0, g = 0
        #pragma unroll
        for (int c = 0; c < NH; ++c) {
            const int i = wave + ICA_WAVES * c;                      // (uniform over the wave; i < KC)
            double g = 0.0, gp = 0.0;
            if (i < k) {
                double y = 0.0;
                #pragma unroll
                for (int t = 0; t < KC; ++t) y += s_w[i * KC + t] * s_x[t][lane];
                ica_contrast<FUN>(y, alpha, g, gp);
            }
            s_g[i][lane] = g;
            hacc[c] += live ? gp : 0.0;
        }
        __syncthreads();
        #pragma unroll
        for (int c = 0; c < NACC; ++c) {
            const int e = tid + ICA_T * c;
            if (e < KC * KC) {
                const int i = e / KC, t = e % KC;
                double a = acc[c];
                #pragma unroll 8
                for (int m = 0; m < ICA_TS; ++m) a += s_g[i][m] * s_x[t][m];
                acc[c] = a;
            }
        }
    }
    #pragma unroll
    for (int c = 0; c < NACC; ++c) {
        const int e = tid + ICA_T * c, i = e / KC, t = e % KC;
        if (e < KC * KC && i < k && t < k) Pg[((long)blockIdx.x * k + i) * k + t] = acc[c];
    }
    __syncthreads();
    #pragma unroll
    for (int c = 0; c < NH; ++c) s_g[wave + ICA_WAVES * c][lane] = hacc[c];
    __syncthreads();
    if (tid < k) {
        double h = 0.0;
        for (int m = 0; m < ICA_TS; ++m) h += s_g[tid][m];
        Ph[(long)blockIdx.x * k + tid] = h;
    }
}

// one wave per entry (i, t): lane l adds the workgroups l, l + 64, ... in ascending order, a butterfly adds the lanes
__global__ __launch_bounds__(ICA_T) void ica_reduce(const double* __restrict__ Pg, const double* __restrict__ Ph, long G,
                                                    int k, long n, const double* __restrict__ W, double* __restrict__ A) {
    const int lane = threadIdx.x & (AMX_WAVE - 1);
    const int e = blockIdx.x * ICA_WAVES + threadIdx.x / AMX_WAVE;  // (uniform over the wave)
    if (e >= k * k) return;
    const int i = e / k;
    double s = 0.0, h = 0.0;
    for (long b = lane; b < G; b += AMX_WAVE) {
        s += Pg[b * k * k + e];
        h += Ph[b * k + i];
    }
    #pragma unroll
    for (int m = AMX_WAVE / 2; m >= 1; m >>= 1) {
        s += __shfl_xor(s, m);
        h += __shfl_xor(h, m);
    }
    if (lane == 0) A[e] = s / (double)n - (h / (double)n) * W[e];
}

__global__ __launch_bounds__(ICA_T) void ica_rowstd(const double* __restrict__ S, long n, double* __restrict__ sd) {
    __shared__ double s_p[ICA_T];
    __shared__ double s_mean;
    const int tid = threadIdx.x;
    const double* row = S + (long)blockIdx.x * n;
    double a = 0.0;
    for (long j = tid; j < n; j += ICA_T) a += row[j];
    s_p[tid] = a;
    __syncthreads();
    if (tid == 0) {
        double v = 0.0;
        for (int m = 0; m < ICA_T; ++m) v += s_p[m];
        s_mean = v / (double)n;
    }
    __syncthreads();
    const double mu = s_mean;
    a = 0.0;
    for (long j = tid; j < n; j += ICA_T) a += (row[j] - mu) * (row[j] - mu);
    s_p[tid] = a;                                                    // (thread 0 finished reading s_p before the barrier above)
    __syncthreads();
    if (tid == 0) {
        double v = 0.0;
        for (int m = 0; m < ICA_T; ++m) v += s_p[m];
        sd[blockIdx.x] = sqrt(v / (double)n);
    }
}

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" long amx_ica_blocks(long n, int k) {
    if (n < 1 || n >= 2147483647L || k < 1 || k > ICA_KMAX) return 0;
    const long chunk = ica_chunk(n);
    return (n + chunk - 1) / chunk;
}

template <typename TX>
static void ica_project_dispatch(const TX* X, long n, long d, const double* mean, const double* M, int k, double scale,
                                 double* out, hipStream_t st) {
    const int kc = ica_kc(k);
    const long rows = (long)ICA_WAVES * (32 / kc);
    const dim3 grid((unsigned)((n + rows - 1) / rows)), block(ICA_T);
    switch (kc) {
        case 4: AMX_LAUNCH((ica_project<TX, 4>), grid, block, 0, st, X, n, d, mean, M, k, scale, out); break;
        case 8: AMX_LAUNCH((ica_project<TX, 8>), grid, block, 0, st, X, n, d, mean, M, k, scale, out); break;
        case 16: AMX_LAUNCH((ica_project<TX, 16>), grid, block, 0, st, X, n, d, mean, M, k, scale, out); break;
        default: AMX_LAUNCH((ica_project<TX, 32>), grid, block, 0, st, X, n, d, mean, M, k, scale, out); break;
    }
}

extern "C" int amx_ica_project(const void* X, int is_f64, long n, long d, const double* mean, const double* M, int k,
                               double scale, double* out, void* stream) {
    if (n < 1 || d < 1 || n >= 2147483647L || d >= 2147483647L) AMX_BADARG(1);
    if (k < 1 || k > ICA_KMAX) AMX_BADARG(2);
    if (!X || !mean || !M || !out) AMX_BADARG(3);
    if (is_f64) ica_project_dispatch<double>((const double*)X, n, d, mean, M, k, scale, out, (hipStream_t)stream);
    else ica_project_dispatch<float>((const float*)X, n, d, mean, M, k, scale, out, (hipStream_t)stream);
    AMX_CHECK_LAUNCH();
    return 0;
}

template <int FUN>
static void ica_step_dispatch(const double* X1, long n, int k, const double* W, double alpha, long chunk, double* Pg,
                              double* Ph, hipStream_t st) {
    const dim3 grid((unsigned)((n + chunk - 1) / chunk)), block(ICA_T);
    switch (ica_kc(k)) {
        case 4: AMX_LAUNCH((ica_step<FUN, 4>), grid, block, 0, st, X1, n, k, W, alpha, chunk, Pg, Ph); break;
        case 8: AMX_LAUNCH((ica_step<FUN, 8>), grid, block, 0, st, X1, n, k, W, alpha, chunk, Pg, Ph); break;
        case 16: AMX_LAUNCH((ica_step<FUN, 16>), grid, block, 0, st, X1, n, k, W, alpha, chunk, Pg, Ph); break;
        default: AMX_LAUNCH((ica_step<FUN, 32>), grid, block, 0, st, X1, n, k, W, alpha, chunk, Pg, Ph); break;
    }
}

extern "C" int amx_ica_step(const double* X1, long n, int k, int fun, double alpha, const double* W, double* Pg, double* Ph,
                            void* stream) {
    if (n < 1 || n >= 2147483647L) AMX_BADARG(1);
    if (k < 1 || k > ICA_KMAX) AMX_BADARG(2);
    if (fun < ICA_LOGCOSH || fun > ICA_CUBE || !(alpha >= 1.0 && alpha <= 2.0)) AMX_BADARG(3);
    if (!X1 || !W || !Pg || !Ph) AMX_BADARG(4);
    const long chunk = ica_chunk(n);
    const hipStream_t st = (hipStream_t)stream;
    if (fun == ICA_LOGCOSH) ica_step_dispatch<ICA_LOGCOSH>(X1, n, k, W, alpha, chunk, Pg, Ph, st);
    else if (fun == ICA_EXP) ica_step_dispatch<ICA_EXP>(X1, n, k, W, alpha, chunk, Pg, Ph, st);
    else ica_step_dispatch<ICA_CUBE>(X1, n, k, W, alpha, chunk, Pg, Ph, st);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_ica_reduce(const double* Pg, const double* Ph, long G, int k, long n, const double* W, double* A,
                              void* stream) {
    if (n < 1 || n >= 2147483647L || G != amx_ica_blocks(n, k)) AMX_BADARG(1);
    if (k < 1 || k > ICA_KMAX) AMX_BADARG(2);
    if (!Pg || !Ph || !W || !A) AMX_BADARG(3);
    AMX_LAUNCH(ica_reduce, dim3((unsigned)((k * k + ICA_WAVES - 1) / ICA_WAVES)), dim3(ICA_T), 0, (hipStream_t)stream, Pg, Ph,
               G, k, n, W, A);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_ica_rowstd(const double* S, int k, long n, double* sd, void* stream) {
    if (n < 1 || n >= 2147483647L) AMX_BADARG(1);
    if (k < 1 || k > ICA_KMAX) AMX_BADARG(2);
    if (!S || !sd) AMX_BADARG(3);
    AMX_LAUNCH(ica_rowstd, dim3((unsigned)k), dim3(ICA_T), 0, (hipStream_t)stream, S, n, sd);
    AMX_CHECK_LAUNCH();
    return 0;
}
