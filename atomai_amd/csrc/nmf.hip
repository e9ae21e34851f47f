// nmf.hip — non-negative matrix factorisation X ~ W H by coordinate descent, on the device.
//
// Replaces sklearn.decomposition.NMF(solver='cd') behind the reference's imlocal.nmf / imblock_nmf
// (atomai/stat/multivar.py:248-289, 486-528), SlidingFFTNMF.run_nmf (atomai/stat/fft_nmf.py:218-265) and
// SpectralUnmixer(method='nmf') (atomai/stat/unmixer.py).  One half-step of that solver updates one factor T (R x k) with
// the other one, F (L x k), fixed: it needs XF = X F (R x k) and the Gram matrix FF = F^T F (k x k); row i of T then reads
// nothing but row i, so the sweep is sequential over the k components only:
//     for t in 0 .. k-1:  grad = -XF[i][t] + sum_r FF[t][r] T[i][r]
//                         violation += |T[i][t] == 0 ? min(0, grad) : grad|
//                         if FF[t][t] != 0:  T[i][t] = max(T[i][t] - grad / FF[t][t], 0)
// Updating W: T = W, F = H^T, R = n, L = d.  Updating H^T: T = H^T, F = W, R = d, L = n, X read transposed.
//   nmf_xf_rows<TX, KC>   (W half)   X[r][j] with the REDUCTION axis j contiguous: a wave owns 32 / KC rows, its lanes run
//                         along j (coalesced), every lane keeps KC accumulators per row and the wave adds them by a
//                         __shfl_xor butterfly.
//   nmf_xf_cols<TX, KC>   (H half)   X[j][r] with the OUTPUT axis r contiguous: a thread owns one row r (lanes run along r,
//                         coalesced), F[j][.] is the same address for the whole wave.
//   Both split the reduction axis into S = amx_nmf_splits(...) chunks (grid.y) and write P[s][r][t]: with a few hundred
//   rows a grid over rows alone would leave most compute units idle.  Every partial is summed in a fixed order.
//   nmf_cd_kernel<KC>     one thread per row of T: adds the partials in split order, runs the sweep with FF in LDS, writes
//                         the row back; the workgroup emits its partial violation and the partial Gram matrix T^T T of
//                         the rows it wrote (the other half-step's FF).  gram_only: no sweep (the first FF).
//   nmf_reduce_kernel     adds the per-workgroup partials in workgroup order -> violation scalar, Gram matrix.
// X keeps its dtype (float32 or float64); every product, sum and update is fp64.  No atomics: two runs give the same bits.
//
// Roofline.  One half-step moves n d sizeof(X) bytes for 2 n d k flops: k / 2 flop per byte of float32 X.  Against
// 8 TB/s of HBM and 78.6 TFLOP/s of fp64 vector arithmetic the balance is ~10 flop/byte, i.e. k ~ 20 for float32 and
// k ~ 40 for float64: for the k of 3 - 8 that users ask for the step is HBM-bound (L2-bound when X fits the 256 MB
// last-level cache, as the 841 x 4096 matrix of SlidingFFTNMF does).  The register budget drives the tiling: with k
// accumulators per owned row, 32 fp64 accumulators (64 VGPRs) per thread is the ceiling, so a thread of nmf_xf_rows owns
// 32 / KC rows (8, 4, 2, 1 for KC = 4, 8, 16, 32) and a thread of nmf_xf_cols owns one row of up to 32 accumulators.
// Resources of every instantiation: profiles/nmf_kernel_resources.txt (no scratch).
#include "amx_device.h"

#define NMF_KMAX 32
#define NMF_T 256                      // threads of an xf workgroup
#define NMF_CD_T 128                   // rows (= threads) of a cd workgroup
#define NMF_ROWS_CHUNK 256             // smallest reduction chunk of nmf_xf_rows (4 trips of a wave)
#define NMF_COLS_CHUNK 32              // smallest reduction chunk of nmf_xf_cols
#define NMF_TARGET_BLOCKS 512          // (2 per compute unit; a constant, so that the splits depend on the shape only)
#define NMF_MAX_SPLITS 32

static inline int nmf_kc(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }
static inline long nmf_row_block(int k, int trans) { return trans ? NMF_T : (NMF_T / AMX_WAVE) * (32 / nmf_kc(k)); }

// chunk length of the reduction axis; the number of splits is ceil(L / chunk)
static long nmf_chunk(long R, long L, int k, int trans) {
    const long rb = (R + nmf_row_block(k, trans) - 1) / nmf_row_block(k, trans);
    const long min_chunk = trans ? NMF_COLS_CHUNK : NMF_ROWS_CHUNK;
    long want = (NMF_TARGET_BLOCKS + rb - 1) / rb;
    want = want > NMF_MAX_SPLITS ? NMF_MAX_SPLITS : want;
    long chunk = (L + want - 1) / want;
    chunk = chunk < min_chunk ? min_chunk : chunk;
    return trans ? chunk : (chunk + AMX_WAVE - 1) / AMX_WAVE * AMX_WAVE;      // (rows: whole trips of a wave)
}

template <typename TX, int KC>
__global__ __launch_bounds__(NMF_T) void nmf_xf_rows(const TX* __restrict__ X, long R, long L, const double* __restrict__ F,
                                                     int k, long chunk, double* __restrict__ P) {
    constexpr int RPT = 32 / KC;
    const int lane = threadIdx.x & (AMX_WAVE - 1), wave = threadIdx.x / AMX_WAVE;
    const long r0 = ((long)blockIdx.x * (NMF_T / AMX_WAVE) + wave) * RPT;
    const long s = blockIdx.y, lo = s * chunk, hi = lo + chunk < L ? lo + chunk : L;
    double acc[RPT][KC];
    #pragma unroll
    for (int i = 0; i < RPT; ++i)
        #pragma unroll
        for (int t = 0; t < KC; ++t) acc[i][t] = 0.0;
    for (long j = lo + lane; j < hi; j += AMX_WAVE) {
        double f[KC];
        #pragma unroll
        for (int t = 0; t < KC; ++t) f[t] = t < k ? F[j * k + t] : 0.0;
        #pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const double x = r0 + i < R ? (double)X[(r0 + i) * L + j] : 0.0;
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
                if (lane == 0 && r0 + i < R) P[(s * R + r0 + i) * k + t] = v;
            }
        }
    }
}

template <typename TX, int KC>
__global__ __launch_bounds__(NMF_T) void nmf_xf_cols(const TX* __restrict__ X, long R, long L, const double* __restrict__ F,
                                                     int k, long chunk, double* __restrict__ P) {
    const long r = (long)blockIdx.x * NMF_T + threadIdx.x;
    const long s = blockIdx.y, lo = s * chunk, hi = lo + chunk < L ? lo + chunk : L;
    const bool live = r < R;
    double acc[KC];
    #pragma unroll
    for (int t = 0; t < KC; ++t) acc[t] = 0.0;
    #pragma unroll 4
    for (long j = lo; j < hi; ++j) {
        const double x = live ? (double)X[j * R + r] : 0.0;
        #pragma unroll
        for (int t = 0; t < KC; ++t) acc[t] += x * (t < k ? F[j * k + t] : 0.0);
    }
    if (live) {
        #pragma unroll
        for (int t = 0; t < KC; ++t)
            if (t < k) P[(s * R + r) * k + t] = acc[t];
    }
}

template <int KC>
__global__ __launch_bounds__(NMF_CD_T) void nmf_cd_kernel(const double* __restrict__ P, long S, long R, int k,
                                                          const double* __restrict__ FF, double* __restrict__ T,
                                                          int gram_only, double* __restrict__ Pv, double* __restrict__ Pg) {
    __shared__ double s_ff[KC * KC];
    __shared__ double s_w[KC][NMF_CD_T + 1];
    __shared__ double s_v[NMF_CD_T];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * NMF_CD_T + tid;
    const bool live = i < R;
    if (!gram_only)
        for (int e = tid; e < k * k; e += NMF_CD_T) s_ff[(e / k) * KC + e % k] = FF[e];
    double w[KC], xf[KC];
    #pragma unroll
    for (int t = 0; t < KC; ++t) {
        w[t] = (live && t < k) ? T[i * k + t] : 0.0;
        xf[t] = 0.0;
    }
    double viol = 0.0;
    __syncthreads();
    if (live && !gram_only) {
        for (long s = 0; s < S; ++s) {
            #pragma unroll
            for (int t = 0; t < KC; ++t)
                if (t < k) xf[t] += P[(s * R + i) * k + t];
        }
        #pragma unroll
        for (int t = 0; t < KC; ++t) {
            if (t < k) {
                double grad = -xf[t];
                #pragma unroll
                for (int r = 0; r < KC; ++r)
                    if (r < k) grad += s_ff[t * KC + r] * w[r];
                const double pg = w[t] == 0.0 ? (grad < 0.0 ? grad : 0.0) : grad;
                viol += fabs(pg);
                const double hess = s_ff[t * KC + t];
                if (hess != 0.0) {
                    const double nw = w[t] - grad / hess;
                    w[t] = nw > 0.0 ? nw : 0.0;
                }
            }
        }
        #pragma unroll
        for (int t = 0; t < KC; ++t)
            if (t < k) T[i * k + t] = w[t];
    }
    #pragma unroll
    for (int t = 0; t < KC; ++t) s_w[t][tid] = w[t];
    s_v[tid] = viol;
    __syncthreads();
    for (int e = tid; e < k * k; e += NMF_CD_T) {                  // Gram matrix of this workgroup's rows, in row order
        const int a = e / k, b = e % k;
        double g = 0.0;
        for (int m = 0; m < NMF_CD_T; ++m) g += s_w[a][m] * s_w[b][m];
        Pg[(long)blockIdx.x * k * k + e] = g;
    }
    if (tid == 0) {
        double v = 0.0;
        for (int m = 0; m < NMF_CD_T; ++m) v += s_v[m];
        Pv[blockIdx.x] = v;
    }
}

__global__ __launch_bounds__(NMF_T) void nmf_reduce_kernel(const double* __restrict__ Pv, const double* __restrict__ Pg,
                                                           long G, int k, double* __restrict__ viol,
                                                           double* __restrict__ gram) {
    const int e = blockIdx.x * NMF_T + threadIdx.x;
    if (e < k * k) {
        double g = 0.0;
        for (long b = 0; b < G; ++b) g += Pg[b * k * k + e];
        gram[e] = g;
    } else if (e == k * k && viol) {
        double v = 0.0;
        for (long b = 0; b < G; ++b) v += Pv[b];
        *viol = v;
    }
}

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" long amx_nmf_rows(void) { return NMF_CD_T; }

extern "C" long amx_nmf_splits(long n, long d, int k, int trans) {
    if (n < 1 || d < 1 || k < 1 || k > NMF_KMAX) return 0;
    const long R = trans ? d : n, L = trans ? n : d, chunk = nmf_chunk(R, L, k, trans);
    return (L + chunk - 1) / chunk;
}

template <typename TX, int KC>
static void nmf_xf_launch(const TX* X, long R, long L, int trans, const double* F, int k, long chunk, long S, double* P,
                          hipStream_t st) {
    const dim3 grid((unsigned)((R + nmf_row_block(k, trans) - 1) / nmf_row_block(k, trans)), (unsigned)S), block(NMF_T);
    if (trans) AMX_LAUNCH((nmf_xf_cols<TX, KC>), grid, block, 0, st, X, R, L, F, k, chunk, P);
    else AMX_LAUNCH((nmf_xf_rows<TX, KC>), grid, block, 0, st, X, R, L, F, k, chunk, P);
}

template <typename TX>
static void nmf_xf_dispatch(const TX* X, long R, long L, int trans, const double* F, int k, long chunk, long S, double* P,
                            hipStream_t st) {
    switch (nmf_kc(k)) {
        case 4: nmf_xf_launch<TX, 4>(X, R, L, trans, F, k, chunk, S, P, st); break;
        case 8: nmf_xf_launch<TX, 8>(X, R, L, trans, F, k, chunk, S, P, st); break;
        case 16: nmf_xf_launch<TX, 16>(X, R, L, trans, F, k, chunk, S, P, st); break;
        default: nmf_xf_launch<TX, 32>(X, R, L, trans, F, k, chunk, S, P, st); break;
    }
}

extern "C" int amx_nmf_xf(const void* X, int is_f64, long n, long d, int trans, const double* F, int k, double* P,
                          void* stream) {
    if (n < 1 || d < 1 || n >= 2147483647L || d >= 2147483647L) AMX_BADARG(1);
    if (k < 1 || k > NMF_KMAX) AMX_BADARG(2);
    if (!X || !F || !P) AMX_BADARG(3);
    const long R = trans ? d : n, L = trans ? n : d, chunk = nmf_chunk(R, L, k, trans), S = (L + chunk - 1) / chunk;
    if ((R + nmf_row_block(k, trans) - 1) / nmf_row_block(k, trans) >= 2147483647L || S > 65535) AMX_BADARG(4);
    if (is_f64) nmf_xf_dispatch<double>((const double*)X, R, L, trans != 0, F, k, chunk, S, P, (hipStream_t)stream);
    else nmf_xf_dispatch<float>((const float*)X, R, L, trans != 0, F, k, chunk, S, P, (hipStream_t)stream);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_nmf_cd(const double* P, long S, long R, int k, const double* FF, double* T, int gram_only, double* Pv,
                          double* Pg, void* stream) {
    if (R < 1 || R >= 2147483647L || S < 0) AMX_BADARG(1);
    if (k < 1 || k > NMF_KMAX) AMX_BADARG(2);
    if (!T || !Pv || !Pg || (!gram_only && (!P || !FF || S < 1))) AMX_BADARG(3);
    const dim3 grid((unsigned)((R + NMF_CD_T - 1) / NMF_CD_T)), block(NMF_CD_T);
    const hipStream_t st = (hipStream_t)stream;
    switch (nmf_kc(k)) {
        case 4: AMX_LAUNCH((nmf_cd_kernel<4>), grid, block, 0, st, P, S, R, k, FF, T, gram_only, Pv, Pg); break;
        case 8: AMX_LAUNCH((nmf_cd_kernel<8>), grid, block, 0, st, P, S, R, k, FF, T, gram_only, Pv, Pg); break;
        case 16: AMX_LAUNCH((nmf_cd_kernel<16>), grid, block, 0, st, P, S, R, k, FF, T, gram_only, Pv, Pg); break;
        default: AMX_LAUNCH((nmf_cd_kernel<32>), grid, block, 0, st, P, S, R, k, FF, T, gram_only, Pv, Pg); break;
    }
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_nmf_reduce(const double* Pv, const double* Pg, long G, int k, double* viol, double* gram, void* stream) {
    if (G < 1) AMX_BADARG(1);
    if (k < 1 || k > NMF_KMAX) AMX_BADARG(2);
    if (!Pv || !Pg || !gram) AMX_BADARG(3);
    AMX_LAUNCH(nmf_reduce_kernel, dim3((unsigned)((k * k + 1 + NMF_T - 1) / NMF_T)), dim3(NMF_T), 0, (hipStream_t)stream, Pv,
               Pg, G, k, viol, gram);
    AMX_CHECK_LAUNCH();
    return 0;
}
