// signal.hip — the small pointwise kernels of the ImSpec family (im2spec / spec2im) next to conv1d.hip:
//   F.interpolate(scale_factor=2, mode="nearest") on (N, C, L) and its backward      atomai/nets/ed.py:152-154
//   F.avg_pool1d(x, k, k) / F.avg_pool2d(x, k, k) of the one-channel net input       atomai/nets/ed.py:70-76
//   torch.nn.MSELoss (mean) and its gradient in one pass                             atomai/trainers/trainer.py:740-857
// All HBM-bound, one thread per 16 bytes where the layout allows; sums are formed in a fixed order (no atomics).
#include "amx_device.h"

// ------------------------------------------------------------------ nearest x2 along L, channels-last [N][L][Cs]
// u[n][2 l + d][c] = v[n][l][c]: with 2 L even this is u[q] = v[q >> 1] on the flat position index.
__global__ void upsample1d2x_fwd_kernel(const float* __restrict__ v, float* __restrict__ u, long nout4, int G) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nout4; i += (long)gridDim.x * blockDim.x) {
        const long q = i / G; const int cg = (int)(i - q * G);
        amx_st4(u + i * 4, amx_ld4(v + ((q >> 1) * G + cg) * 4));
    }
}
// dv[q] = du[2 q] + du[2 q + 1]
__global__ void upsample1d2x_bwd_kernel(const float* __restrict__ du, float* __restrict__ dv, long nin4, int G) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nin4; i += (long)gridDim.x * blockDim.x) {
        const long q = i / G; const int cg = (int)(i - q * G);
        const float4 a = amx_ld4(du + ((2 * q) * G + cg) * 4), b = amx_ld4(du + ((2 * q + 1) * G + cg) * 4);
        amx_st4(dv + i * 4, make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w));
    }
}

static inline unsigned sig_blocks(long n) {
    long nb = (n + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : nb > 8192 ? 8192 : nb);
}

extern "C" int amx_upsample1d2x_fwd(const float* v, float* u, int N, int L, int Cs, void* stream) {
    if (!v || !u) AMX_BADARG(1);
    if (N <= 0 || L <= 0 || Cs <= 0 || (Cs & 3)) AMX_BADARG(2);
    const long nout4 = (long)N * 2 * L * (Cs >> 2);
    AMX_LAUNCH(upsample1d2x_fwd_kernel, dim3(sig_blocks(nout4)), dim3(256), 0, (hipStream_t)stream, v, u, nout4, Cs >> 2);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_upsample1d2x_bwd(const float* du, float* dv, int N, int L, int Cs, void* stream) {
    if (!du || !dv) AMX_BADARG(1);
    if (N <= 0 || L <= 0 || Cs <= 0 || (Cs & 3)) AMX_BADARG(2);
    const long nin4 = (long)N * L * (Cs >> 2);
    AMX_LAUNCH(upsample1d2x_bwd_kernel, dim3(sig_blocks(nin4)), dim3(256), 0, (hipStream_t)stream, du, dv, nin4, Cs >> 2);
    AMX_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ average pooling of a one-channel input, floor semantics
// x [N][H][W] -> y [N][H / kh][W / kw]; the window is summed in fp64 (row by row, left to right) and rounded once.
__global__ void avgpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long nout, int H, int W, int Ho,
                                   int Wo, int kh, int kw) {
    const double inv = 1.0 / (double)(kh * kw);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nout; i += (long)gridDim.x * blockDim.x) {
        const int xo = (int)(i % Wo); const long r = i / Wo;
        const int yo = (int)(r % Ho); const long n = r / Ho;
        const float* src = x + ((size_t)n * H + (size_t)yo * kh) * W + (size_t)xo * kw;
        double s = 0.0;
        for (int a = 0; a < kh; ++a)
            for (int b = 0; b < kw; ++b) s += (double)src[(size_t)a * W + b];
        y[i] = (float)(s * inv);
    }
}

extern "C" int amx_avgpool_fwd(const float* x, float* y, int N, int H, int W, int kh, int kw, void* stream) {
    if (!x || !y) AMX_BADARG(1);
    if (N <= 0 || H <= 0 || W <= 0) AMX_BADARG(2);
    if (kh <= 0 || kw <= 0 || kh > H || kw > W) AMX_BADARG(3);
    const int Ho = H / kh, Wo = W / kw;
    const long nout = (long)N * Ho * Wo;
    AMX_LAUNCH(avgpool_fwd_kernel, dim3(sig_blocks(nout)), dim3(256), 0, (hipStream_t)stream, x, y, nout, H, W, Ho, Wo, kh,
               kw);
    AMX_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ mean squared error + gradient
// part[b] = sum over the block's elements of (p - t)^2 (fp64 inside the block, fixed order); grad = 2 (p - t) / n.
// The caller folds part with amx_reduce_rows(part, rows, 1, 1, 1 / n, loss): two deterministic stages.
#define MSE_PER_BLOCK 4096
extern "C" int amx_mse_rows(long n) { return n <= 0 ? 0 : (int)((n + MSE_PER_BLOCK - 1) / MSE_PER_BLOCK); }

__global__ __launch_bounds__(256) void mse_fwd_bwd_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                          float* __restrict__ grad, float* __restrict__ part, long n,
                                                          float gscale) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long i0 = (long)blockIdx.x * MSE_PER_BLOCK;
    const long i1 = i0 + MSE_PER_BLOCK < n ? i0 + MSE_PER_BLOCK : n;
    double s = 0.0;
    for (long i = i0 + tid; i < i1; i += 256) {
        const float d = p[i] - t[i];
        s += (double)d * (double)d;
        if (grad) grad[i] = d * gscale;
    }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) part[blockIdx.x] = (float)red[0];
}

extern "C" int amx_mse_fwd_bwd(const float* p, const float* t, float* grad, float* part, long n, int rows, void* stream) {
    if (!p || !t || !part) AMX_BADARG(1);
    if (n <= 0 || n > (long)0x7fffffff * MSE_PER_BLOCK) AMX_BADARG(2);
    if (rows != amx_mse_rows(n)) AMX_BADARG(3);
    AMX_LAUNCH(mse_fwd_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, p, t, grad, part, n,
               (float)(2.0 / (double)n));
    AMX_CHECK_LAUNCH();
    return 0;
}
