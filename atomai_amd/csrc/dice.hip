// dice.hip — the reference's Dice and focal losses (atomai/losses_metrics/losses.py:13-89, selected at :148-151).
//
//   dice_loss(eps): probas = softmax over K (K == 1: the two channels (sigmoid, 1 - sigmoid) against (y, 1 - y), y =
//   labels.squeeze(1).long()); per BIN j  I_j = sum probas * onehot,  C_j = sum (probas + onehot);
//   loss = 1 - mean_j 2 I_j / (C_j + eps).  The sums run over dims = (0,) + range(2, labels.ndimension()) (losses.py:85):
//     K == 1  labels (N,1,H,W) -> dims (0,2,3): 2 bins (foreground, background), each over every pixel;
//     K >= 2  labels (N,H,W)   -> dims (0,2):   only N and H are summed, K * W bins, one per (class, image column).
//   Both are the contract.  Gradient with B bins:  a_j = -2 / (B (C_j + eps)),  b_j = 2 I_j / (B (C_j + eps)^2),
//   g = a_j * onehot + b_j = d loss / d probas;  K >= 2: dlogit_k = p_k (g_k - sum_m p_m g_m);  K == 1: dlogit =
//   s (1 - s) (g_fg - g_bg).  Two passes: the bin sums, the [B][2] table (a_j, b_j), then the gradient.
//
//   focal_loss(alpha, gamma): c = mean BCEWithLogits (amx_bce_fwd_bwd / amx_px_ce_train), pt = exp(-c),
//   F = alpha (1 - pt)^gamma c — a scalar function of the MEAN BCE (losses.py:45-50), not a per-pixel focal term.
//
// Everything is fp32 and deterministic: a bin's partial sum lives in ONE thread's registers (a thread owns an image column
// and walks down a range of (n, h) rows), partial rows are folded in row order (amx_reduce_rows_chunked, then the
// finalize kernel in fp64); no floating-point atomics.
#include "amx_device.h"

#define DICE_MAXCLS 8           // classes whose probabilities a thread holds in registers (more: re-read, as head.hip)
#define DICE_U 4                // rows of a thread in flight: every load of the group is issued before the first use

extern "C" int amx_dice_bins(int K, int W) { return K == 1 ? 2 : K * W; }

// rows of the partial tensor [rows][2][B] both sums kernels write (I then C), sized so that 4 waves per SIMD are resident
extern "C" int amx_dice_rows(int N, int H, int W, int K) {
    if (N <= 0 || H <= 0 || W <= 0 || K < 1) return 0;
    if (K == 1) {
        const long r = ((long)N * H * W + 1023) / 1024;
        return (int)(r < 1 ? 1 : r > 1024 ? 1024 : r);
    }
    const long nh = (long)N * H;
    return (int)(nh < 512 ? nh : 512);
}

// ------------------------------------------------------------------ bin sums on NCHW logits, K >= 2
// grid (rows, ceil(W / 256)): a thread owns column w and rows [r0, r1) of the N*H image rows.
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                        float* __restrict__ part, int NH, int H, int W, int K, int rpb) {
    const int w = blockIdx.y * 256 + threadIdx.x;
    if (w >= W) return;
    const size_t HW = (size_t)H * W;
    const int r0 = blockIdx.x * rpb;
    const int r1 = r0 + rpb < NH ? r0 + rpb : NH;
    float* prow = part + (size_t)blockIdx.x * 2 * K * W;
    for (int k0 = 0; k0 < K; k0 += DICE_MAXCLS) {               // (one trip for K <= DICE_MAXCLS)
        const int kc = K - k0 < DICE_MAXCLS ? K - k0 : DICE_MAXCLS;
        float I[DICE_MAXCLS], Cs[DICE_MAXCLS];
        #pragma unroll
        for (int k = 0; k < DICE_MAXCLS; ++k) { I[k] = 0.f; Cs[k] = 0.f; }
        for (int r = r0; r < r1; r += DICE_U) {
            float v[DICE_U][DICE_MAXCLS];
            int t[DICE_U];
            const float* xp[DICE_U];
            #pragma unroll
            for (int u = 0; u < DICE_U; ++u) {
                const int ru = r + u < r1 ? r + u : r;          // (clamped: loads are unconditional)
                const int n = ru / H, h = ru - n * H;
                xp[u] = x + (size_t)n * K * HW + (size_t)h * W + w;
                #pragma unroll
                for (int k = 0; k < DICE_MAXCLS; ++k) v[u][k] = k < kc ? xp[u][(size_t)(k0 + k) * HW] : 0.f;
                t[u] = (int)tgt[(size_t)ru * W + w];
            }
            #pragma unroll
            for (int u = 0; u < DICE_U; ++u) {
                if (r + u >= r1) continue;
                float mx = -3.4e38f, se = 0.f;
                if (K <= DICE_MAXCLS) {
                    #pragma unroll
                    for (int k = 0; k < DICE_MAXCLS; ++k) if (k < kc) mx = fmaxf(mx, v[u][k]);
                    #pragma unroll
                    for (int k = 0; k < DICE_MAXCLS; ++k) if (k < kc) { v[u][k] = expf(v[u][k] - mx); se += v[u][k]; }
                } else {                                         // the whole class axis re-read for max and sum
                    for (int k = 0; k < K; ++k) mx = fmaxf(mx, xp[u][(size_t)k * HW]);
                    for (int k = 0; k < K; ++k) se += expf(xp[u][(size_t)k * HW] - mx);
                    #pragma unroll
                    for (int k = 0; k < DICE_MAXCLS; ++k) if (k < kc) v[u][k] = expf(v[u][k] - mx);
                }
                const float inv_s = 1.f / se;
                #pragma unroll
                for (int k = 0; k < DICE_MAXCLS; ++k) {
                    if (k >= kc) break;
                    const float p = v[u][k] * inv_s, oh = (k0 + k == t[u]) ? 1.f : 0.f;
                    I[k] = fmaf(p, oh, I[k]);
                    Cs[k] += p + oh;
                }
            }
        }
        #pragma unroll
        for (int k = 0; k < DICE_MAXCLS; ++k) {
            if (k >= kc) break;
            prow[(size_t)(k0 + k) * W + w] = I[k];
            prow[(size_t)(K + k0 + k) * W + w] = Cs[k];
        }
    }
}

// Block sums of four per-thread values in a fixed tree -> out[0..3]
static __device__ __forceinline__ void dice_block_sum4(float* red, float a0, float a1, float a2, float a3, float* out) {
    const int tid = threadIdx.x;
    red[tid] = a0; red[256 + tid] = a1; red[512 + tid] = a2; red[768 + tid] = a3;
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) {
            red[tid] += red[tid + o]; red[256 + tid] += red[256 + tid + o];
            red[512 + tid] += red[512 + tid + o]; red[768 + tid] += red[768 + tid + o];
        }
    }
    if (tid == 0) { out[0] = red[0]; out[1] = red[256]; out[2] = red[512]; out[3] = red[768]; }
}

// ------------------------------------------------------------------ bin sums, K == 1: (I_fg, I_bg, C_fg, C_bg) per workgroup
// labels: float mask (truncated as .long() does) or int64, values 0 / 1 (torch.eye(2)[labels], losses.py:71)
__global__ __launch_bounds__(256) void dice_sums_bin_kernel(const float* __restrict__ x, const long long* __restrict__ ti,
                                                            const float* __restrict__ tf, float* __restrict__ part, long n) {
    __shared__ float red[4 * 256];
    float i1 = 0.f, i0 = 0.f, c1 = 0.f, c0 = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = x[i];
        const long long y = ti ? ti[i] : (long long)tf[i];
        const float e = expf(-fabsf(v));
        const float sg = v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e), ng = 1.f - sg;
        const float o1 = y == 1 ? 1.f : 0.f, o0 = y == 0 ? 1.f : 0.f;
        i1 = fmaf(sg, o1, i1); i0 = fmaf(ng, o0, i0);
        c1 += sg + o1; c0 += ng + o0;
    }
    dice_block_sum4(red, i1, i0, c1, c0, part + (size_t)blockIdx.x * 4);
}

extern "C" int amx_dice_sums(const float* logits, const long long* target, const float* target_f, float* part, int rows,
                             int N, int K, int H, int W, void* stream) {
    if (!logits || !part || N <= 0 || K < 1 || H <= 0 || W <= 0) AMX_BADARG(1);
    if (rows != amx_dice_rows(N, H, W, K)) AMX_BADARG(2);
    if (K == 1) {
        if ((target == nullptr) == (target_f == nullptr)) AMX_BADARG(3);
        AMX_LAUNCH(dice_sums_bin_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, target, target_f, part,
                   (long)N * H * W);
    } else {
        if (!target) AMX_BADARG(3);
        const int NH = N * H, rpb = amx_ceil_div(NH, rows);
        AMX_LAUNCH(dice_sums_kernel, dim3(rows, amx_ceil_div(W, 256)), dim3(256), 0, (hipStream_t)stream, logits, target,
                   part, NH, H, W, K, rpb);
    }
    AMX_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ finalize: [nch][2][B] sums -> table [B][2] and the loss
// (one workgroup: B is K * W at most a few thousand; the nch chunk rows are added in order, in fp64)
__global__ __launch_bounds__(256) void dice_finalize_kernel(const float* __restrict__ sums, int nch, int B, float eps,
                                                            float* __restrict__ table, float* __restrict__ loss) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int j = tid; j < B; j += 256) {
        double i64 = 0.0, c64 = 0.0;
        for (int r = 0; r < nch; ++r) {
            i64 += (double)sums[(size_t)r * 2 * B + j];
            c64 += (double)sums[(size_t)r * 2 * B + B + j];
        }
        const float I = (float)i64, den = (float)c64 + eps;      // (fp32 `cardinality + eps`, as the reference forms it)
        acc += (double)(2.f * I / den);
        table[2 * j] = -2.f / ((float)B * den);
        table[2 * j + 1] = 2.f * I / ((float)B * den * den);
    }
    red[tid] = acc; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) *loss = (float)(1.0 - red[0] / (double)B);
}

extern "C" int amx_dice_finalize(const float* sums, int nch, int B, float eps, float* table, float* loss, void* stream) {
    if (!sums || !table || !loss || nch <= 0 || B <= 0) AMX_BADARG(1);
    AMX_LAUNCH(dice_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sums, nch, B, eps, table, loss);
    AMX_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ gradient on NCHW logits (upstream gradient 1)
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                       const float* __restrict__ table, float* __restrict__ dx,
                                                       long npix, long HW, int W, int K) {
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const long n = p / HW, hw = p - n * HW;
        const int w = (int)(hw % W);
        const float* xp = x + (size_t)n * K * HW + hw;
        float* dp = dx + (size_t)n * K * HW + hw;
        const int t = (int)tgt[p];
        if (K <= DICE_MAXCLS) {
            float v[DICE_MAXCLS], g[DICE_MAXCLS];
            float mx = -3.4e38f;
            #pragma unroll
            for (int k = 0; k < DICE_MAXCLS; ++k) {
                if (k >= K) break;
                v[k] = xp[(size_t)k * HW]; mx = fmaxf(mx, v[k]);
                const float2 ab = *reinterpret_cast<const float2*>(table + 2 * ((size_t)k * W + w));
                g[k] = k == t ? ab.x + ab.y : ab.y;
            }
            float se = 0.f;
            #pragma unroll
            for (int k = 0; k < DICE_MAXCLS; ++k) { if (k >= K) break; v[k] = expf(v[k] - mx); se += v[k]; }
            const float inv_s = 1.f / se;
            float dot = 0.f;
            #pragma unroll
            for (int k = 0; k < DICE_MAXCLS; ++k) { if (k >= K) break; v[k] *= inv_s; dot = fmaf(v[k], g[k], dot); }
            #pragma unroll
            for (int k = 0; k < DICE_MAXCLS; ++k) { if (k >= K) break; dp[(size_t)k * HW] = v[k] * (g[k] - dot); }
        } else {                                                 // re-reading form: same operations in the same order
            float mx = -3.4e38f, se = 0.f, dot = 0.f;
            for (int k = 0; k < K; ++k) mx = fmaxf(mx, xp[(size_t)k * HW]);
            for (int k = 0; k < K; ++k) se += expf(xp[(size_t)k * HW] - mx);
            const float inv_s = 1.f / se;
            for (int k = 0; k < K; ++k) {
                const float2 ab = *reinterpret_cast<const float2*>(table + 2 * ((size_t)k * W + w));
                dot = fmaf(expf(xp[(size_t)k * HW] - mx) * inv_s, k == t ? ab.x + ab.y : ab.y, dot);
            }
            for (int k = 0; k < K; ++k) {
                const float2 ab = *reinterpret_cast<const float2*>(table + 2 * ((size_t)k * W + w));
                dp[(size_t)k * HW] = expf(xp[(size_t)k * HW] - mx) * inv_s * ((k == t ? ab.x + ab.y : ab.y) - dot);
            }
        }
    }
}

__global__ __launch_bounds__(256) void dice_bwd_bin_kernel(const float* __restrict__ x, const long long* __restrict__ ti,
                                                           const float* __restrict__ tf, const float* __restrict__ table,
                                                           float* __restrict__ dx, long n) {
    const float a1 = table[0], b1 = table[1], a0 = table[2], b0 = table[3];      // bins (foreground, background)
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = x[i];
        const long long y = ti ? ti[i] : (long long)tf[i];
        const float e = expf(-fabsf(v));
        const float sg = v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        const float g1 = y == 1 ? a1 + b1 : b1, g0 = y == 0 ? a0 + b0 : b0;
        dx[i] = sg * (1.f - sg) * (g1 - g0);
    }
}

extern "C" int amx_dice_bwd(const float* logits, const long long* target, const float* target_f, const float* table,
                            float* dlogits, int N, int K, int H, int W, void* stream) {
    if (!logits || !table || !dlogits || N <= 0 || K < 1 || H <= 0 || W <= 0) AMX_BADARG(1);
    const long npix = (long)N * H * W;
    long nb = (npix + 255) / 256;
    if (nb > 4096) nb = 4096;
    if (K == 1) {
        if ((target == nullptr) == (target_f == nullptr)) AMX_BADARG(2);
        AMX_LAUNCH(dice_bwd_bin_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, logits, target, target_f,
                   table, dlogits, npix);
    } else {
        if (!target) AMX_BADARG(2);
        AMX_LAUNCH(dice_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, logits, target, table, dlogits,
                   npix, (long)H * W, W, K);
    }
    AMX_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ bin sums fused with the head (training path)
// The last activation a [npix][Cs] in px_bwd's lane layout (G = Cs / 4 lanes share a pixel, PL = 256 / G pixel lanes per
// workgroup; head.hip): a pixel's logits are formed in registers (xor-shuffle dot products, the arithmetic of
// px_ce_train_kernel), softmax / sigmoid, and only the bin partials are written.  grid (rows, ceil(Wv / PL)): pixel lane pl
// owns column w and walks rows [r0, r1) of an image of NHv rows x Wv columns — the real geometry for K >= 2 (bins are
// (class, column)); for K == 1 (two bins over everything) the pixels are taken as rows of PL and the four per-thread sums
// are folded by the fixed tree.  BCESUM (KT == 1): the sum of the BCE-with-logits terms instead (part[blk][0]; the first
// pass of the fused focal loss, whose gradient needs the MEAN over every pixel before the head's backward can be formed).
template <int KT, bool BCESUM = false>
__global__ __launch_bounds__(256) void px_dice_sums_kernel(const float* __restrict__ a, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ w,
                                                           const float* __restrict__ b, const long long* __restrict__ tgt,
                                                           const float* __restrict__ tgtf, float* __restrict__ part,
                                                           long npix, int NHv, int Wv, int C, int Cs, int rpb) {
    constexpr int K = KT;
    __shared__ float red[KT == 1 ? 4 * 256 : 4];
    const int G = Cs >> 2, PL = 256 / G;
    const int tid = threadIdx.x;
    const int pl = tid / G, cg = tid - pl * G;
    float bk[KT];
    float4 wk[KT];
    #pragma unroll
    for (int k = 0; k < KT; ++k) {
        bk[k] = b[k];
        const int c = cg * 4;
        const float* wr = w + (size_t)k * C;
        wk[k].x = c + 0 < C ? wr[c + 0] : 0.f; wk[k].y = c + 1 < C ? wr[c + 1] : 0.f;
        wk[k].z = c + 2 < C ? wr[c + 2] : 0.f; wk[k].w = c + 3 < C ? wr[c + 3] : 0.f;
    }
    float4 sc = make_float4(1, 1, 1, 1), sh = make_float4(0, 0, 0, 0);
    if (scale) { sc = amx_ld4(scale + cg * 4); sh = amx_ld4(shift + cg * 4); }
    const int col = blockIdx.y * PL + pl;
    const int r0 = blockIdx.x * rpb;
    const int r1 = r0 + rpb < NHv ? r0 + rpb : NHv;
    constexpr int NA = KT == 1 ? 2 : KT;
    float I[NA], Cc[NA];
    #pragma unroll
    for (int k = 0; k < NA; ++k) { I[k] = 0.f; Cc[k] = 0.f; }
    for (int r = r0; r < r1; r += DICE_U) {                      // (workgroup-uniform trip count: the shuffles need whole waves)
        float4 av[DICE_U];
        long long tv[DICE_U];
        float tfv[DICE_U];
        bool ok[DICE_U];
        #pragma unroll
        for (int u = 0; u < DICE_U; ++u) {
            const long pu = (long)(r + u) * Wv + col;
            ok[u] = r + u < r1 && col < Wv && pu < npix;
            const long pc = ok[u] ? pu : 0;                       // (loads are unconditional, clamped to pixel 0)
            av[u] = amx_ld4(a + (size_t)pc * Cs + cg * 4);
            if (KT == 1) { tfv[u] = tgtf[pc]; tv[u] = (long long)tfv[u]; } else { tfv[u] = 0.f; tv[u] = tgt[pc]; }
        }
        #pragma unroll
        for (int u = 0; u < DICE_U; ++u) {
            float4 v = av[u];
            v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y);
            v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
            float lg[KT];
            #pragma unroll
            for (int k = 0; k < KT; ++k) {
                float t = v.x * wk[k].x;
                t = fmaf(v.y, wk[k].y, t); t = fmaf(v.z, wk[k].z, t); t = fmaf(v.w, wk[k].w, t);
                for (int o = 1; o < G; o <<= 1) t += __shfl_xor(t, o);
                lg[k] = t + bk[k];
            }
            if (!ok[u]) continue;
            if (KT == 1 && BCESUM) {                             // (the term of bce_fwd_bwd_kernel / px_ce_train_kernel)
                const float xv = lg[0], e = expf(-fabsf(xv));
                I[0] += fmaxf(xv, 0.f) - xv * tfv[u] + log1pf(e);
            } else if (KT == 1) {
                const float xv = lg[0], e = expf(-fabsf(xv));
                const float sg = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e), ng = 1.f - sg;
                const float o1 = tv[u] == 1 ? 1.f : 0.f, o0 = tv[u] == 0 ? 1.f : 0.f;
                I[0] = fmaf(sg, o1, I[0]); I[1] = fmaf(ng, o0, I[1]);
                Cc[0] += sg + o1; Cc[1] += ng + o0;
            } else {
                float mx = lg[0];
                #pragma unroll
                for (int k = 1; k < KT; ++k) mx = fmaxf(mx, lg[k]);
                float se = 0.f;
                #pragma unroll
                for (int k = 0; k < KT; ++k) { lg[k] = expf(lg[k] - mx); se += lg[k]; }
                const float inv_s = 1.f / se;
                #pragma unroll
                for (int k = 0; k < KT; ++k) {
                    const float p = lg[k] * inv_s, oh = (k == (int)tv[u]) ? 1.f : 0.f;
                    I[k] = fmaf(p, oh, I[k]);
                    Cc[k] += p + oh;
                }
            }
        }
    }
    if (KT == 1) {
        const bool mine = cg == 0;                               // (the G lanes of a pixel hold the same sums: one of them counts)
        dice_block_sum4(red, mine ? I[0] : 0.f, mine ? I[1] : 0.f, mine ? Cc[0] : 0.f, mine ? Cc[1] : 0.f,
                        part + (size_t)blockIdx.x * 4);
    } else if (cg == 0 && col < Wv) {
        float* prow = part + (size_t)blockIdx.x * 2 * K * Wv;
        #pragma unroll
        for (int k = 0; k < KT; ++k) {
            prow[(size_t)k * Wv + col] = I[k];
            prow[(size_t)(K + k) * Wv + col] = Cc[k];
        }
    }
}

extern "C" int amx_px_dice_train_supported(int Cs, int K, int W) {
    const int G = Cs >> 2;
    return (Cs > 0 && !(Cs & 3) && Cs <= 256 && (G & (G - 1)) == 0 && K >= 1 && K <= 4 && W >= 1) ? 1 : 0;
}

extern "C" int amx_px_dice_sums(const float* a, const float* scale, const float* shift, const float* w, const float* b,
                                const long long* target, const float* target_f, float* part, int rows, int N, int H,
                                int W, int C, int Cs, int K, void* stream) {
    if (!a || !w || !b || !part || C <= 0 || Cs < C || N <= 0 || H <= 0 || W <= 0) AMX_BADARG(1);
    if (!amx_px_dice_train_supported(Cs, K, W) || (K == 1 ? !target_f : !target)) AMX_BADARG(2);
    if ((scale == nullptr) != (shift == nullptr)) AMX_BADARG(3);
    if (rows != amx_dice_rows(N, H, W, K)) AMX_BADARG(4);
    const long npix = (long)N * H * W;
    const int PL = 256 / (Cs / 4);
    const int Wv = K == 1 ? PL : W;
    const int NHv = K == 1 ? (int)((npix + PL - 1) / PL) : N * H;
    const int rpb = amx_ceil_div(NHv, rows);
    const dim3 grid(rows, amx_ceil_div(Wv, PL));
#define PX_DICE_SUMS_LAUNCH(KT_)                                                                                       \
    AMX_LAUNCH(px_dice_sums_kernel<KT_>, grid, dim3(256), 0, (hipStream_t)stream, a, scale, shift, w, b, target, target_f, \
               part, npix, NHv, Wv, C, Cs, rpb)
    switch (K) {
        case 1: PX_DICE_SUMS_LAUNCH(1); break;
        case 2: PX_DICE_SUMS_LAUNCH(2); break;
        case 3: PX_DICE_SUMS_LAUNCH(3); break;
        default: PX_DICE_SUMS_LAUNCH(4); break;
    }
#undef PX_DICE_SUMS_LAUNCH
    AMX_CHECK_LAUNCH();
    return 0;
}

// Sum of the BCE-with-logits terms of the one-class head over the last activation: part [rows][4], column 0 (rows =
// amx_dice_rows(N, H, W, 1)); amx_reduce_rows(part, rows, 4, 1, 1 / npix) gives the mean c of focal_loss (losses.py:45).
extern "C" int amx_px_bce_sum(const float* a, const float* scale, const float* shift, const float* w, const float* b,
                              const float* target_f, float* part, int rows, int N, int H, int W, int C, int Cs,
                              void* stream) {
    if (!a || !w || !b || !target_f || !part || C <= 0 || Cs < C || N <= 0 || H <= 0 || W <= 0) AMX_BADARG(1);
    if (!amx_px_dice_train_supported(Cs, 1, W)) AMX_BADARG(2);
    if ((scale == nullptr) != (shift == nullptr)) AMX_BADARG(3);
    if (rows != amx_dice_rows(N, H, W, 1)) AMX_BADARG(4);
    const long npix = (long)N * H * W;
    const int PL = 256 / (Cs / 4);
    const int NHv = (int)((npix + PL - 1) / PL);
    AMX_LAUNCH((px_dice_sums_kernel<1, true>), dim3(rows), dim3(256), 0, (hipStream_t)stream, a, scale, shift, w, b,
               (const long long*)nullptr, target_f, part, npix, NHv, PL, C, Cs, amx_ceil_div(NHv, rows));
    AMX_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ focal loss from the mean BCE (two device scalars)
__global__ void focal_from_bce_kernel(const float* __restrict__ c, float alpha, float gamma, float* __restrict__ loss,
                                      float* __restrict__ dfdc) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float ce = *c;
    const float om = -expm1f(-ce), pt = 1.f - om;               // 1 - pt without the cancellation of 1 - exp(-c)
    const float pw = powf(om, gamma);
    *loss = alpha * pw * ce;
    *dfdc = alpha * (pw + ce * gamma * powf(om, gamma - 1.f) * pt);
}

extern "C" int amx_focal_from_bce(const float* c, float alpha, float gamma, float* loss_out, float* dfdc_out, void* stream) {
    if (!c || !loss_out || !dfdc_out) AMX_BADARG(1);
    AMX_LAUNCH(focal_from_bce_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, c, alpha, gamma, loss_out, dfdc_out);
    AMX_CHECK_LAUNCH();
    return 0;
}

// out = a * b: the upstream gradient of the focal loss times dF/dc, the factor amx_scale_unless_one(_multi) then applies
__global__ void mul_scalars_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = *a * *b;
}

extern "C" int amx_mul_scalars(const float* a, const float* b, float* out, void* stream) {
    if (!a || !b || !out) AMX_BADARG(1);
    AMX_LAUNCH(mul_scalars_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, b, out);
    AMX_CHECK_LAUNCH();
    return 0;
}
