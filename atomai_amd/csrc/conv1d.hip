// conv1d.hip — nn.Conv1d(k = 3 | 1, stride 1, padding = dilation) on fp32 MFMA, its data gradient (the same kernel
// on flipped / transposed weight images) and its weight gradient: the 1-D hot path of the ImSpec family.
//
//   ConvBlock(ndim=1) / DilatedBlock(ndim=1): Conv1d -> LeakyReLU -> BatchNorm1d      atomai/nets/blocks.py:61-76, 300-318
//   SignalEncoder / SignalDecoder (im2spec, spec2im)                                  atomai/nets/ed.py:20-157
//
// Activations are the tape's channels-last tensors with H = 1: [N][L][Cs] fp32, Cs = round_up(C, 4), padding channels
// zero.  The N * L positions are walked as ONE flat range (a tile may span a sample boundary); a tap that would leave
// its own sample is masked per position, so nothing leaks between samples and padding contributes zero AFTER the
// producer's BatchNorm affine (the shift never reaches the halo).
//
// Forward = implicit GEMM  positions x Cout  with K walking (tap, 4-channel group):
//   workgroup = 4 waves, sub-tile = 64 positions; the window of a sub-tile, 64 + 2 * dil positions, is staged ONCE in
//   LDS with the pending affine and input LeakyReLU applied; wave w owns positions [16 w, 16 w + 16) and walks the
//   output channels in blocks of 16 with v_mfma_f32_16x16x4_f32 (one ds_read_b128 of A and one 16-byte read of the
//   packed weights feed four MFMAs, the fragment scheme of linear.hip / conv_kernel.h).  K ascends in a fixed order:
//   two runs give the same bits.
//   BatchNorm statistics: a workgroup owns `rows_pix` consecutive positions = one (sum, M2 about the row mean) row of
//   the "mode 1" layout of bn.hip (what amx_dropout_fwd emits), formed by a second sweep over the block's own output.
// Weight gradient = GEMM  Cin x Cout  per tap with K = positions, split over position ranges into partial rows
//   part[rows][taps][ci_pad][co_pad] (the layout amx_wgrad_reduce reads); no floating-point atomics.
#include "amx_device.h"

#define C1D_TP 64                     // positions of a sub-tile (4 waves x 16)
#define C1D_LDS_MAX (160 * 1024)
#define C1D_RED_BYTES (256 * 16)      // the forward kernel's reduction buffer for the statistics, behind the window
#define C1D_WG_TILES 8                // weight gradient: 16 x 16 output tiles a wave accumulates per launch slice

#define C1D_REFUSE(code, text)                    \
    do {                                          \
        amx_set_error(__func__, -(code), text);   \
        return -(code);                           \
    } while (0)

// ------------------------------------------------------------------ weight images
// img[t][k / 4][n][k % 4], k < kpad, n < npad, zero padded.
//   mode 0 (forward):  k = input channel  (kpad = round_up(Cin_s, 16)), n = output channel (npad = round_up(cout, 16)),
//                      img = w[n][k][t]
//   mode 1 (dgrad):    k = output channel (kpad = round_up(cout, 16)),  n = input channel  (npad = round_up(Cin_s, 16)),
//                      img = w[k][n][taps - 1 - t]
__global__ void pack1d_kernel(const float* __restrict__ w, float* __restrict__ dst, int cout, int cin, int taps, int kpad,
                              int npad, int mode, long total) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int e = (int)(i & 3);
        long r = i >> 2;
        const int n = (int)(r % npad); r /= npad;
        const int kg = (int)(r % (kpad >> 2));
        const int t = (int)(r / (kpad >> 2));
        const int k = kg * 4 + e;
        float v = 0.f;
        if (mode == 0) { if (n < cout && k < cin) v = w[((size_t)n * cin + k) * taps + t]; }
        else           { if (k < cout && n < cin) v = w[((size_t)k * cin + n) * taps + (taps - 1 - t)]; }
        dst[i] = v;
    }
}

extern "C" long amx_pack_weights1d_size(int cout, int Cin_s, int taps) {
    if (cout <= 0 || Cin_s <= 0 || taps <= 0) return 0;
    return (long)taps * amx_round_up(Cin_s, 16) * amx_round_up(cout, 16);
}

extern "C" int amx_pack_weights1d(const float* w, float* dst, int cout, int cin, int Cin_s, int taps, int mode,
                                  void* stream) {
    if (!w || !dst) AMX_BADARG(1);
    if (cout <= 0 || cin <= 0 || Cin_s < cin || (Cin_s & 3)) AMX_BADARG(2);
    if (taps != 1 && taps != 3) AMX_BADARG(3);
    if (mode != 0 && mode != 1) AMX_BADARG(4);
    const int kpad = amx_round_up(mode == 0 ? Cin_s : cout, 16), npad = amx_round_up(mode == 0 ? cout : Cin_s, 16);
    const long total = (long)taps * kpad * npad;
    long nb = (total + 255) / 256;
    if (nb > 4096) nb = 4096;
    AMX_LAUNCH(pack1d_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, w, dst, cout, cin, taps, kpad, npad,
               mode, total);
    AMX_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ staging
// Rows [q0 - halo, q0 - halo + wlen) of x [npix][Cs] -> s [wlen][stride], affine and input activation applied, zeros
// outside [0, npix) and in the channel padding [Cs, stride).
static __device__ __forceinline__ void c1d_stage(float* s, const float* __restrict__ x, const float* __restrict__ sc,
                                                 const float* __restrict__ sh, float in_slope, int Cs, long q0, int halo,
                                                 int wlen, int stride, long npix) {
    const int G4 = stride >> 2, Gs = Cs >> 2;
    for (int i = threadIdx.x; i < wlen * G4; i += 256) {
        const int r = i / G4, cg = i - r * G4;
        const long q = q0 - halo + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cg < Gs && q >= 0 && q < npix) {
            v = amx_ld4(x + (size_t)q * Cs + cg * 4);
            if (sc) {
                const float4 a = amx_ld4(sc + cg * 4), b = amx_ld4(sh + cg * 4);
                v.x = fmaf(v.x, a.x, b.x); v.y = fmaf(v.y, a.y, b.y); v.z = fmaf(v.z, a.z, b.z); v.w = fmaf(v.w, a.w, b.w);
            }
            if (in_slope != 1.f) {
                v.x = v.x > 0.f ? v.x : v.x * in_slope; v.y = v.y > 0.f ? v.y : v.y * in_slope;
                v.z = v.z > 0.f ? v.z : v.z * in_slope; v.w = v.w > 0.f ? v.w : v.w * in_slope;
            }
        }
        amx_st4(s + (size_t)r * stride + cg * 4, v);
    }
}

// ------------------------------------------------------------------ forward / data gradient
// Block b owns positions [b * ppb, min(npix, (b + 1) * ppb)).  halo = dil when the side taps can see data (3 taps,
// dil < L), else 0 and only the centre tap (k = 1: the only tap) is evaluated.
__global__ __launch_bounds__(256) void conv1d_fwd_kernel(const float* __restrict__ x, const float* __restrict__ sc,
                                                         const float* __restrict__ sh, float in_slope, int Cs,
                                                         const float* __restrict__ wpk, const float* __restrict__ bias,
                                                         float* __restrict__ y, int cout, int cos, float* __restrict__ stats,
                                                         int cop, long npix, int L, int taps, int dil, int halo,
                                                         float slope, int ppb, int kpad, int npad) {
    AMX_DYN_SMEM(float, s_in);                    // [C1D_TP + 2 * halo][kpad + 4], then red [256] float4
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = lane & 15, g = lane >> 4;
    const int stride = kpad + 4;
    const int wlen = C1D_TP + 2 * halo;
    float4* red = reinterpret_cast<float4*>(s_in + (size_t)wlen * stride);
    const long b0 = (long)blockIdx.x * ppb;
    const long b1 = b0 + ppb < npix ? b0 + ppb : npix;
    const bool side = taps == 3 && halo > 0;
    const int t_lo = (taps == 3 && !side) ? 1 : 0, t_hi = (taps == 3 && !side) ? 2 : taps;
    const int KG = kpad >> 2;

    for (long q0 = b0; q0 < b1; q0 += C1D_TP) {
        c1d_stage(s_in, x, sc, sh, in_slope, Cs, q0, halo, wlen, stride, npix);
        __syncthreads();
        const long q = q0 + wave * 16 + p;
        const bool rowok = q < b1;
        const int l = (int)(q % L);
        bool ok[3];
        int roff[3];
        #pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int off = side ? (t - 1) * dil : 0;
            ok[t] = rowok && l + off >= 0 && l + off < L;
            roff[t] = (wave * 16 + p + halo + off) * stride;
        }
        for (int cb = 0; cb < (npad >> 4); ++cb) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            #pragma unroll
            for (int t = 0; t < 3; ++t) {
                if (t < t_lo || t >= t_hi) continue;
                const float* wt = wpk + (size_t)t * KG * npad * 4;
                for (int kk = 0; kk < (kpad >> 4); ++kk) {
                    float4 a = amx_ld4(s_in + roff[t] + (4 * kk + g) * 4);
                    if (!ok[t]) a = make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 b = amx_ld4(wt + ((size_t)(4 * kk + g) * npad + cb * 16 + p) * 4);
                    // one MFMA contracts the channels {c, 4 + c, 8 + c, 12 + c} of this 16-channel step
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
                }
            }
            // D fragment: column = output channel cb * 16 + p, rows = positions 4 g + r of the wave
            const int co = cb * 16 + p;
            if (co < cos) {
                const float bv = (bias && co < cout) ? bias[co] : 0.f;
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long qq = q0 + wave * 16 + 4 * g + r;
                    if (qq >= b1) continue;
                    float v = acc[r] + bv;
                    v = v > 0.f ? v : v * slope;
                    y[(size_t)qq * cos + co] = v;
                }
            }
        }
        __syncthreads();
    }
    if (!stats) return;
    // (sum, M2 about the row mean) of the block's positions per channel, in a fixed order (dropout.hip's scheme)
    const int G = cos >> 2, P = 256 / G;
    const int cg = tid % G, lp = tid / G;
    const bool act = lp < P;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (act)
        for (long px = b0 + lp; px < b1; px += P) {
            const float4 v = amx_ld4(y + (size_t)px * cos + cg * 4);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    red[tid] = s;
    __syncthreads();
    float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < P; ++j) { const float4 t = red[j * G + cg]; tot.x += t.x; tot.y += t.y; tot.z += t.z; tot.w += t.w; }
    __syncthreads();
    const float inv = 1.0f / (float)(b1 - b0);
    const float4 mu = make_float4(tot.x * inv, tot.y * inv, tot.z * inv, tot.w * inv);
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (act)
        for (long px = b0 + lp; px < b1; px += P) {
            const float4 v = amx_ld4(y + (size_t)px * cos + cg * 4);
            const float dx = v.x - mu.x, dy = v.y - mu.y, dz = v.z - mu.z, dw = v.w - mu.w;
            m.x = fmaf(dx, dx, m.x); m.y = fmaf(dy, dy, m.y); m.z = fmaf(dz, dz, m.z); m.w = fmaf(dw, dw, m.w);
        }
    red[tid] = m;
    __syncthreads();
    if (tid < G) {
        float4 m2 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < P; ++j) { const float4 t = red[j * G + tid]; m2.x += t.x; m2.y += t.y; m2.z += t.z; m2.w += t.w; }
        amx_st4(stats + ((size_t)blockIdx.x * 2) * cop + tid * 4, tot);
        amx_st4(stats + ((size_t)blockIdx.x * 2 + 1) * cop + tid * 4, m2);
    }
}

static size_t c1d_fwd_lds(int Cs, int halo) {
    return (size_t)(C1D_TP + 2 * halo) * (amx_round_up(Cs, 16) + 4) * sizeof(float) + C1D_RED_BYTES;
}

// 1: the launch fits (the staged window of 64 + 2 * dil positions x (round_up(Cs, 16) + 4) channels and the 4 KB
// reduction buffer of the statistics are at most 160 KB of LDS)
extern "C" int amx_conv1d_supported(int Cs, int cout, int L, int taps, int dil) {
    if (Cs <= 0 || (Cs & 3) || cout <= 0 || cout > 1024 || L <= 0 || (taps != 1 && taps != 3) || dil < 1) return 0;
    const int halo = (taps == 3 && dil < L) ? dil : 0;
    if (halo > (1 << 20)) return 0;
    return c1d_fwd_lds(Cs, halo) <= C1D_LDS_MAX;
}

extern "C" int amx_conv1d_fwd(const float* x, const float* sc, const float* sh, float in_slope, int Cs, const float* wpk,
                              const float* bias, float* y, float* stats, int N, int L, int cout, int taps, int dil,
                              float slope, int rows, int rows_pix, void* stream) {
    if (!x || !wpk || !y) C1D_REFUSE(1, "x, wpk and y must not be NULL");
    if ((sc == nullptr) != (sh == nullptr)) C1D_REFUSE(2, "scale and shift come as a pair");
    if (Cs <= 0 || (Cs & 3)) C1D_REFUSE(3, "Cs: stored input channels must be a positive multiple of 4");
    if (N <= 0 || L <= 0) C1D_REFUSE(4, "N, L must be positive");
    if (cout <= 0 || cout > 1024) C1D_REFUSE(5, "cout: 1 .. 1024 output channels");
    if (taps != 1 && taps != 3) C1D_REFUSE(6, "taps: kernel size 3 or 1");
    if (dil < 1 || (taps == 1 && dil != 1)) C1D_REFUSE(7, "dil: dilation >= 1 (1 for a one-tap kernel)");
    const long npix = (long)N * L;
    const int halo = (taps == 3 && dil < L) ? dil : 0;
    if (!amx_conv1d_supported(Cs, cout, L, taps, dil))
        C1D_REFUSE(7, "dil: the window of 64 + 2 * dil positions x round_up(Cs, 16) channels exceeds 160 KB of LDS");
    int ppb = C1D_TP;
    long nblk = (npix + ppb - 1) / ppb;
    if (stats) {
        if (rows <= 0 || rows_pix <= 0 || (long)rows * rows_pix < npix || (long)(rows - 1) * rows_pix >= npix)
            C1D_REFUSE(8, "rows, rows_pix: every statistics row must own at least one position");
        ppb = rows_pix; nblk = rows;
    }
    if (nblk > 0x7fffffffL) C1D_REFUSE(4, "N * L: too many positions for one launch");
    const int cos = amx_round_up(cout, 4), cop = amx_round_up(cout, 16);
    const int kpad = amx_round_up(Cs, 16), npad = cop;
    const size_t lds = c1d_fwd_lds(Cs, halo);
    if (lds > 64 * 1024) AMX_ALLOW_160K_LDS(conv1d_fwd_kernel);
    AMX_LAUNCH(conv1d_fwd_kernel, dim3((unsigned)nblk), dim3(256), lds, (hipStream_t)stream, x, sc, sh, in_slope, Cs, wpk,
               bias, y, cout, cos, stats, cop, npix, L, taps, dil, halo, slope, ppb, kpad, npad);
    AMX_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ weight gradient
// positions per partial row: 256, doubled until at most 512 rows remain
static inline int c1d_wgrad_ppr(long npix) {
    int ppr = 256;
    while ((npix + ppr - 1) / ppr > 512 && ppr < (1 << 30)) ppr *= 2;
    return ppr;
}
extern "C" int amx_conv1d_wgrad_rows(int N, int L) {
    if (N <= 0 || L <= 0) return 0;
    const long npix = (long)N * L;
    const int ppr = c1d_wgrad_ppr(npix);
    return (int)((npix + ppr - 1) / ppr);
}

// grid (rows, slices): block (b, z) owns positions [b * ppr, ...) and the output tiles [32 z, 32 z + 32) of the
// taps x (ci_pad / 16) x (co_pad / 16) tiles of 16 x 16; wave w accumulates tiles 32 z + w + 4 m, m < 8.
__global__ __launch_bounds__(256) void conv1d_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ sc,
                                                           const float* __restrict__ sh, float in_slope, int Cs,
                                                           const float* __restrict__ dpre, int cos,
                                                           float* __restrict__ part, float* __restrict__ bpart, long npix,
                                                           int L, int taps, int dil, int halo, int ppr, int ci_pad,
                                                           int co_pad) {
    AMX_DYN_SMEM(float, smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = lane & 15, g = lane >> 4;
    const int sx = ci_pad + 4, sd = co_pad + 4;
    const int wlen = C1D_TP + 2 * halo;
    float* s_x = smem;                                   // [wlen][sx]
    float* s_d = s_x + (size_t)wlen * sx;                // [C1D_TP][sd]
    int* s_ok = reinterpret_cast<int*>(s_d + (size_t)C1D_TP * sd);      // [3][C1D_TP]
    const long b0 = (long)blockIdx.x * ppr;
    const long b1 = b0 + ppr < npix ? b0 + ppr : npix;
    const bool side = taps == 3 && halo > 0;
    const int CIB = ci_pad >> 4, COB = co_pad >> 4;
    const int nt = taps * CIB * COB;

    int t_of[C1D_WG_TILES], ci0[C1D_WG_TILES], co0[C1D_WG_TILES];
    bool live[C1D_WG_TILES];
    f32x4 acc[C1D_WG_TILES];
    #pragma unroll
    for (int m = 0; m < C1D_WG_TILES; ++m) {
        const int tile = (int)blockIdx.y * (4 * C1D_WG_TILES) + wave + 4 * m;
        const int tt = tile / (CIB * COB), rem = tile - tt * (CIB * COB);
        t_of[m] = tt; ci0[m] = (rem / COB) * 16; co0[m] = (rem % COB) * 16;
        // a side tap that can never see data (dil >= L) keeps its zeros
        live[m] = tile < nt && (taps == 1 || side || tt == 1);
        acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};

    for (long q0 = b0; q0 < b1; q0 += C1D_TP) {
        c1d_stage(s_x, x, sc, sh, in_slope, Cs, q0, halo, wlen, sx, npix);
        const int Gd = sd >> 2, Gc = cos >> 2;
        for (int i = tid; i < C1D_TP * Gd; i += 256) {
            const int r = i / Gd, cg = i - r * Gd;
            const long q = q0 + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cg < Gc && q < b1) v = amx_ld4(dpre + (size_t)q * cos + cg * 4);
            amx_st4(s_d + (size_t)r * sd + cg * 4, v);
        }
        if (tid < 3 * C1D_TP) {
            const int t = tid / C1D_TP, r = tid - t * C1D_TP;
            const long q = q0 + r;
            const int l = (int)(q % L);
            const int off = side ? (t - 1) * dil : 0;
            s_ok[tid] = (q < b1 && l + off >= 0 && l + off < L) ? 1 : 0;
        }
        __syncthreads();
        #pragma unroll
        for (int m = 0; m < C1D_WG_TILES; ++m) {
            if (!live[m]) continue;
            const int off = side ? (t_of[m] - 1) * dil : 0;
            const float* ax = s_x + (size_t)(halo + off + g) * sx + ci0[m] + p;
            const float* bd = s_d + (size_t)g * sd + co0[m] + p;
            const int* okp = s_ok + t_of[m] * C1D_TP + g;
            for (int s = 0; s < C1D_TP / 4; ++s) {                      // K = the four positions 4 s + g
                float a = ax[(size_t)(4 * s) * sx];
                const float b = bd[(size_t)(4 * s) * sd];
                if (!okp[4 * s]) a = 0.f;
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[m], 0, 0, 0);
            }
        }
        if (bpart && blockIdx.y == 0) {
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int co = tid + 256 * u;
                if (co < co_pad)
                    for (int r = 0; r < C1D_TP; ++r) bsum[u] += s_d[(size_t)r * sd + co];
            }
        }
        __syncthreads();
    }
    // D fragment: column = output channel co0 + p, rows = input channels ci0 + 4 g + r
    float* prow = part + (size_t)blockIdx.x * taps * ci_pad * co_pad;
    #pragma unroll
    for (int m = 0; m < C1D_WG_TILES; ++m) {
        const int tile = (int)blockIdx.y * (4 * C1D_WG_TILES) + wave + 4 * m;
        if (tile >= nt) continue;
        #pragma unroll
        for (int r = 0; r < 4; ++r)
            prow[((size_t)t_of[m] * ci_pad + ci0[m] + 4 * g + r) * co_pad + co0[m] + p] = acc[m][r];
    }
    if (bpart && blockIdx.y == 0) {
        #pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int co = tid + 256 * u;
            if (co < co_pad) bpart[(size_t)blockIdx.x * co_pad + co] = bsum[u];
        }
    }
}

static size_t c1d_wgrad_lds(int Cs, int cout, int halo) {
    return ((size_t)(C1D_TP + 2 * halo) * (amx_round_up(Cs, 16) + 4) + (size_t)C1D_TP * (amx_round_up(cout, 16) + 4)
            + 3 * C1D_TP) * sizeof(float);
}

extern "C" int amx_conv1d_wgrad_supported(int Cs, int cout, int L, int taps, int dil) {
    if (!amx_conv1d_supported(Cs, cout, L, taps, dil)) return 0;
    const int halo = (taps == 3 && dil < L) ? dil : 0;
    return c1d_wgrad_lds(Cs, cout, halo) <= C1D_LDS_MAX;
}

extern "C" int amx_conv1d_wgrad(const float* x, const float* sc, const float* sh, float in_slope, int Cs,
                                const float* dpre, float* part, float* bpart, int N, int L, int cout, int taps, int dil,
                                int rows, void* stream) {
    if (!x || !dpre || !part) C1D_REFUSE(1, "x, dpre and part must not be NULL");
    if ((sc == nullptr) != (sh == nullptr)) C1D_REFUSE(2, "scale and shift come as a pair");
    if (Cs <= 0 || (Cs & 3)) C1D_REFUSE(3, "Cs: stored input channels must be a positive multiple of 4");
    if (N <= 0 || L <= 0) C1D_REFUSE(4, "N, L must be positive");
    if (cout <= 0 || cout > 1024) C1D_REFUSE(5, "cout: 1 .. 1024 output channels");
    if (taps != 1 && taps != 3) C1D_REFUSE(6, "taps: kernel size 3 or 1");
    if (dil < 1 || (taps == 1 && dil != 1)) C1D_REFUSE(7, "dil: dilation >= 1 (1 for a one-tap kernel)");
    if (!amx_conv1d_wgrad_supported(Cs, cout, L, taps, dil))
        C1D_REFUSE(7, "dil: the staged window (64 + 2 * dil positions) and the gradient tile exceed 160 KB of LDS");
    if (rows != amx_conv1d_wgrad_rows(N, L)) C1D_REFUSE(8, "rows: must be amx_conv1d_wgrad_rows(N, L)");
    const long npix = (long)N * L;
    const int halo = (taps == 3 && dil < L) ? dil : 0;
    const int cos = amx_round_up(cout, 4);
    const int ci_pad = amx_round_up(Cs, 16), co_pad = amx_round_up(cout, 16);
    const int nt = taps * (ci_pad >> 4) * (co_pad >> 4);
    const int slices = amx_ceil_div(nt, 4 * C1D_WG_TILES);
    if (slices > 65535) C1D_REFUSE(5, "cout x Cs: too many 16 x 16 gradient tiles for one launch");
    const size_t lds = c1d_wgrad_lds(Cs, cout, halo);
    if (lds > 64 * 1024) AMX_ALLOW_160K_LDS(conv1d_wgrad_kernel);
    AMX_LAUNCH(conv1d_wgrad_kernel, dim3((unsigned)rows, (unsigned)slices), dim3(256), lds, (hipStream_t)stream, x, sc, sh,
               in_slope, Cs, dpre, cos, part, bpart, npix, L, taps, dil, halo, c1d_wgrad_ppr(npix), ci_pad, co_pad);
    AMX_CHECK_LAUNCH();
    return 0;
}
