// joint.hip — the discrete (Gumbel-Softmax) channel of the joint VAEs jVAE / jrVAE, forward and backward.
//
//   encoder heads:  alpha_h = softmax(fc13[h](x), dim=1)                                  atomai/nets/ed.py:400-403
//   sample:         g = -log(-log(u + 1e-12) + 1e-12);  y = softmax((log(alpha + 1e-12) + g) / tau)
//                                                                              atomai/trainers/vitrainer.py:237-248
//   KL to uniform:  sum_k alpha_k (log(alpha_k + 1e-12) - log(1 / K + 1e-12))      atomai/losses_metrics/vi_losses.py:60-74
//
// The H heads of sizes K_0..K_{H-1} lie side by side in one (B, D) row, D = sum K_h ("segment table", passed by value).
// Limits: H <= AMX_JOINT_MAX_HEADS, D <= AMX_JOINT_MAX_D (include/atomai_amd.h).  B * D is a few thousand floats: these
// kernels are launch-latency bound, so the design goal is ONE launch each way and no host synchronisation.  One wave
// owns one sample (4 waves = 4 samples per block); its lanes stride over the categories of a head, so K = 1, K not a
// multiple of 64 and K > 64 are the same loop.  Reductions are xor butterflies over the 64 lanes: a fixed order, the
// same value in every lane, no atomics.  fp32 throughout.
#include "amx_device.h"

#ifndef AMX_JOINT_MAX_HEADS
#define AMX_JOINT_MAX_HEADS 16
#define AMX_JOINT_MAX_D 4096
#endif
#define JOINT_EPS 1e-12f
#define JOINT_WAVES 4

struct JointSegs {
    int H;
    int off[AMX_JOINT_MAX_HEADS + 1];      // off[h] .. off[h + 1]: the columns of head h; off[H] = D
    float h2[AMX_JOINT_MAX_HEADS];         // log(1 / K_h + 1e-12), in fp32 as log(alpha + 1e-12) is (exactly 0 for K = 1)
};

// Host side: sizes -> table.  Returns nonzero for a table outside the limits.
static int joint_make_segs(const int* sizes, int H, JointSegs* S) {
    if (!sizes || H < 1 || H > AMX_JOINT_MAX_HEADS) return 1;
    int off = 0;
    for (int h = 0; h < H; ++h) {
        const int K = sizes[h];
        if (K < 1 || K > AMX_JOINT_MAX_D) return 1;
        S->off[h] = off;
        S->h2[h] = logf(1.f / (float)K + JOINT_EPS);
        off += K;
        if (off > AMX_JOINT_MAX_D) return 1;
    }
    S->H = H;
    S->off[H] = off;
    return 0;
}

static __device__ __forceinline__ float joint_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
static __device__ __forceinline__ float joint_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ------------------------------------------------------------------ (a) segmented row softmax
__global__ __launch_bounds__(64 * JOINT_WAVES) void segsoftmax_fwd_kernel(const float* __restrict__ logits, JointSegs S,
                                                                           int B, float* __restrict__ alpha) {
    const int b = blockIdx.x * JOINT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;                                          // wave-uniform
    const int D = S.off[S.H];
    for (int h = 0; h < S.H; ++h) {
        const int K = S.off[h + 1] - S.off[h];
        const float* x = logits + (size_t)b * D + S.off[h];
        float* a = alpha + (size_t)b * D + S.off[h];
        float m = -INFINITY;
        for (int k = lane; k < K; k += 64) m = fmaxf(m, x[k]);
        m = joint_wave_max(m);
        float s = 0.f;
        for (int k = lane; k < K; k += 64) { const float e = expf(x[k] - m); a[k] = e; s += e; }
        s = joint_wave_sum(s);
        for (int k = lane; k < K; k += 64) a[k] = a[k] / s;      // re-read by the lane that wrote it
    }
}

// dlogits = alpha * (dalpha - sum_seg alpha * dalpha)
__global__ __launch_bounds__(64 * JOINT_WAVES) void segsoftmax_bwd_kernel(const float* __restrict__ alpha,
                                                                           const float* __restrict__ dalpha, JointSegs S,
                                                                           int B, float* __restrict__ dlogits) {
    const int b = blockIdx.x * JOINT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const int D = S.off[S.H];
    for (int h = 0; h < S.H; ++h) {
        const int K = S.off[h + 1] - S.off[h];
        const size_t base = (size_t)b * D + S.off[h];
        float dot = 0.f;
        for (int k = lane; k < K; k += 64) dot = fmaf(alpha[base + k], dalpha[base + k], dot);
        dot = joint_wave_sum(dot);
        for (int k = lane; k < K; k += 64) dlogits[base + k] = alpha[base + k] * (dalpha[base + k] - dot);
    }
}

extern "C" int amx_segsoftmax_fwd(const float* logits, const int* seg_sizes, int H, int B, float* alpha, void* stream) {
    if (!logits || !alpha || B <= 0) AMX_BADARG(1);
    JointSegs S;
    if (joint_make_segs(seg_sizes, H, &S)) AMX_BADARG(2);
    AMX_LAUNCH(segsoftmax_fwd_kernel, dim3(amx_ceil_div(B, JOINT_WAVES)), dim3(64 * JOINT_WAVES), 0, (hipStream_t)stream,
               logits, S, B, alpha);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_segsoftmax_bwd(const float* alpha, const float* dalpha, const int* seg_sizes, int H, int B,
                                  float* dlogits, void* stream) {
    if (!alpha || !dalpha || !dlogits || B <= 0) AMX_BADARG(1);
    JointSegs S;
    if (joint_make_segs(seg_sizes, H, &S)) AMX_BADARG(2);
    AMX_LAUNCH(segsoftmax_bwd_kernel, dim3(amx_ceil_div(B, JOINT_WAVES)), dim3(64 * JOINT_WAVES), 0, (hipStream_t)stream,
               alpha, dalpha, S, B, dlogits);
    AMX_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ (b) joint latent
// What amx_rvae_latent_fwd does for the continuous latents (z = mean + exp(logsd) * eps, the (phi, dx, dy) / content
// split with the translation prior), plus the Gumbel-Softmax sample of every head appended to the content latents and
// the per-sample KL of the heads to the uniform categorical.  Row of zdec: [Z - coord content latents | D samples].
// Parts are switched off by null pointers: u == NULL -> no sample (zdec row = content latents only), kl == NULL -> no
// KL, Z == 0 -> no continuous part.
__global__ __launch_bounds__(64 * JOINT_WAVES) void joint_latent_fwd_kernel(
    const float* __restrict__ zmean, const float* __restrict__ zlogsd, const float* __restrict__ eps,
    const float* __restrict__ alpha, const float* __restrict__ u, JointSegs S, int B, int Z, int coord, float dx_prior,
    float tau, float* __restrict__ theta, float* __restrict__ zdec, float* __restrict__ kl) {
    const int b = blockIdx.x * JOINT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const int D = S.off[S.H];
    const int W = Z - coord + (u ? D : 0);
    for (int d = lane; d < Z; d += 64) {
        const size_t i = (size_t)b * Z + d;
        const float z = fmaf(expf(zlogsd[i]), eps[i], zmean[i]);
        if (d >= coord) zdec[(size_t)b * W + d - coord] = z;
        else if (d == 0) theta[b * 3] = z;
        else theta[b * 3 + d] = z * dx_prior;
    }
    if (coord == 1 && lane == 0) { theta[b * 3 + 1] = 0.f; theta[b * 3 + 2] = 0.f; }
    float klacc = 0.f;
    for (int h = 0; h < S.H; ++h) {
        const int K = S.off[h + 1] - S.off[h];
        const float* a = alpha + (size_t)b * D + S.off[h];
        if (kl) {
            const float h2 = S.h2[h];
            for (int k = lane; k < K; k += 64) { const float al = a[k]; klacc += al * (logf(al + JOINT_EPS) - h2); }
        }
        if (u) {
            const float* uu = u + (size_t)b * D + S.off[h];
            float* y = zdec + (size_t)b * W + (Z - coord) + S.off[h];
            float m = -INFINITY;
            for (int k = lane; k < K; k += 64) {
                const float g = -logf(-logf(uu[k] + JOINT_EPS) + JOINT_EPS);
                const float l = (logf(a[k] + JOINT_EPS) + g) / tau;
                y[k] = l;
                m = fmaxf(m, l);
            }
            m = joint_wave_max(m);
            float s = 0.f;
            for (int k = lane; k < K; k += 64) { const float e = expf(y[k] - m); y[k] = e; s += e; }
            s = joint_wave_sum(s);
            for (int k = lane; k < K; k += 64) y[k] = y[k] / s;
        }
    }
    if (kl) {
        klacc = joint_wave_sum(klacc);
        if (lane == 0) kl[b] = klacc;
    }
}

// Backward of the above.  zdec is the forward's output (its sample columns are y).  Continuous part as
// amx_rvae_latent_bwd.  Discrete part, sample path and KL path summed into dalpha:
//   dlogit = y (dy - sum y dy) / tau;  dalpha = dlogit / (alpha + 1e-12) + g_kl (log(alpha + 1e-12) - h2 + alpha / (alpha + 1e-12))
// dzdec == NULL -> no sample path (and zero content gradients), g_kl == NULL -> no KL path, dtheta == NULL -> zeros.
__global__ __launch_bounds__(64 * JOINT_WAVES) void joint_latent_bwd_kernel(
    const float* __restrict__ zlogsd, const float* __restrict__ eps, const float* __restrict__ alpha,
    const float* __restrict__ zdec, const float* __restrict__ dtheta, const float* __restrict__ dzdec,
    const float* __restrict__ g_kl, JointSegs S, int B, int Z, int coord, float dx_prior, float tau, int sampled,
    float* __restrict__ dmean, float* __restrict__ dlogsd, float* __restrict__ dalpha) {
    const int b = blockIdx.x * JOINT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const int D = S.off[S.H];
    const int W = Z - coord + (sampled ? D : 0);
    for (int d = lane; d < Z; d += 64) {
        const size_t i = (size_t)b * Z + d;
        float dz;
        if (d >= coord) dz = dzdec ? dzdec[(size_t)b * W + d - coord] : 0.f;
        else if (d == 0) dz = dtheta ? dtheta[b * 3] : 0.f;
        else dz = dtheta ? dtheta[b * 3 + d] * dx_prior : 0.f;
        dmean[i] = dz;
        dlogsd[i] = dz * eps[i] * expf(zlogsd[i]);
    }
    if (!dalpha) return;                                         // kernel-uniform
    const bool sample_path = sampled && dzdec;
    const float gk = g_kl ? g_kl[b] : 0.f;
    for (int h = 0; h < S.H; ++h) {
        const int K = S.off[h + 1] - S.off[h];
        const float* a = alpha + (size_t)b * D + S.off[h];
        const size_t yo = (size_t)b * W + (Z - coord) + S.off[h];
        float dot = 0.f;
        if (sample_path) {
            for (int k = lane; k < K; k += 64) dot = fmaf(zdec[yo + k], dzdec[yo + k], dot);
            dot = joint_wave_sum(dot);
        }
        const float h2 = S.h2[h];
        for (int k = lane; k < K; k += 64) {
            const float al = a[k], den = al + JOINT_EPS;
            float g = 0.f;
            if (sample_path) g = zdec[yo + k] * (dzdec[yo + k] - dot) / tau / den;
            if (g_kl) g += gk * (logf(den) - h2 + al / den);
            dalpha[(size_t)b * D + S.off[h] + k] = g;
        }
    }
}

extern "C" int amx_joint_latent_fwd(const float* zmean, const float* zlogsd, const float* eps, const float* alpha,
                                    const float* u, const int* seg_sizes, int H, int B, int Z, int coord, float dx_prior,
                                    float tau, float* theta, float* zdec, float* kl_disc, void* stream) {
    if (B <= 0 || Z < 0 || !(coord == 0 || coord == 1 || coord == 3) || Z < coord) AMX_BADARG(1);
    if (Z > 0 && (!zmean || !zlogsd || !eps)) AMX_BADARG(2);
    JointSegs S;
    if (!alpha || joint_make_segs(seg_sizes, H, &S)) AMX_BADARG(3);
    if (coord > 0 && !theta) AMX_BADARG(4);
    if ((u || Z > coord) && !zdec) AMX_BADARG(5);
    if (u && !(tau > 0.f)) AMX_BADARG(6);
    if (!u && !kl_disc && Z == 0) AMX_BADARG(7);                 // nothing to do
    AMX_LAUNCH(joint_latent_fwd_kernel, dim3(amx_ceil_div(B, JOINT_WAVES)), dim3(64 * JOINT_WAVES), 0, (hipStream_t)stream,
               zmean, zlogsd, eps, alpha, u, S, B, Z, coord, dx_prior, tau, theta, zdec, kl_disc);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_joint_latent_bwd(const float* zlogsd, const float* eps, const float* alpha, const float* zdec,
                                    const float* dtheta, const float* dzdec, const float* g_kl, const int* seg_sizes,
                                    int H, int B, int Z, int coord, float dx_prior, float tau, int sampled, float* dmean,
                                    float* dlogsd, float* dalpha, void* stream) {
    if (B <= 0 || Z < 0 || !(coord == 0 || coord == 1 || coord == 3) || Z < coord) AMX_BADARG(1);
    if (Z > 0 && (!zlogsd || !eps || !dmean || !dlogsd)) AMX_BADARG(2);
    JointSegs S;
    if (!alpha || joint_make_segs(seg_sizes, H, &S)) AMX_BADARG(3);
    if (sampled && dzdec && (!zdec || !(tau > 0.f))) AMX_BADARG(4);
    if (!dalpha && Z == 0) AMX_BADARG(5);
    AMX_LAUNCH(joint_latent_bwd_kernel, dim3(amx_ceil_div(B, JOINT_WAVES)), dim3(64 * JOINT_WAVES), 0, (hipStream_t)stream,
               zlogsd, eps, alpha, zdec, dtheta, dzdec, g_kl, S, B, Z, coord, dx_prior, tau, sampled, dmean, dlogsd, dalpha);
    AMX_CHECK_LAUNCH();
    return 0;
}
