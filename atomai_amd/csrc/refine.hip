// refine.hip — Gaussian peak refinement of atom positions, on the device.
//
// Replaces the per-atom scipy.optimize.curve_fit loop of the reference's peak_refinement (atomai/utils/coords.py:
// 179-231; model gaussian_2d, coords.py:152-176) and the cKDTree query behind its default half-side
// (get_nn_distances_, coords.py:86-113):
//   refine_kernel       one WAVE per atom, REF_WAVES atoms per workgroup.  The (2d)^2 patch is copied once from the fp32
//                       frame into the wave's slice of LDS; lanes stride over its pixels (any 2 <= d <= 32, patches smaller
//                       than a wave included).  Levenberg-Marquardt with the analytic Jacobian, everything in fp64: per
//                       iteration the 28 + 7 + 1 sums of J^T J, J^T r and r^T r are reduced over the wave with an xor
//                       butterfly (a + b is commutative, so after every stage both partners hold the same bits: all 64
//                       lanes end with identical sums and the control flow below stays wave-uniform), then EVERY lane
//                       solves the damped 7 x 7 system redundantly (Cholesky with a pivot check, fully unrolled in
//                       registers).  No atomics, no cross-wave traffic: bit-reproducible.
//   nn2_kernel          one workgroup per frame: brute force over the frame's atoms, tiled through LDS, fp64 distances,
//                       the two smallest per atom, summed in a fixed order.
// Damping follows MINPACK's scaling (D_j = largest column norm of J seen so far, 1 for a zero column: at the start
// sigma_x = sigma_y makes the theta column exactly zero) with Nielsen's gain-ratio update of lambda.  Stopping rules
// (both at least as tight as the reference's ftol = xtol = 1.49e-8): relative actual AND predicted reduction of the sum
// of squares <= REF_FTOL, or scaled step <= REF_XTOL * scaled parameter norm.  REF_MAX_ITER bounds the number of
// Jacobian evaluations: the reference's maxfev = 200 * (7 + 1) function calls pays for 200 forward-difference
// Jacobians of 7 + 1 calls each.
#include "amx_device.h"

#define REF_WAVES 4                    // atoms per workgroup
#define REF_NP 7                       // amp, xo, yo, sigma_x, sigma_y, theta, offset
#define REF_NS 36                      // 28 (upper triangle of J^T J) + 7 (J^T r) + 1 (r^T r)
#define REF_MAX_ITER 200
#define REF_MAX_TRIALS 64              // damped solves per Jacobian (lambda grows by >= 2x per rejection)
#define REF_LAMBDA0 1.0                // first damping, relative to D^2: the start (sigma = 1, theta = 0, offset = 0) is a
                                       // poor guess, and 1e-3 let the first, nearly undamped step overshoot into a one-pixel
                                       // spike (sigma -> 0.01) when the atom sits 4 px from the patch centre
#define REF_FTOL 1e-12
#define REF_XTOL 1e-10
#define REF_DMAX 32

enum { REF_FITTED = 0, REF_KEPT_PATCH = 1, REF_KEPT_GATE = 2, REF_KEPT_NOCONV = 3, REF_BAD_ROW = 4 };

// Packed index of element (i, j), i <= j, of the upper triangle of a symmetric 7 x 7 matrix (row-major).
static __host__ __device__ constexpr int ref_ut(int i, int j) { return i * REF_NP - i * (i - 1) / 2 + (j - i); }

static __device__ __forceinline__ double ref_wave_sum(double v) {
    #pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

struct RefQuad { double a, b, c; };    // exponent a dx^2 + 2 b dx dy + c dy^2

static __device__ __forceinline__ RefQuad ref_quad(double sx, double sy, double th) {
    const double ct = cos(th), st = sin(th), s2 = sin(2.0 * th);
    RefQuad q;
    q.a = ct * ct / (2.0 * sx * sx) + st * st / (2.0 * sy * sy);
    q.b = -s2 / (4.0 * sx * sx) + s2 / (4.0 * sy * sy);
    q.c = st * st / (2.0 * sx * sx) + ct * ct / (2.0 * sy * sy);
    return q;
}

// Sum of squared residuals of parameters p over the patch (all lanes return the same bits).
static __device__ __forceinline__ double ref_sse(const float* patch, int side, int lane, const double* p) {
    const RefQuad q = ref_quad(p[3], p[4], p[5]);
    double s = 0.0;
    for (int k = lane; k < side * side; k += AMX_WAVE) {
        const double dx = (double)(k / side) - p[1], dy = (double)(k % side) - p[2];
        const double r = p[6] + p[0] * exp(-(q.a * dx * dx + 2.0 * q.b * dx * dy + q.c * dy * dy)) - (double)patch[k];
        s += r * r;
    }
    return ref_wave_sum(s);
}

// Cholesky solve of the symmetric positive definite 7 x 7 system (A + lam * diag(D2)) x = g, A given by its upper
// triangle in row-major packed order.  Returns false when a pivot is not positive (or not a number).
static __device__ __forceinline__ bool ref_solve(const double* A, const double* D2, double lam, const double* g, double* x) {
    double Lm[REF_NP][REF_NP];
    #pragma unroll
    for (int i = 0; i < REF_NP; ++i) {
        #pragma unroll
        for (int j = i; j < REF_NP; ++j) Lm[j][i] = A[ref_ut(i, j)] + (i == j ? lam * D2[i] : 0.0);
    }
    #pragma unroll
    for (int j = 0; j < REF_NP; ++j) {
        double v = Lm[j][j];
        #pragma unroll
        for (int k = 0; k < j; ++k) v -= Lm[j][k] * Lm[j][k];
        if (!(v > 0.0) || !(v < 1e300)) return false;
        const double piv = sqrt(v);
        Lm[j][j] = piv;
        #pragma unroll
        for (int i = j + 1; i < REF_NP; ++i) {
            double w = Lm[i][j];
            #pragma unroll
            for (int k = 0; k < j; ++k) w -= Lm[i][k] * Lm[j][k];
            Lm[i][j] = w / piv;
        }
    }
    double y[REF_NP];
    #pragma unroll
    for (int i = 0; i < REF_NP; ++i) {
        double v = g[i];
        #pragma unroll
        for (int k = 0; k < i; ++k) v -= Lm[i][k] * y[k];
        y[i] = v / Lm[i][i];
    }
    #pragma unroll
    for (int i = REF_NP - 1; i >= 0; --i) {
        double v = y[i];
        #pragma unroll
        for (int k = i + 1; k < REF_NP; ++k) v -= Lm[k][i] * x[k];
        x[i] = v / Lm[i][i];
    }
    return true;
}

__global__ __launch_bounds__(REF_WAVES * AMX_WAVE) void refine_kernel(const float* __restrict__ frames, int B, int H, int W,
                                                                      const double* __restrict__ coords,
                                                                      const int* __restrict__ meta,
                                                                      const int* __restrict__ dside, int dmax, long n,
                                                                      double* __restrict__ out, int* __restrict__ status) {
    AMX_DYN_SMEM(float, smem);                       // [REF_WAVES][(2 dmax)^2]
    const int lane = threadIdx.x & (AMX_WAVE - 1), wave = threadIdx.x / AMX_WAVE;
    const long atom = (long)blockIdx.x * REF_WAVES + wave;
    if (atom >= n) return;                           // whole waves leave; there is no workgroup barrier below
    float* patch = smem + (long)wave * (4 * dmax * dmax);
    const double row = coords[2 * atom], col = coords[2 * atom + 1];
    const int fr = meta[2 * atom];
    int st = REF_KEPT_PATCH;
    double o0 = row, o1 = col;
    const int d = (fr >= 0 && fr < B) ? dside[fr] : 0;
    const bool in_range = fabs(row) < 1e9 && fabs(col) < 1e9;       // also false for NaN
    const int cx = in_range ? (int)rint(row) : -1, cy = in_range ? (int)rint(col) : -1;    // round half to even
    if (d < 2 || d > dmax) {
        st = REF_BAD_ROW;
    } else if (cx - d >= 0 && cx + d <= H && cy - d >= 0 && cy + d <= W) {
        const int side = 2 * d, npx = side * side;
        const float* src = frames + ((long)fr * H + (cx - d)) * W + (cy - d);
        for (int k = lane; k < npx; k += AMX_WAVE) patch[k] = src[(long)(k / side) * W + (k % side)];
        amx_wave_sync();
        double p[REF_NP] = {(double)patch[d * side + d], (double)d, (double)d, 1.0, 1.0, 0.0, 0.0};
        double D2[REF_NP] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double lam = -1.0, nu = 2.0;
        bool converged = false, failed = false;
        for (int it = 0; it < REF_MAX_ITER && !converged && !failed; ++it) {
            // ---- J^T J, J^T r, r^T r at p
            double s[REF_NS];
            #pragma unroll
            for (int k = 0; k < REF_NS; ++k) s[k] = 0.0;
            {
                const double sx = p[3], sy = p[4];
                const double ct = cos(p[5]), sn = sin(p[5]), s2 = sin(2.0 * p[5]), c2 = cos(2.0 * p[5]);
                const RefQuad q = ref_quad(sx, sy, p[5]);
                const double isx3 = 1.0 / (sx * sx * sx), isy3 = 1.0 / (sy * sy * sy);
                const double hx = 1.0 / (2.0 * sx * sx), hy = 1.0 / (2.0 * sy * sy);
                const double a_sx = -ct * ct * isx3, b_sx = s2 * 0.5 * isx3, c_sx = -sn * sn * isx3;
                const double a_sy = -sn * sn * isy3, b_sy = -s2 * 0.5 * isy3, c_sy = -ct * ct * isy3;
                const double a_th = s2 * (hy - hx), b_th = c2 * (hy - hx), c_th = s2 * (hx - hy);
                for (int k = lane; k < npx; k += AMX_WAVE) {
                    const double dx = (double)(k / side) - p[1], dy = (double)(k % side) - p[2];
                    const double xx = dx * dx, xy = 2.0 * dx * dy, yy = dy * dy;
                    const double E = exp(-(q.a * xx + q.b * xy + q.c * yy));
                    const double aE = p[0] * E;
                    double J[REF_NP];
                    J[0] = E;
                    J[1] = aE * (2.0 * q.a * dx + 2.0 * q.b * dy);
                    J[2] = aE * (2.0 * q.b * dx + 2.0 * q.c * dy);
                    J[3] = -aE * (a_sx * xx + b_sx * xy + c_sx * yy);
                    J[4] = -aE * (a_sy * xx + b_sy * xy + c_sy * yy);
                    J[5] = -aE * (a_th * xx + b_th * xy + c_th * yy);
                    J[6] = 1.0;
                    const double r = p[6] + aE - (double)patch[k];
                    #pragma unroll
                    for (int i = 0; i < REF_NP; ++i) {
                        #pragma unroll
                        for (int j = i; j < REF_NP; ++j) s[ref_ut(i, j)] += J[i] * J[j];
                        s[28 + i] += J[i] * r;
                    }
                    s[35] += r * r;
                }
            }
            #pragma unroll
            for (int k = 0; k < REF_NS; ++k) s[k] = ref_wave_sum(s[k]);
            bool finite = true;
            #pragma unroll
            for (int k = 0; k < REF_NS; ++k) finite = finite && (fabs(s[k]) < 1e300);
            if (!finite) { failed = true; break; }
            const double S = s[35];
            double g[REF_NP];
            #pragma unroll
            for (int i = 0; i < REF_NP; ++i) {
                g[i] = -s[28 + i];
                D2[i] = fmax(D2[i], s[ref_ut(i, i)]);
            }
            double Ds[REF_NP];
            #pragma unroll
            for (int i = 0; i < REF_NP; ++i) Ds[i] = D2[i] > 0.0 ? D2[i] : 1.0;
            if (lam < 0.0) lam = REF_LAMBDA0;
            if (S == 0.0) { converged = true; break; }
            // ---- damped steps until one reduces the sum of squares
            bool accepted = false;
            for (int trial = 0; trial < REF_MAX_TRIALS && !accepted && !converged; ++trial) {
                double dl[REF_NP], pn[REF_NP];
                if (!ref_solve(s, Ds, lam, g, dl)) { lam *= nu; nu *= 2.0; continue; }
                double pred = 0.0, step2 = 0.0, norm2 = 0.0;
                #pragma unroll
                for (int i = 0; i < REF_NP; ++i) {
                    pn[i] = p[i] + dl[i];
                    pred += dl[i] * (g[i] + lam * Ds[i] * dl[i]);
                    step2 += Ds[i] * dl[i] * dl[i];
                    norm2 += Ds[i] * p[i] * p[i];
                }
                const double Sn = ref_sse(patch, side, lane, pn);
                const bool ok = Sn <= S;                            // false for NaN / inf
                const double act = ok ? (S - Sn) / S : -1.0, prel = pred / S;
                if (ok) {
                    #pragma unroll
                    for (int i = 0; i < REF_NP; ++i) p[i] = pn[i];
                    accepted = true;
                    const double rho = pred > 0.0 ? (S - Sn) / pred : 0.0, t = 2.0 * rho - 1.0;
                    lam *= fmax(1.0 / 3.0, 1.0 - t * t * t);
                    nu = 2.0;
                    if (act <= REF_FTOL && prel <= REF_FTOL) converged = true;
                } else {
                    lam *= nu;
                    nu *= 2.0;
                }
                if (step2 <= REF_XTOL * REF_XTOL * norm2) converged = true;
            }
            if (!accepted && !converged) failed = true;
        }
        if (converged && !failed) {
            const double ex = p[1] - (double)d, ey = p[2] - (double)d;
            if (sqrt(ex * ex + ey * ey) < 3.0) {
                o0 = (p[1] + (double)cx) - (double)d;
                o1 = (p[2] + (double)cy) - (double)d;
                st = REF_FITTED;
            } else st = REF_KEPT_GATE;
        } else st = REF_KEPT_NOCONV;
    }
    if (lane == 0) {
        out[2 * atom] = o0;
        out[2 * atom + 1] = o1;
        status[atom] = st;
    }
}

// ---------------------------------------------------------------------------------------------- default half-side
#define NN_T 256

// First row of the (frame-sorted) table whose frame is >= f.
static __device__ __forceinline__ long nn_lower(const int* meta, long n, int f) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) / 2;
        if (meta[2 * mid] < f) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(NN_T) void nn2_kernel(const double* __restrict__ coords, const int* __restrict__ meta, long n,
                                                   int* __restrict__ dside) {
    __shared__ double s_r[NN_T], s_c[NN_T], s_sum[NN_T];
    const int tid = threadIdx.x, f = blockIdx.x;
    const long lo = nn_lower(meta, n, f), hi = nn_lower(meta, n, f + 1);
    const long cnt = hi - lo;
    double mine = 0.0;                               // this thread's atoms, in table order
    for (long base = lo; base < hi; base += NN_T) {  // (block-uniform bounds: every thread reaches the barriers)
        const long i = base + tid;
        const bool live = i < hi;
        const double ri = live ? coords[2 * i] : 0.0, ci = live ? coords[2 * i + 1] : 0.0;
        double m1 = INFINITY, m2 = INFINITY;         // the two smallest squared distances to OTHER atoms
        for (long tile = lo; tile < hi; tile += NN_T) {
            const long j = tile + tid;
            __syncthreads();
            s_r[tid] = j < hi ? coords[2 * j] : 0.0;
            s_c[tid] = j < hi ? coords[2 * j + 1] : 0.0;
            __syncthreads();
            const int m = (int)(hi - tile < NN_T ? hi - tile : NN_T);
            if (live) {
                for (int k = 0; k < m; ++k) {
                    if (tile + k == i) continue;
                    const double dr = s_r[k] - ri, dc = s_c[k] - ci;
                    const double q = dr * dr + dc * dc;
                    if (q < m1) { m2 = m1; m1 = q; } else if (q < m2) m2 = q;
                }
            }
        }
        if (live && cnt >= 3) mine += sqrt(m1) + sqrt(m2);
    }
    __syncthreads();
    s_sum[tid] = mine;
    __syncthreads();
    for (int w = NN_T / 2; w >= 1; w >>= 1) {        // fixed tree
        if (tid < w) s_sum[tid] += s_sum[tid + w];
        __syncthreads();
    }
    // int(np.mean(distances) * 0.25); fewer than 3 atoms have no two neighbours: 0, which the host refuses
    if (tid == 0) dside[f] = cnt >= 3 ? (int)(s_sum[0] / (double)(2 * cnt) * 0.25) : 0;
}

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" int amx_peak_refine(const float* frames, int B, int H, int W, const double* coords, const int* meta,
                               const int* d, int dmax, long n, double* out, int* status, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || n < 0) AMX_BADARG(1);
    if (dmax < 2 || dmax > REF_DMAX) AMX_BADARG(2);
    if (n == 0) return 0;
    if (!frames || !coords || !meta || !d || !out || !status) AMX_BADARG(3);
    const long blocks = (n + REF_WAVES - 1) / REF_WAVES;
    if (blocks >= 2147483647L) AMX_BADARG(4);
    const size_t lds = (size_t)REF_WAVES * 4 * dmax * dmax * sizeof(float);      // <= 64 KB
    AMX_LAUNCH(refine_kernel, dim3((unsigned)blocks), dim3(REF_WAVES * AMX_WAVE), lds, (hipStream_t)stream, frames, B, H,
               W, coords, meta, d, dmax, n, out, status);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_nn2_quarter_mean(const double* coords, const int* meta, long n, int B, int* d, void* stream) {
    if (B <= 0 || n < 0 || !d) AMX_BADARG(1);
    if (n > 0 && (!coords || !meta)) AMX_BADARG(2);
    AMX_LAUNCH(nn2_kernel, dim3((unsigned)B), dim3(NN_T), 0, (hipStream_t)stream, coords, meta, n, d);
    AMX_CHECK_LAUNCH();
    return 0;
}
