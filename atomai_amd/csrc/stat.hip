// stat.hip — Gaussian-mixture EM over a stack of flattened sub-images (atomai/stat/multivar.py:110-172: imlocal.gmm =
// sklearn.mixture.GaussianMixture, 'diag' / 'spherical'), k-means (its initialisation) and the column sums PCA needs.
//   gmm_pass_kernel      one workgroup per GMM_ROWS rows of X [N][D].  E phase: the rows are staged through LDS in
//                        GMM_SUB x GMM_DC tiles; thread (row = lane, components wave, wave + 4, ...) forms
//                        c_k - 1/2 sum_d (x_d - mu_kd)^2 prec_kd in the DIRECT difference form (the expanded form sklearn
//                        uses cancels badly in fp32 at D in the thousands), in fp64 from the fp32 operands: an fp32
//                        quadratic form is off by ~2^-23 of a sum in the thousands, and near a class boundary that error
//                        goes straight into the responsibilities (dr = r (1 - r) dlogp) and from there into every sum
//                        of the M step; the E phase is 3 flops per (row, component, column) against the column's 4
//                        bytes of HBM traffic per row.  Log-sum-exp, responsibilities and the arg-max label per row in
//                        fp64.  M phase: the same rows are read again (they are still in L2) and n_k, S1 = r^T (X - s),
//                        S2 = r^T (X - s)^2 are formed with v_mfma_f32_16x16x4_f32 — A = r^T [16 components][4 rows],
//                        B = [4 rows][16 columns] — over the workgroup's GMM_ROWS rows: no fp32 chain is longer than
//                        GMM_ROWS (<= 1024) terms.
//   gmm_reduce_kernel    adds the per-workgroup partial rows in workgroup order in fp64 (no float atomics anywhere: two
//                        runs give the same bits).
//   gmm_finalize_kernel  the M step in fp64 over [K][D] (sklearn/mixture/_gaussian_mixture.py:
//                        _estimate_gaussian_parameters): means, variances + reg_covar, precisions, weights, and the
//                        per-component constants of the next pass.
// The shift s (the data's column mean) keeps var = S2/n - (S1/n)^2 from being a difference of two large uncentred sums.
#include "amx_device.h"
#include <cfloat>
#include <cmath>

#define GMM_T 256                          // 4 waves
#define GMM_SUB 64                         // rows per tile = lanes of a wave
#define GMM_NSUB 1                         // row tiles per workgroup: 1 measured 1.13 ms per pass against 1.89 ms for 2
                                           // (20 000 x 3072, K = 10): twice the workgroups outweigh twice the partial rows
#define GMM_ROWS (GMM_SUB * GMM_NSUB)      // rows per workgroup = length of the fp32 MFMA chains
#define GMM_DC 64                          // columns per tile: 4 waves x 16 MFMA columns
#define GMM_KMAX 32
#define GMM_XLD (GMM_DC + 1)               // odd row strides: lanes that walk down a column hit different banks
#define GMM_RLD (GMM_KMAX + 1)
#define GMM_LDS_BYTES ((2 * GMM_KMAX * GMM_DC + GMM_ROWS) * 8 + (GMM_SUB * GMM_XLD + GMM_ROWS * GMM_RLD) * 4 + GMM_ROWS * 4)

// Stages rows [rbase, rbase + 64) x columns [d0, d0 + 64) of X (minus shift, if given) into Xs; zero outside the matrix.
static __device__ __forceinline__ void gmm_stage_x(const float* __restrict__ X, long N, int D, long rbase, int d0,
                                                   const float* __restrict__ shift, float* Xs) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, d = d0 + lane;
    const float s = (shift && d < D) ? shift[d] : 0.f;
    #pragma unroll 4
    for (int i = 0; i < GMM_SUB / 4; ++i) {
        const int r = w + 4 * i;
        const long gr = rbase + r;
        Xs[r * GMM_XLD + lane] = (gr < N && d < D) ? X[gr * D + d] - s : 0.f;
    }
}

// sum_d (x_d - mu_kd)^2 prec_kd over one staged tile for the NJ components wave, wave + 4, ... of this thread's row.
template <int NJ>
static __device__ __forceinline__ void gmm_quad(const float* xr, const double* Md, const double* Pd, int wave, double* acc) {
    #pragma unroll 2
    for (int d = 0; d < GMM_DC; ++d) {
        const double x = (double)xr[d];
        #pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int o = (wave + 4 * j) * GMM_DC + d;     // (wave-uniform address: an LDS broadcast)
            const double t = x - Md[o];
            acc[j] += t * t * Pd[o];
        }
    }
}

__global__ __launch_bounds__(GMM_T) void gmm_pass_kernel(const float* __restrict__ X, long N, int D, int K,
                                                         const float* __restrict__ mean, const float* __restrict__ prec,
                                                         const double* __restrict__ cst, const float* __restrict__ shift,
                                                         int hard, const int* __restrict__ prev, float* __restrict__ P1,
                                                         float* __restrict__ P2, double* __restrict__ Pn,
                                                         double* __restrict__ Pl, int* __restrict__ Pc,
                                                         double* __restrict__ logp, int* __restrict__ label) {
    AMX_DYN_SMEM(double, smem);
    double* Md = smem;                                         // [GMM_KMAX][GMM_DC] means of one tile of columns
    double* Pd = Md + GMM_KMAX * GMM_DC;                       // precisions
    double* Ls = Md;                                           // [GMM_KMAX][GMM_SUB] log-probabilities of one tile of rows:
                                                               // written when the tile's last column tile has been read
    double* lse_s = Pd + GMM_KMAX * GMM_DC;                    // [GMM_ROWS]
    float* Xs = reinterpret_cast<float*>(lse_s + GMM_ROWS);    // [GMM_SUB][GMM_XLD]
    float* Rs = Xs + GMM_SUB * GMM_XLD;                        // [GMM_ROWS][GMM_RLD] responsibilities
    int* chg = reinterpret_cast<int*>(Rs + GMM_ROWS * GMM_RLD);    // [GMM_ROWS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * GMM_ROWS;
    const int nj = (K + 3) >> 2;                               // components per wave, rows K .. 4 nj - 1 staged as zeros

    // ---------------------------------------------------------------- E phase
    for (int sb = 0; sb < GMM_NSUB; ++sb) {
        const long rbase = row0 + (long)sb * GMM_SUB;          // (block-uniform: every thread reaches the same barriers)
        double acc[GMM_KMAX / 4];
        #pragma unroll
        for (int j = 0; j < GMM_KMAX / 4; ++j) acc[j] = 0.0;
        if (rbase < N) {
            for (int d0 = 0; d0 < D; d0 += GMM_DC) {
                __syncthreads();
                gmm_stage_x(X, N, D, rbase, d0, nullptr, Xs);
                for (int i = tid; i < 4 * nj * GMM_DC; i += GMM_T) {
                    const int k = i / GMM_DC, d = d0 + (i % GMM_DC);
                    const bool in = k < K && d < D;            // zero precision: padding adds nothing
                    Md[i] = in ? (double)mean[(long)k * D + d] : 0.0;
                    Pd[i] = in ? (double)prec[(long)k * D + d] : 0.0;
                }
                __syncthreads();
                const float* xr = Xs + lane * GMM_XLD;
                switch (nj) {
                    case 1: gmm_quad<1>(xr, Md, Pd, wave, acc); break;
                    case 2: gmm_quad<2>(xr, Md, Pd, wave, acc); break;
                    case 3: gmm_quad<3>(xr, Md, Pd, wave, acc); break;
                    case 4: gmm_quad<4>(xr, Md, Pd, wave, acc); break;
                    case 5: gmm_quad<5>(xr, Md, Pd, wave, acc); break;
                    case 6: gmm_quad<6>(xr, Md, Pd, wave, acc); break;
                    case 7: gmm_quad<7>(xr, Md, Pd, wave, acc); break;
                    default: gmm_quad<8>(xr, Md, Pd, wave, acc); break;
                }
            }
        }
        __syncthreads();
        #pragma unroll
        for (int j = 0; j < GMM_KMAX / 4; ++j) {
            const int k = wave + 4 * j;
            if (k < K) Ls[k * GMM_SUB + lane] = cst[k] - 0.5 * acc[j];
        }
        __syncthreads();
        if (tid < GMM_SUB) {
            const long gr = rbase + tid;
            float* rr = Rs + (sb * GMM_SUB + tid) * GMM_RLD;
            double lse = 0.0;
            int changed = 0;
            if (gr < N) {
                int best = 0;
                double m = Ls[tid];
                for (int k = 1; k < K; ++k) {
                    const double v = Ls[k * GMM_SUB + tid];
                    if (v > m) { m = v; best = k; }
                }
                double s = 0.0;
                for (int k = 0; k < K; ++k) s += exp(Ls[k * GMM_SUB + tid] - m);
                lse = m + log(s);
                for (int k = 0; k < K; ++k) {
                    const double v = Ls[k * GMM_SUB + tid];
                    rr[k] = hard ? (k == best ? 1.f : 0.f) : (float)exp(v - lse);
                    if (logp) logp[gr * K + k] = v;
                }
                for (int k = K; k < GMM_KMAX; ++k) rr[k] = 0.f;
                if (label) label[gr] = best;
                if (prev) changed = prev[gr] != best;
            } else {
                for (int k = 0; k < GMM_KMAX; ++k) rr[k] = 0.f;
            }
            lse_s[sb * GMM_SUB + tid] = lse;
            chg[sb * GMM_SUB + tid] = changed;
        }
    }
    __syncthreads();
    if (tid < K) {                                             // n_k of this workgroup, of the fp32 values the MFMAs read
        double s = 0.0;
        for (int r = 0; r < GMM_ROWS; ++r) s += (double)Rs[r * GMM_RLD + tid];
        Pn[(long)blockIdx.x * K + tid] = s;
    }
    if (tid == GMM_SUB) {
        double s = 0.0;
        for (int r = 0; r < GMM_ROWS; ++r) s += lse_s[r];
        Pl[blockIdx.x] = s;
    }
    if (tid == 2 * GMM_SUB) {
        int c = 0;
        for (int r = 0; r < GMM_ROWS; ++r) c += chg[r];
        Pc[blockIdx.x] = c;
    }
    if (!P1) return;                                           // labels / log-probabilities only

    // ---------------------------------------------------------------- M phase
    const int p = lane & 15, g = lane >> 4, mtiles = (K + 15) >> 4;
    for (int d0 = 0; d0 < D; d0 += GMM_DC) {
        f32x4 a1[2], a2[2];
        #pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            a1[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            a2[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int sb = 0; sb < GMM_NSUB; ++sb) {
            const long rbase = row0 + (long)sb * GMM_SUB;
            if (rbase >= N) break;
            __syncthreads();
            gmm_stage_x(X, N, D, rbase, d0, shift, Xs);
            __syncthreads();
            #pragma unroll 4
            for (int s = 0; s < GMM_SUB / 4; ++s) {
                const int r = 4 * s + g;                       // A[i][k] sits in lane i + 16 k, B[k][j] in lane j + 16 k
                const float b = Xs[r * GMM_XLD + wave * 16 + p], b2 = b * b;
                const float* rr = Rs + (sb * GMM_SUB + r) * GMM_RLD + p;
                #pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    if (mt < mtiles) {
                        const float a = rr[mt * 16];
                        a1[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, a1[mt], 0, 0, 0);
                        a2[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b2, a2[mt], 0, 0, 0);
                    }
                }
            }
        }
        const int d = d0 + wave * 16 + p;                      // D fragment: column p, rows 4 g + reg
        #pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            #pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int k = mt * 16 + 4 * g + reg;
                if (k < K && d < D) {
                    const long o = ((long)blockIdx.x * K + k) * D + d;
                    P1[o] = a1[mt][reg];
                    P2[o] = a2[mt][reg];
                }
            }
        }
    }
}

// Adds the G partial rows of the pass in workgroup order, in fp64.
__global__ __launch_bounds__(GMM_T) void gmm_reduce_kernel(const float* __restrict__ P1, const float* __restrict__ P2,
                                                           const double* __restrict__ Pn, const double* __restrict__ Pl,
                                                           const int* __restrict__ Pc, long G, int K, int D,
                                                           double* __restrict__ S1, double* __restrict__ S2,
                                                           double* __restrict__ nk, double* __restrict__ lse_sum,
                                                           long* __restrict__ changed) {
    const long e = (long)blockIdx.x * GMM_T + threadIdx.x, KD = (long)K * D;
    if (e < KD && S1) {
        double s1 = 0.0, s2 = 0.0;
        for (long gi = 0; gi < G; ++gi) {
            s1 += (double)P1[gi * KD + e];
            s2 += (double)P2[gi * KD + e];
        }
        S1[e] = s1;
        S2[e] = s2;
    }
    if (e < K && nk) {
        double s = 0.0;
        for (long gi = 0; gi < G; ++gi) s += Pn[gi * K + e];
        nk[e] = s;
    }
    if (e == 0 && lse_sum) {
        double s = 0.0;
        for (long gi = 0; gi < G; ++gi) s += Pl[gi];
        *lse_sum = s;
    }
    if (e == 0 && changed) {
        long c = 0;
        for (long gi = 0; gi < G; ++gi) c += Pc[gi];
        *changed = c;
    }
}

static __device__ __forceinline__ double gmm_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = GMM_T / 2; w >= 1; w >>= 1) {                 // fixed tree
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// One workgroup per component.
__global__ __launch_bounds__(GMM_T) void gmm_finalize_kernel(const double* __restrict__ nk, const double* __restrict__ S1,
                                                             const double* __restrict__ S2, const float* __restrict__ shift,
                                                             int D, double N, double reg, int spherical,
                                                             double* __restrict__ mean, double* __restrict__ var,
                                                             double* __restrict__ prec, float* __restrict__ mean32,
                                                             float* __restrict__ prec32, double* __restrict__ weights,
                                                             double* __restrict__ cst) {
    __shared__ double red[GMM_T];
    const int k = blockIdx.x, tid = threadIdx.x;
    const double n = nk[k] + 10.0 * DBL_EPSILON;
    const double* s1 = S1 + (long)k * D;
    const double* s2 = S2 + (long)k * D;
    double vsph = 0.0;
    if (spherical) {
        double vs = 0.0;
        for (int d = tid; d < D; d += GMM_T) {
            const double m = s1[d] / n;
            vs += fmax(s2[d] / n - m * m, 0.0);
        }
        vsph = gmm_block_sum(vs, red) / (double)D + reg;
    }
    double ls = 0.0;
    for (int d = tid; d < D; d += GMM_T) {
        const double m = s1[d] / n;
        const double v = spherical ? vsph : fmax(s2[d] / n - m * m, 0.0) + reg;
        const double pr = 1.0 / v, mu = m + (double)shift[d];
        const float pf = (float)pr;
        const long o = (long)k * D + d;
        if (mean) { mean[o] = mu; var[o] = v; prec[o] = pr; }
        mean32[o] = (float)mu;
        prec32[o] = pf;
        ls += log((double)pf);                                 // of the value the next pass multiplies by
    }
    ls = gmm_block_sum(ls, red);
    if (tid == 0) {
        weights[k] = n / N;
        cst[k] = log(n / N) + 0.5 * ls - 0.5 * (double)D * log(2.0 * M_PI);
    }
}

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" long amx_gmm_rows(void) { return GMM_ROWS; }

extern "C" int amx_gmm_pass(const float* X, long N, int D, int K, const float* mean, const float* prec, const double* cst,
                            const float* shift, int hard, const int* prev_label, float* P1, float* P2, double* Pn,
                            double* Pl, int* Pc, double* logp, int* label, void* stream) {
    if (N <= 0 || D < 1) AMX_BADARG(1);
    if (K < 1 || K > GMM_KMAX) AMX_BADARG(2);
    if (!X || !mean || !prec || !cst || !Pn || !Pl || !Pc) AMX_BADARG(3);
    if ((P1 == nullptr) != (P2 == nullptr) || (P1 && !shift)) AMX_BADARG(4);
    const long G = (N + GMM_ROWS - 1) / GMM_ROWS;
    if (G >= 2147483647L) AMX_BADARG(5);
    AMX_ALLOW_160K_LDS(gmm_pass_kernel);
    AMX_LAUNCH(gmm_pass_kernel, dim3((unsigned)G), dim3(GMM_T), (size_t)GMM_LDS_BYTES, (hipStream_t)stream, X, N, D, K,
               mean, prec, cst, shift, hard, prev_label, P1, P2, Pn, Pl, Pc, logp, label);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_gmm_reduce(const float* P1, const float* P2, const double* Pn, const double* Pl, const int* Pc, long G,
                              int K, int D, double* S1, double* S2, double* nk, double* lse_sum, long* changed,
                              void* stream) {
    if (G <= 0 || K < 1 || K > GMM_KMAX || D < 1) AMX_BADARG(1);
    if (!Pn || !Pl || !Pc) AMX_BADARG(2);
    if ((S1 == nullptr) != (S2 == nullptr) || (S1 && (!P1 || !P2))) AMX_BADARG(3);
    const long blocks = ((long)K * D + GMM_T - 1) / GMM_T;
    AMX_LAUNCH(gmm_reduce_kernel, dim3((unsigned)blocks), dim3(GMM_T), 0, (hipStream_t)stream, P1, P2, Pn, Pl, Pc, G, K, D,
               S1, S2, nk, lse_sum, changed);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_gmm_finalize(const double* nk, const double* S1, const double* S2, const float* shift, int K, int D,
                                double N, double reg_covar, int spherical, double* mean, double* var, double* prec,
                                float* mean32, float* prec32, double* weights, double* cst, void* stream) {
    if (K < 1 || K > GMM_KMAX || D < 1 || !(N > 0.0)) AMX_BADARG(1);
    if (!nk || !S1 || !S2 || !shift || !mean32 || !prec32 || !weights || !cst) AMX_BADARG(2);
    if (mean && (!var || !prec)) AMX_BADARG(3);
    AMX_LAUNCH(gmm_finalize_kernel, dim3((unsigned)K), dim3(GMM_T), 0, (hipStream_t)stream, nk, S1, S2, shift, D, N,
               reg_covar, spherical, mean, var, prec, mean32, prec32, weights, cst);
    AMX_CHECK_LAUNCH();
    return 0;
}
