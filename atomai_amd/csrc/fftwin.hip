// fftwin.hip — the front end of SlidingFFTNMF (atomai/stat/fft_nmf.py:154-216, process_fft): per window an optional
// Hamming table, fft2, fftshift, abs, log1p, a centre crop and scipy.ndimage.zoom(order=1).
//
// Only the cropped frequencies are ever looked at, so the kernel evaluates exactly those by a direct DFT in two passes
// instead of a full transform: shifted index s is frequency (s - N/2) mod N (integer division), and
//     B[x][v] = sum_y a[x][y] e^(-2 pi i fy(v) y / wy)              rows,    wx x ncy complex
//     A[u][v] = sum_x B[x][v] e^(-2 pi i fx(u) x / wx)              columns, ncx x ncy complex
// with the twiddles from fp64 tables built on the host as cos / sin of 2 pi ((f m) mod N) / N (the index is carried
// incrementally, so the argument is always reduced exactly).  Then mag = log1p(|A|) and the separable linear zoom from
// host-built tables (index pair and weights per output row / column; an output whose source coordinate falls outside
// the crop is 0, which is scipy's mode='constant').  One workgroup per window writes one fp64 row of the feature matrix
// and one flag word (bit 0: some output is non-zero, bit 1: some output is not finite) for the reference's ValueError.
//
// Window origins come from (base, two strides, two steps): pixel (x, y) of window (a, b) is
// img[base + (a step0 + x) stride0 + (b step1 + y) stride1], so the same kernel reads overlapping windows straight from
// the normalised image (strides (W, 1), steps (sx, sy)) or a materialised (n, wx, wy) stack (strides (wy, 1), steps
// (wx, 0), one window per grid row).
//
// LDS budget at 128 x 128 with the full crop (zoom_factor 1: ncx = ncy = 128), the worst case:
//     mag    ncx ncy fp64            128 * 128 * 8       = 131072 B
//     B      wx FW_VT complex fp64   128 * 8 * 16        =  16384 B   (the columns are done FW_VT frequencies at a time)
//     tables cos, sin for both axes  2 * (128 + 128) * 8 =   4096 B
//     flags  one int per thread      256 * 4             =   1024 B
//                                                          152576 B = 149 KB of the 160 KB of a compute unit.
// The window itself is not staged: lanes of a wave share x (the frequency index runs fastest), so its reads are
// broadcasts out of L1/L2, and staging 128 KB more would not fit.  With the defaults (zoom_factor 2) mag is 32 KB and
// three workgroups share a compute unit.  Everything is fp64; every output has one writer.
#include "amx_device.h"

#define FW_T 256
#define FW_VT 8
#define FW_MAX 128

struct FwArgs {
    const double* img;
    long base, stride0, stride1, step0, step1, nw1;
    int wx, wy, x_min, ncx, y_min, ncy, nox, noy;
    const double* ham;                 // [wx][wy] or NULL
    const double *cx, *sx, *cy, *sy;   // twiddle tables [wx], [wx], [wy], [wy]
    const int *zx0, *zx1, *zy0, *zy1;  // zoom tables [nox], [nox], [noy], [noy]; zx0 < 0: outside
    const double *zxa, *zxb, *zya, *zyb;
    double* out;                       // [n][nox * noy]
    int* flags;                        // [n]
};

__global__ __launch_bounds__(FW_T) void fftwin_kernel(FwArgs A) {
    AMX_DYN_SMEM(double, smem);
    double* s_mag = smem;                                   // [ncx][ncy]
    double* s_b = s_mag + (long)A.ncx * A.ncy;              // [wx][FW_VT][2]
    double* s_cx = s_b + (long)A.wx * FW_VT * 2;
    double* s_sx = s_cx + A.wx;
    double* s_cy = s_sx + A.wx;
    double* s_sy = s_cy + A.wy;
    int* s_flag = reinterpret_cast<int*>(s_sy + A.wy);      // [FW_T]
    const int tid = threadIdx.x;
    const long w = blockIdx.x;
    const long origin = A.base + (w / A.nw1) * A.step0 * A.stride0 + (w % A.nw1) * A.step1 * A.stride1;
    for (int m = tid; m < A.wx; m += FW_T) { s_cx[m] = A.cx[m]; s_sx[m] = A.sx[m]; }
    for (int m = tid; m < A.wy; m += FW_T) { s_cy[m] = A.cy[m]; s_sy[m] = A.sy[m]; }
    __syncthreads();
    for (int v0 = 0; v0 < A.ncy; v0 += FW_VT) {
        const int vt = A.ncy - v0 < FW_VT ? A.ncy - v0 : FW_VT;
        for (int item = tid; item < A.wx * vt; item += FW_T) {            // rows: B[x][v0 + vi]
            const int x = item / vt, vi = item % vt;
            const int fy = ((A.y_min + v0 + vi - A.wy / 2) % A.wy + A.wy) % A.wy;
            const double* row = A.img + origin + (long)x * A.stride0;
            double re = 0.0, im = 0.0;
            int idx = 0;
            for (int y = 0; y < A.wy; ++y) {
                double a = row[(long)y * A.stride1];
                if (A.ham) a *= A.ham[x * A.wy + y];
                re += a * s_cy[idx];
                im -= a * s_sy[idx];
                idx += fy;
                idx -= idx >= A.wy ? A.wy : 0;
            }
            s_b[(x * FW_VT + vi) * 2] = re;
            s_b[(x * FW_VT + vi) * 2 + 1] = im;
        }
        __syncthreads();
        for (int item = tid; item < A.ncx * vt; item += FW_T) {           // columns: A[u][v0 + vi]
            const int u = item / vt, vi = item % vt;
            const int fx = ((A.x_min + u - A.wx / 2) % A.wx + A.wx) % A.wx;
            double re = 0.0, im = 0.0;
            int idx = 0;
            for (int x = 0; x < A.wx; ++x) {
                const double br = s_b[(x * FW_VT + vi) * 2], bi = s_b[(x * FW_VT + vi) * 2 + 1];
                const double c = s_cx[idx], s = s_sx[idx];
                re += br * c + bi * s;
                im += bi * c - br * s;
                idx += fx;
                idx -= idx >= A.wx ? A.wx : 0;
            }
            s_mag[u * A.ncy + v0 + vi] = log1p(hypot(re, im));
        }
        __syncthreads();
    }
    int flag = 0;
    const int nout = A.nox * A.noy;
    for (int o = tid; o < nout; o += FW_T) {
        const int ox = o / A.noy, oy = o % A.noy;
        const int i0 = A.zx0[ox], i1 = A.zx1[ox], j0 = A.zy0[oy], j1 = A.zy1[oy];
        double v = 0.0;
        const bool inside = i0 >= 0 && i0 < A.ncx && i1 >= 0 && i1 < A.ncx && j0 >= 0 && j0 < A.ncy && j1 >= 0 && j1 < A.ncy;
        if (inside) {                                                     // scipy's order: axis 0 outer, axis 1 inner
            const double xa = A.zxa[ox], xb = A.zxb[ox], ya = A.zya[oy], yb = A.zyb[oy];
            v += s_mag[i0 * A.ncy + j0] * xa * ya;
            v += s_mag[i0 * A.ncy + j1] * xa * yb;
            v += s_mag[i1 * A.ncy + j0] * xb * ya;
            v += s_mag[i1 * A.ncy + j1] * xb * yb;
        }
        A.out[w * nout + o] = v;
        flag |= (v != 0.0 ? 1 : 0) | ((v - v == 0.0) ? 0 : 2);             // (v - v is NaN for an infinite or NaN v)
    }
    s_flag[tid] = flag;
    __syncthreads();
    if (tid == 0) {
        int f = 0;
        for (int m = 0; m < FW_T; ++m) f |= s_flag[m];
        A.flags[w] = f;
    }
}

extern "C" int amx_fftwin(const double* img, long len, long base, long stride0, long stride1, long step0, long step1,
                          long nw0, long nw1, int wx, int wy, const double* ham, const double* cx, const double* sx,
                          const double* cy, const double* sy, int x_min, int ncx, int y_min, int ncy, const int* zx0,
                          const int* zx1, const double* zxa, const double* zxb, int nox, const int* zy0, const int* zy1,
                          const double* zya, const double* zyb, int noy, double* out, int* flags, void* stream) {
    if (wx < 1 || wy < 1 || wx > FW_MAX || wy > FW_MAX) AMX_BADARG(1);
    if (nw0 < 1 || nw1 < 1 || nw0 * nw1 >= 2147483647L || base < 0 || stride0 < 0 || stride1 < 0 || step0 < 0 || step1 < 0)
        AMX_BADARG(2);
    if (x_min < 0 || ncx < 1 || x_min + ncx > wx || y_min < 0 || ncy < 1 || y_min + ncy > wy) AMX_BADARG(3);
    if (nox < 1 || noy < 1 || (long)nox * noy >= 2147483647L) AMX_BADARG(4);
    // the last pixel the kernel can read must lie inside the buffer
    const long last = base + ((nw0 - 1) * step0 + wx - 1) * stride0 + ((nw1 - 1) * step1 + wy - 1) * stride1;
    if (len < 1 || last >= len) AMX_BADARG(5);
    if (!img || !cx || !sx || !cy || !sy || !zx0 || !zx1 || !zxa || !zxb || !zy0 || !zy1 || !zya || !zyb || !out || !flags)
        AMX_BADARG(6);
    FwArgs A;
    A.img = img; A.base = base; A.stride0 = stride0; A.stride1 = stride1; A.step0 = step0; A.step1 = step1; A.nw1 = nw1;
    A.wx = wx; A.wy = wy; A.x_min = x_min; A.ncx = ncx; A.y_min = y_min; A.ncy = ncy; A.nox = nox; A.noy = noy;
    A.ham = ham; A.cx = cx; A.sx = sx; A.cy = cy; A.sy = sy;
    A.zx0 = zx0; A.zx1 = zx1; A.zy0 = zy0; A.zy1 = zy1; A.zxa = zxa; A.zxb = zxb; A.zya = zya; A.zyb = zyb;
    A.out = out; A.flags = flags;
    const size_t lds = ((size_t)ncx * ncy + (size_t)wx * FW_VT * 2 + 2 * (size_t)(wx + wy)) * sizeof(double)
                       + FW_T * sizeof(int);
    AMX_ALLOW_160K_LDS(fftwin_kernel);
    AMX_LAUNCH(fftwin_kernel, dim3((unsigned)(nw0 * nw1)), dim3(FW_T), lds, (hipStream_t)stream, A);
    AMX_CHECK_LAUNCH();
    return 0;
}
