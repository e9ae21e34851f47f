// lattice.hip — training sets for the Segmentor, on the device: atom stamps rasterised into masks, windows gathered.
//
// Replaces the per-atom host loops of the reference's create_lattice_mask / create_multiclass_lattice_mask
// (atomai/utils/imgen.py:82-229: one slice assignment per atom per frame) and the two scikit-learn extract_patches_2d
// calls per frame behind extract_patches / the per-window copies of extract_random_subimages (atomai/utils/img.py:183-389).
// All frames of a call form ONE flat atom table and go through in one pair of launches:
//   lt_owner_kernel   one wave per table row, lanes over the m x m square of its stamp: which row owns a pixel.
//   lt_fill_kernel    one thread per pixel: the owners' stamp values into every channel, plus the background channel.
//   lt_crop_kernel    one workgroup per window: a bit copy of [ph][pw][C] elements of 4 or 8 bytes, and a flag.
// All three are bandwidth-bound passes: the stores of a wave are contiguous (a pixel's channels lie side by side, the
// pixels of a wave side by side along W); the crop moves 16 bytes per lane where the window's rows allow it.
//
// The rule (imgen.py:121-131, :210-229).  For row i of the table, in table order: x = rint(row coordinate),
// y = rint(column coordinate), half to even as numpy.around; its stamp is a square of odd side m; with r1 = (m + 1) / 2
// and r2 = (m - 1) / 2 (= int(m/2 + .5), int(m/2 - .5)) the assignment is mask[x-r1 : x+r2, y-r1 : y+r2, ch] = stamp: NOT
// centred (m = 5: rows x-3 .. x+1), and the whole square is assigned, zeros included, so on every pixel of a channel the
// LATEST row whose square covers it wins.  Channels do not interact.
//
// Determinism.  The only atomic is atomicMin on int32: owner = min over the covering rows of -(i + 1), 0 where none;
// `bad` = the smallest refused row.  Both are minima over a fixed set, whatever the order of execution.  No float
// atomics; one writer per output element: two runs give the same bits.
//
// Safety.  lt_square takes every guard before the first store: a non-finite coordinate, a frame, channel or stamp id out
// of range, an even side or one above LT_MAXSIDE, a square that leaves its frame.  Such a row writes nothing and
// records itself in `bad`; no table can make the kernels write outside `owner` / `out`, and lt_fill_kernel repeats
// the guards (and tests the stamp offsets) before it reads a stamp.
#include "amx_device.h"

#define LT_T 256
#define LT_MAXSIDE 63
#define LT_MAXBLOCKS 8192                                   // grid-stride beyond this many workgroups

// the square of table row i: top-left corner (x0, y0), side m, frame f, channel c, stamp sid; false = refused
static __device__ __forceinline__ bool lt_square(const double* __restrict__ xy, const int* __restrict__ meta,
                                                 const int* __restrict__ sside, long i, int K, int F, int H, int W, int C,
                                                 int& f, int& c, int& sid, int& m, int& x0, int& y0) {
    f = meta[3 * i];
    c = meta[3 * i + 1];
    sid = meta[3 * i + 2];
    if (f < 0 || f >= F || c < 0 || c >= C || sid < 0 || sid >= K) return false;
    m = sside[sid];
    if (m < 1 || m > LT_MAXSIDE || (m & 1) == 0) return false;
    const double x = xy[2 * i], y = xy[2 * i + 1];
    if (!(fabs(x) < INFINITY) || !(fabs(y) < INFINITY)) return false;       // (false for NaN too)
    const double rx = rint(x), ry = rint(y);
    const int r1 = (m + 1) / 2, r2 = (m - 1) / 2;
    if (!(rx - (double)r1 >= 0.0) || !(rx + (double)r2 <= (double)H)) return false;
    if (!(ry - (double)r1 >= 0.0) || !(ry + (double)r2 <= (double)W)) return false;
    x0 = (int)rx - r1;                                      // (r1 <= rx <= H: the conversions are exact)
    y0 = (int)ry - r1;
    return true;
}

__global__ __launch_bounds__(LT_T) void lt_owner_kernel(const double* __restrict__ xy, const int* __restrict__ meta, long N,
                                                        const int* __restrict__ sside, int K, int F, int H, int W, int C,
                                                        int* owner, int* bad) {
    const int lane = threadIdx.x & (AMX_WAVE - 1);
    const long i = (long)blockIdx.x * (LT_T / AMX_WAVE) + (threadIdx.x / AMX_WAVE);
    if (i >= N) return;
    int f, c, sid, m, x0, y0;
    if (!lt_square(xy, meta, sside, i, K, F, H, W, C, f, c, sid, m, x0, y0)) {
        if (lane == 0) atomicMin(bad, (int)i);
        return;
    }
    const int key = -(int)(i + 1);
    for (int e = lane; e < m * m; e += AMX_WAVE) {
        const int a = e / m, b = e - a * m;                 // 0 <= x0 + a < H, 0 <= y0 + b < W by lt_square
        atomicMin(&owner[(((long)f * H + (x0 + a)) * W + (y0 + b)) * C + c], key);
    }
}

// value of owner key k < 0 at pixel (f, p, q), channel c; 0 for a key that does not name a row covering the pixel
static __device__ __forceinline__ double lt_value(int k, const double* __restrict__ xy, const int* __restrict__ meta, long N,
                                                  const int* __restrict__ sside, const long* __restrict__ soff, int K,
                                                  const double* __restrict__ stamps, long S, int F, int H, int W, int C,
                                                  int f, int p, int q, int c) {
    const long i = -(long)k - 1;
    if (i < 0 || i >= N) return 0.0;
    int fi, ci, sid, m, x0, y0;
    if (!lt_square(xy, meta, sside, i, K, F, H, W, C, fi, ci, sid, m, x0, y0)) return 0.0;
    const int a = p - x0, b = q - y0;
    if (fi != f || ci != c || a < 0 || a >= m || b < 0 || b >= m) return 0.0;
    const long off = soff[sid];
    if (off < 0 || off + (long)m * m > S) return 0.0;
    return stamps[off + (long)a * m + b];
}

// out [F][H][W][CO], CO = C + background.  background = 0: channel c = the stamp value (0 where no row owns the pixel).
// background = 1, n = nch[f]: channels c < n as above, s = their sum added in the order c = 0, 1, ... in fp64, channel n =
// 1 - s, channels above n = 0; then every value < 0 becomes 0 (the reference clamps the class channels as well as the
// background, after the sum).
template <typename T>
__global__ __launch_bounds__(LT_T) void lt_fill_kernel(const int* __restrict__ owner, const double* __restrict__ xy,
                                                       const int* __restrict__ meta, long N, const int* __restrict__ sside,
                                                       const long* __restrict__ soff, int K,
                                                       const double* __restrict__ stamps, long S,
                                                       const int* __restrict__ nch, int F, int H, int W, int C,
                                                       int background, T* __restrict__ out) {
    const long HW = (long)H * W, npix = HW * F;
    const int CO = C + (background ? 1 : 0);
    for (long pix = (long)blockIdx.x * LT_T + threadIdx.x; pix < npix; pix += (long)gridDim.x * LT_T) {
        const int f = (int)(pix / HW);
        const long rem = pix - (long)f * HW;
        const int p = (int)(rem / W), q = (int)(rem - (long)p * W);
        int n = C;
        if (background) {
            n = nch[f];
            n = n < 0 ? 0 : (n > C ? C : n);
        }
        const int* __restrict__ ow = owner + pix * C;
        T* __restrict__ o = out + pix * CO;
        double s = 0.0;
        for (int c = 0; c < CO; ++c) {
            double v = 0.0;
            if (c < n) {
                const int k = ow[c];
                if (k < 0) v = lt_value(k, xy, meta, N, sside, soff, K, stamps, S, F, H, W, C, f, p, q, c);
                s = s + v;
            } else if (c == n) {                            // (only with background: n <= C < CO)
                v = 1.0 - s;
            }
            if (background && v < 0.0) v = 0.0;
            o[c] = (T)v;
        }
    }
}

// 1 if the 16 bytes hold a NaN of the element type
static __device__ __forceinline__ int lt_nan4(unsigned u) { return (u & 0x7fffffffu) > 0x7f800000u ? 1 : 0; }
static __device__ __forceinline__ int lt_nan8(unsigned lo, unsigned hi) {
    const unsigned h = hi & 0x7fffffffu;
    return (h > 0x7ff00000u || (h == 0x7ff00000u && lo != 0u)) ? 1 : 0;
}
template <typename E> static __device__ __forceinline__ int lt_nan_elem(E v);
template <> __device__ __forceinline__ int lt_nan_elem<unsigned>(unsigned v) { return lt_nan4(v); }
template <> __device__ __forceinline__ int lt_nan_elem<unsigned long long>(unsigned long long v) {
    return lt_nan8((unsigned)v, (unsigned)(v >> 32));
}
template <typename E> static __device__ __forceinline__ int lt_nan_vec(uint4 v);
template <> __device__ __forceinline__ int lt_nan_vec<unsigned>(uint4 v) {
    return lt_nan4(v.x) | lt_nan4(v.y) | lt_nan4(v.z) | lt_nan4(v.w);
}
template <> __device__ __forceinline__ int lt_nan_vec<unsigned long long>(uint4 v) {
    return lt_nan8(v.x, v.y) | lt_nan8(v.z, v.w);
}

// One workgroup per window.  A window row is pw * C contiguous elements of src and of dst.  Where the row length, the
// frame's row pitch and the window's first element are all multiples of 16 bytes the copy moves 16 bytes per lane,
// otherwise one element per lane; both walk the window as one flat range, so a wave's loads are contiguous within a
// window row and its stores contiguous throughout.
template <typename E>
__global__ __launch_bounds__(LT_T) void lt_crop_kernel(const E* __restrict__ src, const int* __restrict__ win, int F, int H,
                                                       int W, int C, int ph, int pw, int is_float, E* __restrict__ dst,
                                                       int* __restrict__ flag) {
    __shared__ int s_nan[LT_T];
    const int tid = threadIdx.x;
    const long w = blockIdx.x;
    const int f = win[3 * w], r0 = win[3 * w + 1], c0 = win[3 * w + 2];
    if (f < 0 || f >= F || r0 < 0 || c0 < 0 || (long)r0 + ph > H || (long)c0 + pw > W) {     // (uniform over the workgroup)
        if (tid == 0) flag[w] = -1;
        return;
    }
    constexpr int V = 16 / (int)sizeof(E);
    const long rowlen = (long)pw * C, pitch = (long)W * C, total = rowlen * ph;
    const long first = (((long)f * H + r0) * W + c0) * C;
    const E* __restrict__ s0 = src + first;
    E* __restrict__ d0 = dst + w * total;
    int nan = 0;
    const bool vec = rowlen % V == 0 && pitch % V == 0 && first % V == 0 &&
                     (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    if (vec) {
        const long rv = rowlen / V, tv = rv * ph;
        for (long e = tid; e < tv; e += LT_T) {
            const long r = e / rv, t = e - r * rv;
            const uint4 v = *reinterpret_cast<const uint4*>(s0 + r * pitch + t * V);
            *reinterpret_cast<uint4*>(d0 + e * V) = v;
            if (is_float) nan |= lt_nan_vec<E>(v);
        }
    } else {
        for (long e = tid; e < total; e += LT_T) {
            const long r = e / rowlen, t = e - r * rowlen;
            const E v = s0[r * pitch + t];
            d0[e] = v;
            if (is_float) nan |= lt_nan_elem<E>(v);
        }
    }
    s_nan[tid] = nan;
    __syncthreads();
    for (int h = LT_T / 2; h >= 1; h >>= 1) {
        if (tid < h) s_nan[tid] = s_nan[tid] | s_nan[tid + h];
        __syncthreads();
    }
    if (tid == 0) flag[w] = s_nan[0];
}

// ---------------------------------------------------------------------------------------------- C ABI
#define LT_MAXN 2147483647L

extern "C" int amx_lattice_max_side(void) { return LT_MAXSIDE; }

extern "C" int amx_lattice_owner(const double* xy, const int* meta, long N, const int* sside, int K, int F, int H, int W,
                                 int C, int* owner, int* bad, void* stream) {
    if (N < 0 || N >= LT_MAXN || K < 0 || F < 1 || H < 1 || W < 1 || C < 1) AMX_BADARG(1);
    if (!owner || !bad) AMX_BADARG(2);
    if (N == 0) return 0;
    if (!xy || !meta || (K > 0 && !sside)) AMX_BADARG(3);
    const long per = LT_T / AMX_WAVE;
    AMX_LAUNCH(lt_owner_kernel, dim3((unsigned)((N + per - 1) / per)), dim3(LT_T), 0, (hipStream_t)stream, xy, meta, N, sside,
               K, F, H, W, C, owner, bad);
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_lattice_fill(const int* owner, const double* xy, const int* meta, long N, const int* sside,
                                const long* soff, int K, const double* stamps, long S, const int* nch, int F, int H, int W,
                                int C, int background, void* out, int out_f64, void* stream) {
    if (N < 0 || N >= LT_MAXN || K < 0 || S < 0 || F < 1 || H < 1 || W < 1 || C < 1) AMX_BADARG(1);
    if (!owner || !out || (background && !nch)) AMX_BADARG(2);
    if (N > 0 && (!xy || !meta || !sside || !soff || !stamps)) AMX_BADARG(3);
    const long npix = (long)F * H * W;
    long G = (npix + LT_T - 1) / LT_T;
    G = G > LT_MAXBLOCKS ? LT_MAXBLOCKS : G;
    if (out_f64) {
        AMX_LAUNCH(lt_fill_kernel<double>, dim3((unsigned)G), dim3(LT_T), 0, (hipStream_t)stream, owner, xy, meta, N, sside,
                   soff, K, stamps, S, nch, F, H, W, C, background, (double*)out);
    } else {
        AMX_LAUNCH(lt_fill_kernel<float>, dim3((unsigned)G), dim3(LT_T), 0, (hipStream_t)stream, owner, xy, meta, N, sside,
                   soff, K, stamps, S, nch, F, H, W, C, background, (float*)out);
    }
    AMX_CHECK_LAUNCH();
    return 0;
}

extern "C" int amx_crop_windows(const void* src, int esize, int is_float, int F, int H, int W, int C, const int* win, long P,
                                int ph, int pw, void* dst, int* flag, void* stream) {
    if ((esize != 4 && esize != 8) || F < 1 || H < 1 || W < 1 || C < 1 || ph < 1 || pw < 1) AMX_BADARG(1);
    if (P < 0 || P >= LT_MAXN) AMX_BADARG(2);
    if (P == 0) return 0;
    if (!src || !win || !dst || !flag) AMX_BADARG(3);
    if (esize == 4) {
        AMX_LAUNCH(lt_crop_kernel<unsigned>, dim3((unsigned)P), dim3(LT_T), 0, (hipStream_t)stream, (const unsigned*)src, win,
                   F, H, W, C, ph, pw, is_float, (unsigned*)dst, flag);
    } else {
        AMX_LAUNCH(lt_crop_kernel<unsigned long long>, dim3((unsigned)P), dim3(LT_T), 0, (hipStream_t)stream,
                   (const unsigned long long*)src, win, F, H, W, C, ph, pw, is_float, (unsigned long long*)dst, flag);
    }
    AMX_CHECK_LAUNCH();
    return 0;
}
