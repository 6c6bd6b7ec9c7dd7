// Spline zoom and the pointwise tail of the inference product (include/gandanet.h, "spline zoom"): scipy.ndimage.zoom at
// orders 0, 1 and 3 along one axis of a dense tensor seen as (outer, L, inner), the cubic B-spline prefilter behind order
// 3, and ((x + trend) * scale + mean) * unit with a mask.  Storage fp32 or fp64; all arithmetic is fp64 and a result is
// rounded to its storage type once.  No atomics; all index arithmetic is 64-bit.
//
// Order 3 is two kernels through the caller's workspace: the prefilter writes the fp64 coefficients (of the line padded
// by 12 edge samples either way in 'nearest' mode), the interpolation kernel reads four of them per output.  The
// prefilter's recursion runs along a line, so a line is cut into chunks and every chunk is warm-started: |z| = 0.268, so
// SP_H = 40 samples of look-back (look-ahead for the anticausal pass) leave z^40 = 1.3e-23 of the unknown state.  The
// exact boundary sums apply where a chunk's horizon reaches the end of the line.
// From elem_util.h: gd_stream_grid, gd_dtype_ok, gd_elem_aligned, gd_aligned, GD_S.
#include "elem_util.h"

#include <math.h>

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_H = 40;        // warm-start horizon of a chunk, in samples
constexpr int SP_SUM = 64;      // terms kept of the boundary sum: z^65 = 7e-38
constexpr int SP_REFL = 96;     // the far end's terms of the boundary sum (z^(n-1) and smaller) are kept up to this length
constexpr int SP_PAD = 12;      // scipy's edge padding in front of the prefilter in 'nearest' mode
constexpr int SP_CHUNK = 64;    // inner > 1: samples of a line per thread
constexpr int SP_CR = 9;        // inner == 1: samples per thread; odd, so lanes 9 doubles apart meet no LDS bank twice
constexpr int SP_CPS = SP_THREADS;                 // inner == 1: chunks of one row segment at most
constexpr int SP_OCAP = SP_THREADS * SP_CR;        // doubles of the coefficient tile
constexpr int SP_XCAP = 3072;                      // doubles of the sample tile: >= SP_CPS * SP_CR + 2 * SP_H + 2

constexpr double SP_Z = -0.26794919243112281;      // sqrt(3) - 2 in fp64, the pole of the cubic B-spline
constexpr double SP_GAIN = (1.0 - SP_Z) * (1.0 - 1.0 / SP_Z);

// the last coefficient of a line from the causal values at n - 1 and n - 2
__device__ __forceinline__ double anticausal_init(double cp, double prev, bool reflect) {
    return reflect ? cp * (SP_Z / (SP_Z - 1.0)) : (SP_Z * prev + cp) * (SP_Z / (SP_Z * SP_Z - 1.0));
}

// the first causal value of a line of n >= 2 samples.  X(i) is sample i.  The sum runs over the whole line in scipy; its
// terms fall like z^i, so SP_SUM of them are kept, and the far end's share (z^(n-1) c[n-1-i]) only on short lines.
template <typename GetX>
__device__ __forceinline__ double causal_init(long n, bool reflect, GetX X) {
    const bool far = n <= SP_REFL;
    const long e = reflect ? n : n - 1;          // the far end enters with z^e; the sum runs to i = e - 1
    double ze = 0.0;
    if (far) {
        ze = 1.0;
        for (long k = 0; k < e; ++k) ze *= SP_Z;
    }
    const double c0 = SP_GAIN * X(0);
    double sum = c0 + (far ? ze * (SP_GAIN * X(n - 1)) : 0.0);
    const long last = e - 1 < SP_SUM ? e - 1 : SP_SUM;
    double zi = SP_Z;
    for (long i = 1; i <= last; ++i) {
        double t = SP_GAIN * X(i);
        if (far) t += ze * (SP_GAIN * X(n - 1 - i));
        sum += zi * t;
        zi *= SP_Z;
    }
    if (reflect) return c0 + sum * (SP_Z / (1.0 - ze * ze));
    return sum / (1.0 - ze * ze);
}

// Coefficients [a, b) of a line of n samples (0 <= a < b <= n).  X(i): sample i, any i in [max(0, a - SP_H),
// min(n, b + SP_H + 1)) and, where a <= SP_H, what causal_init reads.  put(i, v) / get(i): the caller's storage for
// position i in [a, b); get returns what this thread put.
//   causal      c+[i] = gain x[i] + z c+[i-1], started SP_H samples early from gain x[s], or exactly at s = 0
//   anticausal  c[i] = z (c[i+1] - c+[i]).  Its start c[b] = -z sum_{j < m} z^j c+[b+j] + z^m c[b+m] comes from running
//               the causal pass m = min(SP_H, n - 1 - b) samples on, without storing them: the last term is the exact
//               end condition where b + m reaches n - 1 and is dropped (z^40) elsewhere.
template <typename GetX, typename Put, typename Get>
__device__ __forceinline__ void prefilter_chunk(long a, long b, long n, bool reflect, GetX X, Put put, Get get) {
    if (n == 1) {
        put(0, X(0));
        return;
    }
    long s = a - SP_H;
    double cp;
    if (s <= 0) {
        s = 0;
        cp = causal_init(n, reflect, X);
    } else {
        cp = SP_GAIN * X(s);
    }
    if (s >= a) put(s, cp);
    double prev = cp;
    for (long i = s + 1; i < b; ++i) {
        prev = cp;
        cp = SP_GAIN * X(i) + SP_Z * cp;
        if (i >= a) put(i, cp);
    }
    double cm;
    long e;
    if (b == n) {
        e = n - 1;
        cm = anticausal_init(cp, prev, reflect);
        put(e, cm);
    } else {
        e = b;
        const long m = n - 1 - b < SP_H ? n - 1 - b : SP_H;
        double acc = 0.0, zj = 1.0;
        for (long j = 0; j < m; ++j) {
            prev = cp;
            cp = SP_GAIN * X(b + j) + SP_Z * cp;
            acc += zj * cp;
            zj *= SP_Z;
        }
        cm = -SP_Z * acc;
        if (b + m == n - 1) {
            prev = cp;
            cp = SP_GAIN * X(n - 1) + SP_Z * cp;
            cm += zj * anticausal_init(cp, prev, reflect);
        }
    }
    for (long i = e - 1; i >= a; --i) {
        cm = SP_Z * (cm - get(i));
        put(i, cm);
    }
}

// a product and a sum that each round on their own: hipcc contracts a * b + c into one FMA unless told otherwise (HIP's
// *_rn intrinsics are plain operators and contract too), and scipy and numpy round twice
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

__device__ __forceinline__ long clampl(long q, long hi) { return q < 0 ? 0 : (q > hi ? hi : q); }

// ---- prefilter, inner > 1: lanes along `inner`, one thread per (line, chunk of SP_CHUNK samples) ----------------------
// The thread walks its chunk in global memory: the causal values go to dst and come back (the thread's own stores) on
// the way down.  A wave's 64 lanes read and write 64 consecutive elements of one row at every step.
template <typename T>
__global__ __launch_bounds__(SP_THREADS) void prefilter_inner_kernel(const T* __restrict__ src, double* dst, long nsrc, long n,
                                                                     long inner, long nchunks, long items, long pad,
                                                                     int reflect) {
    for (long it = (long)blockIdx.x * SP_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * SP_THREADS) {
        const long col = it % inner;
        const long t = it / inner;
        const long ch = t % nchunks, o = t / nchunks;
        const T* s = src + o * nsrc * inner + col;
        double* d = dst + o * n * inner + col;
        const long a = ch * SP_CHUNK, b = a + SP_CHUNK < n ? a + SP_CHUNK : n;
        prefilter_chunk(
            a, b, n, reflect != 0, [&](long i) { return (double)s[clampl(i - pad, nsrc - 1) * inner]; },
            [&](long i, double v) { d[i * inner] = v; }, [&](long i) { return d[i * inner]; });
    }
}

// ---- prefilter, inner == 1: lanes along the line, rows staged in LDS ---------------------------------------------------
// One workgroup takes `rt` rows x one segment of cps * SP_CR samples.  The segment and SP_H samples on either side (one
// more at the far end, for the end condition) are staged as fp64 with consecutive lanes on consecutive elements; thread
// (r, c) then computes the SP_CR coefficients of chunk c of row r from the staged samples into a second tile, and the
// tile is written out with consecutive lanes on consecutive elements again.  Lanes of one row are SP_CR = 9 doubles
// apart in both tiles: 18 dwords, every even bank once per 32 lanes, so ds_read_b64 / ds_write_b64 meet no conflict;
// rows are `ws` (odd) doubles apart.
template <typename T>
__global__ __launch_bounds__(SP_THREADS) void prefilter_row_kernel(const T* __restrict__ src, double* __restrict__ dst,
                                                                   long outer, long nsrc, long n, long pad, int reflect,
                                                                   int cps, int rt, int ws, long sb0) {
    __shared__ double xs[SP_XCAP];
    __shared__ double cs[SP_OCAP];
    const int tid = threadIdx.x;
    const long seg = (long)cps * SP_CR;
    const long row0 = (long)blockIdx.x * rt, seg0 = (sb0 + blockIdx.y) * seg;
    const int rows = (int)(outer - row0 < rt ? outer - row0 : rt);
    const long w0 = seg0 - SP_H > 0 ? seg0 - SP_H : 0;
    const long w1 = seg0 + seg + SP_H + 1 < n ? seg0 + seg + SP_H + 1 : n;
    const int width = (int)(w1 - w0);
    for (int idx = tid; idx < rows * width; idx += SP_THREADS) {
        const int r = idx / width, j = idx - r * width;
        xs[r * ws + j] = (double)src[(row0 + r) * nsrc + clampl(w0 + j - pad, nsrc - 1)];
    }
    __syncthreads();
    const int r = tid / cps, c = tid - r * cps;
    const long a = seg0 + (long)c * SP_CR;
    if (r < rows && a < n) {
        const long b = a + SP_CR < n ? a + SP_CR : n;
        const double* x = xs + r * ws;
        double* o = cs + r * (int)seg;
        prefilter_chunk(
            a, b, n, reflect != 0, [&](long i) { return x[(int)(i - w0)]; }, [&](long i, double v) { o[(int)(i - seg0)] = v; },
            [&](long i) { return o[(int)(i - seg0)]; });
    }
    __syncthreads();
    const int segw = (int)(n - seg0 < seg ? n - seg0 : seg);
    for (int idx = tid; idx < rows * segw; idx += SP_THREADS) {
        const int rr = idx / segw, j = idx - rr * segw;
        dst[(row0 + rr) * n + seg0 + j] = cs[rr * seg + j];
    }
}

template <typename T>
static void prefilter_launch(const T* src, double* dst, long outer, long nsrc, long inner, long pad, int reflect,
                             hipStream_t st) {
    const long n = nsrc + 2 * pad;
    if (inner == 1) {
        long cps = (n + SP_CR - 1) / SP_CR;
        cps = cps > SP_CPS ? SP_CPS : cps;
        const long seg = cps * SP_CR;
        const long w = n < seg + 2 * SP_H + 1 ? n : seg + 2 * SP_H + 1;
        const int ws = (int)(w | 1);
        long rt = SP_THREADS / cps;
        rt = rt > SP_XCAP / ws ? SP_XCAP / ws : rt;
        rt = rt > outer ? outer : rt;
        const long rblocks = (outer + rt - 1) / rt, segs = (n + seg - 1) / seg;
        for (long sb0 = 0; sb0 < segs; sb0 += 65535) {
            const long gy = segs - sb0 < 65535 ? segs - sb0 : 65535;
            hipLaunchKernelGGL((prefilter_row_kernel<T>), dim3((unsigned)rblocks, (unsigned)gy), dim3(SP_THREADS), 0, st, src,
                               dst, outer, nsrc, n, pad, reflect, (int)cps, (int)rt, ws, sb0);
        }
        return;
    }
    const long nchunks = (n + SP_CHUNK - 1) / SP_CHUNK;
    const long items = outer * nchunks * inner;
    long g = (items + SP_THREADS - 1) / SP_THREADS;
    g = g > (1L << 22) ? (1L << 22) : g;
    hipLaunchKernelGGL((prefilter_inner_kernel<T>), dim3((unsigned)g), dim3(SP_THREADS), 0, st, src, dst, nsrc, n, inner,
                       nchunks, items, pad, reflect);
}

// ---- interpolation: one output per thread, lanes along the flattened (outer, Lout, inner) ------------------------------
// whole-sample symmetric fold of a tap outside [0, n - 1]: period 2 (n - 1); n == 1 is all position 0
__device__ __forceinline__ long mirror_idx(long i, long n) {
    if (i >= 0 && i < n) return i;
    if (n == 1) return 0;
    const long p = 2 * (n - 1);
    long j = i % p;
    if (j < 0) j += p;
    return j < n ? j : p - j;
}

// src: the samples (orders 0 and 1) or the prefilter's coefficients (order 3), nsrc long along the axis; the coordinate
// of output l is l * step + pad, product and sum rounded separately as scipy's are.  I: the integer type of the index
// split, 32-bit where the output has fewer than 2^31 elements.
template <typename TS, typename TD, typename I, int ORDER>
__global__ __launch_bounds__(SP_THREADS) void zoom_interp_kernel(const TS* __restrict__ src, TD* __restrict__ dst, long nsrc,
                                                                 long Lout, long inner, long total, double step, double pad) {
    for (long idx = (long)blockIdx.x * SP_THREADS + threadIdx.x; idx < total; idx += (long)gridDim.x * SP_THREADS) {
        long r = idx, i = 0;
        if (inner > 1) {
            r = (long)((I)idx / (I)inner);
            i = idx - r * inner;
        }
        const long o = (long)((I)r / (I)Lout);
        const long l = r - o * Lout;
        const double c = add_rn(mul_rn((double)l, step), pad);
        const TS* s = src + o * nsrc * inner + i;
        double v;
        if constexpr (ORDER == 0) {
            v = (double)s[mirror_idx((long)floor(c + 0.5), nsrc) * inner];
        } else if constexpr (ORDER == 1) {
            const double fl = floor(c), t = c - fl;
            const long f = (long)fl;
            v = (1.0 - t) * (double)s[mirror_idx(f, nsrc) * inner];
            v += t * (double)s[mirror_idx(f + 1, nsrc) * inner];
        } else {
            const double fl = floor(c), t = c - fl, u = 1.0 - t;
            const long f = (long)fl;
            const double w0 = u * u * u / 6.0;
            const double w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
            const double w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
            const double w3 = 1.0 - w0 - w1 - w2;
            v = w0 * (double)s[mirror_idx(f - 1, nsrc) * inner];
            v += w1 * (double)s[mirror_idx(f, nsrc) * inner];
            v += w2 * (double)s[mirror_idx(f + 1, nsrc) * inner];
            v += w3 * (double)s[mirror_idx(f + 2, nsrc) * inner];
        }
        dst[idx] = (TD)v;
    }
}

static int stream_grid(long n) { return gd_stream_grid(n, SP_THREADS, 1L << 20); }

template <typename TS, typename TD, int ORDER>
static void interp_launch_o(const TS* src, TD* dst, long outer, long nsrc, long Lin, long Lout, long inner, double pad,
                            hipStream_t st) {
    const long total = outer * Lout * inner;
    const double step = Lout > 1 ? (double)(Lin - 1) / (double)(Lout - 1) : 1.0;
    const dim3 g(stream_grid(total)), b(SP_THREADS);
    if (total < (1L << 31))
        hipLaunchKernelGGL((zoom_interp_kernel<TS, TD, unsigned int, ORDER>), g, b, 0, st, src, dst, nsrc, Lout, inner, total,
                           step, pad);
    else
        hipLaunchKernelGGL((zoom_interp_kernel<TS, TD, unsigned long, ORDER>), g, b, 0, st, src, dst, nsrc, Lout, inner, total,
                           step, pad);
}

template <typename TS, typename TD>
static void interp_launch(const TS* src, TD* dst, long outer, long nsrc, long Lin, long Lout, long inner, int order,
                          double pad, hipStream_t st) {
    if (order == 0) interp_launch_o<TS, TD, 0>(src, dst, outer, nsrc, Lin, Lout, inner, pad, st);
    else if (order == 1) interp_launch_o<TS, TD, 1>(src, dst, outer, nsrc, Lin, Lout, inner, pad, st);
    else interp_launch_o<TS, TD, 3>(src, dst, outer, nsrc, Lin, Lout, inner, pad, st);
}

// ---- ((x + trend) * scale + mean) * unit, NaN where the mask is 0 ------------------------------------------------------
// mul_rn / add_rn are never contracted into an FMA: every operation rounds as numpy's does
template <typename TX, typename TT, typename TD>
__global__ __launch_bounds__(SP_THREADS) void restore_units_kernel(const TX* x, const TT* __restrict__ trend,
                                                                   const unsigned char* __restrict__ mask, long n, long hw,
                                                                   double scale, double mean, double unit, TD* dst) {
    for (long i = (long)blockIdx.x * SP_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * SP_THREADS) {
        double v = (double)x[i];
        if (trend) v = add_rn(v, (double)trend[i]);
        v = mul_rn(add_rn(mul_rn(v, scale), mean), unit);
        if (mask && mask[i % hw] == 0) v = (double)NAN;
        dst[i] = (TD)v;
    }
}

template <typename TX, typename TT>
static void restore_launch_d(const TX* x, const TT* trend, const unsigned char* mask, long n, long hw, double scale,
                             double mean, double unit, void* dst, int dst_dtype, hipStream_t st) {
    const dim3 g(stream_grid(n)), b(SP_THREADS);
    if (dst_dtype == GD_FILTER_F64)
        hipLaunchKernelGGL((restore_units_kernel<TX, TT, double>), g, b, 0, st, x, trend, mask, n, hw, scale, mean, unit,
                           (double*)dst);
    else
        hipLaunchKernelGGL((restore_units_kernel<TX, TT, float>), g, b, 0, st, x, trend, mask, n, hw, scale, mean, unit,
                           (float*)dst);
}

template <typename TX>
static void restore_launch(const TX* x, const void* trend, int trend_dtype, const unsigned char* mask, long n, long hw,
                           double scale, double mean, double unit, void* dst, int dst_dtype, hipStream_t st) {
    if (trend_dtype == GD_FILTER_F64)
        restore_launch_d<TX, double>(x, (const double*)trend, mask, n, hw, scale, mean, unit, dst, dst_dtype, st);
    else
        restore_launch_d<TX, float>(x, (const float*)trend, mask, n, hw, scale, mean, unit, dst, dst_dtype, st);
}

// a product of three positive longs that does not fit in 2^62 is refused rather than wrapped
static bool fits(long a, long b, long c) { return a <= (1L << 62) / b && a * b <= (1L << 62) / c; }

}  // namespace

extern "C" size_t gd_zoom_axis_ws_bytes(long outer, long Lin, long inner, int order, int mode) {
    if (order != 3 || outer <= 0 || Lin <= 0 || inner <= 0) return 0;
    const long n = Lin + (mode == GD_ZOOM_NEAREST ? 2 * SP_PAD : 0);
    if (!fits(outer, n, inner)) return 0;
    return (size_t)outer * (size_t)n * (size_t)inner * sizeof(double);
}

extern "C" int gd_zoom_axis(const void* src, void* dst, int src_dtype, int dst_dtype, long outer, long Lin, long Lout,
                            long inner, int order, int mode, void* ws, size_t ws_bytes, void* stream) {
    GD_CHECK_ARG(src && dst, "gd_zoom_axis: null pointer");
    GD_CHECK_ARG(src != dst, "gd_zoom_axis: src == dst (the zoom is not in place)");
    GD_CHECK_ARG(gd_dtype_ok(src_dtype) && gd_dtype_ok(dst_dtype), "gd_zoom_axis: dtype outside {0, 1}");
    GD_CHECK_ARG(Lin > 0 && outer > 0 && inner > 0, "gd_zoom_axis: L <= 0 (or outer, inner <= 0)");
    GD_CHECK_ARG(Lout > 0, "gd_zoom_axis: Lout <= 0");
    GD_CHECK_ARG(order == 0 || order == 1 || order == 3, "gd_zoom_axis: order outside {0, 1, 3}");
    GD_CHECK_ARG(mode == GD_ZOOM_MIRROR || mode == GD_ZOOM_NEAREST, "gd_zoom_axis: unknown mode");
    GD_CHECK_ARG(fits(outer, Lin + 2 * SP_PAD, inner) && fits(outer, Lout, inner), "gd_zoom_axis: tensor of 2^62 elements or more");
    GD_CHECK_ARG(gd_elem_aligned(src, src_dtype) && gd_elem_aligned(dst, dst_dtype), "gd_zoom_axis: pointer not element aligned");
    const long pad = order == 3 && mode == GD_ZOOM_NEAREST ? SP_PAD : 0;
    if (order == 3) {
        GD_CHECK_ARG(ws, "gd_zoom_axis: null pointer (order 3 needs the workspace)");
        GD_CHECK_ARG(ws_bytes >= gd_zoom_axis_ws_bytes(outer, Lin, inner, order, mode),
                     "gd_zoom_axis: workspace smaller than gd_zoom_axis_ws_bytes");
        GD_CHECK_ARG(gd_aligned(ws, 8) && ws != src && ws != dst, "gd_zoom_axis: workspace not 8-byte aligned, or src / dst");
        double* coef = (double*)ws;
        if (src_dtype == GD_FILTER_F64) prefilter_launch<double>((const double*)src, coef, outer, Lin, inner, pad, pad != 0, GD_S);
        else prefilter_launch<float>((const float*)src, coef, outer, Lin, inner, pad, pad != 0, GD_S);
        if (dst_dtype == GD_FILTER_F64)
            interp_launch<double, double>(coef, (double*)dst, outer, Lin + 2 * pad, Lin, Lout, inner, 3, (double)pad, GD_S);
        else
            interp_launch<double, float>(coef, (float*)dst, outer, Lin + 2 * pad, Lin, Lout, inner, 3, (double)pad, GD_S);
    } else if (src_dtype == GD_FILTER_F64) {
        if (dst_dtype == GD_FILTER_F64)
            interp_launch<double, double>((const double*)src, (double*)dst, outer, Lin, Lin, Lout, inner, order, 0.0, GD_S);
        else
            interp_launch<double, float>((const double*)src, (float*)dst, outer, Lin, Lin, Lout, inner, order, 0.0, GD_S);
    } else {
        if (dst_dtype == GD_FILTER_F64)
            interp_launch<float, double>((const float*)src, (double*)dst, outer, Lin, Lin, Lout, inner, order, 0.0, GD_S);
        else
            interp_launch<float, float>((const float*)src, (float*)dst, outer, Lin, Lin, Lout, inner, order, 0.0, GD_S);
    }
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_spline_prefilter_axis(const void* src, double* dst, int src_dtype, long outer, long L, long inner,
                                        void* stream) {
    GD_CHECK_ARG(src && dst, "gd_spline_prefilter_axis: null pointer");
    GD_CHECK_ARG(src != (const void*)dst, "gd_spline_prefilter_axis: src == dst (the filter is not in place)");
    GD_CHECK_ARG(gd_dtype_ok(src_dtype), "gd_spline_prefilter_axis: dtype outside {0, 1}");
    GD_CHECK_ARG(L > 0 && outer > 0 && inner > 0, "gd_spline_prefilter_axis: L <= 0 (or outer, inner <= 0)");
    GD_CHECK_ARG(fits(outer, L, inner), "gd_spline_prefilter_axis: tensor of 2^62 elements or more");
    GD_CHECK_ARG(gd_elem_aligned(src, src_dtype) && gd_aligned(dst, 8), "gd_spline_prefilter_axis: pointer not element aligned");
    if (src_dtype == GD_FILTER_F64) prefilter_launch<double>((const double*)src, dst, outer, L, inner, 0, 0, GD_S);
    else prefilter_launch<float>((const float*)src, dst, outer, L, inner, 0, 0, GD_S);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_restore_units(const void* x, int x_dtype, const void* trend, int trend_dtype, const unsigned char* mask,
                                long planes, long hw, double scale, double mean, double unit, void* dst, int dst_dtype,
                                void* stream) {
    GD_CHECK_ARG(x && dst, "gd_restore_units: null pointer");
    GD_CHECK_ARG(gd_dtype_ok(x_dtype) && gd_dtype_ok(dst_dtype) && (!trend || gd_dtype_ok(trend_dtype)), "gd_restore_units: dtype outside {0, 1}");
    GD_CHECK_ARG(planes > 0 && hw > 0, "gd_restore_units: n <= 0");
    GD_CHECK_ARG(fits(planes, hw, 1), "gd_restore_units: tensor of 2^62 elements or more");
    GD_CHECK_ARG(x != dst || x_dtype == dst_dtype, "gd_restore_units: dst aliases x with another dtype");
    GD_CHECK_ARG(dst != trend && dst != (const void*)mask, "gd_restore_units: dst aliases trend or mask");
    GD_CHECK_ARG(gd_elem_aligned(x, x_dtype) && gd_elem_aligned(dst, dst_dtype) && (!trend || gd_elem_aligned(trend, trend_dtype)),
                 "gd_restore_units: pointer not element aligned");
    const long n = planes * hw;
    if (!trend) trend_dtype = GD_FILTER_F64;
    if (x_dtype == GD_FILTER_F64)
        restore_launch<double>((const double*)x, trend, trend_dtype, mask, n, hw, scale, mean, unit, dst, dst_dtype, GD_S);
    else
        restore_launch<float>((const float*)x, trend, trend_dtype, mask, n, hw, scale, mean, unit, dst, dst_dtype, GD_S);
    GD_LAUNCH_CHECK();
    return 0;
}
