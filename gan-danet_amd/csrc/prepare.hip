// Dataset preparation (include/gandanet.h, "dataset preparation"): the per-channel StandardScaler of datasets.py's
// load_data() -- fit as (count, mean, M2) records, transform and inverse with the optional change to the dataset's stored
// (N, C, H, W) layout -- and frequency_domain_augmentation() restated as a cosine sum along one axis.  Storage fp32 or
// fp64; all arithmetic fp64 with one rounding to the output type.  No atomics: every reduction runs in a fixed order that
// depends on the shape alone, so the same input gives the same bits.  All index arithmetic is 64-bit.
// From elem_util.h: gd_vec16, gd_shfl_down_d, gd_stream_grid, gd_dtype_ok, gd_elem_aligned, gd_aligned, GD_S.
#include "elem_util.h"

#include <math.h>

namespace {

constexpr int PR_THREADS = 256;

// ---- channel moments ----------------------------------------------------------------------------------------------------
// the record of one channel: count, mean, M2 = sum (x - mean)^2
struct Mom {
    double n, mean, m2;
};

// Chan et al. (the co-moment merge of evalstats.hip without the second variable): statistics of A followed by B
__host__ __device__ inline Mom mom_merge(const Mom& a, const Mom& b) {
    if (!(b.n > 0)) return a;
    if (!(a.n > 0)) return b;
    Mom r;
    r.n = a.n + b.n;
    const double d = b.mean - a.mean, fb = b.n / r.n;
    r.mean = a.mean + d * fb;
    r.m2 = a.m2 + b.m2 + d * d * (a.n * fb);
    return r;
}

// Kahan's compensated running sum
struct Comp {
    double s, c;
    __device__ __forceinline__ void add(double v) {
        const double y = v - c, t = s + y;
        c = (t - s) - y;
        s = t;
    }
};

// rows per workgroup: the same for every (M, C), whatever the device does
constexpr long MOM_MAX_BLOCKS = 2048;
constexpr int MOM_CHUNK = PR_THREADS;   // channels one workgroup covers

static long mom_groups(long C) { return C >= MOM_CHUNK ? 1 : MOM_CHUNK / C; }
static long mom_rows_per_block(long M, long C) {
    const long G = mom_groups(C);
    long rb = (M + MOM_MAX_BLOCKS - 1) / MOM_MAX_BLOCKS;
    if (rb < 8 * G) rb = 8 * G;
    return (rb + G - 1) / G * G;
}
static long mom_blocks(long M, long C) {
    const long rb = mom_rows_per_block(M, C);
    return (M + rb - 1) / rb;
}

// Pass one.  Workgroup (blockIdx.x, blockIdx.y) owns rows [blockIdx.x * rb, + rb) of the channels [blockIdx.y * 256, + cw).
// Thread tid = g * cw + c takes channel c of the rows g, g + G, g + 2G, ... of that range, so where cw == C (C <= 256) step i
// of the workgroup reads the G * C consecutive elements from (row0 + i * G) * C on: one contiguous run, lane after lane.
// A thread sums x - K and (x - K)^2 compensated, K its first sample (a constant channel gives M2 == 0 exactly); the G
// records of a channel are then merged along a fixed tree in LDS and record [block][channel] goes to the workspace.
template <typename T>
__global__ __launch_bounds__(PR_THREADS) void moments_partial_kernel(const T* __restrict__ x, long M, long C, long rb, int cw_full,
                                                                    int G, double* __restrict__ part) {
    __shared__ double red[PR_THREADS * 3];
    const int tid = threadIdx.x;
    const long c0 = (long)blockIdx.y * MOM_CHUNK;
    const int cw = C - c0 < cw_full ? (int)(C - c0) : cw_full;
    const int g = tid / cw_full, cl = tid - g * cw_full;
    const bool active = g < G && cl < cw;
    const long r0 = (long)blockIdx.x * rb, r1 = r0 + rb < M ? r0 + rb : M;
    Mom m = {0.0, 0.0, 0.0};
    if (active && r0 + g < r1) {
        const T* p = x + (r0 + g) * C + c0 + cl;
        const long step = (long)G * C, cnt = (r1 - r0 - g + G - 1) / G;
        const double K = (double)p[0];
        Comp s = {0.0, 0.0}, q = {0.0, 0.0};
#pragma unroll 4
        for (long i = 1; i < cnt; ++i) {
            const double d = (double)p[i * step] - K;
            s.add(d);
            q.add(d * d);
        }
        const double n = (double)cnt, sd = s.s - s.c, qd = q.s - q.c;
        m.n = n;
        m.mean = K + sd / n;
        m.m2 = qd - sd * sd / n;
        if (m.m2 < 0.0) m.m2 = 0.0;
    }
    red[tid * 3 + 0] = m.n;
    red[tid * 3 + 1] = m.mean;
    red[tid * 3 + 2] = m.m2;
    __syncthreads();
    int span = 1;
    while (span < G) span <<= 1;
    for (int st = span >> 1; st > 0; st >>= 1) {
        if (active && g < st && g + st < G) {
            const int o = (tid + st * cw_full) * 3;
            const Mom a = {red[tid * 3], red[tid * 3 + 1], red[tid * 3 + 2]}, b = {red[o], red[o + 1], red[o + 2]};
            const Mom r = mom_merge(a, b);
            red[tid * 3 + 0] = r.n;
            red[tid * 3 + 1] = r.mean;
            red[tid * 3 + 2] = r.m2;
        }
        __syncthreads();
    }
    if (active && g == 0) {
        double* o = part + ((long)blockIdx.x * C + c0 + cl) * 3;
        o[0] = red[tid * 3];
        o[1] = red[tid * 3 + 1];
        o[2] = red[tid * 3 + 2];
    }
}

// Pass two: one wave per channel.  Lane l merges its contiguous run of partial records in block order, then the lanes are
// merged in ascending order along a fixed tree (evalstats.hip, stage 2).
__global__ __launch_bounds__(64) void moments_merge_kernel(const double* __restrict__ part, long nblocks, long C, long cb0,
                                                           double* __restrict__ rec) {
    const long c = cb0 + blockIdx.x;
    const int lane = threadIdx.x;
    const long per = (nblocks + 63) / 64;
    Mom r = {0.0, 0.0, 0.0};
    for (long i = lane * per; i < (lane + 1) * per && i < nblocks; ++i) {
        const double* s = part + (i * C + c) * 3;
        const Mom b = {s[0], s[1], s[2]};
        r = mom_merge(r, b);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        Mom b;
        b.n = gd_shfl_down_d(r.n, o);
        b.mean = gd_shfl_down_d(r.mean, o);
        b.m2 = gd_shfl_down_d(r.m2, o);
        if ((lane & (2 * o - 1)) == 0) r = mom_merge(r, b);
    }
    if (lane == 0) {
        rec[c * 3 + 0] = r.n;
        rec[c * 3 + 1] = r.mean;
        rec[c * 3 + 2] = r.m2;
    }
}

// ---- channel affine -----------------------------------------------------------------------------------------------------
// sklearn's two operations, each rounded on its own (hipcc would contract x * scale + mean into one FMA)
__device__ __forceinline__ double affine(double x, double mean, double scale, int inverse) {
#pragma clang fp contract(off)
    if (inverse) {
        const double p = x * scale;
        return p + mean;
    }
    const double d = x - mean;
    return d / scale;
}

// four consecutive elements: one 16-byte access of fp32, two of fp64
template <typename T> __device__ __forceinline__ void load4(const T* p, double* o) {
#pragma unroll
    for (int k = 0; k < 4; k += gd_vec16<T>::W) gd_vec16<T>::load(p + k, o + k);
}
template <typename T> __device__ __forceinline__ void store4(T* p, const double* o) {
#pragma unroll
    for (int k = 0; k < 4; k += gd_vec16<T>::W) gd_vec16<T>::store(p + k, o + k);
}

// Same layout in and out: item i is the VW consecutive elements from e0 + i * VW on; the channel of an element is its
// flat index mod C, found once per thread and advanced with the grid stride.
template <typename TS, typename TD, int VW>
__global__ __launch_bounds__(PR_THREADS) void affine_flat_kernel(const TS* __restrict__ src, TD* __restrict__ dst, long e0,
                                                                long nitems, long C, const double* __restrict__ mean,
                                                                const double* __restrict__ scale, int inverse) {
    const long stride = (long)gridDim.x * PR_THREADS;
    long it = (long)blockIdx.x * PR_THREADS + threadIdx.x;
    if (it >= nitems) return;
    long c = (e0 + it * VW) % C;
    const long cstep = (stride * VW) % C;
    for (; it < nitems; it += stride) {
        const long e = e0 + it * VW;
        double v[VW];
        if constexpr (VW == 4) load4(src + e, v);
        else v[0] = (double)src[e];
        long cc = c;
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            v[k] = affine(v[k], mean[cc], scale[cc], inverse);
            if (++cc == C) cc = 0;
        }
        if constexpr (VW == 4) store4(dst + e, v);
        else dst[e] = (TD)v[0];
        c += cstep;
        if (c >= C) c -= C;
    }
}

// (N, HW, C) -> (N, C, HW): a tile of `th` positions x up to 64 channels goes through LDS.  It is read row after row of
// the source (where the tile spans all C channels that is one contiguous run of th * C elements) and written channel
// after channel, a wave storing 64 consecutive positions of one channel.  The odd pitch spreads both access patterns
// over the banks.
constexpr int TR_CH = 64;
constexpr int TR_LDS = 256 * 17;   // elements: th = 256 positions x <= 16 channels, or 64 x 64 (pitch 65)

template <typename TS, typename TD>
__global__ __launch_bounds__(PR_THREADS) void affine_nchw_kernel(const TS* __restrict__ src, TD* __restrict__ dst, long n0, long HW,
                                                                long C, int th_log2, const double* __restrict__ mean,
                                                                const double* __restrict__ scale, int inverse) {
    __shared__ TS tile[TR_LDS];
    const int th = 1 << th_log2, tid = threadIdx.x;
    const long n = n0 + blockIdx.z, h0 = (long)blockIdx.x * th, c0 = (long)blockIdx.y * TR_CH;
    const int cw = C - c0 < TR_CH ? (int)(C - c0) : TR_CH;
    const int rows = HW - h0 < th ? (int)(HW - h0) : th;
    const int pitch = cw | 1;
    const TS* s = src + (n * HW + h0) * C + c0;
    for (int idx = tid; idx < rows * cw; idx += PR_THREADS) {
        const int row = idx / cw, cc = idx - row * cw;
        tile[row * pitch + cc] = s[(long)row * C + cc];
    }
    __syncthreads();
    TD* d = dst + (n * C + c0) * HW + h0;
    for (int idx = tid; idx < (cw << th_log2); idx += PR_THREADS) {
        const int cc = idx >> th_log2, row = idx & (th - 1);
        if (row < rows)
            d[(long)cc * HW + row] = (TD)affine((double)tile[row * pitch + cc], mean[c0 + cc], scale[c0 + cc], inverse);
    }
}

// ---- frequency augmentation ---------------------------------------------------------------------------------------------
// out[o, t, p] = x[o, t, p] + sum_{k < K1} noise[o, k, p] * coef[k, t].  Item `it` of a launch is the VW consecutive series
// from column (it % (inner / VW)) * VW of outer index it / (inner / VW); a thread keeps its K1 * VW noise values in
// registers (KMAX is the compile-time capacity) and walks t over [t0, t1) = chunk blockIdx.y of the axis, so every load
// and store of a wave is a run of consecutive elements of one row.  The chunk's columns of the table sit in LDS (at most
// GD_FREQ_LDS_BYTES: a longer axis is cut into more chunks) and a wave reads coef[k, t] as a broadcast.  The terms are added in ascending k and x is added last.
template <typename T> struct Vec2;   // two consecutive elements: 8 bytes of fp32, 16 of fp64
template <> struct Vec2<float> { typedef float2 type; };
template <> struct Vec2<double> { typedef double2 type; };

template <typename T, int VW, int KMAX>
__global__ __launch_bounds__(PR_THREADS) void freq_augment_kernel(const T* __restrict__ src, T* __restrict__ dst, long L, long inner,
                                                                 long nitems, long tchunk, const double* __restrict__ noise, int K1,
                                                                 const double* __restrict__ coef) {
    extern __shared__ double ctab[];   // [K1][tlen]
    typedef typename Vec2<T>::type V;
    const long t0 = (long)blockIdx.y * tchunk, t1 = t0 + tchunk < L ? t0 + tchunk : L;
    const int tlen = (int)(t1 - t0);
    for (int i = threadIdx.x; i < K1 * tlen; i += PR_THREADS) {
        const int k = i / tlen, tt = i - k * tlen;
        ctab[i] = coef[(long)k * L + t0 + tt];
    }
    __syncthreads();
    const long it = (long)blockIdx.x * PR_THREADS + threadIdx.x;
    if (it >= nitems) return;
    const long per = inner / VW, o = it / per, col = (it - o * per) * VW;
    double nz[KMAX][VW];
    const double* np = noise + o * K1 * inner + col;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
#pragma unroll
        for (int e = 0; e < VW; ++e) nz[k][e] = k < K1 ? np[(long)k * inner + e] : 0.0;
    const T* s = src + (o * L + t0) * inner + col;
    T* d = dst + (o * L + t0) * inner + col;
    for (int tt = 0; tt < tlen; ++tt) {
        double x[VW], acc[VW];
        if constexpr (VW == 2) {
            const V v = *reinterpret_cast<const V*>(s + (long)tt * inner);
            x[0] = (double)v.x;
            x[1] = (double)v.y;
        } else {
            x[0] = (double)s[(long)tt * inner];
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k < K1) {
                const double cf = ctab[k * tlen + tt];
#pragma unroll
                for (int e = 0; e < VW; ++e) acc[e] = fma(nz[k][e], cf, acc[e]);
            }
        }
        if constexpr (VW == 2) {
            V w;
            w.x = (T)(x[0] + acc[0]);
            w.y = (T)(x[1] + acc[1]);
            *reinterpret_cast<V*>(d + (long)tt * inner) = w;
        } else {
            d[(long)tt * inner] = (T)(x[0] + acc[0]);
        }
    }
}

// chunks of the axis per series: 1 (a thread walks the whole axis) once there are enough series to fill the device;
// a function of the shape alone
static long freq_chunks(long nitems, long L, int K1) {
    const long fit = GD_FREQ_LDS_BYTES / (long)sizeof(double) / K1;   // columns of the table one workgroup may hold
    const long least = (L + fit - 1) / fit;
    if (nitems >= 65536) return least;
    long want = (65536 + nitems - 1) / nitems, most = (L + 7) / 8;
    want = want < most ? want : most;
    return want > least ? want : least;
}

template <typename T, int VW>
static void freq_launch(const T* src, T* dst, long outer, long L, long inner, const double* noise, int K1, const double* coef,
                        hipStream_t st) {
    const long nitems = outer * (inner / VW);
    const long chunks = freq_chunks(nitems, L, K1), tchunk = (L + chunks - 1) / chunks, ny = (L + tchunk - 1) / tchunk;
    const size_t lds = (size_t)K1 * (size_t)tchunk * sizeof(double);
    const dim3 grid((unsigned)((nitems + PR_THREADS - 1) / PR_THREADS), (unsigned)ny);
    if (K1 <= 16)
        hipLaunchKernelGGL((freq_augment_kernel<T, VW, 16>), grid, dim3(PR_THREADS), lds, st, src, dst, L, inner, nitems, tchunk,
                           noise, K1, coef);
    else
        hipLaunchKernelGGL((freq_augment_kernel<T, VW, GD_FREQ_MAX_BINS>), grid, dim3(PR_THREADS), lds, st, src, dst, L, inner,
                           nitems, tchunk, noise, K1, coef);
}

static int stream_grid(long n) { return gd_stream_grid(n, PR_THREADS, 65536); }

template <typename TS, typename TD>
static void affine_launch(const TS* src, TD* dst, long M, long C, const double* mean, const double* scale, int inverse, long N,
                          long HW, hipStream_t st) {
    if (N > 0) {
        const int th_log2 = C <= 16 ? 8 : 6;
        const long tiles = (HW + (1L << th_log2) - 1) >> th_log2, chunks = (C + TR_CH - 1) / TR_CH;
        for (long n0 = 0; n0 < N; n0 += 65535) {
            const unsigned gz = (unsigned)(N - n0 < 65535 ? N - n0 : 65535);
            hipLaunchKernelGGL((affine_nchw_kernel<TS, TD>), dim3((unsigned)tiles, (unsigned)chunks, gz), dim3(PR_THREADS), 0, st,
                               src, dst, n0, HW, C, th_log2, mean, scale, inverse);
        }
        return;
    }
    const long n = M * C;
    const long n4 = gd_aligned(src, 16) && gd_aligned(dst, 16) ? n / 4 : 0;
    if (n4 > 0)
        hipLaunchKernelGGL((affine_flat_kernel<TS, TD, 4>), dim3(stream_grid(n4)), dim3(PR_THREADS), 0, st, src, dst, 0L, n4, C, mean,
                           scale, inverse);
    if (n - 4 * n4 > 0)
        hipLaunchKernelGGL((affine_flat_kernel<TS, TD, 1>), dim3(stream_grid(n - 4 * n4)), dim3(PR_THREADS), 0, st, src, dst, 4 * n4,
                           n - 4 * n4, C, mean, scale, inverse);
}

}  // namespace

extern "C" size_t gd_channel_moments_ws_bytes(long M, long C) {
    if (M <= 0 || C <= 0) return 0;
    return (size_t)mom_blocks(M, C) * (size_t)C * 3 * sizeof(double);
}

extern "C" int gd_channel_moments(const void* x, int dtype, long M, long C, double* rec, void* ws, size_t ws_bytes, void* stream) {
    GD_CHECK_ARG(x && rec && ws, "gd_channel_moments: null pointer");
    GD_CHECK_ARG(gd_dtype_ok(dtype), "gd_channel_moments: dtype outside {0, 1}");
    GD_CHECK_ARG(M > 0 && C > 0, "gd_channel_moments: M <= 0 or C <= 0");
    GD_CHECK_ARG(C <= 65535L * MOM_CHUNK && M < (1L << 53) / C, "gd_channel_moments: C or M * C too large");
    GD_CHECK_ARG(ws_bytes >= gd_channel_moments_ws_bytes(M, C), "gd_channel_moments: workspace too small");
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(rec, 8) && gd_aligned(ws, 8),
                 "gd_channel_moments: pointer not element aligned");
    const long rb = mom_rows_per_block(M, C), nb = mom_blocks(M, C), chunks = (C + MOM_CHUNK - 1) / MOM_CHUNK;
    const int cw = (int)(C < MOM_CHUNK ? C : MOM_CHUNK), G = (int)mom_groups(C);
    const dim3 grid((unsigned)nb, (unsigned)chunks);
    if (dtype == GD_FILTER_F64)
        hipLaunchKernelGGL((moments_partial_kernel<double>), grid, dim3(PR_THREADS), 0, GD_S, (const double*)x, M, C, rb, cw, G,
                           (double*)ws);
    else
        hipLaunchKernelGGL((moments_partial_kernel<float>), grid, dim3(PR_THREADS), 0, GD_S, (const float*)x, M, C, rb, cw, G,
                           (double*)ws);
    for (long cb0 = 0; cb0 < C; cb0 += 1L << 30) {
        const unsigned g = (unsigned)(C - cb0 < (1L << 30) ? C - cb0 : (1L << 30));
        hipLaunchKernelGGL(moments_merge_kernel, dim3(g), dim3(64), 0, GD_S, (const double*)ws, nb, C, cb0, rec);
    }
    GD_LAUNCH_CHECK();
    return 0;
}

// Host only.  sklearn's StandardScaler from the records: var_ = M2 / count (ddof 0), scale_ = sqrt(var_), and scale_ = 1
// where _is_constant_feature holds: var_ <= count * eps * var_ + (count * mean_ * eps)^2, eps = 2^-52.
extern "C" int gd_scale_from_moments_host(const double* rec, long C, double* mean, double* var, double* scale) {
    GD_CHECK_ARG(rec && mean && var && scale, "gd_scale_from_moments_host: null pointer");
    GD_CHECK_ARG(C > 0, "gd_scale_from_moments_host: C <= 0");
    const double eps = 2.220446049250313e-16;
    for (long c = 0; c < C; ++c) GD_CHECK_ARG(rec[3 * c] >= 1.0, "gd_scale_from_moments_host: a channel without samples");
    for (long c = 0; c < C; ++c) {
        const double n = rec[3 * c], m = rec[3 * c + 1], v = rec[3 * c + 2] / n;
        const double t = n * m * eps, bound = n * eps * v + t * t;
        mean[c] = m;
        var[c] = v;
        scale[c] = v <= bound ? 1.0 : sqrt(v);
    }
    return 0;
}

extern "C" int gd_channel_affine(const void* src, int src_dtype, void* dst, int dst_dtype, long M, long C, const double* mean_dev,
                                 const double* scale_dev, int inverse, long N, long HW, void* stream) {
    GD_CHECK_ARG(src && dst && mean_dev && scale_dev, "gd_channel_affine: null pointer");
    GD_CHECK_ARG(src != dst, "gd_channel_affine: src == dst");
    GD_CHECK_ARG(gd_dtype_ok(src_dtype) && gd_dtype_ok(dst_dtype), "gd_channel_affine: dtype outside {0, 1}");
    GD_CHECK_ARG(M > 0 && C > 0, "gd_channel_affine: M <= 0 or C <= 0");
    GD_CHECK_ARG(M < (1L << 53) / C, "gd_channel_affine: M * C too large");
    GD_CHECK_ARG(inverse == 0 || inverse == 1, "gd_channel_affine: inverse outside {0, 1}");
    GD_CHECK_ARG(N >= 0 && (N == 0 || (HW > 0 && M / N == HW && M % N == 0)), "gd_channel_affine: layout change needs N * HW == M");
    GD_CHECK_ARG(N == 0 || (C <= 65535L * TR_CH), "gd_channel_affine: C too large for the layout change");
    GD_CHECK_ARG(gd_elem_aligned(src, src_dtype) && gd_elem_aligned(dst, dst_dtype) && gd_aligned(mean_dev, 8) &&
                     gd_aligned(scale_dev, 8),
                 "gd_channel_affine: pointer not element aligned");
    if (src_dtype == GD_FILTER_F64 && dst_dtype == GD_FILTER_F64)
        affine_launch((const double*)src, (double*)dst, M, C, mean_dev, scale_dev, inverse, N, HW, GD_S);
    else if (src_dtype == GD_FILTER_F64)
        affine_launch((const double*)src, (float*)dst, M, C, mean_dev, scale_dev, inverse, N, HW, GD_S);
    else if (dst_dtype == GD_FILTER_F64)
        affine_launch((const float*)src, (double*)dst, M, C, mean_dev, scale_dev, inverse, N, HW, GD_S);
    else
        affine_launch((const float*)src, (float*)dst, M, C, mean_dev, scale_dev, inverse, N, HW, GD_S);
    GD_LAUNCH_CHECK();
    return 0;
}

// Host only.  coef[k * L + t] = cos(2 pi ((k t) mod L) / L) / L: the argument is reduced in integers, so it stays in
// [0, 2 pi) however large k * t is.
extern "C" int gd_freq_cos_table_host(long L, int K1, double* coef) {
    GD_CHECK_ARG(coef, "gd_freq_cos_table_host: null pointer");
    GD_CHECK_ARG(L > 0, "gd_freq_cos_table_host: L <= 0");
    GD_CHECK_ARG(K1 >= 1 && K1 <= L && K1 <= GD_FREQ_MAX_BINS, "gd_freq_cos_table_host: K1 outside 1..min(L, 33)");
    const double two_pi = 2.0 * M_PI, dl = (double)L;
    for (long k = 0; k < K1; ++k)
        for (long t = 0; t < L; ++t) coef[k * L + t] = cos(two_pi * (double)((k * t) % L) / dl) / dl;
    return 0;
}

extern "C" int gd_freq_augment_axis(const void* src, void* dst, int dtype, long outer, long L, long inner, const double* noise,
                                    int K1, const double* coef, void* stream) {
    GD_CHECK_ARG(src && dst && noise && coef, "gd_freq_augment_axis: null pointer");
    GD_CHECK_ARG(src != dst, "gd_freq_augment_axis: src == dst (the input is never modified)");
    GD_CHECK_ARG(gd_dtype_ok(dtype), "gd_freq_augment_axis: dtype outside {0, 1}");
    GD_CHECK_ARG(L > 0 && outer > 0 && inner > 0, "gd_freq_augment_axis: L <= 0 (or outer, inner <= 0)");
    GD_CHECK_ARG(K1 >= 1, "gd_freq_augment_axis: K1 < 1");
    GD_CHECK_ARG(K1 <= L, "gd_freq_augment_axis: K1 > L");
    GD_CHECK_ARG(K1 <= GD_FREQ_MAX_BINS, "gd_freq_augment_axis: K1 > 33");
    GD_CHECK_ARG((long)K1 * L * (long)sizeof(double) <= GD_FREQ_MAX_TABLE_BYTES,
                 "gd_freq_augment_axis: table of K1 * L doubles over the cap (GD_FREQ_MAX_TABLE_BYTES)");
    GD_CHECK_ARG(outer < (1L << 53) / L / inner, "gd_freq_augment_axis: tensor too large");
    GD_CHECK_ARG(gd_elem_aligned(src, dtype) && gd_elem_aligned(dst, dtype) && gd_aligned(noise, 8) && gd_aligned(coef, 8),
                 "gd_freq_augment_axis: pointer not element aligned");
    GD_CHECK_ARG((outer * inner + PR_THREADS - 1) / PR_THREADS < (1L << 31), "gd_freq_augment_axis: outer * inner too large");
    // two series per lane where the rows are whole pairs and both tensors start on a 16-byte boundary; one otherwise
    const bool vec = inner % 2 == 0 && gd_aligned(src, 16) && gd_aligned(dst, 16);
    if (dtype == GD_FILTER_F64) {
        if (vec) freq_launch<double, 2>((const double*)src, (double*)dst, outer, L, inner, noise, K1, coef, GD_S);
        else freq_launch<double, 1>((const double*)src, (double*)dst, outer, L, inner, noise, K1, coef, GD_S);
    } else {
        if (vec) freq_launch<float, 2>((const float*)src, (float*)dst, outer, L, inner, noise, K1, coef, GD_S);
        else freq_launch<float, 1>((const float*)src, (float*)dst, outer, L, inner, noise, K1, coef, GD_S);
    }
    GD_LAUNCH_CHECK();
    return 0;
}
