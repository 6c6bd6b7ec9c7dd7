// Smoothing and gap filling of the auxiliary fields (include/gandanet.h, "filters"): scipy.ndimage's separable correlate
// along one axis (gaussian_filter's pass, and the interior of savgol_filter), savgol_filter's mode='interp' edge rule, the
// rank filter of median_filter over a small box, and the pointwise head and tail of the normalised-convolution gap fill.
// A dense tensor is seen as (outer, L, inner) around the filtered axis.  Storage fp32 or fp64; every sum is fp64 and is
// rounded to the storage type once per pass, as scipy's correlate1d does.  No atomics; all index arithmetic is 64-bit.
// From elem_util.h: gd_vec16, gd_head_of, gd_stream_grid, gd_dtype_ok, gd_elem_aligned, gd_aligned, GD_S.
#include "elem_util.h"

#include <math.h>

namespace {

constexpr int FT_THREADS = 256;
constexpr int FT_MAXW = 2 * GD_FILTER_MAX_RADIUS + 1;

// the weights of one pass travel by value in the kernel arguments: no device allocation, no copy, and a wave reads
// w[k] (k is the same in every lane) through the scalar cache
struct CorrW {
    double w[FT_MAXW];
};

// scipy's 'reflect' (half-sample symmetric: d c b a | a b c d | d c b a) for ANY q: the extension has period 2L, so the
// rule holds when the radius is several times L, and L == 1 maps everything to 0
__device__ __forceinline__ long reflect_idx(long q, long L) {
    if (q >= 0 && q < L) return q;
    const long p = 2 * L;
    long j = q % p;
    if (j < 0) j += p;
    return j < L ? j : p - 1 - j;
}

// ---- correlate, inner > 1: lanes along `inner`, a wave walks the axis --------------------------------------------------
// block (64, 4): threadIdx.x picks VW consecutive columns of `inner` (one 16-byte access per row when VW > 1),
// threadIdx.y a run of CORR_LR consecutive positions of the axis.  A thread reads the 2 * radius + CORR_LR rows its run
// needs once each and feeds every row to the up to CORR_LR outputs it belongs to (kk = the row's tap for output j, the
// same in every lane), so a row costs one load per CORR_LR outputs instead of one per output; neighbouring runs re-read
// the 2 * radius halo rows from cache.  Every output adds its taps in ascending order.
// Grid: blockIdx.x runs along the axis, blockIdx.y over the column blocks, blockIdx.z over outer, so workgroups that share
// halo rows are dispatched one after the other and meet them in cache, however large `inner` is.
// Columns: item `it` of a launch is column c0 + (it < skip_from ? it : it + skip_len) * VW -- the 16-byte instance covers
// the aligned body, the scalar one the head and the tail around it (or every column).
constexpr int CORR_LR = 4;
constexpr int CORR_TY = 4;

template <typename T, int VW>
__global__ __launch_bounds__(64 * CORR_TY) void corr_inner_kernel(const T* __restrict__ src, T* __restrict__ dst, long L,
                                                                  long inner, long c0, long nitems, long skip_from,
                                                                  long skip_len, long o0, long lb0, long cb0, CorrW W,
                                                                  int radius, int edge) {
    const long it = (cb0 + blockIdx.y) * 64 + threadIdx.x;
    const long l0 = ((lb0 + blockIdx.x) * CORR_TY + threadIdx.y) * CORR_LR;
    if (it >= nitems || l0 >= L) return;
    const long col = c0 + (it < skip_from ? it : it + skip_len) * VW;
    const long base = (o0 + blockIdx.z) * L * inner + col;
    const T* s = src + base;
    T* d = dst + base;
    double acc[CORR_LR][VW];
#pragma unroll
    for (int j = 0; j < CORR_LR; ++j)
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[j][e] = 0.0;
    for (int m = -radius; m < radius + CORR_LR; ++m) {
        long q = l0 + m;
        if (edge == GD_EDGE_INTERIOR) {
            if (q < 0 || q >= L) continue;   // such a row only reaches outputs that stay unwritten
        } else {
            q = reflect_idx(q, L);
        }
        T v[VW];
        if constexpr (VW > 1) {
            gd_vec16<T>::load(s + q * inner, v);
        } else {
            v[0] = s[q * inner];
        }
#pragma unroll
        for (int j = 0; j < CORR_LR; ++j) {
            const int kk = m - j + radius;
            if (kk >= 0 && kk <= 2 * radius) {
                const double w = W.w[kk];
#pragma unroll
                for (int e = 0; e < VW; ++e) acc[j][e] = fma(w, (double)v[e], acc[j][e]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CORR_LR; ++j) {
        const long l = l0 + j;
        if (l >= L || (edge == GD_EDGE_INTERIOR && (l < radius || l >= L - radius))) continue;
        if constexpr (VW > 1) {
            gd_vec16<T>::store(d + l * inner, acc[j]);
        } else {
            d[l * inner] = (T)acc[j][0];
        }
    }
}

// ---- correlate, inner == 1: lanes along the axis, a row segment plus halo in LDS ----------------------------------------
// One workgroup per (row, segment of ROW_SEG outputs).  The segment and `radius` elements on either side (rounded up to
// whole 16-byte vectors, so the staged window starts on a vector boundary of the row) are staged once: 16-byte loads
// where the row starts on a 16-byte boundary and the vector lies inside it, else element by element through the reflect
// rule.  Thread t then computes outputs t, t + 256, t + 512, t + 768 of the segment: consecutive lanes read consecutive
// LDS words (conflict free) and store consecutive elements (256 or 512 contiguous bytes per wave instruction).
constexpr int ROW_SEG = 1024;
constexpr int ROW_PER = ROW_SEG / FT_THREADS;

template <typename T>
__global__ __launch_bounds__(FT_THREADS) void corr_row_kernel(const T* __restrict__ src, T* __restrict__ dst, long L, long o0,
                                                              long sb0, CorrW W, int radius, int edge) {
    typedef typename gd_vec16<T>::type V;
    constexpr int VW = gd_vec16<T>::W;
    __shared__ __attribute__((aligned(16))) T tile[ROW_SEG + 2 * GD_FILTER_MAX_RADIUS];
    const int tid = threadIdx.x;
    const long row = o0 + blockIdx.x, seg0 = (sb0 + blockIdx.y) * ROW_SEG;
    const T* s = src + row * L;
    T* d = dst + row * L;
    const int rp = (radius + VW - 1) / VW * VW;
    const long a0 = seg0 - rp;                                   // first staged position, a multiple of VW
    const long seg_end = seg0 + ROW_SEG < L ? seg0 + ROW_SEG : L;
    const int nvec = (int)((seg_end + rp - a0 + VW - 1) / VW);   // <= (ROW_SEG + 2 * rp) / VW
    const bool vec_ok = ((uintptr_t)s & 15u) == 0;
    for (int v = tid; v < nvec; v += FT_THREADS) {
        const long p = a0 + (long)v * VW;
        if (vec_ok && p >= 0 && p + VW <= L) {
            *reinterpret_cast<V*>(tile + v * VW) = *reinterpret_cast<const V*>(s + p);
        } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) tile[v * VW + e] = s[reflect_idx(p + e, L)];
        }
    }
    __syncthreads();
    double acc[ROW_PER];
#pragma unroll
    for (int j = 0; j < ROW_PER; ++j) acc[j] = 0.0;
    const int b = tid + rp - radius;
    for (int kk = 0; kk <= 2 * radius; ++kk) {
        const double w = W.w[kk];
#pragma unroll
        for (int j = 0; j < ROW_PER; ++j) acc[j] = fma(w, (double)tile[b + kk + j * FT_THREADS], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < ROW_PER; ++j) {
        const long l = seg0 + tid + j * FT_THREADS;
        if (l >= L || (edge == GD_EDGE_INTERIOR && (l < radius || l >= L - radius))) continue;
        d[l] = (T)acc[j];
    }
}

template <typename T>
static void corr_launch(const T* src, T* dst, long outer, long L, long inner, const CorrW& W, int radius, int edge,
                        hipStream_t st) {
    if (inner == 1) {
        const long segs = (L + ROW_SEG - 1) / ROW_SEG;
        constexpr long ROWS = 1L << 23;   // rows per launch: grid.x * 256 threads stays below 2^32
        for (long o0 = 0; o0 < outer; o0 += ROWS)
            for (long sb0 = 0; sb0 < segs; sb0 += 65535) {
                const long gx = outer - o0 < ROWS ? outer - o0 : ROWS;
                const long gy = segs - sb0 < 65535 ? segs - sb0 : 65535;
                hipLaunchKernelGGL((corr_row_kernel<T>), dim3((unsigned)gx, (unsigned)gy), dim3(FT_THREADS), 0, st, src, dst, L,
                                   o0, sb0, W, radius, edge);
            }
        return;
    }
    constexpr int VW = gd_vec16<T>::W;
    // 16-byte path: the row stride is a whole number of vectors and both tensors reach a 16-byte boundary after the same
    // `head` columns; the scalar instance takes the head and the tail, or everything
    long head = gd_head_of(src), nv = 0;
    if (inner % VW == 0 && head == gd_head_of(dst) && head <= inner) nv = (inner - head) / VW;
    else head = 0;
    const long rest = inner - nv * VW;
    const long lblocks = (L + CORR_TY * CORR_LR - 1) / (CORR_TY * CORR_LR);
    const dim3 blk(64, CORR_TY);
    constexpr long LBMAX = 1L << 24;   // axis blocks per launch: grid.x * 64 threads stays below 2^32
    const auto go = [&](auto kernel, long nitems, long c0, long skip_from, long skip_len) {
        const long cblocks = (nitems + 63) / 64;
        for (long o0 = 0; o0 < outer; o0 += 65535)
            for (long cb0 = 0; cb0 < cblocks; cb0 += 65535)
                for (long lb0 = 0; lb0 < lblocks; lb0 += LBMAX) {
                    const unsigned gz = (unsigned)(outer - o0 < 65535 ? outer - o0 : 65535);
                    const unsigned gy = (unsigned)(cblocks - cb0 < 65535 ? cblocks - cb0 : 65535);
                    const unsigned gx = (unsigned)(lblocks - lb0 < LBMAX ? lblocks - lb0 : LBMAX);
                    hipLaunchKernelGGL(kernel, dim3(gx, gy, gz), blk, 0, st, src, dst, L, inner, c0, nitems, skip_from, skip_len,
                                       o0, lb0, cb0, W, radius, edge);
                }
    };
    if (nv > 0) go(corr_inner_kernel<T, VW>, nv, head, nv, 0L);
    if (rest > 0) go(corr_inner_kernel<T, 1>, rest, 0L, head, nv * VW);
}

// ---- savgol_filter mode='interp': the first and last window / 2 outputs ------------------------------------------------
// output (o, side, p, i) = sum_j edge[side][p][j] * src[o, (side ? L - window : 0) + j, i]; lanes along inner
template <typename T>
__global__ __launch_bounds__(FT_THREADS) void savgol_edges_kernel(const T* __restrict__ src, T* __restrict__ dst, long outer,
                                                                  long L, long inner, const double* __restrict__ edge,
                                                                  int window) {
    const int h = window / 2;
    const long total = outer * 2 * h * inner;
    for (long t = (long)blockIdx.x * FT_THREADS + threadIdx.x; t < total; t += (long)gridDim.x * FT_THREADS) {
        const long i = t % inner;
        long r = t / inner;
        const int p = (int)(r % h);
        r /= h;
        const int side = (int)(r & 1);
        const long o = r >> 1;
        const long first = side ? L - window : 0;
        const T* s = src + (o * L + first) * inner + i;
        const double* e = edge + ((long)side * h + p) * window;
        double acc = 0.0;
        for (int j = 0; j < window; ++j) acc = fma(e[j], (double)s[(long)j * inner], acc);
        dst[(o * L + (side ? L - h + p : p)) * inner + i] = (T)acc;
    }
}

// ---- median over a box of COUNT elements ------------------------------------------------------------------------------
// order-preserving integer keys: a < b as numbers <=> key(a) < key(b) as unsigned integers (-0 below +0; NaN unspecified)
template <typename T> struct Key;
template <> struct Key<float> {
    typedef unsigned int type;
    static constexpr int BITS = 32;
    __device__ static type of(float f) {
        const unsigned int u = __float_as_uint(f);
        return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    }
    __device__ static float back(type k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
};
template <> struct Key<double> {
    typedef unsigned long long type;
    static constexpr int BITS = 64;
    __device__ static type of(double f) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(f);
        return u ^ ((u >> 63) ? 0xffffffffffffffffull : 0x8000000000000000ull);
    }
    __device__ static double back(type k) {
        return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : 0xffffffffffffffffull)));
    }
};

// 'reflect' for an offset of at most 2 either way: one fold is enough when L >= 2, and L == 1 is all position 0
__device__ __forceinline__ long reflect_near(long q, long L) {
    if (L == 1) return 0;
    return q < 0 ? -q - 1 : (q >= L ? 2 * L - 1 - q : q);
}

// One output per thread.  The window's keys live in registers (COUNT is a compile-time constant; the per-axis sizes are
// not, their product is) and the median is found by bisection on the key bits: the largest v with #{key < v} <= COUNT / 2
// is the (COUNT / 2)-th smallest key, one of the inputs, so the result is exact.
template <typename T, int COUNT>
__global__ __launch_bounds__(FT_THREADS) void median_kernel(const T* __restrict__ src, T* __restrict__ dst, long n0, long n1,
                                                            long n2, long n3, int s0, int s1, int s2, int s3) {
    typedef typename Key<T>::type K;
    const long total = n0 * n1 * n2 * n3;
    for (long idx = (long)blockIdx.x * FT_THREADS + threadIdx.x; idx < total; idx += (long)gridDim.x * FT_THREADS) {
        const long c3 = idx % n3;
        long t = idx / n3;
        const long c2 = t % n2;
        t /= n2;
        const long c1 = t % n1, c0 = t / n1;
        K key[COUNT];
        int d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
        for (int e = 0; e < COUNT; ++e) {
            const long i0 = reflect_near(c0 + d0 - s0 / 2, n0), i1 = reflect_near(c1 + d1 - s1 / 2, n1);
            const long i2 = reflect_near(c2 + d2 - s2 / 2, n2), i3 = reflect_near(c3 + d3 - s3 / 2, n3);
            key[e] = Key<T>::of(src[((i0 * n1 + i1) * n2 + i2) * n3 + i3]);
            if (++d3 == s3) {
                d3 = 0;
                if (++d2 == s2) {
                    d2 = 0;
                    if (++d1 == s1) {
                        d1 = 0;
                        ++d0;
                    }
                }
            }
        }
        K res = 0;
        for (int bit = Key<T>::BITS - 1; bit >= 0; --bit) {
            const K cand = res | ((K)1 << bit);
            int below = 0;
#pragma unroll
            for (int e = 0; e < COUNT; ++e) below += key[e] < cand ? 1 : 0;
            if (below <= COUNT / 2) res = cand;
        }
        dst[idx] = Key<T>::back(res);
    }
}

static int stream_grid(long n) { return gd_stream_grid(n, FT_THREADS, 65536); }

template <typename T>
static bool median_launch(const T* src, T* dst, const long* n, const int* s, int count, hipStream_t st) {
    const long total = n[0] * n[1] * n[2] * n[3];
    // one output is hundreds of instructions: more workgroups than a streaming kernel would want
    long g = (total + FT_THREADS - 1) / FT_THREADS;
    g = g > (1L << 22) ? (1L << 22) : g;
#define MED_GO(C)                                                                                                          \
    hipLaunchKernelGGL((median_kernel<T, C>), dim3((unsigned)g), dim3(FT_THREADS), 0, st, src, dst, n[0], n[1], n[2], n[3], \
                       s[0], s[1], s[2], s[3])
    switch (count) {
        case 3: MED_GO(3); break;
        case 5: MED_GO(5); break;
        case 9: MED_GO(9); break;
        case 25: MED_GO(25); break;
        case 27: MED_GO(27); break;
        case 81: MED_GO(81); break;
        default: return false;
    }
#undef MED_GO
    return true;
}

// ---- gap fill, pointwise ----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(FT_THREADS) void fill_prepare_kernel(const T* __restrict__ x, double placeholder,
                                                                  T* __restrict__ vals, T* __restrict__ mask, long n) {
    for (long i = (long)blockIdx.x * FT_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * FT_THREADS) {
        const T v = x[i];
        const bool gap = (double)v <= placeholder;
        vals[i] = gap ? (T)0 : v;
        mask[i] = gap ? (T)0 : (T)1;
    }
}
template <typename T>
__global__ __launch_bounds__(FT_THREADS) void fill_ratio_kernel(const T* __restrict__ x, const T* __restrict__ num,
                                                                const T* __restrict__ den, double placeholder,
                                                                T* __restrict__ dst, long n) {
    for (long i = (long)blockIdx.x * FT_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * FT_THREADS) {
        const T v = x[i];
        T out = v;
        if ((double)v <= placeholder) {
            const double dn = (double)den[i];
            out = (T)((double)num[i] / (dn == 0.0 ? 1.0 : dn));
        }
        dst[i] = out;
    }
}

// np.sum's pairwise order for n < 8, and for 8 <= n <= 128 its eight running sums: the normalisation of the Gaussian
// taps then rounds as scipy's `phi_x / phi_x.sum()` does
static double pairwise_sum(const double* a, int n) {
    if (n < 8) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += a[i];
        return s;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) s += a[i];
        return s;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum(a, n2) + pairwise_sum(a + n2, n - n2);
}

}  // namespace

// Host only.  scipy.ndimage._filters._gaussian_kernel1d at order 0.
extern "C" int gd_gaussian_weights_host(double sigma, double truncate, double* w, int cap) {
    GD_CHECK_ARG(w, "gd_gaussian_weights_host: null pointer");
    GD_CHECK_ARG(sigma > 0.0 && sigma == sigma, "gd_gaussian_weights_host: sigma <= 0");
    GD_CHECK_ARG(truncate >= 0.0 && truncate * sigma + 0.5 < 1e9, "gd_gaussian_weights_host: truncate * sigma out of range");
    const int radius = (int)(truncate * sigma + 0.5);
    GD_CHECK_ARG(2L * radius + 1 <= (long)cap, "gd_gaussian_weights_host: 2 * radius + 1 exceeds the capacity of w");
    const double c = -0.5 / (sigma * sigma);
    for (int k = -radius; k <= radius; ++k) w[k + radius] = exp(c * (double)(k * k));
    const double sum = pairwise_sum(w, 2 * radius + 1);
    for (int k = 0; k <= 2 * radius; ++k) w[k] /= sum;
    return radius;
}

extern "C" int gd_correlate1d_axis(const void* src, void* dst, int dtype, long outer, long L, long inner, const double* w_host,
                                   int radius, int edge_mode, void* stream) {
    GD_CHECK_ARG(src && dst && w_host, "gd_correlate1d_axis: null pointer");
    GD_CHECK_ARG(src != dst, "gd_correlate1d_axis: src == dst (the filter is not in place)");
    GD_CHECK_ARG(gd_dtype_ok(dtype), "gd_correlate1d_axis: dtype outside {0, 1}");
    GD_CHECK_ARG(L > 0 && outer > 0 && inner > 0, "gd_correlate1d_axis: L <= 0 (or outer, inner <= 0)");
    GD_CHECK_ARG(radius >= 0 && radius <= GD_FILTER_MAX_RADIUS, "gd_correlate1d_axis: radius outside 0..64");
    GD_CHECK_ARG(inner < (1L << 32), "gd_correlate1d_axis: inner >= 2^32 (split the trailing dimensions)");
    GD_CHECK_ARG(edge_mode == GD_EDGE_REFLECT || edge_mode == GD_EDGE_INTERIOR, "gd_correlate1d_axis: unknown edge mode");
    GD_CHECK_ARG(gd_elem_aligned(src, dtype) && gd_elem_aligned(dst, dtype), "gd_correlate1d_axis: pointer not element aligned");
    CorrW W;
    for (int k = 0; k < FT_MAXW; ++k) W.w[k] = k <= 2 * radius ? w_host[k] : 0.0;
    if (dtype == GD_FILTER_F64) corr_launch<double>((const double*)src, (double*)dst, outer, L, inner, W, radius, edge_mode, GD_S);
    else corr_launch<float>((const float*)src, (float*)dst, outer, L, inner, W, radius, edge_mode, GD_S);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_savgol_edges_axis(const void* src, void* dst, int dtype, long outer, long L, long inner,
                                    const double* edge_dev, int window, void* stream) {
    GD_CHECK_ARG(src && dst && edge_dev, "gd_savgol_edges_axis: null pointer");
    GD_CHECK_ARG(src != dst, "gd_savgol_edges_axis: src == dst");
    GD_CHECK_ARG(gd_dtype_ok(dtype), "gd_savgol_edges_axis: dtype outside {0, 1}");
    GD_CHECK_ARG(L > 0 && outer > 0 && inner > 0, "gd_savgol_edges_axis: L <= 0 (or outer, inner <= 0)");
    GD_CHECK_ARG(window >= 1 && (window & 1) && window <= GD_SAVGOL_MAX_WINDOW, "gd_savgol_edges_axis: window must be odd and <= 33");
    GD_CHECK_ARG(window <= L, "gd_savgol_edges_axis: window longer than the axis");
    GD_CHECK_ARG(gd_elem_aligned(src, dtype) && gd_elem_aligned(dst, dtype) && gd_aligned(edge_dev, 8),
                 "gd_savgol_edges_axis: pointer not element aligned");
    if (window == 1) return 0;
    const int g = stream_grid(outer * 2 * (window / 2) * inner);
    if (dtype == GD_FILTER_F64)
        hipLaunchKernelGGL((savgol_edges_kernel<double>), dim3(g), dim3(FT_THREADS), 0, GD_S, (const double*)src, (double*)dst,
                           outer, L, inner, edge_dev, window);
    else
        hipLaunchKernelGGL((savgol_edges_kernel<float>), dim3(g), dim3(FT_THREADS), 0, GD_S, (const float*)src, (float*)dst,
                           outer, L, inner, edge_dev, window);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_median_nd(const void* src, void* dst, int dtype, const int64_t* shape4, const int* size4, void* stream) {
    GD_CHECK_ARG(src && dst && shape4 && size4, "gd_median_nd: null pointer");
    GD_CHECK_ARG(src != dst, "gd_median_nd: src == dst");
    GD_CHECK_ARG(gd_dtype_ok(dtype), "gd_median_nd: dtype outside {0, 1}");
    long n[4];
    int count = 1;
    for (int a = 0; a < 4; ++a) {
        GD_CHECK_ARG(shape4[a] > 0, "gd_median_nd: shape <= 0");
        GD_CHECK_ARG(size4[a] == 1 || size4[a] == 3 || size4[a] == 5, "gd_median_nd: size outside {1, 3, 5}");
        n[a] = (long)shape4[a];
        count *= size4[a];
    }
    GD_CHECK_ARG(count == 3 || count == 5 || count == 9 || count == 25 || count == 27 || count == 81,
                 "gd_median_nd: window count outside {3, 5, 9, 25, 27, 81}");
    GD_CHECK_ARG(gd_elem_aligned(src, dtype) && gd_elem_aligned(dst, dtype), "gd_median_nd: pointer not element aligned");
    const bool ok = dtype == GD_FILTER_F64 ? median_launch<double>((const double*)src, (double*)dst, n, size4, count, GD_S)
                                           : median_launch<float>((const float*)src, (float*)dst, n, size4, count, GD_S);
    GD_CHECK_ARG(ok, "gd_median_nd: window count outside {3, 5, 9, 25, 27, 81}");
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_fill_prepare(const void* x, double placeholder, void* vals, void* mask, int dtype, long n, void* stream) {
    GD_CHECK_ARG(x && vals && mask, "gd_fill_prepare: null pointer");
    GD_CHECK_ARG(x != vals && x != mask && vals != mask, "gd_fill_prepare: x, vals and mask must be three buffers");
    GD_CHECK_ARG(gd_dtype_ok(dtype), "gd_fill_prepare: dtype outside {0, 1}");
    GD_CHECK_ARG(n > 0, "gd_fill_prepare: n <= 0");
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_elem_aligned(vals, dtype) && gd_elem_aligned(mask, dtype),
                 "gd_fill_prepare: pointer not element aligned");
    if (dtype == GD_FILTER_F64)
        hipLaunchKernelGGL((fill_prepare_kernel<double>), dim3(stream_grid(n)), dim3(FT_THREADS), 0, GD_S, (const double*)x,
                           placeholder, (double*)vals, (double*)mask, n);
    else
        hipLaunchKernelGGL((fill_prepare_kernel<float>), dim3(stream_grid(n)), dim3(FT_THREADS), 0, GD_S, (const float*)x,
                           placeholder, (float*)vals, (float*)mask, n);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_fill_ratio(const void* x, const void* num, const void* den, double placeholder, void* dst, int dtype, long n,
                             void* stream) {
    GD_CHECK_ARG(x && num && den && dst, "gd_fill_ratio: null pointer");
    GD_CHECK_ARG(dst != x && dst != num && dst != den, "gd_fill_ratio: dst must be a buffer of its own");
    GD_CHECK_ARG(gd_dtype_ok(dtype), "gd_fill_ratio: dtype outside {0, 1}");
    GD_CHECK_ARG(n > 0, "gd_fill_ratio: n <= 0");
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_elem_aligned(num, dtype) && gd_elem_aligned(den, dtype) && gd_elem_aligned(dst, dtype),
                 "gd_fill_ratio: pointer not element aligned");
    if (dtype == GD_FILTER_F64)
        hipLaunchKernelGGL((fill_ratio_kernel<double>), dim3(stream_grid(n)), dim3(FT_THREADS), 0, GD_S, (const double*)x,
                           (const double*)num, (const double*)den, placeholder, (double*)dst, n);
    else
        hipLaunchKernelGGL((fill_ratio_kernel<float>), dim3(stream_grid(n)), dim3(FT_THREADS), 0, GD_S, (const float*)x,
                           (const float*)num, (const float*)den, placeholder, (float*)dst, n);
    GD_LAUNCH_CHECK();
    return 0;
}
