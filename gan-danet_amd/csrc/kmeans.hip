// k-means on pixel series (include/gandanet.h, "Regionalisation"): the assignment of every series of a (T, M) cube to its
// nearest of K centroids, the ordered sums that make the new centroids, and the farthest-point search of the deterministic
// initialisation.  The per-element arithmetic is kmeans_core.h, shared with the host twins.
//
// gd_km_assign  A workgroup of KM_THREADS = 256 threads owns 256 neighbouring series, one per thread, so every row segment
//               x[t, m .. m + 255] is one coalesced read and the cube is read exactly once, whatever K is.  The centroids are
//               staged in LDS GD_KM_CHUNK = 64 time steps at a time as sc[step][k] (KP * 64 doubles: 4 KiB at KP = 8, 32 KiB at
//               KP = 64, so two or more workgroups share the 160 KiB of a CU); every thread reads the same word, a wave-uniform
//               broadcast.  The K running sums stay in registers: the kernel is a template on KP = K rounded up to 8 / 16 / 32 /
//               64 with fully unrolled loops over k (the padding centroids are zeros whose sums are never looked at), and the
//               samples are loaded eight steps ahead of their use.
//               Registers (hipcc -O3 for gfx950, -Rpass-analysis=kernel-resource-usage); no instance uses scratch memory:
//                   KP      VGPRs (fp64 / fp32 storage)  AGPRs  SGPRs  scratch  waves/SIMD  LDS
//                    8       76 /  76                        0     68        0           6   4 KiB
//                   16       86 /  84                        0     54        0           5   8 KiB
//                   32      176 / 176                        0     54        0           2  16 KiB
//                   64      256 / 256                        6     52        0           1  32 KiB
//               The K = 64 instance takes the whole file of a wave (64 sums are 128 registers, the staged samples and the
//               centroid words the compiler reads ahead fill the rest, six copies sit in AGPRs), so it runs one wave per
//               SIMD: a block of 256 threads is then exactly one wave on each of the four SIMDs of a CU, which is why
//               KM_THREADS = 256; a larger block could not be resident at K = 64, a smaller one would leave SIMDs idle.
// gd_km_update  The pixels are cut into slabs of GD_KM_SLAB = 1024 neighbouring series.  A one-wave workgroup owns one slab
//               and 64 time steps, one step per lane: it walks the pixels of the slab in ascending order, and since all lanes
//               are at the same pixel the label is wave-uniform and the addend w * v goes onto acc[label][lane] in LDS (K * 64
//               doubles) without a conflict.  A lane reads its own row, 64 rows per load; the 64 cache lines are each used by
//               the next 16 (fp64) or 32 (fp32) pixels, so the cube still comes from HBM once.  Lane 0 of the first 64 steps
//               also keeps wsum, count and within of the slab.  The slab's sums, all started from +0.0, go to the workspace;
//               one thread per entry then adds the slabs in ascending order onto running totals that started from +0.0, and a
//               last pass divides by wsum.  THE ORDER: every sum is (((0 + S_0) + S_1) + ..) over the slabs s = 0, 1, .. with
//               S_s = ((0 + a_m0) + a_m0+1 + ..) over the member pixels of slab s in ascending m: a function of (M, labels)
//               alone.  With a workspace that holds fewer than all slabs the slabs are walked in chunks, each chunk added onto
//               the totals before the next is formed: the same additions in the same order.
// gd_km_farthest one workgroup of 1024 threads: a grid-stride scan keeps each thread's best (value, index) pair, wave
//               shuffles and one LDS round reduce the pairs under gd_km_ahead.  An excluded index is looked up (a list of at
//               most GD_KM_MAX_K entries in LDS) only when a candidate would take the lead.
// No atomics.  From elem_util.h: gd_dtype_ok, gd_elem_aligned, gd_aligned, gd_with_dtype, gd_for_items, GD_S.
#include <vector>

#include "elem_util.h"
#include "kmeans_core.h"

namespace {

constexpr int KM_THREADS = 256, KM_AHEAD = 8, KM_UP_LANES = 64, KM_FAR_THREADS = 1024;

// ---- assignment ------------------------------------------------------------------------------------------------------------------
// the epilogue of one series, shared with the host twin: acc[0 .. K - 1] are its distances
__host__ __device__ inline void km_put(const double* acc, int K, bool ok, long m, int* label, double* dist, int* label2, double* dist2) {
    const double nan = (double)NAN;
    double d1 = (double)INFINITY, d2 = (double)INFINITY;
    int k1 = -1, k2 = -1;
    if (ok) {
        for (int k = 0; k < K; ++k) gd_km_pick(acc[k], k, d1, k1, d2, k2);
    }
    label[m] = k1;
    dist[m] = k1 >= 0 ? d1 : nan;
    if (label2) label2[m] = k1 >= 0 ? k2 : -1;
    if (dist2) dist2[m] = (k1 >= 0 && k2 >= 0) ? d2 : nan;
}

template <typename E, int KP>
__global__ __launch_bounds__(KM_THREADS) void km_assign_kernel(const E* __restrict__ x, long T, long M, const double* __restrict__ cent, int K,
                                                                const double* __restrict__ shift, const double* __restrict__ scale,
                                                                const unsigned char* __restrict__ mask, int* __restrict__ label,
                                                                double* __restrict__ dist, int* __restrict__ label2,
                                                                double* __restrict__ dist2) {
    __shared__ double sc[GD_KM_CHUNK * KP];                             // sc[step * KP + k]
    const int tid = (int)threadIdx.x;
    const long m = (long)blockIdx.x * KM_THREADS + tid;
    const bool live = m < M && (!mask || mask[m] != 0);
    const double sh = (live && shift) ? shift[m] : 0.0, sl = (live && scale) ? scale[m] : 1.0;
    double acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.0;
    bool ok = live;
    for (long t0 = 0; t0 < T; t0 += GD_KM_CHUNK) {
        const int n = (int)(T - t0 < GD_KM_CHUNK ? T - t0 : GD_KM_CHUNK);
        __syncthreads();                                                // the chunk before is used up
        for (int i = tid; i < GD_KM_CHUNK * KP; i += KM_THREADS) {
            const int tt = i / KP, k = i - tt * KP;
            sc[i] = (k < K && tt < n) ? cent[(long)k * T + t0 + tt] : 0.0;
        }
        __syncthreads();
        if (live) {
            const E* px = x + t0 * M + m;
            int tt = 0;
            for (; tt + KM_AHEAD <= n; tt += KM_AHEAD) {
                double v[KM_AHEAD];
#pragma unroll
                for (int u = 0; u < KM_AHEAD; ++u) v[u] = gd_km_value((double)px[(long)(tt + u) * M], sh, sl);
#pragma unroll
                for (int u = 0; u < KM_AHEAD; ++u) {
                    ok = ok && gd_km_finite(v[u]);
                    const double* c = sc + (tt + u) * KP;
#pragma unroll
                    for (int k = 0; k < KP; ++k) gd_km_add(acc[k], gd_km_term(v[u], c[k]));
                }
            }
            for (; tt < n; ++tt) {
                const double v = gd_km_value((double)px[(long)tt * M], sh, sl);
                ok = ok && gd_km_finite(v);
                const double* c = sc + tt * KP;
#pragma unroll
                for (int k = 0; k < KP; ++k) gd_km_add(acc[k], gd_km_term(v, c[k]));
            }
        }
    }
    if (m >= M) return;
    // the scan of km_put over registers: unrolled, so acc is never indexed by a run-time value
    const double nan = (double)NAN;
    double d1 = (double)INFINITY, d2 = (double)INFINITY;
    int k1 = -1, k2 = -1;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (ok && k < K) gd_km_pick(acc[k], k, d1, k1, d2, k2);
    }
    label[m] = k1;
    dist[m] = k1 >= 0 ? d1 : nan;
    if (label2) label2[m] = k1 >= 0 ? k2 : -1;
    if (dist2) dist2[m] = (k1 >= 0 && k2 >= 0) ? d2 : nan;
}

template <typename E, int KP>
void km_assign_launch(const E* x, long T, long M, const double* cent, int K, const double* shift, const double* scale, const unsigned char* mask,
                      int* label, double* dist, int* label2, double* dist2, hipStream_t st) {
    hipLaunchKernelGGL((km_assign_kernel<E, KP>), dim3((unsigned)gd_cdiv(M, KM_THREADS)), dim3(KM_THREADS), 0, st, x, T, M, cent, K, shift, scale,
                       mask, label, dist, label2, dist2);
}

template <typename E> struct AssignHostBody {
    const E* x;
    long T, M;
    const double* cent;
    int K;
    const double *shift, *scale;
    const unsigned char* mask;
    int* label;
    double* dist;
    int* label2;
    double* dist2;
    void operator()(long m) const {
        double acc[GD_KM_MAX_K];
        for (int k = 0; k < K; ++k) acc[k] = 0.0;
        bool ok = !mask || mask[m] != 0;
        if (ok) {
            const double sh = shift ? shift[m] : 0.0, sl = scale ? scale[m] : 1.0;
            for (long t = 0; t < T; ++t) {
                const double v = gd_km_value((double)x[t * M + m], sh, sl);
                ok = ok && gd_km_finite(v);
                for (int k = 0; k < K; ++k) gd_km_add(acc[k], gd_km_term(v, cent[(long)k * T + t]));
            }
        }
        km_put(acc, K, ok, m, label, dist, label2, dist2);
    }
};

// ---- update ----------------------------------------------------------------------------------------------------------------------
// grid: (slabs of the chunk, ceil(T / 64)); dynamic LDS: (K * 64 + 3 K) doubles; slabs: the chunk's part of the workspace
template <typename E>
__global__ __launch_bounds__(KM_UP_LANES) void km_update_kernel(const E* __restrict__ x, long T, long M, const int* __restrict__ label,
                                                                 const double* __restrict__ dist, const double* __restrict__ w,
                                                                 const double* __restrict__ shift, const double* __restrict__ scale, int K,
                                                                 long slab0, double* __restrict__ slabs) {
    extern __shared__ double km_sm[];
    double* acc = km_sm;                                                // [K][64]
    double* side = km_sm + K * KM_UP_LANES;                             // wsum[K], count[K], within[K]
    const int lane = (int)threadIdx.x;
    const long t = (long)blockIdx.y * KM_UP_LANES + lane;
    const bool row = t < T, first = blockIdx.y == 0 && lane == 0;
    const long m_begin = (slab0 + blockIdx.x) * GD_KM_SLAB, m_stop = m_begin + GD_KM_SLAB < M ? m_begin + GD_KM_SLAB : M;
    for (int i = lane; i < K * KM_UP_LANES + 3 * K; i += KM_UP_LANES) km_sm[i] = 0.0;
    __syncthreads();
    const E* px = x + (row ? t : 0) * M;
#pragma unroll 4
    for (long m = m_begin; m < m_stop; ++m) {
        const int l = label[m];
        const double xv = row ? (double)px[m] : 0.0;
        if (l < 0 || l >= K) continue;                                  // wave-uniform
        const double wm = w ? w[m] : 1.0;
        if (row) gd_km_wadd(acc[l * KM_UP_LANES + lane], wm, gd_km_value(xv, shift ? shift[m] : 0.0, scale ? scale[m] : 1.0));
        if (first) {
            gd_km_add(side[l], wm);
            gd_km_add(side[K + l], 1.0);
            gd_km_wadd(side[2 * K + l], wm, dist[m]);
        }
    }
    __syncthreads();
    double* out = slabs + (long)blockIdx.x * gd_km_slab_doubles(T, K);
    if (row) {
        for (int k = 0; k < K; ++k) out[(long)k * T + t] = acc[k * KM_UP_LANES + lane];
    }
    if (blockIdx.y == 0) {
        for (int i = lane; i < 3 * K; i += KM_UP_LANES) out[(long)K * T + i] = side[i];
    }
}

// entry e of the totals takes the `ns` slabs of a chunk in ascending order; `start`: the totals begin at +0.0
struct SlabSumBody {
    const double* slabs;
    long ns, sd;
    int start;
    double* tot;
    __host__ __device__ void operator()(long e) const {
        double s = start ? 0.0 : tot[e];
        for (long i = 0; i < ns; ++i) gd_km_add(s, slabs[i * sd + e]);
        tot[e] = s;
    }
};

// item i < K T: centroid entry (k, t), kept where wsum[k] is not > 0; item K T + k: wsum, count, within of cluster k
struct FinishBody {
    const double* tot;
    long T;
    int K;
    double *cent, *wsum;
    long long* count;
    double* within;
    __host__ __device__ void operator()(long i) const {
        const long kt = (long)K * T;
        if (i < kt) {
            const double ws = tot[kt + i / T];
            if (ws > 0.0) cent[i] = tot[i] / ws;
        } else {
            const long k = i - kt;
            wsum[k] = tot[kt + k];
            count[k] = (long long)tot[kt + K + k];
            within[k] = tot[kt + 2 * K + k];
        }
    }
};

template <typename E>
void km_update_host(const E* x, long T, long M, const int* label, const double* dist, const double* w, const double* shift, const double* scale,
                    int K, double* cent, double* wsum, long long* count, double* within) {
    const long sd = gd_km_slab_doubles(T, K), kt = (long)K * T;
    std::vector<double> part((size_t)sd), tot((size_t)sd, 0.0);
    for (long m_begin = 0; m_begin < M; m_begin += GD_KM_SLAB) {
        const long m_stop = m_begin + GD_KM_SLAB < M ? m_begin + GD_KM_SLAB : M;
        for (long e = 0; e < sd; ++e) part[e] = 0.0;
        for (long m = m_begin; m < m_stop; ++m) {
            const int l = label[m];
            if (l < 0 || l >= K) continue;
            const double wm = w ? w[m] : 1.0, sh = shift ? shift[m] : 0.0, sl = scale ? scale[m] : 1.0;
            for (long t = 0; t < T; ++t) gd_km_wadd(part[(long)l * T + t], wm, gd_km_value((double)x[t * M + m], sh, sl));
            gd_km_add(part[kt + l], wm);
            gd_km_add(part[kt + K + l], 1.0);
            gd_km_wadd(part[kt + 2 * K + l], wm, dist[m]);
        }
        gd_for_items<256>(true, sd, nullptr, SlabSumBody{part.data(), 1, sd, 0, tot.data()});
    }
    gd_for_items<256>(true, kt + K, nullptr, FinishBody{tot.data(), T, K, cent, wsum, count, within});
}

// ---- farthest --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KM_FAR_THREADS) void km_farthest_kernel(const double* __restrict__ d, long M, const int* __restrict__ exclude,
                                                                      int n_exclude, int* __restrict__ index) {
    __shared__ int sx[GD_KM_MAX_K];
    __shared__ double rv[KM_FAR_THREADS / 64];
    __shared__ int ri[KM_FAR_THREADS / 64];
    const int tid = (int)threadIdx.x;
    if (tid < n_exclude) sx[tid] = exclude[tid];
    __syncthreads();
    double bv = -(double)INFINITY;
    int bi = INT_MAX;
    for (long i = tid; i < M; i += KM_FAR_THREADS) {
        const double v = d[i];
        if (gd_km_finite(v) && gd_km_ahead(v, (int)i, bv, bi)) {
            bool out = false;
            for (int j = 0; j < n_exclude; ++j) out = out || sx[j] == (int)i;
            if (!out) {
                bv = v;
                bi = (int)i;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (gd_km_ahead(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if ((tid & 63) == 0) {
        rv[tid >> 6] = bv;
        ri[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < KM_FAR_THREADS / 64; ++wv) {
            if (gd_km_ahead(rv[wv], ri[wv], bv, bi)) {
                bv = rv[wv];
                bi = ri[wv];
            }
        }
        *index = bi == INT_MAX ? -1 : bi;
    }
}

}  // namespace

// the checks an entry shares with its host twin
#define KM_SHAPE_CHECKS(fn)                                                                                                \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                        \
    GD_CHECK_ARG(T >= 1 && T <= GD_KM_MAX_T, fn ": T outside 1..GD_KM_MAX_T");                                             \
    GD_CHECK_ARG(K >= 1 && K <= GD_KM_MAX_K, fn ": K outside 1..GD_KM_MAX_K");                                             \
    GD_CHECK_ARG(M > 0 && M < (1L << 31), fn ": M <= 0 or too many series")

#define KM_ASSIGN_CHECKS(fn)                                                                                               \
    GD_CHECK_ARG(x && cent && label && dist, fn ": null pointer");                                                        \
    KM_SHAPE_CHECKS(fn);                                                                                                   \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(cent, 8) && gd_aligned(shift, 8) && gd_aligned(scale, 8) &&       \
                     gd_aligned(label, 4) && gd_aligned(dist, 8) && gd_aligned(label2, 4) && gd_aligned(dist2, 8),        \
                 fn ": pointer not element aligned")

extern "C" int gd_km_assign(const void* x, int dtype, long T, long M, const double* cent, int K, const double* shift, const double* scale,
                            const unsigned char* mask, int* label, double* dist, int* label2, double* dist2, void* stream) {
    KM_ASSIGN_CHECKS("gd_km_assign");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        const E* xe = (const E*)x;
        if (K <= 8) km_assign_launch<E, 8>(xe, T, M, cent, K, shift, scale, mask, label, dist, label2, dist2, GD_S);
        else if (K <= 16) km_assign_launch<E, 16>(xe, T, M, cent, K, shift, scale, mask, label, dist, label2, dist2, GD_S);
        else if (K <= 32) km_assign_launch<E, 32>(xe, T, M, cent, K, shift, scale, mask, label, dist, label2, dist2, GD_S);
        else km_assign_launch<E, 64>(xe, T, M, cent, K, shift, scale, mask, label, dist, label2, dist2, GD_S);
    });
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_km_assign_host(const void* x, int dtype, long T, long M, const double* cent, int K, const double* shift, const double* scale,
                                 const unsigned char* mask, int* label, double* dist, int* label2, double* dist2) {
    KM_ASSIGN_CHECKS("gd_km_assign_host");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        // a plain loop, not gd_for_items: that would also instantiate a device kernel of this body, whose acc[] is indexed
        // at run time and would live in scratch memory
        const AssignHostBody<E> body{(const E*)x, T, M, cent, K, shift, scale, mask, label, dist, label2, dist2};
        for (long m = 0; m < M; ++m) body(m);
    });
    return 0;
}

extern "C" size_t gd_km_update_min_ws_bytes(long T, int K) {
    if (T < 1 || T > GD_KM_MAX_T || K < 1 || K > GD_KM_MAX_K) return 0;
    return 2 * (size_t)gd_km_slab_doubles(T, K) * sizeof(double);
}

extern "C" size_t gd_km_update_ws_bytes(long T, long M, int K) {
    if (T < 1 || T > GD_KM_MAX_T || K < 1 || K > GD_KM_MAX_K || M <= 0) return 0;
    return (1 + (size_t)((M + GD_KM_SLAB - 1) / GD_KM_SLAB)) * (size_t)gd_km_slab_doubles(T, K) * sizeof(double);
}

#define KM_UPDATE_CHECKS(fn)                                                                                               \
    GD_CHECK_ARG(x && label && dist && cent && wsum && count && within, fn ": null pointer");                             \
    KM_SHAPE_CHECKS(fn);                                                                                                   \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(label, 4) && gd_aligned(dist, 8) && gd_aligned(w, 8) &&           \
                     gd_aligned(shift, 8) && gd_aligned(scale, 8) && gd_aligned(cent, 8) && gd_aligned(wsum, 8) &&        \
                     gd_aligned(count, 8) && gd_aligned(within, 8),                                                       \
                 fn ": pointer not element aligned")

extern "C" int gd_km_update(const void* x, int dtype, long T, long M, const int* label, const double* dist, const double* w, const double* shift,
                            const double* scale, int K, double* cent, double* wsum, long long* count, double* within, void* workspace,
                            size_t workspace_bytes, void* stream) {
    KM_UPDATE_CHECKS("gd_km_update");
    GD_CHECK_ARG(workspace && gd_aligned(workspace, 8), "gd_km_update: workspace NULL or not 8-byte aligned");
    const long sd = gd_km_slab_doubles(T, K), nslab = (M + GD_KM_SLAB - 1) / GD_KM_SLAB;
    GD_CHECK_ARG(workspace_bytes >= gd_km_update_min_ws_bytes(T, K), "gd_km_update: workspace smaller than gd_km_update_min_ws_bytes(T, K)");
    long chunk = (long)(workspace_bytes / ((size_t)sd * sizeof(double))) - 1;
    chunk = chunk > nslab ? nslab : chunk;
    double *tot = (double*)workspace, *slabs = tot + sd;
    const size_t lds = (size_t)(K * KM_UP_LANES + 3 * K) * sizeof(double);
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        for (long s0 = 0; s0 < nslab; s0 += chunk) {
            const long ns = s0 + chunk < nslab ? chunk : nslab - s0;
            hipLaunchKernelGGL(km_update_kernel<E>, dim3((unsigned)ns, (unsigned)gd_cdiv(T, KM_UP_LANES)), dim3(KM_UP_LANES), lds, GD_S, (const E*)x,
                               T, M, label, dist, w, shift, scale, K, s0, slabs);
            gd_for_items<KM_THREADS>(false, sd, GD_S, SlabSumBody{slabs, ns, sd, s0 == 0, tot});
        }
    });
    gd_for_items<KM_THREADS>(false, (long)K * T + K, GD_S, FinishBody{tot, T, K, cent, wsum, count, within});
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_km_update_host(const void* x, int dtype, long T, long M, const int* label, const double* dist, const double* w,
                                 const double* shift, const double* scale, int K, double* cent, double* wsum, long long* count,
                                 double* within) {
    KM_UPDATE_CHECKS("gd_km_update_host");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        km_update_host((const E*)x, T, M, label, dist, w, shift, scale, K, cent, wsum, count, within);
    });
    return 0;
}

#define KM_FARTHEST_CHECKS(fn)                                                                                             \
    GD_CHECK_ARG(d && index, fn ": null pointer");                                                                        \
    GD_CHECK_ARG(M > 0 && M < (1L << 31), fn ": M <= 0 or too many entries");                                             \
    GD_CHECK_ARG(n_exclude >= 0 && n_exclude <= GD_KM_MAX_K && (n_exclude == 0 || exclude), fn ": n_exclude outside 0..GD_KM_MAX_K, or no list"); \
    GD_CHECK_ARG(gd_aligned(d, 8) && gd_aligned(exclude, 4) && gd_aligned(index, 4), fn ": pointer not element aligned")

extern "C" int gd_km_farthest(const double* d, long M, const int* exclude, int n_exclude, int* index, void* stream) {
    KM_FARTHEST_CHECKS("gd_km_farthest");
    hipLaunchKernelGGL(km_farthest_kernel, dim3(1), dim3(KM_FAR_THREADS), 0, GD_S, d, M, exclude, n_exclude, index);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_km_farthest_host(const double* d, long M, const int* exclude, int n_exclude, int* index) {
    KM_FARTHEST_CHECKS("gd_km_farthest_host");
    double bv = -(double)INFINITY;
    int bi = INT_MAX;
    for (long i = 0; i < M; ++i) {
        const double v = d[i];
        if (gd_km_finite(v) && gd_km_ahead(v, (int)i, bv, bi)) {
            bool out = false;
            for (int j = 0; j < n_exclude; ++j) out = out || exclude[j] == (int)i;
            if (!out) {
                bv = v;
                bi = (int)i;
            }
        }
    }
    *index = bi == INT_MAX ? -1 : bi;
    return 0;
}
