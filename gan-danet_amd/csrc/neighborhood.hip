// Neighbourhood verification (include/gandanet.h, "Neighbourhood verification"): the fractions skill score of two (T, H, W)
// cubes over K thresholds and S window widths, and the fraction field of one cube.  The arithmetic is neighborhood_core.h,
// shared with the host twins.
//
// T is walked in chunks of as many steps as the workspace holds.  Per chunk:
//   rows     one wave per row of a plane: threshold the 64 pixels of a segment into packed words (valid, I_f, I_o), inclusive
//            scan across the lanes (__shfl_up), add the carry of the segments before (lane 63 broadcast), store at (i + 1, j + 1).
//            The planes go in groups of NBR_GROUP whose thresholds travel as kernel arguments.
//   columns  one thread per column of a table, top to bottom in place, so a wave reads and writes whole rows; writes row 0.
//   score    grid (workgroups of a plane, K, steps): a thread owns GD_NBR_ITEMS centre pixels, finds them and their validity
//            once and then takes the scales in turn -- four corner words per window, all scales of a table while it is in
//            L2 -- with a block sum per scale into one partial per workgroup.
//   final    one thread per (step, k, s) adds the partials in ascending order and writes the record; the base record is the
//            last word of the table.
//   maps     (optional) one thread per (pixel, s, k) adds the chunk's steps in ascending t onto its own three sums.
// No atomics.  From elem_util.h: gd_dtype_ok, gd_elem_aligned, gd_aligned, gd_with_dtype, gd_block_sum_d, GD_S.
#include <vector>

#include "elem_util.h"
#include "neighborhood_core.h"

namespace {

constexpr int NBR_GROUP = 8;          // planes per launch of the row kernel: their thresholds are kernel arguments
constexpr long NBR_MAX_PLANES = 4096; // steps in flight at most (grid.z of the score kernel)

struct NbrThr {
    double f[NBR_GROUP][GD_NBR_MAX_K], o[NBR_GROUP][GD_NBR_MAX_K];
};
struct NbrScales {
    int h[GD_NBR_MAX_S];   // half widths
};

__device__ __forceinline__ gd_nbr_word nbr_wave_scan(gd_nbr_word v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const gd_nbr_word u = __shfl_up(v, o, 64);
        v += lane >= o ? u : 0ull;
    }
    return v;
}

// f, o, tab: at the first plane of the group
template <typename T>
__global__ __launch_bounds__(GD_NBR_THREADS) void nbr_rows_kernel(const T* __restrict__ f, const T* __restrict__ o,
                                                                  const unsigned char* __restrict__ mask, int H, int W, int K, int G, int below,
                                                                  NbrThr thr, gd_nbr_word* __restrict__ tab) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (GD_NBR_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= (long)G * H) return;   // the whole wave leaves; the kernel holds no barrier
    const int g = (int)(row / H), i = (int)(row - (long)g * H);
    const long W1 = W + 1, plane = gd_nbr_plane_words(H, W);
    const T* fr = f + ((long)g * H + i) * W;
    const T* orow = o + ((long)g * H + i) * W;
    const unsigned char* mr = mask ? mask + (long)i * W : mask;
    gd_nbr_word* out = tab + (long)g * K * plane + (long)(i + 1) * W1;
    gd_nbr_word carry[GD_NBR_MAX_K];
#pragma unroll
    for (int k = 0; k < GD_NBR_MAX_K; ++k) carry[k] = 0ull;
    for (int j0 = 0; j0 < W; j0 += 64) {
        const int j = j0 + lane;
        const bool in = j < W;
        const T fv = in ? fr[j] : (T)0, ov = in ? orow[j] : (T)0;
        const bool live = in && (!mr || mr[j] != 0);
#pragma unroll
        for (int k = 0; k < GD_NBR_MAX_K; ++k) {
            if (k < K) {
                const gd_nbr_word w = nbr_wave_scan(gd_nbr_indicator(fv, ov, live, thr.f[g][k], thr.o[g][k], below), lane) + carry[k];
                if (in) out[(long)k * plane + j + 1] = w;
                carry[k] = __shfl(w, 63, 64);
            }
        }
    }
    if (lane == 0) {
        for (int k = 0; k < K; ++k) out[(long)k * plane] = 0ull;
    }
}

// tables: n of them, one after the other
__global__ __launch_bounds__(GD_NBR_THREADS) void nbr_cols_kernel(gd_nbr_word* __restrict__ tab, int H, int W, long n) {
    const long W1 = W + 1, idx = (long)blockIdx.x * GD_NBR_THREADS + threadIdx.x;
    if (idx >= n * W1) return;
    const long t = idx / W1, c = idx - t * W1;
    gd_nbr_word* col = tab + t * gd_nbr_plane_words(H, W) + c;
    gd_nbr_word acc = 0ull;
    col[0] = 0ull;
    int r = 1;
    for (; r + 3 <= H; r += 4) {   // the four loads ahead of the four stores
        const gd_nbr_word a0 = col[(long)r * W1], a1 = col[(long)(r + 1) * W1], a2 = col[(long)(r + 2) * W1], a3 = col[(long)(r + 3) * W1];
        col[(long)r * W1] = acc += a0;
        col[(long)(r + 1) * W1] = acc += a1;
        col[(long)(r + 2) * W1] = acc += a2;
        col[(long)(r + 3) * W1] = acc += a3;
    }
    for (; r <= H; ++r) col[(long)r * W1] = acc += col[(long)r * W1];
}

// the block sum of three values, valid in thread 0: gd_block_sum_d for the fp64 sums, its integer likeness for the others
__device__ __forceinline__ void nbr_block_sum(double (&v)[3], double (*red)[3]) { gd_block_sum_d<3, GD_NBR_THREADS / 64>(v, red); }
__device__ __forceinline__ void nbr_block_sum(unsigned long long (&v)[3], unsigned long long (*red)[3]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) red[tid >> 6][c] = v[c];
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < GD_NBR_THREADS / 64; ++w) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] += red[w][c];
        }
    }
}

// grid (gd_nbr_blocks, K, steps of the chunk); part: (steps, K, S, blocks, 3)
template <typename A>
__global__ __launch_bounds__(GD_NBR_THREADS) void nbr_score_kernel(const gd_nbr_word* __restrict__ tab, int H, int W, int S, NbrScales sc,
                                                                   A* __restrict__ part) {
    __shared__ A red[GD_NBR_THREADS / 64][3];
    const int K = gridDim.y, gx = gridDim.x;
    const long pk = (long)blockIdx.z * K + blockIdx.y;
    const gd_nbr_word* t = tab + pk * gd_nbr_plane_words(H, W);
    int pi[GD_NBR_ITEMS], pj[GD_NBR_ITEMS];
    bool ok[GD_NBR_ITEMS];
#pragma unroll
    for (int q = 0; q < GD_NBR_ITEMS; ++q) {
        const int idx = blockIdx.x * GD_NBR_TILE + threadIdx.x + q * GD_NBR_THREADS;
        const bool in = idx < H * W;
        pi[q] = in ? idx / W : 0;
        pj[q] = in ? idx - pi[q] * W : 0;
        ok[q] = in && gd_nbr_centre(t, H, W, pi[q], pj[q]);
    }
    for (int s = 0; s < S; ++s) {
        const long h = sc.h[s];
        A v[3] = {(A)0, (A)0, (A)0};
#pragma unroll
        for (int q = 0; q < GD_NBR_ITEMS; ++q) {
            if (ok[q]) gd_nbr_add(gd_nbr_window(t, H, W, pi[q], pj[q], h), v);
        }
        nbr_block_sum(v, red);
        if (threadIdx.x == 0) {
            A* p = part + ((pk * S + s) * gx + blockIdx.x) * 3;
            p[0] = v[0];
            p[1] = v[1];
            p[2] = v[2];
        }
        __syncthreads();   // red is written again in the next round
    }
}

// one thread per (step of the chunk, k, s): sums (T, K, S, 3) and base (T, K, 3) at the chunk's first step
template <typename A>
__global__ __launch_bounds__(GD_NBR_THREADS) void nbr_final_kernel(const gd_nbr_word* __restrict__ tab, const A* __restrict__ part, int H, int W,
                                                                   int K, int S, long gx, long n, A* __restrict__ sums,
                                                                   unsigned long long* __restrict__ base) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * GD_NBR_THREADS + threadIdx.x;
    if (idx >= n * K * S) return;
    const A* p = part + idx * gx * 3;
    A a0 = (A)0, a1 = (A)0, a2 = (A)0;
    for (long b = 0; b < gx; ++b) {
        a0 += p[b * 3];
        a1 += p[b * 3 + 1];
        a2 += p[b * 3 + 2];
    }
    sums[idx * 3] = a0;
    sums[idx * 3 + 1] = a1;
    sums[idx * 3 + 2] = a2;
    if (idx % S == 0) {
        const long pk = idx / S;
        const gd_nbr_word w = tab[(pk + 1) * gd_nbr_plane_words(H, W) - 1];
        base[pk * 3] = (unsigned long long)gd_nbr_f_of(w);
        base[pk * 3 + 1] = (unsigned long long)gd_nbr_o_of(w);
        base[pk * 3 + 2] = (unsigned long long)gd_nbr_valid_of(w);
    }
}

// grid (pixels / threads, S, K); maps: (K, S, H, W, 3); the n steps of the chunk in ascending order
template <typename A>
__global__ __launch_bounds__(GD_NBR_THREADS) void nbr_maps_kernel(const gd_nbr_word* __restrict__ tab, int H, int W, NbrScales sc, long n,
                                                                  A* __restrict__ maps) {
    const int idx = blockIdx.x * GD_NBR_THREADS + threadIdx.x;
    if (idx >= H * W) return;
    const int K = gridDim.z, S = gridDim.y, k = blockIdx.z, s = blockIdx.y;
    const int pi = idx / W, pj = idx - pi * W;
    const long h = sc.h[s], plane = gd_nbr_plane_words(H, W);
    A* m = maps + (((long)k * S + s) * H * W + idx) * 3;
    A v[3] = {m[0], m[1], m[2]};
    for (long p = 0; p < n; ++p) gd_nbr_map_step(tab + (p * K + k) * plane, H, W, pi, pj, h, v);
    m[0] = v[0];
    m[1] = v[1];
    m[2] = v[2];
}

// tables of K = 1; out: (steps, H, W) at the chunk's first step
__global__ __launch_bounds__(GD_NBR_THREADS) void nbr_fraction_kernel(const gd_nbr_word* __restrict__ tab, int H, int W, long n, long h, double n2,
                                                                      int normalize, double* __restrict__ out) {
    const long idx = (long)blockIdx.x * GD_NBR_THREADS + threadIdx.x, hw = (long)H * W;
    if (idx >= n * hw) return;
    const long p = idx / hw, r = idx - p * hw, pi = r / W, pj = r - pi * W;
    out[idx] = gd_nbr_fraction_one(tab + p * gd_nbr_plane_words(H, W), H, W, pi, pj, h, n2, normalize);
}

// ---- host twins of the stages ---------------------------------------------------------------------------------------------------
// the K tables of one step
template <typename T>
void nbr_tables_host(const T* f, const T* o, const unsigned char* mask, long H, long W, int K, const double* tf, const double* to, int below,
                     gd_nbr_word* tab) {
    const long W1 = W + 1, plane = gd_nbr_plane_words(H, W);
    for (int k = 0; k < K; ++k) {
        gd_nbr_word* t = tab + k * plane;
        for (long c = 0; c < W1; ++c) t[c] = 0ull;
        for (long i = 0; i < H; ++i) {
            gd_nbr_word acc = 0ull;
            t[(i + 1) * W1] = 0ull;
            for (long j = 0; j < W; ++j) {
                acc += gd_nbr_indicator(f[i * W + j], o[i * W + j], !mask || mask[i * W + j] != 0, tf[k], to[k], below);
                t[(i + 1) * W1 + j + 1] = acc;
            }
        }
        for (long c = 0; c < W1; ++c) {
            gd_nbr_word acc = 0ull;
            for (long r = 1; r <= H; ++r) t[r * W1 + c] = acc += t[r * W1 + c];
        }
    }
}

// the record of one table at one scale, in the order of the score and final kernels
template <typename A> void nbr_score_host(const gd_nbr_word* t, long H, long W, long h, A* rec) {
#pragma clang fp contract(off)
    static thread_local A part[GD_NBR_THREADS][3];
    const long gx = gd_nbr_blocks(H, W);
    A a[3] = {(A)0, (A)0, (A)0}, v[3];
    for (long b = 0; b < gx; ++b) {
        for (int j = 0; j < GD_NBR_THREADS; ++j) gd_nbr_thread_sums(t, H, W, b, j, h, part[j]);
        gd_nbr_block_sum_host(part, v);
        for (int c = 0; c < 3; ++c) a[c] += v[c];
    }
    for (int c = 0; c < 3; ++c) rec[c] = a[c];
}

template <typename A, typename T>
void nbr_fss_host(const T* f, const T* o, long Tn, long H, long W, const unsigned char* mask, const double* thr_f, const double* thr_o, int K,
                  int below, const int* scales, int S, A* sums, unsigned long long* base, A* maps) {
    const long hw = H * W, plane = gd_nbr_plane_words(H, W);
    std::vector<gd_nbr_word> tab((size_t)K * plane);
    if (maps) {
        for (long i = 0; i < (long)K * S * hw * 3; ++i) maps[i] = (A)0;
    }
    for (long t = 0; t < Tn; ++t) {
        nbr_tables_host(f + t * hw, o + t * hw, mask, H, W, K, thr_f + t * K, thr_o + t * K, below, tab.data());
        for (int k = 0; k < K; ++k) {
            const gd_nbr_word* tk = tab.data() + k * plane;
            for (int s = 0; s < S; ++s) {
                const long h = (scales[s] - 1) / 2;
                nbr_score_host(tk, H, W, h, sums + ((t * K + k) * S + s) * 3);
                if (maps) {
                    for (long idx = 0; idx < hw; ++idx) gd_nbr_map_step(tk, H, W, idx / W, idx % W, h, maps + (((long)k * S + s) * hw + idx) * 3);
                }
            }
            const gd_nbr_word w = tk[plane - 1];
            base[(t * K + k) * 3] = (unsigned long long)gd_nbr_f_of(w);
            base[(t * K + k) * 3 + 1] = (unsigned long long)gd_nbr_o_of(w);
            base[(t * K + k) * 3 + 2] = (unsigned long long)gd_nbr_valid_of(w);
        }
    }
}

// ---- the device side: the chunk loop ------------------------------------------------------------------------------------------
size_t nbr_plane_bytes(long H, long W, int K) {
    return (size_t)K * ((size_t)gd_nbr_plane_words(H, W) + (size_t)GD_NBR_MAX_S * gd_nbr_blocks(H, W) * 3) * 8;
}

NbrScales nbr_half_widths(const int* scales, int S) {
    NbrScales sc;
    for (int s = 0; s < GD_NBR_MAX_S; ++s) sc.h[s] = s < S ? (scales[s] - 1) / 2 : 0;
    return sc;
}

// the tables of the steps [t0, t0 + n) into tab
template <typename T>
void nbr_tables_dev(hipStream_t st, const T* f, const T* o, const unsigned char* mask, long H, long W, int K, const double* thr_f,
                    const double* thr_o, int below, long t0, long n, gd_nbr_word* tab) {
    const long hw = H * W, plane = gd_nbr_plane_words(H, W);
    for (long g0 = 0; g0 < n; g0 += NBR_GROUP) {
        const int G = (int)(n - g0 < NBR_GROUP ? n - g0 : NBR_GROUP);
        NbrThr thr;
        for (int g = 0; g < NBR_GROUP; ++g) {
            for (int k = 0; k < GD_NBR_MAX_K; ++k) {
                const bool in = g < G && k < K;
                thr.f[g][k] = in ? thr_f[(t0 + g0 + g) * K + k] : 0.0;
                thr.o[g][k] = in ? thr_o[(t0 + g0 + g) * K + k] : 0.0;
            }
        }
        hipLaunchKernelGGL(nbr_rows_kernel<T>, dim3(gd_cdiv((long)G * H, GD_NBR_THREADS / 64)), dim3(GD_NBR_THREADS), 0, st, f + (t0 + g0) * hw,
                           o + (t0 + g0) * hw, mask, (int)H, (int)W, K, G, below, thr, tab + g0 * K * plane);
    }
    hipLaunchKernelGGL(nbr_cols_kernel, dim3(gd_cdiv(n * K * (W + 1), GD_NBR_THREADS)), dim3(GD_NBR_THREADS), 0, st, tab, (int)H, (int)W, n * K);
}

template <typename A, typename T>
void nbr_fss_dev(hipStream_t st, const T* f, const T* o, long Tn, long H, long W, const unsigned char* mask, const double* thr_f,
                 const double* thr_o, int K, int below, const int* scales, int S, A* sums, unsigned long long* base, A* maps, void* ws,
                 long planes) {
    const long hw = H * W, plane = gd_nbr_plane_words(H, W), gx = gd_nbr_blocks(H, W);
    gd_nbr_word* tab = (gd_nbr_word*)ws;
    A* part = (A*)(tab + planes * K * plane);
    const NbrScales sc = nbr_half_widths(scales, S);
    if (maps) (void)hipMemsetAsync(maps, 0, (size_t)K * S * hw * 3 * 8, st);
    for (long t0 = 0; t0 < Tn; t0 += planes) {
        const long n = Tn - t0 < planes ? Tn - t0 : planes;
        nbr_tables_dev(st, f, o, mask, H, W, K, thr_f, thr_o, below, t0, n, tab);
        hipLaunchKernelGGL(nbr_score_kernel<A>, dim3((unsigned)gx, K, (unsigned)n), dim3(GD_NBR_THREADS), 0, st, tab, (int)H, (int)W, S, sc, part);
        hipLaunchKernelGGL(nbr_final_kernel<A>, dim3(gd_cdiv(n * K * S, GD_NBR_THREADS)), dim3(GD_NBR_THREADS), 0, st, tab, part, (int)H, (int)W, K,
                           S, gx, n, sums + t0 * K * S * 3, base + t0 * K * 3);
        if (maps)
            hipLaunchKernelGGL(nbr_maps_kernel<A>, dim3(gd_cdiv(hw, GD_NBR_THREADS), S, K), dim3(GD_NBR_THREADS), 0, st, tab, (int)H, (int)W, sc, n,
                               maps);
    }
}

long nbr_planes(long H, long W, int K, long Tn, size_t ws_bytes) {
    long p = (long)(ws_bytes / nbr_plane_bytes(H, W, K));
    p = p > NBR_MAX_PLANES ? NBR_MAX_PLANES : p;
    return p > Tn ? Tn : p;
}

bool nbr_any_nan(const double* a, long n) {
    for (long i = 0; i < n; ++i) {
        if (a[i] != a[i]) return true;
    }
    return false;
}

bool nbr_scales_ok(const int* scales, int S) {
    for (int s = 0; s < S; ++s) {
        if (scales[s] < 1 || scales[s] % 2 == 0) return false;
    }
    return true;
}

}  // namespace

extern "C" size_t gd_nbr_ws_bytes(long H, long W, int K, long planes) {
    if (H <= 0 || W <= 0 || H > GD_NBR_MAX_HW || W > GD_NBR_MAX_HW || H * W > GD_NBR_MAX_HW || K < 1 || K > GD_NBR_MAX_K || planes < 1 ||
        planes > (1L << 31))
        return 0;
    return nbr_plane_bytes(H, W, K) * (size_t)planes;
}

// the checks an entry shares with its host twin
#define NBR_CUBE_CHECKS(fn)                                                                                                       \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1} (both cubes have the one dtype)");                                \
    GD_CHECK_ARG(T > 0 && H > 0 && W > 0, fn ": T, H or W <= 0");                                                                 \
    GD_CHECK_ARG(H <= GD_NBR_MAX_HW && W <= GD_NBR_MAX_HW && H * W <= GD_NBR_MAX_HW, fn ": H W above GD_NBR_MAX_HW = 2^20");      \
    GD_CHECK_ARG(T < (1L << 31) && T * H * W < (1L << 31), fn ": T H W reaches 2^31");                                            \
    GD_CHECK_ARG(below == 0 || below == 1, fn ": below outside {0, 1}");                                                          \
    GD_CHECK_ARG(normalize == GD_NBR_WINDOW || normalize == GD_NBR_VALID, fn ": normalize is neither window nor valid")

#define NBR_FSS_CHECKS(fn)                                                                                                        \
    GD_CHECK_ARG(f && o && thr_f && thr_o && scales && sums && base, fn ": null pointer");                                        \
    NBR_CUBE_CHECKS(fn);                                                                                                          \
    GD_CHECK_ARG(K >= 1 && K <= GD_NBR_MAX_K, fn ": K outside 1..GD_NBR_MAX_K");                                                  \
    GD_CHECK_ARG(S >= 1 && S <= GD_NBR_MAX_S, fn ": S outside 1..GD_NBR_MAX_S");                                                  \
    GD_CHECK_ARG(nbr_scales_ok(scales, S), fn ": a scale is even or < 1");                                                        \
    GD_CHECK_ARG(!nbr_any_nan(thr_f, T * K) && !nbr_any_nan(thr_o, T * K), fn ": a threshold is NaN");                            \
    GD_CHECK_ARG(gd_elem_aligned(f, dtype) && gd_elem_aligned(o, dtype) && gd_aligned(sums, 8) && gd_aligned(base, 8) && gd_aligned(maps, 8), \
                 fn ": pointer not element aligned")

#define NBR_WS_CHECKS(fn, k)                                                                                                      \
    GD_CHECK_ARG(ws && gd_aligned(ws, 8) && ws_bytes >= nbr_plane_bytes(H, W, k), fn ": workspace missing, misaligned or below gd_nbr_ws_bytes(H, W, K, 1)")

extern "C" int gd_nbr_fss(const void* f, const void* o, int dtype, long T, long H, long W, const unsigned char* mask, const double* thr_f,
                          const double* thr_o, int K, int below, const int* scales, int S, int normalize, void* sums,
                          unsigned long long* base, void* maps, void* ws, size_t ws_bytes, void* stream) {
    NBR_FSS_CHECKS("gd_nbr_fss");
    NBR_WS_CHECKS("gd_nbr_fss", K);
    const long planes = nbr_planes(H, W, K, T, ws_bytes);
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        if (normalize == GD_NBR_VALID)
            nbr_fss_dev<double>(GD_S, (const E*)f, (const E*)o, T, H, W, mask, thr_f, thr_o, K, below, scales, S, (double*)sums, base,
                                (double*)maps, ws, planes);
        else
            nbr_fss_dev<unsigned long long>(GD_S, (const E*)f, (const E*)o, T, H, W, mask, thr_f, thr_o, K, below, scales, S,
                                            (unsigned long long*)sums, base, (unsigned long long*)maps, ws, planes);
    });
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_nbr_fss_host(const void* f, const void* o, int dtype, long T, long H, long W, const unsigned char* mask, const double* thr_f,
                               const double* thr_o, int K, int below, const int* scales, int S, int normalize, void* sums,
                               unsigned long long* base, void* maps) {
    NBR_FSS_CHECKS("gd_nbr_fss_host");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        if (normalize == GD_NBR_VALID)
            nbr_fss_host<double>((const E*)f, (const E*)o, T, H, W, mask, thr_f, thr_o, K, below, scales, S, (double*)sums, base, (double*)maps);
        else
            nbr_fss_host<unsigned long long>((const E*)f, (const E*)o, T, H, W, mask, thr_f, thr_o, K, below, scales, S,
                                             (unsigned long long*)sums, base, (unsigned long long*)maps);
    });
    return 0;
}

#define NBR_FRACTION_CHECKS(fn)                                                                                                   \
    GD_CHECK_ARG(x && thr && out, fn ": null pointer");                                                                           \
    NBR_CUBE_CHECKS(fn);                                                                                                          \
    GD_CHECK_ARG(scale >= 1 && scale % 2 == 1, fn ": the scale is even or < 1");                                                  \
    GD_CHECK_ARG(!nbr_any_nan(thr, T), fn ": a threshold is NaN");                                                                \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(out, 8), fn ": pointer not element aligned")

extern "C" int gd_nbr_fraction(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* thr, int below,
                               int scale, int normalize, double* out, void* ws, size_t ws_bytes, void* stream) {
    NBR_FRACTION_CHECKS("gd_nbr_fraction");
    NBR_WS_CHECKS("gd_nbr_fraction", 1);
    const long planes = nbr_planes(H, W, 1, T, ws_bytes), hw = H * W, h = (scale - 1) / 2;
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        for (long t0 = 0; t0 < T; t0 += planes) {
            const long n = T - t0 < planes ? T - t0 : planes;
            nbr_tables_dev(GD_S, (const E*)x, (const E*)x, mask, H, W, 1, thr, thr, below, t0, n, (gd_nbr_word*)ws);
            hipLaunchKernelGGL(nbr_fraction_kernel, dim3(gd_cdiv(n * hw, GD_NBR_THREADS)), dim3(GD_NBR_THREADS), 0, GD_S, (const gd_nbr_word*)ws,
                               (int)H, (int)W, n, h, (double)scale * (double)scale, normalize, out + t0 * hw);
        }
    });
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_nbr_fraction_host(const void* x, int dtype, long T, long H, long W, const unsigned char* mask, const double* thr, int below,
                                    int scale, int normalize, double* out) {
    NBR_FRACTION_CHECKS("gd_nbr_fraction_host");
    const long hw = H * W, h = (scale - 1) / 2;
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        std::vector<gd_nbr_word> tab((size_t)gd_nbr_plane_words(H, W));
        for (long t = 0; t < T; ++t) {
            nbr_tables_host((const E*)x + t * hw, (const E*)x + t * hw, mask, H, W, 1, thr + t, thr + t, below, tab.data());
            for (long idx = 0; idx < hw; ++idx)
                out[t * hw + idx] = gd_nbr_fraction_one(tab.data(), H, W, idx / W, idx % W, h, (double)scale * (double)scale, normalize);
        }
    });
    return 0;
}
