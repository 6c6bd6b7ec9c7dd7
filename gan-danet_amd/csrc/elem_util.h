// Shared host and device plumbing of the analysis kernels (evalstats, gradguard, filters, spline, prepare, basins, stl,
// series, trend, ensverify, eof, spectra, drought, ccl, neighborhood, quantmap, lagcorr, tcol): the fp32 / fp64 dtype tag, its alignment
// checks and its dispatch (gd_with_dtype: stl, series, trend, ensverify, eof, spectra, drought, ccl, neighborhood, quantmap,
// lagcorr, tcol),
// 16-byte vector access with a scalar head and tail, launch-grid sizing, the one-thread-per-item launcher with its host twin
// (gd_for_items: series, eof, drought, ccl, quantmap, lagcorr, tcol), and the fixed-order fp64 reductions.  The training-path kernels do
// not include this file.
#pragma once
#include "common.h"
#include "../../include/gandanet.h"

// ---- dtype tag (GD_FILTER_F32 / GD_FILTER_F64), pointers, streams --------------------------------------------------------
static inline bool gd_dtype_ok(int d) { return d == GD_FILTER_F32 || d == GD_FILTER_F64; }
static inline bool gd_aligned(const void* p, int bytes) { return ((uintptr_t)p % bytes) == 0; }
static inline bool gd_elem_aligned(const void* p, int dtype) { return gd_aligned(p, dtype ? 8 : 4); }
#define GD_S ((hipStream_t)stream)   // inside an entry point: its `void* stream` argument as the HIP stream

// f(T{}) with T the element type of the tag (host only): gd_with_dtype(dtype, [&](auto zero) { using T = decltype(zero); ... })
template <class F> static inline auto gd_with_dtype(int dtype, F&& f) {
    if (dtype == GD_FILTER_F64) return f(double{});
    return f(float{});
}

// elements of T from `p` up to the next 16-byte boundary (p is element aligned)
template <typename T> __host__ __device__ inline long gd_head_of(const T* p) {
    const unsigned long mis = (unsigned long)(uintptr_t)p & 15ul;
    return mis ? (long)((16ul - mis) / sizeof(T)) : 0;
}

// one 16-byte access: W consecutive elements of T at a 16-byte aligned address, widened or narrowed on the way
template <typename T> struct gd_vec16;
template <> struct gd_vec16<float> {
    typedef float4 type;
    static constexpr int W = 4;
    template <typename O> __device__ __forceinline__ static void unpack(const float4& v, O* o) {
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
    template <typename O> __device__ __forceinline__ static void load(const float* p, O* o) {
        unpack(*reinterpret_cast<const float4*>(p), o);
    }
    __device__ __forceinline__ static void store(float* p, const double* o) {
        *reinterpret_cast<float4*>(p) = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
    }
};
template <> struct gd_vec16<double> {
    typedef double2 type;
    static constexpr int W = 2;
    template <typename O> __device__ __forceinline__ static void unpack(const double2& v, O* o) { o[0] = v.x; o[1] = v.y; }
    template <typename O> __device__ __forceinline__ static void load(const double* p, O* o) {
        unpack(*reinterpret_cast<const double2*>(p), o);
    }
    __device__ __forceinline__ static void store(double* p, const double* o) {
        *reinterpret_cast<double2*>(p) = make_double2(o[0], o[1]);
    }
};

// ---- launch grids --------------------------------------------------------------------------------------------------------
// workgroups of a grid-stride kernel over n items: one item per thread up to `cap` workgroups
static inline int gd_stream_grid(long n, int threads, long cap) {
    const long g = (n + threads - 1) / threads;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
// workgroups per plane of a (gx, planes) reduction grid, one per `elems_per_block` elements of a plane, at most 64 and
// about 2048 over all planes (they fill the chip): a function of the shape alone, the partials' order is part of the result
static inline int gd_plane_gx(long planes, long hw, int elems_per_block) {
    long gx = (hw + elems_per_block - 1) / elems_per_block;
    long cap = 2048 / planes;
    cap = cap < 1 ? 1 : cap;
    gx = gx > cap ? cap : gx;
    return (int)(gx < 1 ? 1 : (gx > 64 ? 64 : gx));
}

// ---- one thread per item --------------------------------------------------------------------------------------------------
// body(i) for every i in [0, n): `Body` is a plain struct of an entry's arguments whose __host__ __device__ operator()(long)
// holds the one per-item call, so the device kernel and the host twin (host = true: a loop on the calling thread, `st` is
// not used) unpack the arguments in the same line.  CAP = 0: gd_cdiv(n, THREADS) workgroups, a thread per item; CAP > 0: a
// grid-stride loop on gd_stream_grid(n, THREADS, CAP) workgroups.
template <int THREADS, long CAP, class Body> __global__ __launch_bounds__(THREADS) void gd_item_kernel(long n, Body body) {
    const long i0 = (long)blockIdx.x * THREADS + threadIdx.x;
    if constexpr (CAP > 0) {
        for (long i = i0; i < n; i += (long)gridDim.x * THREADS) body(i);
    } else {
        if (i0 < n) body(i0);
    }
}
template <int THREADS, long CAP = 0, class Body> static inline void gd_for_items(bool host, long n, hipStream_t st, Body body) {
    if (host) {
        for (long i = 0; i < n; ++i) body(i);
        return;
    }
    const int grid = CAP > 0 ? gd_stream_grid(n, THREADS, CAP) : gd_cdiv(n, THREADS);
    hipLaunchKernelGGL((gd_item_kernel<THREADS, CAP, Body>), dim3(grid), dim3(THREADS), 0, st, n, body);
}

// ---- fp64 reductions in a fixed order ------------------------------------------------------------------------------------
__device__ __forceinline__ double gd_shfl_down_d(double v, int o) { return __shfl_down(v, o, 64); }

// Sums of K doubles over a 1-D block of NW waves, valid in thread 0: every value goes through gd_wave_sum_d, lane 0 of
// wave w leaves its sums in red[w], and thread 0 adds the rows 1 .. NW - 1 in ascending order onto its own wave's sums.
// All threads of the block must call it (it holds a barrier); `red` is LDS.
template <int K, int NW> __device__ __forceinline__ void gd_block_sum_d(double (&v)[K], double (*red)[K]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = gd_wave_sum_d(v[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; ++w) {
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] += red[w][k];
        }
    }
}
