// STL decomposition (include/gandanet.h, "STL decomposition"): detrend_and_compare of the reference's datasets.py, which
// runs statsmodels' STL(y, seasonal=13, period=12).fit() once per grid point in a Python double loop, for all series of a
// (T, M) array in one launch.  The arithmetic is stl_core.h, shared with the host twin gd_stl_decompose_host.
//
// A workgroup of 256 threads owns S neighbouring series (S from T and the period alone, so that four workgroups fit the
// LDS of a CU where a series allows it).  Their six working arrays live in LDS as images [t][S]: the S series of a group
// are S consecutive doubles of a row of the input, and lanes that hold neighbouring (point, series) pairs read
// neighbouring 8-byte words of LDS (a window clamped at an end of the series is one address for several lanes: a
// broadcast).  Every step of the fit hands its (series, output point) pairs to the threads round-robin, a barrier between
// steps; a pair's value is computed by one thread from start to end in an order fixed by (T, parameters), so a series'
// result depends on nothing but the series: not on M, its place in the group, or the launch.  No global atomics, no
// workspace.  The order statistics behind the robustness weights are found by counting ranks in LDS.
// From elem_util.h: gd_dtype_ok, gd_elem_aligned, GD_S.
#include "elem_util.h"
#include "stl_core.h"

#include <vector>

namespace {

constexpr int STL_THREADS = 256;
constexpr long STL_LDS_TARGET = 40960;    // a quarter of a CU's 160 KiB
constexpr long STL_LDS_MAX = 160 * 1024;
constexpr int STL_MAX_GROUP = 16;

// series per workgroup: as many as fit STL_LDS_TARGET, at least one (GD_STL_MAX_T keeps one series inside STL_LDS_MAX)
static int stl_group(long n, long np) {
    const long per = gd_stl_work_doubles(n, np, 1) * (long)sizeof(double);
    const long s = STL_LDS_TARGET / per;
    return (int)(s < 1 ? 1 : (s > STL_MAX_GROUP ? STL_MAX_GROUP : s));
}

struct DeviceExec {
    template <class F> __device__ __forceinline__ void each(int count, F f) const {
        for (int idx = threadIdx.x; idx < count; idx += STL_THREADS) f(idx);
        __syncthreads();
    }
};
struct HostExec {
    template <class F> void each(int count, F f) const {
        for (int idx = 0; idx < count; ++idx) f(idx);
    }
};

template <typename T>
__global__ __launch_bounds__(STL_THREADS) void stl_kernel(const T* __restrict__ x, long M, GdStlParams P, int S, T* __restrict__ trend,
                                                          T* __restrict__ seasonal, T* __restrict__ resid, T* __restrict__ weights) {
    extern __shared__ double stl_lds[];
    GdStlWork A;
    gd_stl_carve(stl_lds, P.n, P.np, S, &A);
    const int tid = threadIdx.x, n = P.n;
    const long m0 = (long)blockIdx.x * S;
    const int ms = M - m0 < S ? (int)(M - m0) : S;   // series of this group; the columns beyond hold zeros and are not stored
    for (int idx = tid; idx < n * S; idx += STL_THREADS) {
        const int t = idx / S, s = idx - t * S;
        A.y[idx] = s < ms ? (double)x[(long)t * M + m0 + s] : 0.0;
        A.tr[idx] = 0.0;
        A.rw[idx] = 1.0;
    }
    if (tid < 2 * S) A.sel[tid] = 0.0;
    __syncthreads();
    gd_stl_fit(DeviceExec{}, A, P);
    for (int idx = tid; idx < n * S; idx += STL_THREADS) {
        const int t = idx / S, s = idx - t * S;
        if (s >= ms) continue;
        const long g = (long)t * M + m0 + s;
        const double y = A.y[idx], se = A.w3[idx], tr = A.tr[idx];
        trend[g] = (T)tr;
        seasonal[g] = (T)se;
        resid[g] = (T)(y - se - tr);
        if (weights) weights[g] = (T)A.rw[idx];
    }
}

template <typename T>
static int stl_launch(const T* x, long M, const GdStlParams& P, T* trend, T* seasonal, T* resid, T* weights, hipStream_t st) {
    const int S = stl_group(P.n, P.np);
    const size_t bytes = (size_t)gd_stl_work_doubles(P.n, P.np, S) * sizeof(double);
    if (bytes > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&stl_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)bytes);
        if (e != hipSuccess) {
            gd_set_error(hipGetErrorString(e));
            return -2;
        }
    }
    hipLaunchKernelGGL(stl_kernel<T>, dim3((unsigned)((M + S - 1) / S)), dim3(STL_THREADS), bytes, st, x, M, P, S, trend, seasonal, resid,
                       weights);
    GD_LAUNCH_CHECK();
    return 0;
}

template <typename T>
static void stl_host(const T* x, long M, const GdStlParams& P, T* trend, T* seasonal, T* resid, T* weights) {
    std::vector<double> buf((size_t)gd_stl_work_doubles(P.n, P.np, 1));
    GdStlWork A;
    gd_stl_carve(buf.data(), P.n, P.np, 1, &A);
    for (long m = 0; m < M; ++m) {
        for (int t = 0; t < P.n; ++t) {
            A.y[t] = (double)x[(long)t * M + m];
            A.tr[t] = 0.0;
            A.rw[t] = 1.0;
        }
        A.sel[0] = A.sel[1] = 0.0;
        gd_stl_fit(HostExec{}, A, P);
        for (int t = 0; t < P.n; ++t) {
            const long g = (long)t * M + m;
            trend[g] = (T)A.tr[t];
            seasonal[g] = (T)A.w3[t];
            resid[g] = (T)(A.y[t] - A.w3[t] - A.tr[t]);
            if (weights) weights[g] = (T)A.rw[t];
        }
    }
}

static bool odd3(int v) { return v >= 3 && (v & 1); }

}  // namespace

// the checks gd_stl_decompose and its host twin share
#define STL_CHECKS(fn)                                                                                                       \
    GD_CHECK_ARG(x && trend_out && seasonal_out && resid_out, fn ": null pointer");                                        \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                         \
    GD_CHECK_ARG(T > 0 && M > 0, fn ": T <= 0 or M <= 0");                                                                  \
    GD_CHECK_ARG(period >= 2, fn ": period < 2");                                                                           \
    GD_CHECK_ARG(odd3(seasonal), fn ": seasonal must be an odd integer >= 3");                                             \
    GD_CHECK_ARG(odd3(trend), fn ": trend must be an odd integer >= 3");                                                   \
    GD_CHECK_ARG(odd3(low_pass), fn ": low_pass must be an odd integer >= 3");                                             \
    GD_CHECK_ARG(trend > period, fn ": trend must be larger than the period");                                             \
    GD_CHECK_ARG(low_pass > period, fn ": low_pass must be larger than the period");                                       \
    GD_CHECK_ARG((seasonal_deg | 1) == 1 && (trend_deg | 1) == 1 && (low_pass_deg | 1) == 1, fn ": a degree outside {0, 1}"); \
    GD_CHECK_ARG(inner_iter >= 1, fn ": inner_iter < 1");                                                                   \
    GD_CHECK_ARG(outer_iter >= 0, fn ": outer_iter < 0");                                                                   \
    GD_CHECK_ARG(T <= GD_STL_MAX_T, fn ": T above GD_STL_MAX_T");                                                          \
    GD_CHECK_ARG(T >= 2L * period, fn ": T < 2 * period");                                                                  \
    GD_CHECK_ARG(M < (1L << 31) && M < (1L << 53) / T, fn ": too many series");                                             \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_elem_aligned(trend_out, dtype) && gd_elem_aligned(seasonal_out, dtype) &&  \
                     gd_elem_aligned(resid_out, dtype) && gd_elem_aligned(weights_out, dtype),                               \
                 fn ": pointer not element aligned");                                                                        \
    const GdStlParams P = {(int)T, period, seasonal, trend, low_pass, seasonal_deg, trend_deg, low_pass_deg, inner_iter, outer_iter}

extern "C" int gd_stl_decompose(const void* x, int dtype, long T, long M, int period, int seasonal, int trend, int low_pass,
                                int seasonal_deg, int trend_deg, int low_pass_deg, int inner_iter, int outer_iter, void* trend_out,
                                void* seasonal_out, void* resid_out, void* weights_out, void* stream) {
    STL_CHECKS("gd_stl_decompose");
    static_assert(gd_stl_work_doubles(GD_STL_MAX_T, GD_STL_MAX_T / 2, 1) * 8 <= STL_LDS_MAX, "one series at the cap must fit the LDS");
    return gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        return stl_launch((const E*)x, M, P, (E*)trend_out, (E*)seasonal_out, (E*)resid_out, (E*)weights_out, GD_S);
    });
}

// Host only, no GPU call: the same fit (stl_core.h) in plain loops, series after series, every pointer in HOST memory.
extern "C" int gd_stl_decompose_host(const void* x, int dtype, long T, long M, int period, int seasonal, int trend, int low_pass,
                                     int seasonal_deg, int trend_deg, int low_pass_deg, int inner_iter, int outer_iter, void* trend_out,
                                     void* seasonal_out, void* resid_out, void* weights_out) {
    STL_CHECKS("gd_stl_decompose_host");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        stl_host((const E*)x, M, P, (E*)trend_out, (E*)seasonal_out, (E*)resid_out, (E*)weights_out);
    });
    return 0;
}
