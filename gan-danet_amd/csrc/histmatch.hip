// mild_histogram_matching of the inference notebook (test.ipynb c1:69-85) on the device, per sample:
//   s_vals, bin_idx, s_counts = np.unique(source);  t_vals, t_counts = np.unique(reference)
//   s_q = cumsum(s_counts) / sum;  t_q = cumsum(t_counts) / sum            (float64)
//   matched = np.interp(s_q, t_q, t_vals)[bin_idx]
//   adjusted = (1 - weight) * source + weight * matched                     (float64 result)
// Restated on sorted arrays instead of unique ones: for an element of value v, s_q = (#source elements <= v) / n_s
// = upper_bound(v) / n_s; the unique target value of rank j ends its run at a position e_j of the sorted target and
// t_q[j] = e_j / n_t, so np.interp's bracket [t_q[j], t_q[j+1]) is found by locating the largest run end e with
// e / n_t <= s_q.  All quantiles are the same IEEE double divisions numpy performs, so the bracket decisions are
// identical.  Sorting: hipcub::DeviceRadixSort (rocPRIM) -- the one library primitive of this file.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <utility>
#include <vector>

#include "common.h"
#include "histmatch_core.h"
#include "../../include/gandanet.h"

namespace {

__global__ void iota_kernel(unsigned int* idx, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) idx[i] = (unsigned int)i;
}

// the sort keys of one sample: every NaN becomes the positive quiet NaN, which the radix sort's bit order puts last
__global__ void keys_kernel(const float* __restrict__ src, float* __restrict__ keys, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) keys[i] = gd_hm_key(src[i]);
}

__global__ __launch_bounds__(256) void hist_match_kernel(const float* __restrict__ skeys, const unsigned int* __restrict__ sidx,
                                                        long ns, const float* __restrict__ tkeys, long nt, double weight,
                                                        double* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < ns; i += (long)gridDim.x * 256)
        out[sidx[i]] = gd_hm_element(skeys, ns, tkeys, nt, weight, i);
}

}  // namespace

// workspace: source keys (NaNs made positive) and sorted source keys, indices (in and out), sorted target keys + the radix
// sort's own temp
static size_t sort_temp_bytes(long ns, long nt) {
    size_t a = 0, b = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const float*)nullptr, (float*)nullptr, (const unsigned int*)nullptr,
                                       (unsigned int*)nullptr, (int)ns);
    hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const float*)nullptr, (float*)nullptr, (int)nt);
    return a > b ? a : b;
}
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" size_t gd_hist_match_ws_bytes(long ns, long nt) {
    if (ns <= 0 || nt <= 0 || ns > 0x7fffffffL || nt > 0x7fffffffL) return 0;
    return align256(ns * 4) * 4 + align256(nt * 4) + align256(sort_temp_bytes(ns, nt)) + 256;
}

extern "C" int gd_hist_match(const float* src, const float* ref, int B, long ns, long nt, double weight, double* out,
                             void* ws, size_t ws_bytes, void* stream) {
    GD_CHECK_ARG(src && ref && out && ws && B > 0 && ns > 0 && nt > 0, "gd_hist_match: bad arguments");
    GD_CHECK_ARG(ns <= 0x7fffffffL && nt <= 0x7fffffffL, "gd_hist_match: samples of more than 2^31 elements");
    GD_CHECK_ARG(ws_bytes >= gd_hist_match_ws_bytes(ns, nt), "gd_hist_match: workspace smaller than gd_hist_match_ws_bytes");
    hipStream_t s = (hipStream_t)stream;
    char* p = (char*)(((size_t)ws + 255) & ~(size_t)255);
    float* kin = (float*)p;             p += align256(ns * 4);
    float* skeys = (float*)p;           p += align256(ns * 4);
    unsigned int* iidx = (unsigned int*)p;  p += align256(ns * 4);
    unsigned int* sidx = (unsigned int*)p;  p += align256(ns * 4);
    float* tkeys = (float*)p;           p += align256(nt * 4);
    size_t temp = sort_temp_bytes(ns, nt);
    void* tmp = p;
    const dim3 grid(gd_cdiv(ns, 256) > 2048 ? 2048 : gd_cdiv(ns, 256));
    hipLaunchKernelGGL(iota_kernel, grid, dim3(256), 0, s, iidx, ns);
    for (int b = 0; b < B; ++b) {
        hipLaunchKernelGGL(keys_kernel, grid, dim3(256), 0, s, src + (long)b * ns, kin, ns);
        if (hipcub::DeviceRadixSort::SortPairs(tmp, temp, kin, skeys, iidx, sidx, (int)ns, 0, 32, s) != hipSuccess ||
            hipcub::DeviceRadixSort::SortKeys(tmp, temp, ref + (long)b * nt, tkeys, (int)nt, 0, 32, s) != hipSuccess) {
            gd_set_error("gd_hist_match: radix sort failed");
            return -2;
        }
        hipLaunchKernelGGL(hist_match_kernel, grid, dim3(256), 0, s, skeys, sidx, ns, tkeys, nt, weight, out + (long)b * ns);
    }
    GD_LAUNCH_CHECK();
    return 0;
}

// Host twin: a stable sort of (key, index) pairs in the key order of histmatch_core.h, then the same per-element function.
extern "C" int gd_hist_match_host(const float* src, const float* ref, int B, long ns, long nt, double weight, double* out) {
    GD_CHECK_ARG(src && ref && out && B > 0 && ns > 0 && nt > 0, "gd_hist_match_host: bad arguments");
    GD_CHECK_ARG(ns <= 0x7fffffffL && nt <= 0x7fffffffL, "gd_hist_match_host: samples of more than 2^31 elements");
    std::vector<std::pair<float, unsigned int>> pairs((size_t)ns);
    std::vector<float> skeys((size_t)ns), tkeys((size_t)nt);
    for (int b = 0; b < B; ++b) {
        const float* sb = src + (long)b * ns;
        for (long i = 0; i < ns; ++i) pairs[(size_t)i] = {gd_hm_key(sb[i]), (unsigned int)i};
        std::stable_sort(pairs.begin(), pairs.end(),
                         [](const std::pair<float, unsigned int>& x, const std::pair<float, unsigned int>& y) { return gd_hm_less(x.first, y.first); });
        for (long i = 0; i < ns; ++i) skeys[(size_t)i] = pairs[(size_t)i].first;
        std::copy(ref + (long)b * nt, ref + (long)(b + 1) * nt, tkeys.begin());
        std::stable_sort(tkeys.begin(), tkeys.end(), gd_hm_less);
        double* ob = out + (long)b * ns;
        for (long i = 0; i < ns; ++i) ob[pairs[(size_t)i].second] = gd_hm_element(skeys.data(), ns, tkeys.data(), nt, weight, i);
    }
    return 0;
}
