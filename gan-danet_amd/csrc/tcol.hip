// Triple collocation (include/gandanet.h, "Triple collocation"): the error variances, squared correlations with the unknown
// truth and scale factors of three collocated (T, M) cubes per pixel, and their moving-block bootstrap over time.  The
// per-step arithmetic, the finalising and the summaries are tcol_core.h, shared with the host twins.
//
// gd_tc_estimate: one thread per series, lanes along the pixels, so every step is one coalesced row read of each cube; two
// passes (the listwise means, then the nine sums).  Memory-bound.
// gd_tc_bootstrap, per chunk of pixels that the workspace holds, three kernels:
//   replicates  A workgroup owns G = gd_tc_group(T) neighbouring series (8 up to T = 340): it reads their 3 T G values as runs of
//               G elements (32- or 64-byte segments), one thread per pixel runs the mean recurrence over the staged values,
//               and the centred series stay in LDS as three arrays per pixel (24 T G bytes <= 64 KB), NaN marking a deleted
//               step.  A thread then runs whole replicates: the 64 lanes of a wave are neighbouring replicates b of ONE
//               pixel, so the index row idx[t, b .. b + 63] is one 128-byte read (the table sits in L2) and the LDS base is
//               wave-uniform; each step gathers u, v, w at the drawn time with three 8-byte LDS reads (random across the
//               lanes by construction) and adds them onto nine sums held in registers.  The eight statistics of the
//               replicate go to the workspace as (statistic, pixel of the chunk, b), consecutive lanes to consecutive
//               words, and to `replicates` when that is given.
//   quantiles   one wave per (pixel, statistic): the B values become sort keys in LDS (NaN as the pad key, padded to a
//               power of two), a bitonic sort runs there, and the lanes emit the Q quantiles (the LDS route of quantmap.hip).
//   moments     one thread per (pixel, statistic) runs the mean / std recurrence over ascending b.
// No atomics; a pixel's results depend on its series, the table and the parameters alone.
// From elem_util.h: gd_dtype_ok, gd_elem_aligned, gd_aligned, gd_with_dtype, gd_for_items, GD_S.
#include <stdio.h>

#include <vector>

#include "elem_util.h"
#include "tcol_core.h"

namespace {

constexpr int TC_THREADS = 256, TC_MAX_GROUP = 8, TC_LDS_BYTES = 65536, TC_WS_HEAD = 8;

// pixels per workgroup: the largest of 8, 4, 2, 1 whose staged series (3 T G doubles) and means (3 G doubles) fit 64 KB
inline int tc_group(long Tn) {
    if (Tn < 1 || Tn > GD_TC_MAX_T) return 0;
    int g = TC_MAX_GROUP;
    while (g > 1 && (size_t)(3 * Tn * g + 3 * g) * sizeof(double) > (size_t)TC_LDS_BYTES) g >>= 1;
    return g;
}
inline size_t tc_lds_bytes(long Tn, int G) { return (size_t)(3 * Tn * G + 3 * G) * sizeof(double); }
inline size_t tc_pixel_bytes(long B) { return (size_t)GD_TC_STATS * (size_t)B * sizeof(double); }

// ---- point estimate -----------------------------------------------------------------------------------------------------------
template <typename T> struct EstimateBody {
    const T *x, *y, *z;
    long Tn, M;
    int min_samples;
    const unsigned char* mask;
    double *stats, *cov;
    int *n, *flags;
    __host__ __device__ void operator()(long m) const {
        double st[GD_TC_STATS], cv[GD_TC_COVS];
        GdTcAcc acc = gd_tc_zero();
        int f;
        if (mask && mask[m] == 0) {                                   // not read: everything NaN, n = 0
            gd_tc_finish(acc, min_samples, st, cv);
            f = GD_TC_FLAG_MASKED;
        } else {
            int k = 0;
            double mx = 0.0, my = 0.0, mz = 0.0;
            for (long t = 0; t < Tn; ++t) gd_tc_mean_push(k, mx, my, mz, (double)x[t * M + m], (double)y[t * M + m], (double)z[t * M + m]);
            for (long t = 0; t < Tn; ++t) {
                double u, v, w;
                gd_tc_centre((double)x[t * M + m], (double)y[t * M + m], (double)z[t * M + m], mx, my, mz, u, v, w);
                gd_tc_add(acc, u, v, w);
            }
            f = gd_tc_finish(acc, min_samples, st, cv);
        }
#pragma unroll
        for (int k = 0; k < GD_TC_STATS; ++k) stats[(long)k * M + m] = st[k];
        if (cov) {
#pragma unroll
            for (int k = 0; k < GD_TC_COVS; ++k) cov[(long)k * M + m] = cv[k];
        }
        n[m] = acc.n;
        flags[m] = f;
    }
};

// ---- bootstrap: the index check -------------------------------------------------------------------------------------------------
struct IndexCheckBody {
    const uint16_t* idx;
    int Tn;
    int* bad;
    __host__ __device__ void operator()(long i) const {
        if ((int)idx[i] >= Tn) *bad = 1;                              // every writer stores the same word
    }
};

// ---- bootstrap: the replicates of one chunk [m_begin, m_end) -------------------------------------------------------------------
// grid: ceil((m_end - m_begin) / G) workgroups; dynamic LDS: tc_lds_bytes(Tn, G); ws: (GD_TC_STATS, m_end - m_begin, B)
template <typename T>
__global__ __launch_bounds__(TC_THREADS) void tc_replicate_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z,
                                                                   int Tn, long M, long m_begin, long m_end, int G,
                                                                   const uint16_t* __restrict__ idx, int B, int min_samples,
                                                                   const unsigned char* __restrict__ mask, double* __restrict__ ws,
                                                                   double* __restrict__ replicates) {
    extern __shared__ double tc_smem[];
    const int tid = (int)threadIdx.x;
    const int GT = G * Tn;
    double* su = tc_smem;                                             // [3][G][Tn]: x, y, z of pixel g, then u, v, w in place
    double* mean = tc_smem + 3 * GT;                                  // [3][G]
    const long m0 = m_begin + (long)blockIdx.x * G;
    const double nan = (double)NAN;

    // the raw values, element (c, t, g) by thread: G neighbouring pixels of one row are one 32- or 64-byte segment
    for (int i = tid; i < 3 * GT; i += TC_THREADS) {
        const int c = i / GT, r = i - c * GT, t = r / G, g = r - t * G;
        const long m = m0 + g;
        const T* src = c == 0 ? x : (c == 1 ? y : z);
        double val = nan;
        if (m < m_end && (!mask || mask[m] != 0)) val = (double)src[(long)t * M + m];
        su[(c * G + g) * Tn + t] = val;
    }
    __syncthreads();
    if (tid < G) {                                                    // the means of the ORIGINAL series, in time order
        int k = 0;
        double mx = 0.0, my = 0.0, mz = 0.0;
        const double *px = su + tid * Tn, *py = px + GT, *pz = py + GT;
        for (int t = 0; t < Tn; ++t) gd_tc_mean_push(k, mx, my, mz, px[t], py[t], pz[t]);
        mean[tid] = mx;
        mean[G + tid] = my;
        mean[2 * G + tid] = mz;
    }
    __syncthreads();
    for (int i = tid; i < GT; i += TC_THREADS) {                      // i = g * Tn + t
        const int g = i / Tn;
        double u, v, w;
        gd_tc_centre(su[i], su[GT + i], su[2 * GT + i], mean[g], mean[G + g], mean[2 * G + g], u, v, w);
        su[i] = u;
        su[GT + i] = v;
        su[2 * GT + i] = w;
    }
    __syncthreads();

    const int Bp = (B + 63) & ~63;                                    // a wave never straddles two pixels
    const long mc = m_end - m_begin;
    for (int item = tid; item < G * Bp; item += TC_THREADS) {
        const int g = __builtin_amdgcn_readfirstlane(item / Bp);
        const int b = item - g * Bp;
        const long m = m0 + g;
        if (b >= B || m >= m_end) continue;
        const double *pu = su + g * Tn, *pv = pu + GT, *pw = pv + GT;
        const uint16_t* col = idx + b;
        GdTcAcc acc = gd_tc_zero();
#pragma unroll 4
        for (int t = 0; t < Tn; ++t) {
            const int j = (int)col[(long)t * B];
            gd_tc_add(acc, pu[j], pv[j], pw[j]);
        }
        double st[GD_TC_STATS], cv[GD_TC_COVS];
        gd_tc_finish(acc, min_samples, st, cv);
        double* out = ws + (m - m_begin) * (long)B + b;
#pragma unroll
        for (int s = 0; s < GD_TC_STATS; ++s) out[(long)s * mc * B] = st[s];
        if (replicates) {
#pragma unroll
            for (int s = 0; s < GD_TC_STATS; ++s) replicates[((long)b * GD_TC_STATS + s) * M + m] = st[s];
        }
    }
}

// ---- bootstrap: the quantiles of one (statistic, pixel of the chunk) -----------------------------------------------------------
// one 64-thread workgroup per item i = s * mc + ml; P: the power of two >= max(B, 64); dynamic LDS: P keys
__global__ __launch_bounds__(64) void tc_quantile_kernel(const double* __restrict__ ws, int B, int P, long mc, long m_begin, long M,
                                                          const double* __restrict__ q, int Q, double* __restrict__ summary) {
    extern __shared__ int64_t tc_keys[];
    const int lane = (int)threadIdx.x;
    const long i = blockIdx.x;
    const int s = (int)(i / mc);
    const long m = m_begin + (i - (long)s * mc);
    const double* v = ws + i * (long)B;
    int cnt = 0;
    for (int k = lane; k < P; k += 64) {
        const double val = k < B ? v[k] : (double)NAN;
        const bool ok = val == val;
        tc_keys[k] = ok ? gd_qm_key(val) : GD_QM_PAD;
        cnt += ok;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = lane; p < (P >> 1); p += 64) {
                int lo, hi;
                bool up;
                gd_qm_bitonic_pair(p, k, j, lo, hi, up);
                const int64_t ka = tc_keys[lo], kb = tc_keys[hi];
                if (up ? kb < ka : ka < kb) {
                    tc_keys[lo] = kb;
                    tc_keys[hi] = ka;
                }
            }
            __syncthreads();
        }
    }
    double* out = summary + ((long)s * (2 + Q) + 2) * M + m;
    for (int j = lane; j < Q; j += 64) out[(long)j * M] = cnt >= 2 ? gd_tc_quantile(tc_keys, cnt, q[j]) : (double)NAN;
}

// ---- bootstrap: mean, std and n_ok of one (statistic, pixel of the chunk) ------------------------------------------------------
struct MomentBody {
    const double* ws;
    int B, Q;
    long mc, m_begin, M;
    double* summary;
    int* n_ok;
    __host__ __device__ void operator()(long i) const {
        const int s = (int)(i / mc);
        const long m = m_begin + (i - (long)s * mc);
        const double* v = ws + i * (long)B;
        int k = 0;
        double mu = 0.0, m2 = 0.0, mean, sd;
        for (int b = 0; b < B; ++b) gd_tc_moment_push(k, mu, m2, v[b]);
        gd_tc_moment_finish(k, mu, m2, mean, sd);
        double* out = summary + (long)s * (2 + Q) * M + m;
        out[0] = mean;
        out[M] = sd;
        n_ok[(long)s * M + m] = k;
    }
};

template <typename T>
int tc_bootstrap_device(const T* x, const T* y, const T* z, long Tn, long M, const uint16_t* idx, long B, int min_samples, const double* q,
                        int Q, const unsigned char* mask, double* summary, int* n_ok, double* replicates, double* ws, long chunk, hipStream_t st) {
    const int G = tc_group(Tn);
    int P = 64;
    while (P < B) P <<= 1;
    for (long m_begin = 0; m_begin < M; m_begin += chunk) {
        const long m_end = m_begin + chunk < M ? m_begin + chunk : M, mc = m_end - m_begin;
        hipLaunchKernelGGL(tc_replicate_kernel<T>, dim3((unsigned)((mc + G - 1) / G)), dim3(TC_THREADS), tc_lds_bytes(Tn, G), st, x, y, z, (int)Tn,
                           M, m_begin, m_end, G, idx, (int)B, min_samples, mask, ws, replicates);
        hipLaunchKernelGGL(tc_quantile_kernel, dim3((unsigned)(GD_TC_STATS * mc)), dim3(64), (size_t)P * sizeof(int64_t), st, ws, (int)B, P, mc,
                           m_begin, M, q, Q, summary);
        gd_for_items<TC_THREADS>(false, GD_TC_STATS * mc, st, MomentBody{ws, (int)B, Q, mc, m_begin, M, summary, n_ok});
        GD_LAUNCH_CHECK();
    }
    return 0;
}

// The host twin: the same staging, replicate, sort and recurrence code, one pixel at a time.
template <typename T>
void tc_bootstrap_host(const T* x, const T* y, const T* z, long Tn, long M, const uint16_t* idx, long B, int min_samples, const double* q, int Q,
                       const unsigned char* mask, double* summary, int* n_ok, double* replicates) {
    int P = 64;
    while (P < B) P <<= 1;
    std::vector<double> u((size_t)Tn), v((size_t)Tn), w((size_t)Tn), vals((size_t)GD_TC_STATS * (size_t)B);
    std::vector<int64_t> keys((size_t)P);
    const double nan = (double)NAN;
    for (long m = 0; m < M; ++m) {
        const bool live = !mask || mask[m] != 0;
        for (long t = 0; t < Tn; ++t) {
            u[t] = live ? (double)x[t * M + m] : nan;
            v[t] = live ? (double)y[t * M + m] : nan;
            w[t] = live ? (double)z[t * M + m] : nan;
        }
        int k = 0;
        double mx = 0.0, my = 0.0, mz = 0.0;
        for (long t = 0; t < Tn; ++t) gd_tc_mean_push(k, mx, my, mz, u[t], v[t], w[t]);
        for (long t = 0; t < Tn; ++t) gd_tc_centre(u[t], v[t], w[t], mx, my, mz, u[t], v[t], w[t]);
        for (long b = 0; b < B; ++b) {
            GdTcAcc acc = gd_tc_zero();
            for (long t = 0; t < Tn; ++t) {
                const int j = (int)idx[t * B + b];
                gd_tc_add(acc, u[j], v[j], w[j]);
            }
            double st[GD_TC_STATS], cv[GD_TC_COVS];
            gd_tc_finish(acc, min_samples, st, cv);
            for (int s = 0; s < GD_TC_STATS; ++s) {
                vals[(size_t)s * B + b] = st[s];
                if (replicates) replicates[(b * GD_TC_STATS + s) * M + m] = st[s];
            }
        }
        for (int s = 0; s < GD_TC_STATS; ++s) {
            MomentBody{vals.data(), (int)B, Q, 1, m, M, summary, n_ok}(s);
            int cnt = 0;
            for (int p = 0; p < P; ++p) {
                const double val = p < B ? vals[(size_t)s * B + p] : nan;
                const bool ok = val == val;
                keys[p] = ok ? gd_qm_key(val) : GD_QM_PAD;
                cnt += ok;
            }
            for (int kk = 2; kk <= P; kk <<= 1) {
                for (int j = kk >> 1; j > 0; j >>= 1) {
                    for (int p = 0; p < (P >> 1); ++p) {
                        int lo, hi;
                        bool up;
                        gd_qm_bitonic_pair(p, kk, j, lo, hi, up);
                        const int64_t ka = keys[lo], kb = keys[hi];
                        if (up ? kb < ka : ka < kb) {
                            keys[lo] = kb;
                            keys[hi] = ka;
                        }
                    }
                }
            }
            double* out = summary + ((long)s * (2 + Q) + 2) * M + m;
            for (int j = 0; j < Q; ++j) out[(long)j * M] = cnt >= 2 ? gd_tc_quantile(keys.data(), cnt, q[j]) : nan;
        }
    }
}

}  // namespace

// the checks an entry shares with its host twin
#define TC_ESTIMATE_CHECKS(fn)                                                                                             \
    GD_CHECK_ARG(x && y && z && stats && n && flags, fn ": null pointer");                                                \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                        \
    GD_CHECK_ARG(T >= 1 && T <= GD_TC_MAX_T, fn ": T outside 1..GD_TC_MAX_T");                                             \
    GD_CHECK_ARG(M > 0 && M < (1L << 31) / GD_TC_STATS, fn ": M <= 0 or too many series");                                \
    GD_CHECK_ARG(min_samples >= 3, fn ": min_samples < 3");                                                               \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_elem_aligned(y, dtype) && gd_elem_aligned(z, dtype) && gd_aligned(stats, 8) && \
                     gd_aligned(cov, 8) && gd_aligned(n, 4) && gd_aligned(flags, 4),                                      \
                 fn ": pointer not element aligned")

extern "C" int gd_tc_estimate(const void* x, const void* y, const void* z, int dtype, long T, long M, int min_samples, const unsigned char* mask,
                              double* stats, double* cov, int* n, int* flags, void* stream) {
    TC_ESTIMATE_CHECKS("gd_tc_estimate");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        gd_for_items<TC_THREADS>(false, M, GD_S, EstimateBody<E>{(const E*)x, (const E*)y, (const E*)z, T, M, min_samples, mask, stats, cov, n, flags});
    });
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_tc_estimate_host(const void* x, const void* y, const void* z, int dtype, long T, long M, int min_samples,
                                   const unsigned char* mask, double* stats, double* cov, int* n, int* flags) {
    TC_ESTIMATE_CHECKS("gd_tc_estimate_host");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        gd_for_items<TC_THREADS>(true, M, nullptr, EstimateBody<E>{(const E*)x, (const E*)y, (const E*)z, T, M, min_samples, mask, stats, cov, n, flags});
    });
    return 0;
}

extern "C" int gd_tc_group(long T) { return tc_group(T); }

extern "C" size_t gd_tc_bootstrap_workspace(long T, long M, long B) {
    const int G = tc_group(T);
    if (!G || M <= 0 || B < 1 || B > GD_TC_MAX_B) return 0;
    return (size_t)TC_WS_HEAD + (size_t)((M + G - 1) / G) * G * tc_pixel_bytes(B);
}

#define TC_BOOT_CHECKS(fn)                                                                                                 \
    GD_CHECK_ARG(x && y && z && idx && q && summary && n_ok, fn ": null pointer");                                        \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                        \
    GD_CHECK_ARG(T >= 1 && T <= GD_TC_MAX_T, fn ": T outside 1..GD_TC_MAX_T");                                             \
    GD_CHECK_ARG(M > 0 && M < (1L << 31) / GD_TC_STATS, fn ": M <= 0 or too many series");                                \
    GD_CHECK_ARG(B >= 1 && B <= GD_TC_MAX_B, fn ": B outside 1..GD_TC_MAX_B");                                             \
    GD_CHECK_ARG(Q >= 1 && Q <= GD_TC_MAX_Q, fn ": Q outside 1..GD_TC_MAX_Q");                                             \
    GD_CHECK_ARG(min_samples >= 3, fn ": min_samples < 3");                                                               \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_elem_aligned(y, dtype) && gd_elem_aligned(z, dtype) && gd_aligned(idx, 2) && \
                     gd_aligned(q, 8) && gd_aligned(summary, 8) && gd_aligned(n_ok, 4) && gd_aligned(replicates, 8),      \
                 fn ": pointer not element aligned")

extern "C" int gd_tc_bootstrap(const void* x, const void* y, const void* z, int dtype, long T, long M, const uint16_t* idx, long B,
                               int min_samples, const double* q, int Q, const unsigned char* mask, double* summary, int* n_ok,
                               double* replicates, void* workspace, size_t workspace_bytes, void* stream) {
    TC_BOOT_CHECKS("gd_tc_bootstrap");
    GD_CHECK_ARG(workspace && gd_aligned(workspace, 8), "gd_tc_bootstrap: workspace NULL or not 8-byte aligned");
    const int G = tc_group(T);
    const size_t group_bytes = (size_t)G * tc_pixel_bytes(B), least = (size_t)TC_WS_HEAD + group_bytes;
    if (workspace_bytes < least) {
        char msg[160];
        snprintf(msg, sizeof msg, "gd_tc_bootstrap: workspace of %zu bytes is smaller than one group of pixels, %zu bytes needed", workspace_bytes,
                 least);
        gd_set_error(msg);
        return -1;
    }
    // the index check: its verdict comes back before anything gathers through the table
    int* bad = (int*)workspace;
    int bad_host = 0;
    hipError_t e = hipMemsetAsync(bad, 0, TC_WS_HEAD, GD_S);
    if (e == hipSuccess) {
        gd_for_items<TC_THREADS, 1024>(false, T * B, GD_S, IndexCheckBody{idx, (int)T, bad});
        e = hipMemcpyAsync(&bad_host, bad, sizeof(int), hipMemcpyDeviceToHost, GD_S);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(GD_S);
    if (e != hipSuccess) {
        gd_set_error(hipGetErrorString(e));
        return -2;
    }
    GD_CHECK_ARG(bad_host == 0, "gd_tc_bootstrap: an index is >= T");
    long chunk = (long)((workspace_bytes - TC_WS_HEAD) / group_bytes) * G;
    chunk = chunk > M ? M : chunk;
    double* ws = (double*)((char*)workspace + TC_WS_HEAD);
    return gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        return tc_bootstrap_device((const E*)x, (const E*)y, (const E*)z, T, M, idx, B, min_samples, q, Q, mask, summary, n_ok, replicates, ws,
                                   chunk, GD_S);
    });
}

extern "C" int gd_tc_bootstrap_host(const void* x, const void* y, const void* z, int dtype, long T, long M, const uint16_t* idx, long B,
                                    int min_samples, const double* q, int Q, const unsigned char* mask, double* summary, int* n_ok,
                                    double* replicates) {
    TC_BOOT_CHECKS("gd_tc_bootstrap_host");
    for (int j = 0; j < Q; ++j) GD_CHECK_ARG(q[j] >= 0.0 && q[j] <= 1.0, "gd_tc_bootstrap_host: a probability is NaN or outside [0, 1]");
    for (long i = 0; i < T * B; ++i) GD_CHECK_ARG((long)idx[i] < T, "gd_tc_bootstrap_host: an index is >= T");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        tc_bootstrap_host((const E*)x, (const E*)y, (const E*)z, T, M, idx, B, min_samples, q, Q, mask, summary, n_ok, replicates);
    });
    return 0;
}
