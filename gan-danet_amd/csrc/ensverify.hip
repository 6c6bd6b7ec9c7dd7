// Ensemble verification (include/gandanet.h, "Ensemble verification"): CRPS, rank histogram, spread and error of an
// ensemble's members against the truth, per element and as one record of sums and counts.  The per-element arithmetic is
// ensverify_core.h, shared with the host twin.
//
// One lane owns one element and keeps the differences d_i = x_i - y of all M members in fp64 registers (MMAX = 8 or 32
// bounds the unrolled member loops and the width of the sorting network; the registers behind M hold +inf): dword loads,
// 256 contiguous bytes per wave and member.  A thread adds its float sums in registers in the order it meets its elements.
// The counts are integers: a thread counts n, ties and coverage in registers and adds them once to the workgroup's LDS
// counters, and every valid element adds 1 to its rank bin in one of 16 LDS copies of the histogram (thread & 15; 33 bins
// apart, so the copies of a bin lie in different banks).  Integer adds commute, so their order cannot matter.  The float
// sums go through gd_block_sum_d (a fixed tree inside a wave, the waves ascending), every workgroup writes one partial
// record to the workspace, and one wave adds the partials in ascending order, lane f the field f.  No global atomics, no
// float atomics: the same call gives the same bits, and the host twin, which walks the same grid, gives them too.
#include <algorithm>
#include <vector>

#include "elem_util.h"
#include "ensverify_core.h"

#pragma clang fp contract(off)

namespace {

constexpr int ENSV_COPIES = 16;
constexpr int ENSV_WAVES = GD_ENSV_THREADS / 64;

template <typename T> __host__ __device__ inline T ensv_nan();
template <> __host__ __device__ inline float ensv_nan<float>() { return __builtin_nanf(""); }
template <> __host__ __device__ inline double ensv_nan<double>() { return __builtin_nan(""); }

template <typename T, int MMAX, bool MASK>
__global__ __launch_bounds__(GD_ENSV_THREADS) void ens_verify_kernel(const T* __restrict__ x, int M, long mstride, const T* __restrict__ y,
                                                                     long planes, long hw, const unsigned char* __restrict__ mask,
                                                                     double scale, int fair, T* __restrict__ crps_map,
                                                                     T* __restrict__ err_map, T* __restrict__ spread_map,
                                                                     unsigned char* __restrict__ rank_map, double* __restrict__ ws) {
    __shared__ unsigned hist[ENSV_COPIES][GD_ENSV_BINS];
    __shared__ unsigned cnt[6];                        // n, ties, the four coverage counts
    __shared__ double red[ENSV_WAVES][GD_ENSV_SUMS];
    const int tid = threadIdx.x;
    for (int k = tid; k < ENSV_COPIES * GD_ENSV_BINS; k += GD_ENSV_THREADS) (&hist[0][0])[k] = 0u;
    if (tid < 6) cnt[tid] = 0u;
    __syncthreads();

    double acc[GD_ENSV_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    unsigned c_n = 0, c_t = 0, c_c[4] = {0, 0, 0, 0};
    unsigned* my_hist = hist[tid & (ENSV_COPIES - 1)];
    for (long pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        for (long i = (long)blockIdx.x * GD_ENSV_THREADS + tid; i < hw; i += (long)gridDim.x * GD_ENSV_THREADS) {
            const long at = pl * hw + i;
            const double yv = (double)y[at];
            bool valid = (MASK ? mask[i] != 0 : true) && yv == yv;
            double d[MMAX];
#pragma unroll
            for (int m = 0; m < MMAX; ++m) {
                d[m] = (double)INFINITY;
                if (m < M) {
                    d[m] = (double)x[(long)m * mstride + at] - yv;
                    valid = valid && d[m] == d[m];
                }
            }
            gd_ensv_sort<MMAX>(d);
            GdEnsvElem r;
            gd_ensv_elem<MMAX>(d, M, fair != 0, scale, r);
            acc[0] += valid ? r.crps : 0.0;
            acc[1] += valid ? r.crps_gauss : 0.0;
            acc[2] += valid ? r.abs_e : 0.0;
            acc[3] += valid ? r.e2 : 0.0;
            acc[4] += valid ? r.s2 : 0.0;
            if (valid) {
                c_n += 1u;
                c_t += r.ties > 0 ? 1u : 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) c_c[k] += (unsigned)(r.cover >> k) & 1u;
                atomicAdd(&my_hist[r.bin], 1u);
            }
            if (crps_map) crps_map[at] = valid ? (T)r.crps : ensv_nan<T>();
            if (err_map) err_map[at] = valid ? (T)r.e : ensv_nan<T>();
            if (spread_map) spread_map[at] = valid ? (T)r.s : ensv_nan<T>();
            if (rank_map) rank_map[at] = valid ? (unsigned char)r.bin : (unsigned char)255;
        }
    }
    atomicAdd(&cnt[0], c_n);
    atomicAdd(&cnt[1], c_t);
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicAdd(&cnt[2 + k], c_c[k]);
    gd_block_sum_d<GD_ENSV_SUMS, ENSV_WAVES>(acc, red);
    __syncthreads();                                   // every LDS add of the workgroup has landed
    double* out = ws + (long)GD_ENSV_REC * ((long)blockIdx.y * gridDim.x + blockIdx.x);
    if (tid == 0) {
        out[GD_ENSV_N] = (double)cnt[0];
        out[GD_ENSV_TIED] = (double)cnt[1];
#pragma unroll
        for (int k = 0; k < GD_ENSV_SUMS; ++k) out[GD_ENSV_CRPS + k] = acc[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) out[GD_ENSV_COVER + k] = (double)cnt[2 + k];
    }
    if (tid >= 64 && tid < 64 + GD_ENSV_BINS) {        // the second wave adds the copies of one bin each
        const int b = tid - 64;
        unsigned s = 0;
#pragma unroll
        for (int c = 0; c < ENSV_COPIES; ++c) s += hist[c][b];
        out[GD_ENSV_HIST + b] = (double)s;
    }
}

// Stage 2 (one wave): lane f adds field f of the partial records in ascending order
__global__ __launch_bounds__(64) void ens_verify_final_kernel(const double* __restrict__ ws, int nparts, double* __restrict__ rec) {
    const int f = threadIdx.x;
    if (f >= GD_ENSV_REC) return;
    double s = 0.0;
    for (int p = 0; p < nparts; ++p) s += ws[(long)p * GD_ENSV_REC + f];
    rec[f] = s;
}

template <typename T, int MMAX>
static void ensv_launch_m(const T* x, int M, long mstride, const T* y, long planes, long hw, const unsigned char* mask, double scale,
                          int fair, T* crps_map, T* err_map, T* spread_map, unsigned char* rank_map, double* ws, GdEnsvGrid g, hipStream_t s) {
    const dim3 grid(g.gx, g.gy), blk(GD_ENSV_THREADS);
    if (mask)
        hipLaunchKernelGGL((ens_verify_kernel<T, MMAX, true>), grid, blk, 0, s, x, M, mstride, y, planes, hw, mask, scale, fair, crps_map,
                           err_map, spread_map, rank_map, ws);
    else
        hipLaunchKernelGGL((ens_verify_kernel<T, MMAX, false>), grid, blk, 0, s, x, M, mstride, y, planes, hw, mask, scale, fair, crps_map,
                           err_map, spread_map, rank_map, ws);
}

template <typename T>
static void ensv_launch(const void* x, int M, long mstride, const void* y, long planes, long hw, const unsigned char* mask, double scale,
                        int fair, void* crps_map, void* err_map, void* spread_map, unsigned char* rank_map, double* ws, GdEnsvGrid g,
                        hipStream_t s) {
    if (M <= 8)
        ensv_launch_m<T, 8>((const T*)x, M, mstride, (const T*)y, planes, hw, mask, scale, fair, (T*)crps_map, (T*)err_map, (T*)spread_map,
                            rank_map, ws, g, s);
    else
        ensv_launch_m<T, 32>((const T*)x, M, mstride, (const T*)y, planes, hw, mask, scale, fair, (T*)crps_map, (T*)err_map,
                             (T*)spread_map, rank_map, ws, g, s);
}

// The host twin walks the grid of the device: the elements of thread (bx, by, tid) in the thread's order, the 64 lanes of
// a wave along the butterfly of gd_wave_sum_d, the waves and then the workgroups ascending.  The sorted differences come
// from std::sort.
template <typename T>
static void ensv_host(const T* x, int M, long mstride, const T* y, long planes, long hw, const unsigned char* mask, double scale, bool fair,
                      double* rec, T* crps_map, T* err_map, T* spread_map, unsigned char* rank_map) {
    const GdEnsvGrid g = gd_ensv_grid(planes, hw);
    for (int f = 0; f < GD_ENSV_REC; ++f) rec[f] = 0.0;
    std::vector<double> acc((size_t)GD_ENSV_THREADS * GD_ENSV_SUMS), nxt(acc.size());
    for (int by = 0; by < g.gy; ++by) {
        for (int bx = 0; bx < g.gx; ++bx) {
            double part[GD_ENSV_REC] = {0.0};
            std::fill(acc.begin(), acc.end(), 0.0);
            for (int tid = 0; tid < GD_ENSV_THREADS; ++tid) {
                double* a = &acc[(size_t)tid * GD_ENSV_SUMS];
                for (long pl = by; pl < planes; pl += g.gy) {
                    for (long i = (long)bx * GD_ENSV_THREADS + tid; i < hw; i += (long)g.gx * GD_ENSV_THREADS) {
                        const long at = pl * hw + i;
                        const double yv = (double)y[at];
                        bool valid = (mask ? mask[i] != 0 : true) && yv == yv;
                        double d[32];
                        for (int m = 0; m < M; ++m) {
                            d[m] = (double)x[(long)m * mstride + at] - yv;
                            valid = valid && d[m] == d[m];
                        }
                        GdEnsvElem r;
                        if (valid) {
                            std::sort(d, d + M);
                            gd_ensv_elem<32>(d, M, fair, scale, r);
                            a[0] += r.crps;
                            a[1] += r.crps_gauss;
                            a[2] += r.abs_e;
                            a[3] += r.e2;
                            a[4] += r.s2;
                            part[GD_ENSV_N] += 1.0;
                            part[GD_ENSV_TIED] += r.ties > 0 ? 1.0 : 0.0;
                            for (int k = 0; k < 4; ++k) part[GD_ENSV_COVER + k] += (double)((r.cover >> k) & 1);
                            part[GD_ENSV_HIST + r.bin] += 1.0;
                        }
                        if (crps_map) crps_map[at] = valid ? (T)r.crps : ensv_nan<T>();
                        if (err_map) err_map[at] = valid ? (T)r.e : ensv_nan<T>();
                        if (spread_map) spread_map[at] = valid ? (T)r.s : ensv_nan<T>();
                        if (rank_map) rank_map[at] = valid ? (unsigned char)r.bin : (unsigned char)255;
                    }
                }
            }
            for (int w = 0; w < ENSV_WAVES; ++w) {                 // gd_wave_sum_d: v[l] += v[l ^ o], o = 32 .. 1
                for (int o = 32; o > 0; o >>= 1) {
                    for (int l = 0; l < 64; ++l)
                        for (int k = 0; k < GD_ENSV_SUMS; ++k)
                            nxt[(size_t)(w * 64 + l) * GD_ENSV_SUMS + k] =
                                acc[(size_t)(w * 64 + l) * GD_ENSV_SUMS + k] + acc[(size_t)(w * 64 + (l ^ o)) * GD_ENSV_SUMS + k];
                    std::copy(nxt.begin() + (size_t)w * 64 * GD_ENSV_SUMS, nxt.begin() + (size_t)(w + 1) * 64 * GD_ENSV_SUMS,
                              acc.begin() + (size_t)w * 64 * GD_ENSV_SUMS);
                }
            }
            for (int k = 0; k < GD_ENSV_SUMS; ++k) {
                double s = acc[k];
                for (int w = 1; w < ENSV_WAVES; ++w) s += acc[(size_t)w * 64 * GD_ENSV_SUMS + k];
                part[GD_ENSV_CRPS + k] = s;
            }
            for (int f = 0; f < GD_ENSV_REC; ++f) rec[f] += part[f];
        }
    }
}

}  // namespace

// the checks an entry shares with its host twin
#define ENSV_CHECKS(fn)                                                                                                        \
    GD_CHECK_ARG(x && y && rec, fn ": null pointer");                                                                          \
    GD_CHECK_ARG(planes > 0 && hw > 0, fn ": n <= 0");                                                                         \
    GD_CHECK_ARG(M >= 1 && M <= GD_ENSV_MAX_M, fn ": M outside 1..32");                                                        \
    GD_CHECK_ARG(M == 1 || member_stride >= planes * hw, fn ": member stride smaller than n");                                 \
    GD_CHECK_ARG(scale - scale == 0.0 && scale > 0.0, fn ": scale is not finite and positive");                                \
    GD_CHECK_ARG((flags & ~(GD_ENSV_F64 | GD_ENSV_FAIR)) == 0, fn ": unknown flag");                                           \
    GD_CHECK_ARG(!(flags & GD_ENSV_FAIR) || M > 1, fn ": the fair CRPS needs M >= 2");                                         \
    const int f64 = flags & GD_ENSV_F64;                                                                                       \
    GD_CHECK_ARG(gd_elem_aligned(x, f64) && gd_elem_aligned(y, f64) && gd_aligned(rec, 8) && gd_elem_aligned(crps_map, f64) && \
                     gd_elem_aligned(err_map, f64) && gd_elem_aligned(spread_map, f64),                                        \
                 fn ": pointer not element aligned")

extern "C" size_t gd_ens_verify_ws_bytes(long n) {
    if (n <= 0) return 0;
    // the partial count depends on how the planes are cut; GD_ENSV_BLOCKS records cover every cut
    return (size_t)GD_ENSV_BLOCKS * GD_ENSV_REC * sizeof(double);
}

extern "C" int gd_ens_verify(const void* x, int M, long member_stride, const void* y, long planes, long hw, const unsigned char* mask,
                             double scale, int flags, double* rec, void* crps_map, void* err_map, void* spread_map,
                             unsigned char* rank_map, void* ws, size_t ws_bytes, void* stream) {
    ENSV_CHECKS("gd_ens_verify");
    GD_CHECK_ARG(ws, "gd_ens_verify: null pointer");
    GD_CHECK_ARG(gd_aligned(ws, 8), "gd_ens_verify: pointer not element aligned");
    GD_CHECK_ARG(ws_bytes >= gd_ens_verify_ws_bytes(planes * hw), "gd_ens_verify: workspace smaller than gd_ens_verify_ws_bytes");
    if (!mask) {   // nothing repeats per plane: one plane of n elements
        hw *= planes;
        planes = 1;
    }
    const GdEnsvGrid g = gd_ensv_grid(planes, hw);
    const int fair = (flags & GD_ENSV_FAIR) ? 1 : 0;
    gd_with_dtype(f64 ? GD_FILTER_F64 : GD_FILTER_F32, [&](auto zero) {
        ensv_launch<decltype(zero)>(x, M, member_stride, y, planes, hw, mask, scale, fair, crps_map, err_map, spread_map, rank_map, (double*)ws,
                                    g, GD_S);
    });
    hipLaunchKernelGGL(ens_verify_final_kernel, dim3(1), dim3(64), 0, GD_S, (const double*)ws, g.gx * g.gy, rec);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_ens_verify_host(const void* x, int M, long member_stride, const void* y, long planes, long hw, const unsigned char* mask,
                                  double scale, int flags, double* rec, void* crps_map, void* err_map, void* spread_map,
                                  unsigned char* rank_map) {
    ENSV_CHECKS("gd_ens_verify_host");
    if (!mask) {
        hw *= planes;
        planes = 1;
    }
    const bool fair = (flags & GD_ENSV_FAIR) != 0;
    gd_with_dtype(f64 ? GD_FILTER_F64 : GD_FILTER_F32, [&](auto zero) {
        using E = decltype(zero);
        ensv_host((const E*)x, M, member_stride, (const E*)y, planes, hw, mask, scale, fair, rec, (E*)crps_map, (E*)err_map, (E*)spread_map,
                  rank_map);
    });
    return 0;
}

// Host only.  Adds k records in the given order and derives the metrics.
extern "C" int gd_ens_verify_merge_host(const double* recs, long k, int M, double* rec_out, double* metrics) {
    GD_CHECK_ARG(metrics, "gd_ens_verify_merge_host: null pointer");
    GD_CHECK_ARG(k >= 0 && (recs || k == 0), "gd_ens_verify_merge_host: k records but no pointer");
    GD_CHECK_ARG(M >= 1 && M <= GD_ENSV_MAX_M, "gd_ens_verify_merge_host: M outside 1..32");
    double r[GD_ENSV_REC] = {0.0};
    for (long i = 0; i < k; ++i)
        for (int f = 0; f < GD_ENSV_REC; ++f) r[f] += recs[i * GD_ENSV_REC + f];
    if (rec_out)
        for (int f = 0; f < GD_ENSV_REC; ++f) rec_out[f] = r[f];
    const double n = r[GD_ENSV_N];
    if (!(n > 0)) {
        for (int f = 0; f < GD_ENSV_METRICS; ++f) metrics[f] = NAN;
        return 0;
    }
    const double rmse = sqrt(r[GD_ENSV_E2] / n), spread = sqrt(r[GD_ENSV_S2] / n);
    metrics[GD_ENSV_M_CRPS] = r[GD_ENSV_CRPS] / n;
    metrics[GD_ENSV_M_CRPS_GAUSS] = r[GD_ENSV_CRPS_GAUSS] / n;
    metrics[GD_ENSV_M_MAE] = r[GD_ENSV_ABS_E] / n;
    metrics[GD_ENSV_M_RMSE] = rmse;
    metrics[GD_ENSV_M_SPREAD] = spread;
    metrics[GD_ENSV_M_SPREAD_SKILL] = (M > 1 && rmse > 0.0) ? sqrt((double)(M + 1) / (double)M) * spread / rmse : (double)NAN;
    for (int c = 0; c < 4; ++c) metrics[GD_ENSV_M_COVER + c] = r[GD_ENSV_COVER + c] / n;
    double rel = 0.0;
    for (int b = 0; b < GD_ENSV_BINS; ++b) {
        const double f = r[GD_ENSV_HIST + b] / n;
        metrics[GD_ENSV_M_HIST + b] = f;
        if (b <= M) rel += fabs(f - 1.0 / (double)(M + 1));
    }
    metrics[GD_ENSV_M_RELIABILITY] = rel;
    metrics[GD_ENSV_M_TIED] = r[GD_ENSV_TIED] / n;
    return 0;
}
