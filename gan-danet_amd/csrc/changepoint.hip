// Per-pixel change points (include/gandanet.h, "Per-pixel change points"): the Pettitt test, Buishand's CUSUM statistics and
// the two least-squares two-segment fits (a shift of the mean; two separate lines) for every series of a (T, M) cube.  The
// per-sample arithmetic, the selection rules and the finishing formulas are changepoint_core.h, shared with the host twin.
//
// One wave owns one series (a workgroup is one wave), launched like trend_kernel.  The valid (t, y, i) of the series'
// window sit in LDS, compacted in time order.  A lane owns the candidates k = lane, lane + 64, ...; the loop over the
// samples j is the same for every lane: sample j is read from LDS at one address (a broadcast) and joins the lane's "before"
// or "after" sums by the predicate j <= k, so the O(n^2) sweeps have no divergent trip counts and every sum runs in time
// order.  One more slot after the last candidate is the whole series (k = n - 1, everything "before"): its sums are rss0.
//   Pettitt  V_k is an integer count over all j, U_k an integer wave scan of V_k with a carry from chunk to chunk;
//   CUSUM    O(n) and sequential by definition: lane 0 walks the series;
//   STEP     two sweeps per chunk of candidates (sums; squared deviations);
//   TREND    three (sums; stt and sty; residuals).
// The arg-max and arg-min are wave reductions over (value, k) pairs under the tie rules of changepoint_core.h; the lane that
// owns the winning k writes its planes.  No global atomics, no workspace; a series' result depends on the series and the
// parameters alone.
#include <climits>
#include <vector>

#include "changepoint_core.h"
#include "elem_util.h"

namespace {

constexpr int CP_LANES = 64;

// bytes of LDS of one series: t and y as doubles, then the index of every sample among the T steps
static inline size_t cp_lds_bytes(long T) { return (2 * sizeof(double) + sizeof(int)) * (size_t)T; }

// ---- the planes of one family of one series ---------------------------------------------------------------------------------
__host__ __device__ inline void cp_put_pettitt(double* out, long M, long m, double k, double u, double index, double p) {
    out[GD_CP_PT_K * M + m] = k;
    out[GD_CP_PT_U * M + m] = u;
    out[GD_CP_PT_INDEX * M + m] = index;
    out[GD_CP_PT_P * M + m] = p;
}
__host__ __device__ inline void cp_put_cusum(double* out, long M, long m, const GdCpCusum& c, double index) {
    out[GD_CP_CS_Q * M + m] = c.q;
    out[GD_CP_CS_R * M + m] = c.r;
    out[GD_CP_CS_INDEX * M + m] = index;
    out[GD_CP_CS_P * M + m] = c.p;
}
__host__ __device__ inline void cp_put_step(double* out, long M, long m, int n, double index, double m1, double m2, double rss0, double rss) {
#pragma clang fp contract(off)
    out[GD_CP_ST_INDEX * M + m] = index;
    out[GD_CP_ST_MEAN_BEFORE * M + m] = m1;
    out[GD_CP_ST_MEAN_AFTER * M + m] = m2;
    out[GD_CP_ST_SHIFT * M + m] = m2 - m1;
    out[GD_CP_ST_RSS0 * M + m] = rss0;
    out[GD_CP_ST_RSS * M + m] = rss;
    out[GD_CP_ST_F * M + m] = gd_cp_f_step(rss0, rss, n);
}
__host__ __device__ inline void cp_put_step_none(double* out, long M, long m) {
    const double nan = (double)NAN;
    for (int p = GD_CP_ST_INDEX; p <= GD_CP_ST_F; ++p) out[p * M + m] = p == GD_CP_ST_INDEX ? -1.0 : nan;
}
// tk, tk1: the times of the last sample before and the first after the break
__host__ __device__ inline void cp_put_trend(double* out, long M, long m, int n, double index, const GdCpLine& l1, const GdCpLine& l2, double tk,
                                             double tk1, double rss0, double rss) {
    const double a1 = gd_cp_intercept(l1.ybar, l1.b, l1.tbar), a2 = gd_cp_intercept(l2.ybar, l2.b, l2.tbar);
    out[GD_CP_TR_INDEX * M + m] = index;
    out[GD_CP_TR_SLOPE_BEFORE * M + m] = l1.b;
    out[GD_CP_TR_SLOPE_AFTER * M + m] = l2.b;
    out[GD_CP_TR_INTERCEPT_BEFORE * M + m] = a1;
    out[GD_CP_TR_INTERCEPT_AFTER * M + m] = a2;
    out[GD_CP_TR_JUMP * M + m] = gd_cp_jump(a1, l1.b, a2, l2.b, tk, tk1);
    out[GD_CP_TR_RSS0 * M + m] = rss0;
    out[GD_CP_TR_RSS * M + m] = rss;
    out[GD_CP_TR_F * M + m] = gd_cp_f_trend(rss0, rss, n);
}
__host__ __device__ inline void cp_put_trend_none(double* out, long M, long m) {
    const double nan = (double)NAN;
    for (int p = GD_CP_TR_INDEX; p <= GD_CP_TR_F; ++p) out[p * M + m] = p == GD_CP_TR_INDEX ? -1.0 : nan;
}

// ---- the fit of one slot: the candidate k (j <= k is "before"), or the whole series at k = n - 1 ------------------------------
// STEP: the two means and the two sums of squares, two passes over the samples in time order
__host__ __device__ inline void cp_step_fit(const double* sy, int n, int k, double& m1, double& m2, double& r1, double& r2) {
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < n; ++j) gd_cp_add(s1, s2, j <= k, sy[j]);
    m1 = gd_cp_mean(s1, k + 1);
    m2 = gd_cp_mean(s2, n - k - 1);
    r1 = r2 = 0.0;
    for (int j = 0; j < n; ++j) gd_cp_add_sq(r1, r2, j <= k, sy[j], m1, m2);
}
// TREND: the two lines, three passes
__host__ __device__ inline void cp_trend_fit(const double* st, const double* sy, int n, int k, GdCpLine& l1, GdCpLine& l2) {
    gd_cp_line_zero(l1);
    gd_cp_line_zero(l2);
    for (int j = 0; j < n; ++j) gd_cp_line_pass1(l1, l2, j <= k, st[j], sy[j]);
    gd_cp_line_means(l1, k + 1);
    gd_cp_line_means(l2, n - k - 1);
    for (int j = 0; j < n; ++j) gd_cp_line_pass2(l1, l2, j <= k, st[j], sy[j]);
    gd_cp_line_slope(l1);
    gd_cp_line_slope(l2);
    for (int j = 0; j < n; ++j) gd_cp_line_pass3(l1, l2, j <= k, st[j], sy[j]);
}

__device__ __forceinline__ int cp_wave_scan_i(int v, int lane) {   // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}
// the (value, k) pair that is ahead of all others of the wave, in every lane
__device__ __forceinline__ void cp_wave_argmin(double& v, int& k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int ok = __shfl_xor(k, o, 64);
        if (gd_cp_ahead_min(ov, ok, v, k)) {
            v = ov;
            k = ok;
        }
    }
}
__device__ __forceinline__ void cp_wave_argmax(int& v, int& k, int& u) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ov = __shfl_xor(v, o, 64), ok = __shfl_xor(k, o, 64), ou = __shfl_xor(u, o, 64);
        if (gd_cp_ahead_max(ov, ok, v, k)) {
            v = ov;
            k = ok;
            u = ou;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(CP_LANES) void cp_kernel(const T* __restrict__ x, int Tn, long M, const double* __restrict__ times,
                                                      const unsigned char* __restrict__ mask, const int* __restrict__ window, int min_seg,
                                                      int flags, double* __restrict__ out) {
    extern __shared__ double cp_smem[];
    double* st = cp_smem;
    double* sy = st + Tn;
    int* si = reinterpret_cast<int*>(sy + Tn);
    const long m = blockIdx.x;
    const int lane = threadIdx.x;
    const double nan = (double)NAN;

    // ---- the valid samples of the window into LDS, in time order (a masked series keeps none) -----------------------------
    int n = 0;
    if (!(mask && mask[m] == 0)) {
        int b = 0, e = Tn;
        if (window) gd_cp_window(window[m], window[M + m], Tn, &b, &e);
        for (int k0 = b; k0 < e; k0 += CP_LANES) {
            const int k = k0 + lane;
            const double v = k < e ? (double)x[(long)k * M + m] : nan;
            const bool ok = v == v;
            const unsigned long long bal = __ballot(ok);
            if (ok) {
                const int pos = n + __popcll(bal & ((1ull << lane) - 1));
                sy[pos] = v;
                st[pos] = times[k];
                si[pos] = k;
            }
            n += __popcll(bal);
        }
    }
    __syncthreads();
    if (lane == 0) out[GD_CP_N * M + m] = (double)n;

    // ---- Pettitt -----------------------------------------------------------------------------------------------------------
    if (flags & GD_CP_PETTITT) {
        if (n < 2) {
            if (lane == 0) cp_put_pettitt(out, M, m, nan, nan, -1.0, nan);
        } else {
            int carry = 0, best = -1, bk = INT_MAX, bu = 0;
            for (int k0 = 0; k0 < n - 1; k0 += CP_LANES) {
                const int k = k0 + lane;
                const bool row = k < n - 1;
                const double yk = row ? sy[k] : 0.0;
                int v = 0;
                for (int j = 0; j < n; ++j) v += gd_cp_sign(yk, sy[j]);
                const int u = carry + cp_wave_scan_i(row ? v : 0, lane);
                carry = __shfl(u, CP_LANES - 1, 64);
                const int a = u < 0 ? -u : u;
                if (row && gd_cp_ahead_max(a, k, best, bk)) {
                    best = a;
                    bk = k;
                    bu = u;
                }
            }
            cp_wave_argmax(best, bk, bu);
            if (lane == 0) cp_put_pettitt(out, M, m, (double)best, (double)bu, (double)si[bk], gd_cp_pettitt_p(best, n));
        }
    }

    // ---- CUSUM: sequential, one lane -----------------------------------------------------------------------------------------
    if ((flags & GD_CP_CUSUM) && lane == 0) {
        GdCpCusum c;
        c.q = c.r = c.p = nan;
        c.k = -1;
        if (n >= 1) c = gd_cp_cusum(sy, n);
        cp_put_cusum(out, M, m, c, c.k < 0 ? -1.0 : (double)si[c.k]);
    }

    // ---- the fitted models: the slots c = 0 .. nc - 1 are the candidates k = kmin + c, slot nc is the whole series ---------
    const int kmin = min_seg - 1, nc = n - 2 * min_seg + 1;
    if (flags & GD_CP_STEP) {
        if (nc <= 0) {
            if (lane == 0) cp_put_step_none(out, M, m);
        } else {
            double brss = nan, bm1 = nan, bm2 = nan, rss0 = nan;
            int bk = INT_MAX;
            for (int c0 = 0; c0 <= nc; c0 += CP_LANES) {
                const int c = c0 + lane;
                const int k = c < nc ? kmin + c : n - 1;
                double m1, m2, r1, r2;
                cp_step_fit(sy, n, k, m1, m2, r1, r2);
                const double rss = gd_cp_rss(r1, r2);
                if (c == nc) rss0 = r1;
                if (c < nc && (bk == INT_MAX ? rss == rss : gd_cp_ahead_min(rss, k, brss, bk))) {
                    brss = rss;
                    bk = k;
                    bm1 = m1;
                    bm2 = m2;
                }
            }
            rss0 = __shfl(rss0, nc & (CP_LANES - 1), 64);
            const int mine = bk;
            double wrss = bk == INT_MAX ? (double)INFINITY : brss;
            cp_wave_argmin(wrss, bk);
            if (bk == INT_MAX) {
                if (lane == 0) cp_put_step_none(out, M, m);
            } else if (mine == bk) {
                cp_put_step(out, M, m, n, (double)si[bk], bm1, bm2, rss0, brss);
            }
        }
    }
    if (flags & GD_CP_TREND) {
        if (nc <= 0) {
            if (lane == 0) cp_put_trend_none(out, M, m);
        } else {
            GdCpLine b1, b2;
            gd_cp_line_zero(b1);
            gd_cp_line_zero(b2);
            double brss = nan, rss0 = nan;
            int bk = INT_MAX;
            for (int c0 = 0; c0 <= nc; c0 += CP_LANES) {
                const int c = c0 + lane;
                const int k = c < nc ? kmin + c : n - 1;
                GdCpLine l1, l2;
                cp_trend_fit(st, sy, n, k, l1, l2);
                const double rss = gd_cp_rss(l1.rss, l2.rss);
                if (c == nc) rss0 = l1.rss;
                if (c < nc && (bk == INT_MAX ? rss == rss : gd_cp_ahead_min(rss, k, brss, bk))) {
                    brss = rss;
                    bk = k;
                    b1 = l1;
                    b2 = l2;
                }
            }
            rss0 = __shfl(rss0, nc & (CP_LANES - 1), 64);
            const int mine = bk;
            double wrss = bk == INT_MAX ? (double)INFINITY : brss;
            cp_wave_argmin(wrss, bk);
            if (bk == INT_MAX) {
                if (lane == 0) cp_put_trend_none(out, M, m);
            } else if (mine == bk) {
                cp_put_trend(out, M, m, n, (double)si[bk], b1, b2, st[bk], st[bk + 1], rss0, brss);
            }
        }
    }
}

template <typename T>
static void cp_launch(const T* x, long Tn, long M, const double* times, const unsigned char* mask, const int* window, int min_seg, int flags,
                      double* out, hipStream_t st) {
    hipLaunchKernelGGL((cp_kernel<T>), dim3((unsigned)M), dim3(CP_LANES), cp_lds_bytes(Tn), st, x, (int)Tn, M, times, mask, window, min_seg,
                       flags, out);
}

// The host twin: the same fits of the same slots in ascending order of k, the same selection rules, one series at a time.
template <typename T>
static void cp_host_one(const T* x, long Tn, long M, long m, const double* times, bool masked, const int* window, int min_seg, int flags,
                        double* out) {
    const double nan = (double)NAN;
    std::vector<double> t, y;
    std::vector<int> idx;
    if (!masked) {
        int b = 0, e = (int)Tn;
        if (window) gd_cp_window(window[m], window[M + m], (int)Tn, &b, &e);
        for (int k = b; k < e; ++k) {
            const double v = (double)x[(long)k * M + m];
            if (v == v) {
                y.push_back(v);
                t.push_back(times[k]);
                idx.push_back(k);
            }
        }
    }
    const int n = (int)y.size();
    out[GD_CP_N * M + m] = (double)n;
    if (flags & GD_CP_PETTITT) {
        if (n < 2) {
            cp_put_pettitt(out, M, m, nan, nan, -1.0, nan);
        } else {
            int u = 0, best = -1, bk = INT_MAX, bu = 0;
            for (int k = 0; k < n - 1; ++k) {
                int v = 0;
                for (int j = 0; j < n; ++j) v += gd_cp_sign(y[k], y[j]);
                u += v;
                const int a = u < 0 ? -u : u;
                if (gd_cp_ahead_max(a, k, best, bk)) {
                    best = a;
                    bk = k;
                    bu = u;
                }
            }
            cp_put_pettitt(out, M, m, (double)best, (double)bu, (double)idx[bk], gd_cp_pettitt_p(best, n));
        }
    }
    if (flags & GD_CP_CUSUM) {
        GdCpCusum c;
        c.q = c.r = c.p = nan;
        c.k = -1;
        if (n >= 1) c = gd_cp_cusum(y.data(), n);
        cp_put_cusum(out, M, m, c, c.k < 0 ? -1.0 : (double)idx[c.k]);
    }
    const int kmin = min_seg - 1, nc = n - 2 * min_seg + 1;
    if (flags & GD_CP_STEP) {
        double brss = nan, bm1 = nan, bm2 = nan, m1, m2, r1, r2;
        int bk = INT_MAX;
        for (int c = 0; c < nc; ++c) {
            const int k = kmin + c;
            cp_step_fit(y.data(), n, k, m1, m2, r1, r2);
            const double rss = gd_cp_rss(r1, r2);
            if (bk == INT_MAX ? rss == rss : gd_cp_ahead_min(rss, k, brss, bk)) {
                brss = rss;
                bk = k;
                bm1 = m1;
                bm2 = m2;
            }
        }
        if (bk == INT_MAX) {
            cp_put_step_none(out, M, m);
        } else {
            cp_step_fit(y.data(), n, n - 1, m1, m2, r1, r2);
            cp_put_step(out, M, m, n, (double)idx[bk], bm1, bm2, r1, brss);
        }
    }
    if (flags & GD_CP_TREND) {
        GdCpLine b1, b2, l1, l2;
        double brss = nan;
        int bk = INT_MAX;
        for (int c = 0; c < nc; ++c) {
            const int k = kmin + c;
            cp_trend_fit(t.data(), y.data(), n, k, l1, l2);
            const double rss = gd_cp_rss(l1.rss, l2.rss);
            if (bk == INT_MAX ? rss == rss : gd_cp_ahead_min(rss, k, brss, bk)) {
                brss = rss;
                bk = k;
                b1 = l1;
                b2 = l2;
            }
        }
        if (bk == INT_MAX) {
            cp_put_trend_none(out, M, m);
        } else {
            cp_trend_fit(t.data(), y.data(), n, n - 1, l1, l2);
            cp_put_trend(out, M, m, n, (double)idx[bk], b1, b2, t[bk], t[bk + 1], l1.rss, brss);
        }
    }
}

}  // namespace

// the checks an entry shares with its host twin
#define CP_CHECKS(fn)                                                                                                     \
    GD_CHECK_ARG(x && times && out, fn ": null pointer");                                                                \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                       \
    GD_CHECK_ARG(T >= 2 && T <= GD_CP_MAX_T, fn ": T outside 2..GD_CP_MAX_T");                                            \
    GD_CHECK_ARG(M > 0 && M < (1L << 31), fn ": M <= 0 or too many series");                                              \
    GD_CHECK_ARG(min_seg >= 2 && min_seg <= GD_CP_MAX_T, fn ": min_seg outside 2..GD_CP_MAX_T");                          \
    GD_CHECK_ARG((flags & ~(GD_CP_PETTITT | GD_CP_CUSUM | GD_CP_STEP | GD_CP_TREND)) == 0, fn ": unknown flag");          \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(times, 8) && gd_aligned(out, 8) && gd_aligned(window, 4),        \
                 fn ": pointer not element aligned")

extern "C" int gd_change_point(const void* x, int dtype, long T, long M, const double* times, const unsigned char* mask, const int* window,
                               int min_seg, int flags, double* out, void* stream) {
    CP_CHECKS("gd_change_point");
    gd_with_dtype(dtype, [&](auto zero) { cp_launch((const decltype(zero)*)x, T, M, times, mask, window, min_seg, flags, out, GD_S); });
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_change_point_host(const void* x, int dtype, long T, long M, const double* times, const unsigned char* mask,
                                    const int* window, int min_seg, int flags, double* out) {
    CP_CHECKS("gd_change_point_host");
    for (long k = 0; k < T; ++k)
        GD_CHECK_ARG(times[k] - times[k] == 0.0 && (k == 0 || times[k] > times[k - 1]),
                     "gd_change_point_host: times are not finite and strictly increasing");
    gd_with_dtype(dtype, [&](auto zero) {
        for (long m = 0; m < M; ++m)
            cp_host_one((const decltype(zero)*)x, T, M, m, times, mask && mask[m] == 0, window, min_seg, flags, out);
    });
    return 0;
}
