// Per-pixel trend tests (include/gandanet.h, "Per-pixel trend tests"): the Mann-Kendall test and the Theil-Sen slope with
// its confidence interval for every series of a (T, M) cube, plain or seasonal (Hirsch-Slack).  The per-pair arithmetic and
// the finalising formulas are trend_core.h, shared with the host twin.
//
// One wave owns one series (a workgroup is one wave).  The valid (t, y) samples sit in LDS as fp64, compacted in time order
// -- season by season in the seasonal form, so the pairs that count are those inside one contiguous segment.  A lane owns
// the rows i = lane, lane + 64, ... and walks the offset k, which is the same for every lane: sample i + k is read from LDS
// at 64 consecutive addresses, free of bank conflicts.  Everything accumulated is an integer, so the order of the wave
// reductions cannot matter:
//   count sweep   every row against every sample of its segment: the less-than and equal counts (the rank of y_i, hence
//                 median(y), and the tie counts c_i) and the sign sum over j > i;
//   select sweeps over the pairs i < j of a segment; each recomputes the slopes and counts one 8-bit digit of their monotone
//                 64-bit keys into LDS histograms (integer adds, which commute), one histogram for each distinct prefix among
//                 the up to four wanted ranks; a rank whose bin holds a single slope reads that slope off in the next sweep
//                 and is done.  Nothing proportional to T^2 is stored anywhere.
// No global atomics, no workspace; a series' result depends on the series and the parameters alone.
#include <algorithm>
#include <vector>

#include "elem_util.h"
#include "trend_core.h"

namespace {

constexpr int TR_LANES = 64;
constexpr int TR_DIGIT = 8, TR_BINS = 1 << TR_DIGIT, TR_RANKS = 4;

// bytes of LDS of one series: t and y, the two medians' order statistics, the captured keys, then the histograms (SEN), the
// segment bounds of every sample and the season counters (seasonal form)
static inline size_t trend_lds_bytes(long T, int period, int flags) {
    size_t b = 16 * (size_t)T + 4 * sizeof(double) + TR_RANKS * sizeof(uint64_t);
    if (flags & GD_TREND_SEN) b += TR_RANKS * TR_BINS * sizeof(unsigned);
    if (period) b += 4 * (size_t)T + 4 * (size_t)period;
    return b;
}

// the planes of one series; slope .. slope_hi only where they were asked for
__host__ __device__ inline void trend_put(double* out, long M, long m, int flags, long long n, long long s, const GdTrendStats& r,
                                          double slope, double icpt, double lo, double hi) {
    out[GD_TREND_N * M + m] = (double)n;
    out[GD_TREND_S * M + m] = (double)s;
    out[GD_TREND_VAR_S * M + m] = r.var_s;
    out[GD_TREND_Z * M + m] = r.z;
    out[GD_TREND_P * M + m] = r.p;
    out[GD_TREND_TAU * M + m] = r.tau;
    if (flags & GD_TREND_SEN) {
        out[GD_TREND_SLOPE * M + m] = slope;
        out[GD_TREND_INTERCEPT * M + m] = icpt;
    }
    if (flags & GD_TREND_CI) {
        out[GD_TREND_SLOPE_LO * M + m] = lo;
        out[GD_TREND_SLOPE_HI * M + m] = hi;
    }
}

// a series with fewer than two valid samples (or masked out, n = 0): n, s = 0, NaN elsewhere
__host__ __device__ inline void trend_put_empty(double* out, long M, long m, int flags, long long n) {
    const double nan = (double)NAN;
    GdTrendStats r;
    r.var_s = r.z = r.p = r.tau = nan;
    r.nt = 0;
    trend_put(out, M, m, flags, n, 0, r, nan, nan, nan, nan);
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_scan_u(unsigned v, int lane) {   // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// The bin of a 256-bin histogram that holds rank r (0-based, r < the histogram's total): its digit, the count below it and
// its own count, the same in every lane.  A lane scans four neighbouring bins.
__device__ __forceinline__ void hist_pick(const unsigned* h, unsigned r, int lane, unsigned& digit, unsigned& below, unsigned& count) {
    const uint4 a = *reinterpret_cast<const uint4*>(h + 4 * lane);
    const unsigned sum = a.x + a.y + a.z + a.w;
    const unsigned inc = wave_scan_u(sum, lane);
    unsigned e = inc - sum, c, d;
    const unsigned long long hit = __ballot(e <= r && r < inc);
    const int src = hit ? __ffsll((long long)hit) - 1 : 0;
    if (r < e + a.x) { d = 0; c = a.x; }
    else {
        e += a.x;
        if (r < e + a.y) { d = 1; c = a.y; }
        else {
            e += a.y;
            if (r < e + a.z) { d = 2; c = a.z; }
            else { e += a.z; d = 3; c = a.w; }
        }
    }
    digit = __shfl(4u * lane + d, src, 64);
    below = __shfl(e, src, 64);
    count = __shfl(c, src, 64);
}

template <typename T, bool SEAS>
__global__ __launch_bounds__(TR_LANES) void trend_kernel(const T* __restrict__ x, int Tn, long M, const double* __restrict__ times, int period,
                                                         const unsigned char* __restrict__ mask, int flags, double zq,
                                                         double* __restrict__ out) {
    extern __shared__ double trend_smem[];
    double* st = trend_smem;
    double* sy = st + Tn;
    double* med = sy + Tn;                                            // y and t at the ranks (n - 1) / 2 and n / 2
    unsigned long long* res = reinterpret_cast<unsigned long long*>(med + 4);
    unsigned* hist = reinterpret_cast<unsigned*>(res + TR_RANKS);
    unsigned* seg = hist + ((flags & GD_TREND_SEN) ? TR_RANKS * TR_BINS : 0);   // seasonal: lo | hi << 16 of the sample's segment
    int* sc = reinterpret_cast<int*>(seg + Tn);                       // seasonal: a counter per season
    const long m = blockIdx.x;
    const int lane = threadIdx.x;
    const bool sen = (flags & GD_TREND_SEN) != 0, ci = (flags & GD_TREND_CI) != 0;
    const double nan = (double)NAN;

    if (mask && mask[m] == 0) {
        if (lane == 0) trend_put_empty(out, M, m, flags, 0);
        return;
    }

    // ---- the valid samples into LDS, in time order; seasonal: season by season, time order inside a season ----------------
    int n = 0;
    if constexpr (!SEAS) {
        for (int k0 = 0; k0 < Tn; k0 += TR_LANES) {
            const int k = k0 + lane;
            const double v = k < Tn ? (double)x[(long)k * M + m] : nan;
            const bool ok = v == v;
            const unsigned long long b = __ballot(ok);
            if (ok) {
                const int pos = n + __popcll(b & ((1ull << lane) - 1));
                sy[pos] = v;
                st[pos] = times[k];
            }
            n += __popcll(b);
        }
    } else {
        for (int s = lane; s < period; s += TR_LANES) sc[s] = 0;
        __syncthreads();
        for (int k0 = 0; k0 < Tn; k0 += TR_LANES) {
            const int k = k0 + lane;
            const double v = k < Tn ? (double)x[(long)k * M + m] : nan;
            const bool ok = v == v;
            if (ok) atomicAdd(&sc[k % period], 1);
            n += __popcll(__ballot(ok));
        }
        __syncthreads();
        int carry = 0;                                                // counts -> where each season starts
        for (int s0 = 0; s0 < period; s0 += TR_LANES) {
            const int s = s0 + lane;
            const unsigned c = s < period ? (unsigned)sc[s] : 0u;
            const unsigned inc = wave_scan_u(c, lane);
            if (s < period) sc[s] = carry + (int)(inc - c);
            carry += (int)__shfl(inc, 63, 64);
        }
        __syncthreads();
        for (int k0 = 0; k0 < Tn; k0 += TR_LANES) {
            const int k = k0 + lane;
            const double v = k < Tn ? (double)x[(long)k * M + m] : nan;
            const bool ok = v == v;
            const unsigned long long b = __ballot(ok);
            const int s = k % period;
            int before = 0;                                           // valid samples of this season earlier in the chunk
            for (int l = lane - period; l >= 0; l -= period) before += (int)((b >> l) & 1ull);
            const int base = ok ? sc[s] : 0;
            __syncthreads();
            if (ok) {
                const int pos = base + before;
                sy[pos] = v;
                st[pos] = times[k];
                seg[pos] = (unsigned)s;
                atomicAdd(&sc[s], 1);
            }
            __syncthreads();
        }
        for (int i = lane; i < n; i += TR_LANES) {                    // sc[s] is now the end of season s
            const int s = (int)seg[i];
            seg[i] = (unsigned)(s ? sc[s - 1] : 0) | ((unsigned)sc[s] << 16);
        }
    }
    __syncthreads();
    if (n < 2) {
        if (lane == 0) trend_put_empty(out, M, m, flags, n);
        return;
    }

    // ---- count sweep -------------------------------------------------------------------------------------------------------
    const int r0 = (n - 1) / 2, r1 = n / 2;
    GdTrendSums u{n, 0, 0, 0, 0, 0};
    for (int i0 = 0; i0 < n; i0 += TR_LANES) {
        const int i = i0 + lane;
        const bool row = i < n;
        int lo = 0, hi = n;
        if (SEAS && row) {
            const unsigned g = seg[i];
            lo = (int)(g & 0xffffu);
            hi = (int)(g >> 16);
        }
        const int len = row ? hi - lo : 0;
        const int kmax = SEAS ? wave_max_i(len) : n;
        const double yi = row ? sy[i] : 0.0;
        int lt = 0, eq = 0, sg = 0;
        for (int k = 0; k < kmax; ++k) {
            if (k < len) {
                int j = i + k;
                const bool wrapped = j >= hi;
                if (wrapped) j -= len;
                const double yj = sy[j];
                lt += yj < yi;
                eq += yj == yi;                                       // k = 0 counts the sample itself: eq is c_i
                if (!wrapped) sg += gd_trend_sign(yi, yj);
            }
        }
        if (row) {
            u.s += sg;
            u.k1 += (long long)(len - 1) * (2 * len + 5);
            u.tie += (long long)(eq - 1) * (2 * eq + 5);
            u.tot2 += len - 1;
            u.ytie2 += eq - 1;
            if (!SEAS) {                                              // one segment: lt and eq are the rank of y_i, i that of t_i
                if (lt <= r0 && r0 < lt + eq) med[0] = yi;
                if (lt <= r1 && r1 < lt + eq) med[1] = yi;
                if (i == r0) med[2] = st[i];
                if (i == r1) med[3] = st[i];
            }
        }
    }
    u.s = wave_sum_ll(u.s);
    u.k1 = wave_sum_ll(u.k1);
    u.tie = wave_sum_ll(u.tie);
    u.tot2 = wave_sum_ll(u.tot2);
    u.ytie2 = wave_sum_ll(u.ytie2);
    const GdTrendStats r = gd_trend_stats(u, (flags & GD_TREND_CONTINUITY) != 0);
    if (!sen || r.nt == 0) {
        if (lane == 0) trend_put(out, M, m, flags, n, u.s, r, nan, nan, nan, nan);
        return;
    }

    // ---- seasonal: the medians of y and t are over all samples, so rank every sample among all of them ---------------------
    if constexpr (SEAS) {
        for (int i0 = 0; i0 < n; i0 += TR_LANES) {
            const int i = i0 + lane;
            const bool row = i < n;
            const double yi = row ? sy[i] : 0.0, ti = row ? st[i] : 0.0;
            int lt = 0, eq = 0, ltt = 0;
            for (int k = 0; k < n; ++k) {
                if (row) {
                    int j = i + k;
                    if (j >= n) j -= n;
                    lt += sy[j] < yi;
                    eq += sy[j] == yi;
                    ltt += st[j] < ti;
                }
            }
            if (row) {
                if (lt <= r0 && r0 < lt + eq) med[0] = yi;
                if (lt <= r1 && r1 < lt + eq) med[1] = yi;
                if (ltt == r0) med[2] = ti;
                if (ltt == r1) med[3] = ti;
            }
        }
    }

    // ---- radix select of the wanted order statistics among the nt slopes ---------------------------------------------------
    const int nq = ci ? 4 : 2;
    unsigned long long pre[TR_RANKS] = {0, 0, 0, 0};                  // the key's digits found so far
    unsigned rk[TR_RANKS], cnt[TR_RANKS];                             // rank inside the prefix's bin, and the bin's size
    bool done[TR_RANKS];
    {
        long long rl = 0, ru = 0;
        if (ci) gd_trend_ranks(r.nt, r.var_s, zq, &rl, &ru);
        rk[0] = (unsigned)((r.nt - 1) / 2);
        rk[1] = (unsigned)(r.nt / 2);
        rk[2] = (unsigned)rl;
        rk[3] = (unsigned)ru;
#pragma unroll
        for (int q = 0; q < TR_RANKS; ++q) {
            cnt[q] = (unsigned)r.nt;
            done[q] = q >= nq;
        }
    }
    for (int shift = 64 - TR_DIGIT; shift >= 0; shift -= TR_DIGIT) {
        // ranks with one prefix share the histogram of the first of them; a bin of one slope is read off instead of counted
        const unsigned long long himask = shift + TR_DIGIT >= 64 ? 0ull : ~0ull << (shift + TR_DIGIT);
        int lead[TR_RANKS];
        bool use[TR_RANKS], cap[TR_RANKS];
#pragma unroll
        for (int q = 0; q < TR_RANKS; ++q) {
            lead[q] = q;
#pragma unroll
            for (int e = q - 1; e >= 0; --e)
                if (!done[e] && pre[e] == pre[q]) lead[q] = e;
            use[q] = !done[q] && lead[q] == q;
            cap[q] = cnt[q] == 1;
        }
        for (int e = lane; e < TR_RANKS * TR_BINS; e += TR_LANES) hist[e] = 0;
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += TR_LANES) {
            const int i = i0 + lane;
            const bool row = i < n;
            int hi = n;
            if (SEAS && row) hi = (int)(seg[i] >> 16);
            const int kcnt = row ? hi - 1 - i : 0;
            const int kmax = wave_max_i(kcnt);
            const double yi = row ? sy[i] : 0.0, ti = row ? st[i] : 0.0;
            for (int k = 1; k <= kmax; ++k) {
                if (k <= kcnt) {
                    const unsigned long long key = gd_trend_key(gd_trend_slope(ti, yi, st[i + k], sy[i + k]));
                    const unsigned dig = (unsigned)(key >> shift) & (TR_BINS - 1);
#pragma unroll
                    for (int q = 0; q < TR_RANKS; ++q) {
                        if (use[q] && ((key ^ pre[q]) & himask) == 0) {
                            if (cap[q]) res[q] = key;
                            else atomicAdd(&hist[q * TR_BINS + dig], 1u);
                        }
                    }
                }
            }
        }
        __syncthreads();
        bool all = true;
#pragma unroll
        for (int q = 0; q < TR_RANKS; ++q) {
            if (!done[q]) {
                if (cap[q]) {
                    pre[q] = res[lead[q]];
                    done[q] = true;
                } else {
                    unsigned d, below, c;
                    hist_pick(hist + lead[q] * TR_BINS, rk[q], lane, d, below, c);
                    pre[q] |= (unsigned long long)d << shift;
                    rk[q] -= below;
                    cnt[q] = c;
                    done[q] = shift == 0;
                }
            }
            all = all && done[q];
        }
        if (all) break;
        __syncthreads();                                              // the histograms are read before they are cleared
    }
    if (lane == 0) {
        const double slope = gd_trend_mid(gd_trend_unkey(pre[0]), gd_trend_unkey(pre[1]));
        const double icpt = gd_trend_intercept(gd_trend_mid(med[0], med[1]), slope, gd_trend_mid(med[2], med[3]));
        trend_put(out, M, m, flags, n, u.s, r, slope, icpt, gd_trend_unkey(pre[2]), gd_trend_unkey(pre[3]));
    }
}

template <typename T>
static void trend_launch(const T* x, long Tn, long M, const double* times, int period, const unsigned char* mask, int flags, double zq,
                         double* out, hipStream_t st) {
    const size_t lds = trend_lds_bytes(Tn, period, flags);
    if (period)
        hipLaunchKernelGGL((trend_kernel<T, true>), dim3((unsigned)M), dim3(TR_LANES), lds, st, x, (int)Tn, M, times, period, mask, flags, zq, out);
    else
        hipLaunchKernelGGL((trend_kernel<T, false>), dim3((unsigned)M), dim3(TR_LANES), lds, st, x, (int)Tn, M, times, period, mask, flags, zq, out);
}

// The host twin: the same per-pair arithmetic and finalising formulas, but the order statistics come from storing and
// sorting all slopes of the series, and the medians from sorted copies.
template <typename T>
static void trend_host_one(const T* x, long Tn, long M, long m, const double* times, int period, int flags, double zq, double* out) {
    const double nan = (double)NAN;
    std::vector<double> t, y;
    std::vector<int> sea;
    for (long k = 0; k < Tn; ++k) {
        const double v = (double)x[k * M + m];
        if (v == v) {
            y.push_back(v);
            t.push_back(times[k]);
            sea.push_back(period ? (int)(k % period) : 0);
        }
    }
    const long n = (long)y.size();
    if (n < 2) {
        trend_put_empty(out, M, m, flags, n);
        return;
    }
    GdTrendSums u{n, 0, 0, 0, 0, 0};
    for (long i = 0; i < n; ++i) {
        long ng = 0, c = 0;
        for (long j = 0; j < n; ++j) {
            if (sea[j] != sea[i]) continue;
            ++ng;
            c += y[j] == y[i];
            if (j > i) u.s += gd_trend_sign(y[i], y[j]);
        }
        u.k1 += (ng - 1) * (2 * ng + 5);
        u.tie += (c - 1) * (2 * c + 5);
        u.tot2 += ng - 1;
        u.ytie2 += c - 1;
    }
    const GdTrendStats r = gd_trend_stats(u, (flags & GD_TREND_CONTINUITY) != 0);
    if (!(flags & GD_TREND_SEN) || r.nt == 0) {
        trend_put(out, M, m, flags, n, u.s, r, nan, nan, nan, nan);
        return;
    }
    std::vector<double> sl;
    sl.reserve((size_t)r.nt);
    for (long i = 0; i < n; ++i)
        for (long j = i + 1; j < n; ++j)
            if (sea[j] == sea[i]) sl.push_back(gd_trend_slope(t[i], y[i], t[j], y[j]));
    std::sort(sl.begin(), sl.end());
    const double slope = gd_trend_mid(sl[(r.nt - 1) / 2], sl[r.nt / 2]);
    std::vector<double> ys(y);
    std::sort(ys.begin(), ys.end());
    const double icpt = gd_trend_intercept(gd_trend_mid(ys[(n - 1) / 2], ys[n / 2]), slope, gd_trend_mid(t[(n - 1) / 2], t[n / 2]));
    double lo = nan, hi = nan;
    if (flags & GD_TREND_CI) {
        long long rl, ru;
        gd_trend_ranks(r.nt, r.var_s, zq, &rl, &ru);
        lo = sl[rl];
        hi = sl[ru];
    }
    trend_put(out, M, m, flags, n, u.s, r, slope, icpt, lo, hi);
}

}  // namespace

// the checks an entry shares with its host twin
#define TREND_CHECKS(fn)                                                                                                  \
    GD_CHECK_ARG(x && times && out, fn ": null pointer");                                                                \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                       \
    GD_CHECK_ARG(T >= 2 && T <= GD_TREND_MAX_T, fn ": T outside 2..GD_TREND_MAX_T");                                      \
    GD_CHECK_ARG(M > 0 && M < (1L << 31), fn ": M <= 0 or too many series");                                              \
    GD_CHECK_ARG(period == 0 || (period >= 2 && period <= T), fn ": period is 0 or 2..T");                                \
    GD_CHECK_ARG((flags & ~(GD_TREND_SEN | GD_TREND_CI | GD_TREND_CONTINUITY)) == 0, fn ": unknown flag");                \
    GD_CHECK_ARG(!(flags & GD_TREND_CI) || (flags & GD_TREND_SEN), fn ": the interval (CI) needs the slope (SEN)");       \
    GD_CHECK_ARG(zq - zq == 0.0, fn ": zq is not finite");                                                                \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(times, 8) && gd_aligned(out, 8), fn ": pointer not element aligned")

extern "C" int gd_trend_test(const void* x, int dtype, long T, long M, const double* times, int period, const unsigned char* mask,
                             int flags, double zq, double* out, void* stream) {
    TREND_CHECKS("gd_trend_test");
    gd_with_dtype(dtype, [&](auto zero) { trend_launch((const decltype(zero)*)x, T, M, times, period, mask, flags, zq, out, GD_S); });
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_trend_test_host(const void* x, int dtype, long T, long M, const double* times, int period, const unsigned char* mask,
                                  int flags, double zq, double* out) {
    TREND_CHECKS("gd_trend_test_host");
    for (long k = 0; k < T; ++k)
        GD_CHECK_ARG(times[k] - times[k] == 0.0 && (k == 0 || times[k] > times[k - 1]),
                     "gd_trend_test_host: times are not finite and strictly increasing");
    gd_with_dtype(dtype, [&](auto zero) {
        for (long m = 0; m < M; ++m) {
            if (mask && mask[m] == 0) trend_put_empty(out, M, m, flags, 0);
            else trend_host_one((const decltype(zero)*)x, T, M, m, times, period, flags, zq, out);
        }
    });
    return 0;
}
