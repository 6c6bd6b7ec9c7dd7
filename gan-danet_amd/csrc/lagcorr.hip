// Lagged correlation (include/gandanet.h, "Lagged correlation"): Pearson r of a[t] against b[t + l] for every series of two
// (T, M) cubes and every lag of a closed range, the best lag of every series, the autocorrelation of one cube, and the
// effective sample size / Fisher z / p of a correlation map.  The per-pair arithmetic, the finalising and the choice of the
// best lag are lagcorr_core.h, shared with the host twins.
//
// A workgroup owns 64 neighbouring series; a wave's 64 lanes are those series at LB neighbouring lags, and the NW =
// ceil(NL / LB) waves of the workgroup cover the NL lags, so every (series, lag) has its six sums in the registers of one
// lane from the first sample to the last.  Time is walked in chunks of LC_TC steps: the centred values a - mean_a of the
// chunk (LC_TC rows of 64 doubles) and those of b (a ring of LC_TC + span rows; a chunk adds the LC_TC rows that are new)
// are staged in LDS, NaNs kept, rows outside 0 .. T - 1 as NaN; a lane then reads u[t] once and v[t + l] for its LB lags,
// each a 512-byte row at 64 consecutive addresses (free of bank conflicts), and adds in ascending t.  The product pattern
// is a band (64 series x NL lags of products of two vectors, not a matrix product): fp64 vector arithmetic, no MFMA.
// Every cube is read from memory once by the main loop; the means come from a first pass of waves 0 and 1 over the same
// 64 columns (a second read that the L2 serves), with 1 / n from a table of reciprocals that all threads fill.  The curve is
// written from the registers when it is asked for; the best lag is chosen from LDS.  No atomics, no workspace; a series'
// result depends on the series and the parameters alone, not on M, its column, the chunk length or the launch.
#include <vector>

#include "elem_util.h"
#include "lagcorr_core.h"

namespace {

constexpr int LC_TC = GD_LAG_CHUNK, LC_LANES = 64, LC_MAX_WAVES = 16, LC_THREADS = 256;

// doubles of LDS: the two means, c_0 and n_0 of the standard autocorrelation, the reciprocals 1 / 0 .. T, and the staging
// area (u rows and the ring of v rows), which the curve (NL rows of doubles and of ints) overlays at the end
static inline size_t lag_lds_doubles(long Tn, int span) {
    const size_t stage = (size_t)(2 * LC_TC + span) * LC_LANES, curve = (size_t)(span + 1) * (LC_LANES + LC_LANES / 2);
    return 2 * LC_LANES + LC_LANES + LC_LANES / 2 + (size_t)Tn + 1 + (stage > curve ? stage : curve);
}

// lags per wave: the largest of 1, 2, 4, 9 that leaves four waves or more (at most 16 waves: 9 x 15 covers the 129 lags)
static inline int lag_block(int NL) {
    const int cand[3] = {9, 4, 2};
    for (int c : cand)
        if ((NL + c - 1) / c >= 4) return c;
    return 1;
}

template <typename T, int LB>
__global__ __launch_bounds__(LC_MAX_WAVES * LC_LANES) void lag_kernel(const T* __restrict__ a, const T* __restrict__ b, int Tn, long M, long aM,
                                                                      int lo, int hi, int min_pairs, int select, int kind,
                                                                      const unsigned char* __restrict__ mask, double* __restrict__ r_out,
                                                                      int* __restrict__ n_out, double* __restrict__ best) {
    extern __shared__ double lc_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = (int)(blockDim.x >> 6);
    const int span = hi - lo, NL = span + 1, R = LC_TC + span;
    double* mean = lc_smem;
    double* c0 = mean + 2 * LC_LANES;
    int* n0 = reinterpret_cast<int*>(c0 + LC_LANES);
    double* rcp = c0 + LC_LANES + LC_LANES / 2;
    double* su = rcp + Tn + 1;
    double* sv = su + LC_TC * LC_LANES;
    double* rr = su;
    int* nn = reinterpret_cast<int*>(rr + NL * LC_LANES);
    const long m = (long)blockIdx.x * LC_LANES + lane;
    const bool col = m < M;
    const bool live = col && (!mask || mask[m] != 0);                 // a masked series reads nothing: n = 0, r = NaN
    const long offa = aM == 1 ? 0 : m;
    const double nan = (double)NAN;

    for (int k = (int)threadIdx.x + 1; k <= Tn; k += (int)blockDim.x) rcp[k] = 1.0 / (double)k;
    __syncthreads();

    // ---- the means: wave 0 that of a, wave 1 (wave 0 when it is alone) that of b ------------------------------------------
    for (int w = wave; w < 2; w += nw) {
        const T* x = w ? b + m : a + offa;
        const long stride = w ? M : aM;
        int n = 0;
        double mu = 0.0;
        if (live) {
#pragma unroll 4
            for (int t = 0; t < Tn; ++t) gd_lag_mean_push(n, mu, (double)x[(long)t * stride], rcp[n + 1]);
        }
        mean[w * LC_LANES + lane] = mu;
    }
    __syncthreads();
    const double ma = mean[lane], mb = mean[LC_LANES + lane];

    GdLagAcc acc[LB];                                                 // slot j: lag index wave * LB + j (past NL - 1: never written)
#pragma unroll
    for (int j = 0; j < LB; ++j) acc[j] = gd_lag_zero();

    for (int t0 = 0; t0 < Tn; t0 += LC_TC) {
        for (int i = wave; i < LC_TC; i += nw) {
            const int t = t0 + i;
            double val = nan;
            if (live && t < Tn) val = (double)a[(long)t * aM + offa] - ma;
            su[i * LC_LANES + lane] = val;
        }
        // the rows of b that are new: all of lo .. LC_TC - 1 + hi at first, then the LC_TC behind the last chunk's; sample s
        // lives in row (s - lo) mod R of the ring
        const int s_begin = t0 == 0 ? lo : t0 + hi, s_end = t0 + LC_TC + hi;
        for (int s = s_begin + wave; s < s_end; s += nw) {
            double val = nan;
            if (live && s >= 0 && s < Tn) val = (double)b[(long)s * M + m] - mb;
            sv[((s - lo) % R) * LC_LANES + lane] = val;
        }
        __syncthreads();
        const int tn = min(LC_TC, Tn - t0);
        const int row0 = (t0 + wave * LB) % R;                        // the row of sample t0 + lo + wave * LB
        for (int i = 0; i < tn; ++i) {
            const double u = su[i * LC_LANES + lane];
#pragma unroll
            for (int j = 0; j < LB; ++j) {
                int row = row0 + i + j;                                // < 2 R: i + j <= LC_TC - 1 + LB - 1, LB - 1 <= span
                row -= row >= R ? R : 0;
                gd_lag_add(acc[j], u, sv[row * LC_LANES + lane]);
            }
        }
        __syncthreads();
    }

    // ---- r of every (series, lag); the standard autocorrelation needs the sums of lag 0 first ------------------------------
    if (kind == GD_ACF_STANDARD) {
#pragma unroll
        for (int j = 0; j < LB; ++j) {
            if (wave * LB + j == -lo) {
                c0[lane] = acc[j].suu;
                n0[lane] = acc[j].n;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < LB; ++j) {
        const int k = wave * LB + j;
        if (k < NL) {
            const double r = kind == GD_ACF_STANDARD ? gd_lag_acf(acc[j], min_pairs, n0[lane], c0[lane]) : gd_lag_r(acc[j], min_pairs);
            if (col) {
                if (r_out) r_out[(long)k * M + m] = r;
                if (n_out) n_out[(long)k * M + m] = acc[j].n;
            }
            if (best) {
                rr[k * LC_LANES + lane] = r;
                nn[k * LC_LANES + lane] = acc[j].n;
            }
        }
    }
    if (!best) return;
    __syncthreads();
    if (wave == 0 && col) {
        double o[GD_LAG_PLANES];
        gd_lag_best(lo, hi, select, [&](int k) { return rr[k * LC_LANES + lane]; }, [&](int k) { return nn[k * LC_LANES + lane]; }, o);
#pragma unroll
        for (int q = 0; q < GD_LAG_PLANES; ++q) best[(long)q * M + m] = o[q];
    }
}

template <typename T, int LB>
static int lag_launch_lb(const T* a, const T* b, long Tn, long M, long aM, int lo, int hi, int min_pairs, int select, int kind,
                         const unsigned char* mask, double* r_out, int* n_out, double* best, hipStream_t st) {
    const int NL = hi - lo + 1, nw = (NL + LB - 1) / LB;
    const size_t bytes = lag_lds_doubles(Tn, hi - lo) * sizeof(double);
    if (bytes > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&lag_kernel<T, LB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)bytes);
        if (e != hipSuccess) {
            gd_set_error(hipGetErrorString(e));
            return -2;
        }
    }
    hipLaunchKernelGGL((lag_kernel<T, LB>), dim3((unsigned)((M + LC_LANES - 1) / LC_LANES)), dim3(nw * LC_LANES), bytes, st, a, b, (int)Tn, M, aM,
                       lo, hi, min_pairs, select, kind, mask, r_out, n_out, best);
    GD_LAUNCH_CHECK();
    return 0;
}

template <typename T>
static int lag_launch(const T* a, const T* b, long Tn, long M, long aM, int lo, int hi, int min_pairs, int select, int kind,
                      const unsigned char* mask, double* r_out, int* n_out, double* best, hipStream_t st) {
    switch (lag_block(hi - lo + 1)) {
#define LAG_CASE(lb) case lb: return lag_launch_lb<T, lb>(a, b, Tn, M, aM, lo, hi, min_pairs, select, kind, mask, r_out, n_out, best, st)
        LAG_CASE(9); LAG_CASE(4); LAG_CASE(2);
        default: LAG_CASE(1);
#undef LAG_CASE
    }
}

// The host twin: the same means, sums, finalising and choice, one series and one lag at a time.
template <typename T>
static void lag_host(const T* a, const T* b, long Tn, long M, long aM, int lo, int hi, int min_pairs, int select, int kind,
                     const unsigned char* mask, double* r_out, int* n_out, double* best) {
    const int NL = hi - lo + 1;
    std::vector<double> u((size_t)Tn), v((size_t)Tn), rr((size_t)NL);
    std::vector<int> nn((size_t)NL);
    std::vector<GdLagAcc> acc((size_t)NL);
    for (long m = 0; m < M; ++m) {
        const bool live = !mask || mask[m] != 0;
        const long offa = aM == 1 ? 0 : m;
        int na = 0, nb = 0;
        double ma = 0.0, mb = 0.0;
        if (live) {
            for (long t = 0; t < Tn; ++t) gd_lag_mean_push(na, ma, (double)a[t * aM + offa], 1.0 / (double)(na + 1));
            for (long t = 0; t < Tn; ++t) gd_lag_mean_push(nb, mb, (double)b[t * M + m], 1.0 / (double)(nb + 1));
        }
        for (long t = 0; t < Tn; ++t) {
            u[t] = live ? (double)a[t * aM + offa] - ma : (double)NAN;
            v[t] = live ? (double)b[t * M + m] - mb : (double)NAN;
        }
        for (int k = 0; k < NL; ++k) {
            const long l = lo + k;
            GdLagAcc s = gd_lag_zero();
            for (long t = 0; t < Tn; ++t)
                if (t + l >= 0 && t + l < Tn) gd_lag_add(s, u[t], v[t + l]);
            acc[k] = s;
        }
        for (int k = 0; k < NL; ++k) {
            rr[k] = kind == GD_ACF_STANDARD ? gd_lag_acf(acc[k], min_pairs, acc[-lo].n, acc[-lo].suu) : gd_lag_r(acc[k], min_pairs);
            nn[k] = acc[k].n;
            if (r_out) r_out[(long)k * M + m] = rr[k];
            if (n_out) n_out[(long)k * M + m] = nn[k];
        }
        if (best) {
            double o[GD_LAG_PLANES];
            gd_lag_best(lo, hi, select, [&](int k) { return rr[k]; }, [&](int k) { return nn[k]; }, o);
            for (int q = 0; q < GD_LAG_PLANES; ++q) best[(long)q * M + m] = o[q];
        }
    }
}

// ---- effective sample size, Fisher z, p ---------------------------------------------------------------------------------
struct SignifBody {
    const double *r, *n, *r1a;
    long a_len;
    const double* r1b;
    double *neff, *z, *p;
    __host__ __device__ void operator()(long i) const {
        double ne, zz;
        gd_corr_neff_z(r[i], n[i], r1a[a_len == 1 ? 0 : i], r1b[i], &ne, &zz);
        if (neff) neff[i] = ne;
        if (z) z[i] = zz;
        if (p) p[i] = zz == zz ? erfc(fabs(zz) * 0.7071067811865476) : (double)NAN;
    }
};

}  // namespace

// the checks an entry shares with its host twin
#define LAG_CORR_CHECKS(fn)                                                                                                      \
    GD_CHECK_ARG(a && b, fn ": null pointer");                                                                                  \
    GD_CHECK_ARG(r || n || best, fn ": every output is NULL");                                                                  \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                              \
    GD_CHECK_ARG(T >= 1 && T <= GD_LAG_MAX_T, fn ": T outside 1..GD_LAG_MAX_T");                                                 \
    GD_CHECK_ARG(M > 0 && M < (1L << 31), fn ": M <= 0 or too many series");                                                    \
    GD_CHECK_ARG(a_M == 1 || a_M == M, fn ": a_M is 1 or M");                                                                   \
    GD_CHECK_ARG(-GD_LAG_MAX <= lag_lo && lag_lo <= lag_hi && lag_hi <= GD_LAG_MAX, fn ": lags outside -GD_LAG_MAX <= lo <= hi <= GD_LAG_MAX"); \
    GD_CHECK_ARG(min_pairs >= 2, fn ": min_pairs < 2");                                                                         \
    GD_CHECK_ARG(select >= GD_LAG_SELECT_ABS && select <= GD_LAG_SELECT_MIN, fn ": select outside {0, 1, 2}");                  \
    GD_CHECK_ARG(gd_elem_aligned(a, dtype) && gd_elem_aligned(b, dtype) && gd_aligned(r, 8) && gd_aligned(n, 4) && gd_aligned(best, 8), \
                 fn ": pointer not element aligned")

extern "C" int gd_lag_corr(const void* a, const void* b, int dtype, long T, long M, long a_M, int lag_lo, int lag_hi, int min_pairs,
                           int select, const unsigned char* mask, double* r, int* n, double* best, void* stream) {
    LAG_CORR_CHECKS("gd_lag_corr");
    return gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        return lag_launch((const E*)a, (const E*)b, T, M, a_M, lag_lo, lag_hi, min_pairs, select, GD_ACF_PEARSON, mask, r, n, best, GD_S);
    });
}

extern "C" int gd_lag_corr_host(const void* a, const void* b, int dtype, long T, long M, long a_M, int lag_lo, int lag_hi,
                                int min_pairs, int select, const unsigned char* mask, double* r, int* n, double* best) {
    LAG_CORR_CHECKS("gd_lag_corr_host");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        lag_host((const E*)a, (const E*)b, T, M, a_M, lag_lo, lag_hi, min_pairs, select, GD_ACF_PEARSON, mask, r, n, best);
    });
    return 0;
}

#define SERIES_ACF_CHECKS(fn)                                                                                      \
    GD_CHECK_ARG(x && acf, fn ": null pointer");                                                                  \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                \
    GD_CHECK_ARG(T >= 1 && T <= GD_LAG_MAX_T, fn ": T outside 1..GD_LAG_MAX_T");                                   \
    GD_CHECK_ARG(M > 0 && M < (1L << 31), fn ": M <= 0 or too many series");                                      \
    GD_CHECK_ARG(K >= 0 && K <= GD_LAG_MAX, fn ": K outside 0..GD_LAG_MAX");                                       \
    GD_CHECK_ARG(kind == GD_ACF_PEARSON || kind == GD_ACF_STANDARD, fn ": kind outside {0, 1}");                  \
    GD_CHECK_ARG(min_pairs >= 2, fn ": min_pairs < 2");                                                           \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(acf, 8) && gd_aligned(n, 4), fn ": pointer not element aligned")

extern "C" int gd_series_acf(const void* x, int dtype, long T, long M, int K, int kind, int min_pairs, const unsigned char* mask,
                             double* acf, int* n, void* stream) {
    SERIES_ACF_CHECKS("gd_series_acf");
    return gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        return lag_launch((const E*)x, (const E*)x, T, M, M, 0, K, min_pairs, GD_LAG_SELECT_ABS, kind, mask, acf, n, (double*)nullptr, GD_S);
    });
}

extern "C" int gd_series_acf_host(const void* x, int dtype, long T, long M, int K, int kind, int min_pairs, const unsigned char* mask,
                                  double* acf, int* n) {
    SERIES_ACF_CHECKS("gd_series_acf_host");
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        lag_host((const E*)x, (const E*)x, T, M, M, 0, K, min_pairs, GD_LAG_SELECT_ABS, kind, mask, acf, n, (double*)nullptr);
    });
    return 0;
}

extern "C" int gd_corr_signif(const double* r, const double* n, const double* r1a, long r1a_len, const double* r1b, long M, double* n_eff,
                              double* z, double* p, void* stream) {
    GD_CHECK_ARG(r && n && r1a && r1b, "gd_corr_signif: null pointer");
    GD_CHECK_ARG(n_eff || z || p, "gd_corr_signif: every output is NULL");
    GD_CHECK_ARG(M > 0 && M < (1L << 31), "gd_corr_signif: M <= 0 or too many series");
    GD_CHECK_ARG(r1a_len == 1 || r1a_len == M, "gd_corr_signif: r1a holds 1 or M values");
    GD_CHECK_ARG(gd_aligned(r, 8) && gd_aligned(n, 8) && gd_aligned(r1a, 8) && gd_aligned(r1b, 8) && gd_aligned(n_eff, 8) && gd_aligned(z, 8) &&
                     gd_aligned(p, 8),
                 "gd_corr_signif: pointer not element aligned");
    gd_for_items<LC_THREADS>(false, M, GD_S, SignifBody{r, n, r1a, r1a_len, r1b, n_eff, z, p});
    GD_LAUNCH_CHECK();
    return 0;
}
