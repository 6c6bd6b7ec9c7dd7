// Per-pixel time series (include/gandanet.h, "Per-pixel time series"): skill records of one (T, M) cube against another
// along t, their finalising into maps, a masked least-squares fit of every series against a common (T, P) design matrix,
// amplitude / phase / slope of a harmonic fit, and the NaN-aware block mean.  The arithmetic is series_core.h, shared with
// the host twins.
//
// A thread owns a series (in the record kernel one 16-byte vector of neighbouring series where the rows allow it) and
// walks t in ascending order: lanes read neighbouring columns of a row, so every time step is one coalesced row read, and
// T is never split -- a series' result depends on nothing but the series.  No LDS, no atomics, no workspace.  The basis
// rows of the fit are the same for every lane: they are read at a wave-uniform address and come through the scalar cache.
// From elem_util.h: gd_dtype_ok, gd_elem_aligned, gd_aligned, gd_head_of, gd_vec16, gd_with_dtype, gd_for_items,
// GD_S.
#include "elem_util.h"
#include "series_core.h"

namespace {

constexpr int SR_THREADS = 256;

__host__ __device__ inline GdSeriesRec rec_get(const double* rec, long M, long m) {
    return GdSeriesRec{rec[m], rec[M + m], rec[2 * M + m], rec[3 * M + m], rec[4 * M + m], rec[5 * M + m], rec[6 * M + m], rec[7 * M + m]};
}
__host__ __device__ inline void rec_put(double* rec, long M, long m, const GdSeriesRec& r) {
    rec[m] = r.n; rec[M + m] = r.mp; rec[2 * M + m] = r.mt; rec[3 * M + m] = r.m2p;
    rec[4 * M + m] = r.m2t; rec[5 * M + m] = r.c; rec[6 * M + m] = r.sae; rec[7 * M + m] = r.sse;
}
// the record a call starts from: the stored one under `accumulate` (n <= 0 counts as empty), else empty
__host__ __device__ inline GdSeriesRec rec_start(const double* rec, long M, long m, int accumulate) {
    if (!accumulate) return gd_series_zero();
    const GdSeriesRec r = rec_get(rec, M, m);
    return r.n > 0 ? r : gd_series_zero();
}

// ---- records -------------------------------------------------------------------------------------------------------------
// Item `it` is the VW neighbouring series from (it < skip_from ? it : it + skip_len) * VW: the 16-byte instance covers the
// body from the rows' first 16-byte boundary, the scalar instance the series in front of it and behind the last whole
// vector (or every series, when the rows do not keep their alignment).
template <typename T, int VW, bool SKIPNAN>
__global__ __launch_bounds__(SR_THREADS) void series_stats_kernel(const T* __restrict__ pred, const T* __restrict__ truth, long Tn, long M,
                                                                  long items, long skip_from, long skip_len,
                                                                  const unsigned char* __restrict__ mask, double* __restrict__ rec,
                                                                  int accumulate) {
    const long it = (long)blockIdx.x * SR_THREADS + threadIdx.x;
    if (it >= items) return;
    const long e = (it < skip_from ? it : it + skip_len) * VW;
    GdSeriesRec r[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) r[j] = rec_start(rec, M, e + j, accumulate);
    const T* p = pred + e;
    const T* q = truth + e;
#pragma unroll 4
    for (long t = 0; t < Tn; ++t) {
        double pe[VW], te[VW];
        if constexpr (VW > 1) {
            gd_vec16<T>::load(p + t * M, pe);
            gd_vec16<T>::load(q + t * M, te);
        } else {
            pe[0] = (double)p[t * M];
            te[0] = (double)q[t * M];
        }
#pragma unroll
        for (int j = 0; j < VW; ++j) gd_series_push(r[j], pe[j], te[j], SKIPNAN);
    }
#pragma unroll
    for (int j = 0; j < VW; ++j) {
        if (mask && mask[e + j] == 0) {
            if (!accumulate) rec_put(rec, M, e + j, gd_series_zero());
        } else {
            rec_put(rec, M, e + j, r[j]);
        }
    }
}

template <typename T, bool SKIPNAN>
static void series_stats_launch(const T* pred, const T* truth, long Tn, long M, const unsigned char* mask, double* rec, int accumulate,
                                hipStream_t st) {
    constexpr int W = gd_vec16<T>::W;
    // 16-byte path: both cubes reach a 16-byte boundary after the same `head` series, and a row is a whole number of
    // vectors, so every row keeps that boundary
    long head = gd_head_of(pred), nv = 0;
    if (M % W == 0 && Tn * M >= W && head == gd_head_of(truth) && head <= M) nv = (M - head) / W;
    else head = 0;
    if (nv > 0)
        hipLaunchKernelGGL((series_stats_kernel<T, W, SKIPNAN>), dim3(gd_cdiv(nv, SR_THREADS)), dim3(SR_THREADS), 0, st, pred + head,
                           truth + head, Tn, M, nv, nv, 0L, mask ? mask + head : mask, rec + head, accumulate);
    const long rest = M - nv * W;
    if (rest > 0)
        hipLaunchKernelGGL((series_stats_kernel<T, 1, SKIPNAN>), dim3(gd_cdiv(rest, SR_THREADS)), dim3(SR_THREADS), 0, st, pred, truth, Tn,
                           M, rest, head, nv * W, mask, rec, accumulate);
}

template <typename T>
static void series_stats_host(const T* pred, const T* truth, long Tn, long M, const unsigned char* mask, bool skip, double* rec,
                              int accumulate) {
    for (long m = 0; m < M; ++m) {
        if (mask && mask[m] == 0) {
            if (!accumulate) rec_put(rec, M, m, gd_series_zero());
            continue;
        }
        GdSeriesRec r = rec_start(rec, M, m, accumulate);
        for (long t = 0; t < Tn; ++t) gd_series_push(r, (double)pred[t * M + m], (double)truth[t * M + m], skip);
        rec_put(rec, M, m, r);
    }
}

// ---- maps ----------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void skill_one(const double* rec, long M, long m, int ddof, int which, double* out) {
    double o[GD_SKILL_MAPS];
    gd_series_finalize(rec_get(rec, M, m), ddof, o);
    long j = 0;
#pragma unroll
    for (int k = 0; k < GD_SKILL_MAPS; ++k) {
        if (which >> k & 1) {
            out[j * M + m] = o[k];
            ++j;
        }
    }
}

// One Body per entry (gd_for_items): operator() is the per-item call of the device kernel and of the host twin alike.
struct SkillBody {
    const double* rec;
    long M;
    int ddof, which;
    double* out;
    __host__ __device__ void operator()(long m) const { skill_one(rec, M, m, ddof, which, out); }
};

// ---- least squares -------------------------------------------------------------------------------------------------------
template <typename T, int P> __host__ __device__ inline void lstsq_one(const T* __restrict__ x, long Tn, long M, long m,
                                                                       const double* __restrict__ basis, double* __restrict__ coef,
                                                                       double* __restrict__ rss, double* __restrict__ n_out) {
    GdLsq<P> s;
    gd_lsq_zero(s);
    const T* y = x + m;
#pragma unroll 2
    for (long t = 0; t < Tn; ++t) gd_lsq_add<P>(s, basis + t * P, (double)y[t * M]);
    double c[P];
    const bool ok = gd_lsq_solve<P>(s, c);
    double r2 = (double)NAN;
    if (ok) {
        r2 = 0.0;
        if (rss) {
#pragma unroll 2
            for (long t = 0; t < Tn; ++t) r2 += gd_lsq_resid2<P>(basis + t * P, c, (double)y[t * M]);
        }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) coef[j * M + m] = ok ? c[j] : (double)NAN;
    if (rss) rss[m] = r2;
    if (n_out) n_out[m] = s.n;
}

template <typename T, int P> struct LstsqBody {
    const T* x;
    long Tn, M;
    const double* basis;
    double *coef, *rss, *n_out;
    __host__ __device__ void operator()(long m) const { lstsq_one<T, P>(x, Tn, M, m, basis, coef, rss, n_out); }
};

// called by the device entry (host = false) and by its host twin (host = true, st unused)
void lstsq_run(bool host, hipStream_t st, const void* x, int dtype, long Tn, long M, const double* basis, int P, double* coef, double* rss,
               double* n_out) {
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        switch (P) {
#define LSQ_CASE(p) case p: gd_for_items<SR_THREADS>(host, M, st, LstsqBody<T, p>{(const T*)x, Tn, M, basis, coef, rss, n_out}); break
            LSQ_CASE(1); LSQ_CASE(2); LSQ_CASE(3); LSQ_CASE(4); LSQ_CASE(5); LSQ_CASE(6); LSQ_CASE(7); LSQ_CASE(8);
#undef LSQ_CASE
        }
    });
    static_assert(GD_LSTSQ_MAX_P == 8, "one case per P");
}

// ---- amplitude, phase, slope, rms residual -------------------------------------------------------------------------------
__host__ __device__ inline void harmonic_one(const double* __restrict__ coef, long M, long m, int K, int has_trend, double tau_scale,
                                             const double* __restrict__ rss, const double* __restrict__ n, double* __restrict__ amp,
                                             double* __restrict__ phase, double* __restrict__ slope, double* __restrict__ rms) {
    for (int k = 0; k < K; ++k) {
        const double c = coef[(1 + has_trend + 2 * k) * M + m], s = coef[(2 + has_trend + 2 * k) * M + m];
        if (amp) amp[k * M + m] = hypot(c, s);
        if (phase) phase[k * M + m] = atan2(s, c);
    }
    if (slope) slope[m] = coef[M + m] * tau_scale;
    if (rms) rms[m] = sqrt(rss[m] / n[m]);
}

struct HarmonicBody {
    const double* coef;
    long M;
    int K, has_trend;
    double tau_scale;
    const double *rss, *n;
    double *amp, *phase, *slope, *rms;
    __host__ __device__ void operator()(long m) const { harmonic_one(coef, M, m, K, has_trend, tau_scale, rss, n, amp, phase, slope, rms); }
};

// ---- block mean ----------------------------------------------------------------------------------------------------------
// one thread per output element, neighbouring threads neighbouring blocks of a row: a wave reads fx * 64 consecutive
// elements of each of the fy rows
template <typename T> struct BlockMeanBody {
    const T* x;
    long H, W;
    int fy, fx;
    const double* weights;
    int min_count;
    T* out;
    int* count;
    __host__ __device__ void operator()(long i) const {
        const long Ho = H / fy, Wo = W / fx;
        const long ox = i % Wo, oy = (i / Wo) % Ho, pl = i / (Wo * Ho);
        const long off = oy * fy * W + ox * fx;
        int cnt;
        const double v = gd_block_mean_one(x + pl * H * W + off, weights ? weights + off : weights, W, fy, fx, min_count, &cnt);
        out[i] = (T)v;
        if (count) count[i] = cnt;
    }
};

void block_mean_run(bool host, hipStream_t st, const void* x, int dtype, long total, long H, long W, int fy, int fx, const double* weights,
                    int min_count, void* out, int* count) {
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        gd_for_items<SR_THREADS, 1L << 20>(host, total, st, BlockMeanBody<T>{(const T*)x, H, W, fy, fx, weights, min_count, (T*)out, count});
    });
}

}  // namespace

// the checks an entry shares with its host twin
#define SERIES_STATS_CHECKS(fn)                                                                                        \
    GD_CHECK_ARG(pred && truth && rec, fn ": null pointer");                                                          \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                    \
    GD_CHECK_ARG(T > 0 && M > 0, fn ": T <= 0 or M <= 0");                                                             \
    GD_CHECK_ARG(M < (1L << 31) && M < (1L << 53) / T, fn ": too many series");                                        \
    GD_CHECK_ARG((flags & ~GD_EVAL_SKIP_NAN) == 0, fn ": unknown flag");                                               \
    GD_CHECK_ARG(gd_elem_aligned(pred, dtype) && gd_elem_aligned(truth, dtype) && gd_aligned(rec, 8),                  \
                 fn ": pointer not element aligned")

extern "C" int gd_series_stats(const void* pred, const void* truth, int dtype, long T, long M, const unsigned char* mask, int flags,
                               double* rec, int accumulate, void* stream) {
    SERIES_STATS_CHECKS("gd_series_stats");
    const bool skip = (flags & GD_EVAL_SKIP_NAN) != 0;
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        if (skip) series_stats_launch<E, true>((const E*)pred, (const E*)truth, T, M, mask, rec, accumulate, GD_S);
        else series_stats_launch<E, false>((const E*)pred, (const E*)truth, T, M, mask, rec, accumulate, GD_S);
    });
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_series_stats_host(const void* pred, const void* truth, int dtype, long T, long M, const unsigned char* mask,
                                    int flags, double* rec, int accumulate) {
    SERIES_STATS_CHECKS("gd_series_stats_host");
    const bool skip = (flags & GD_EVAL_SKIP_NAN) != 0;
    gd_with_dtype(dtype, [&](auto zero) {
        using E = decltype(zero);
        series_stats_host((const E*)pred, (const E*)truth, T, M, mask, skip, rec, accumulate);
    });
    return 0;
}

#define SERIES_SKILL_CHECKS(fn)                                                                          \
    GD_CHECK_ARG(rec && out, fn ": null pointer");                                                      \
    GD_CHECK_ARG(M > 0 && M < (1L << 31), fn ": M <= 0 or too many series");                             \
    GD_CHECK_ARG(ddof == 0 || ddof == 1, fn ": ddof outside {0, 1}");                                    \
    GD_CHECK_ARG(which > 0 && which < (1 << GD_SKILL_MAPS), fn ": no map selected or an unknown map");  \
    GD_CHECK_ARG(gd_aligned(rec, 8) && gd_aligned(out, 8), fn ": pointer not element aligned")

extern "C" int gd_series_skill(const double* rec, long M, int ddof, int which, double* out, void* stream) {
    SERIES_SKILL_CHECKS("gd_series_skill");
    gd_for_items<SR_THREADS>(false, M, GD_S, SkillBody{rec, M, ddof, which, out});
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_series_skill_host(const double* rec, long M, int ddof, int which, double* out) {
    SERIES_SKILL_CHECKS("gd_series_skill_host");
    gd_for_items<SR_THREADS>(true, M, nullptr, SkillBody{rec, M, ddof, which, out});
    return 0;
}

#define SERIES_LSTSQ_CHECKS(fn)                                                                                              \
    GD_CHECK_ARG(x && basis && coef, fn ": null pointer");                                                                  \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                          \
    GD_CHECK_ARG(T > 0 && M > 0, fn ": T <= 0 or M <= 0");                                                                   \
    GD_CHECK_ARG(P >= 1 && P <= GD_LSTSQ_MAX_P, fn ": P outside 1..GD_LSTSQ_MAX_P");                                         \
    GD_CHECK_ARG(M < (1L << 31) && M < (1L << 53) / T, fn ": too many series");                                              \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(basis, 8) && gd_aligned(coef, 8) && gd_aligned(rss, 8) &&           \
                     gd_aligned(n_out, 8),                                                                                   \
                 fn ": pointer not element aligned")

extern "C" int gd_series_lstsq(const void* x, int dtype, long T, long M, const double* basis, int P, double* coef, double* rss,
                               double* n_out, void* stream) {
    SERIES_LSTSQ_CHECKS("gd_series_lstsq");
    lstsq_run(false, GD_S, x, dtype, T, M, basis, P, coef, rss, n_out);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_series_lstsq_host(const void* x, int dtype, long T, long M, const double* basis, int P, double* coef, double* rss,
                                    double* n_out) {
    SERIES_LSTSQ_CHECKS("gd_series_lstsq_host");
    lstsq_run(true, nullptr, x, dtype, T, M, basis, P, coef, rss, n_out);
    return 0;
}

extern "C" int gd_harmonic_finalize(const double* coef, int P, long M, int K, int has_trend, double tau_scale, const double* rss,
                                    const double* n, double* amp, double* phase, double* slope, double* rms, void* stream) {
    GD_CHECK_ARG(coef, "gd_harmonic_finalize: null pointer");
    GD_CHECK_ARG(M > 0 && M < (1L << 31), "gd_harmonic_finalize: M <= 0 or too many series");
    GD_CHECK_ARG(K >= 0 && K <= 3, "gd_harmonic_finalize: K outside 0..3");
    GD_CHECK_ARG(has_trend == 0 || has_trend == 1, "gd_harmonic_finalize: has_trend outside {0, 1}");
    GD_CHECK_ARG(P == 1 + has_trend + 2 * K, "gd_harmonic_finalize: P is not 1 + has_trend + 2 K");
    GD_CHECK_ARG(!slope || has_trend, "gd_harmonic_finalize: a slope without a trend column");
    GD_CHECK_ARG(!rms || (rss && n), "gd_harmonic_finalize: rms needs rss and n");
    GD_CHECK_ARG(gd_aligned(coef, 8) && gd_aligned(rss, 8) && gd_aligned(n, 8) && gd_aligned(amp, 8) && gd_aligned(phase, 8) &&
                     gd_aligned(slope, 8) && gd_aligned(rms, 8),
                 "gd_harmonic_finalize: pointer not element aligned");
    gd_for_items<SR_THREADS>(false, M, GD_S, HarmonicBody{coef, M, K, has_trend, tau_scale, rss, n, amp, phase, slope, rms});
    GD_LAUNCH_CHECK();
    return 0;
}

#define BLOCK_MEAN_CHECKS(fn)                                                                                                  \
    GD_CHECK_ARG(x && out, fn ": null pointer");                                                                              \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                            \
    GD_CHECK_ARG(planes > 0 && H > 0 && W > 0, fn ": planes, H or W <= 0");                                                    \
    GD_CHECK_ARG(fy >= 1 && fx >= 1, fn ": a block factor < 1");                                                               \
    GD_CHECK_ARG(H % fy == 0 && W % fx == 0, fn ": the block does not divide the shape");                                      \
    GD_CHECK_ARG(min_count >= 0, fn ": min_count < 0");                                                                        \
    GD_CHECK_ARG(H < (1L << 31) && W < (1L << 31) && planes < (1L << 53) / H / W, fn ": too many elements");                   \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_elem_aligned(out, dtype) && gd_aligned(weights, 8) && gd_aligned(count, 4),   \
                 fn ": pointer not element aligned");                                                                          \
    const long total = planes * (H / fy) * (W / fx)

extern "C" int gd_block_mean(const void* x, int dtype, long planes, long H, long W, int fy, int fx, const double* weights,
                             int min_count, void* out, int* count, void* stream) {
    BLOCK_MEAN_CHECKS("gd_block_mean");
    block_mean_run(false, GD_S, x, dtype, total, H, W, fy, fx, weights, min_count, out, count);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_block_mean_host(const void* x, int dtype, long planes, long H, long W, int fy, int fx, const double* weights,
                                  int min_count, void* out, int* count) {
    BLOCK_MEAN_CHECKS("gd_block_mean_host");
    block_mean_run(true, nullptr, x, dtype, total, H, W, fy, fx, weights, min_count, out, count);
    return 0;
}
