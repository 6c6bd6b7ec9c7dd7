// Drought analysis (include/gandanet.h, "Drought analysis"): the calendar climatology of every series of a (T, M) cube,
// the parametric indices against it (anomaly = water storage deficit, standardised = GRACE-DSI), the non-parametric rank
// index through a table its caller built, the run-theory scan for events and their maps, and the indicator cube that
// gd_zone_mean turns into drought-area series.  The arithmetic is drought_core.h, shared with the host twins.
//
// A thread owns a series and walks it in ascending t: lanes read neighbouring columns of a row, so every step is one
// coalesced row read.  T is never split and nothing is shared between threads: a series' result depends on nothing but the
// series and the parameters.  No LDS, no atomics, no workspace.  The climatology, index and rank kernels take the slots in
// an outer loop (t = first(s); t += period), which keeps a slot's accumulators, mean and deviation in registers; the rank
// kernel re-reads the baseline samples of a slot once per sample of that slot (they come from cache).
// From elem_util.h: gd_dtype_ok, gd_elem_aligned, gd_aligned, gd_stream_grid, gd_with_dtype, gd_for_items, GD_S.
#include "elem_util.h"
#include "drought_core.h"

namespace {

constexpr int DR_THREADS = 256;

// one Body per entry (gd_for_items): operator() is the per-series call of the device kernel and of the host twin alike
template <typename T> struct ClimBody {
    const T* x;
    long M, b0, b1;
    int period, phase;
    const unsigned char* mask;
    double* rec;
    __host__ __device__ void operator()(long m) const {
        gd_drought_clim_one(x + m, M, period, phase, b0, b1, !mask || mask[m] != 0, rec + m);
    }
};

template <typename T> struct IndexBody {
    const T* x;
    long Tn, M;
    const double* rec;
    int period, phase, kind, ddof;
    const unsigned char* mask;
    T* out;
    __host__ __device__ void operator()(long m) const {
        gd_drought_index_one(x + m, Tn, M, rec + m, period, phase, kind, ddof, !mask || mask[m] != 0, out + m);
    }
};

template <typename T> struct RankBody {
    const T* x;
    long Tn, M, b0, b1;
    int period, phase;
    const unsigned char* mask;
    const double* table;
    T* out;
    __host__ __device__ void operator()(long m) const {
        gd_drought_rank_one(x + m, Tn, M, period, phase, b0, b1, !mask || mask[m] != 0, table, out + m);
    }
};

template <typename T> struct EventsBody {
    const T* x;
    long Tn, M;
    double threshold;
    int min_duration, which;
    const unsigned char* mask;
    double* maps;
    unsigned char* in_event;
    __host__ __device__ void operator()(long m) const {
        double o[GD_DROUGHT_EV_MAPS];
        gd_drought_events_one(x + m, Tn, M, threshold, min_duration, !mask || mask[m] != 0, o, in_event ? in_event + m : in_event);
        gd_drought_events_put(o, which, M, maps + m);
    }
};

// exceed keeps a kernel of its own: the __restrict__ of kernel arguments lets the fp32 loop be unrolled with its loads ahead
// of its stores, which a Body's members do not (12 instead of 25 VGPRs, and 14 % slower on the (181, 440, 900) cube)
template <typename T>
__global__ __launch_bounds__(DR_THREADS) void drought_exceed_kernel(const T* __restrict__ x, long n, double threshold, T* __restrict__ out) {
    for (long i = (long)blockIdx.x * DR_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * DR_THREADS)
        out[i] = gd_drought_exceed_one(x[i], threshold);
}

// one function per entry, called by the device entry (host = false) and by its host twin (host = true, st unused)
void clim_run(bool host, hipStream_t st, const void* x, int dtype, long M, int period, int phase, long b0, long b1,
              const unsigned char* mask, double* clim) {
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        gd_for_items<DR_THREADS>(host, M, st, ClimBody<T>{(const T*)x, M, b0, b1, period, phase, mask, clim});
    });
}

void index_run(bool host, hipStream_t st, const void* x, int dtype, long Tn, long M, const double* clim, int period, int phase, int kind,
               int ddof, const unsigned char* mask, void* out) {
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        gd_for_items<DR_THREADS>(host, M, st, IndexBody<T>{(const T*)x, Tn, M, clim, period, phase, kind, ddof, mask, (T*)out});
    });
}

void rank_run(bool host, hipStream_t st, const void* x, int dtype, long Tn, long M, int period, int phase, long b0, long b1,
              const unsigned char* mask, const double* table, void* out) {
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        gd_for_items<DR_THREADS>(host, M, st, RankBody<T>{(const T*)x, Tn, M, b0, b1, period, phase, mask, table, (T*)out});
    });
}

void events_run(bool host, hipStream_t st, const void* index, int dtype, long Tn, long M, double threshold, int min_duration, int which,
                const unsigned char* mask, double* maps, unsigned char* in_event) {
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        gd_for_items<DR_THREADS>(host, M, st, EventsBody<T>{(const T*)index, Tn, M, threshold, min_duration, which, mask, maps, in_event});
    });
}

void exceed_run(bool host, hipStream_t st, const void* index, int dtype, long n, double threshold, void* out) {
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        const T* x = (const T*)index;
        T* o = (T*)out;
        if (host) {
            for (long i = 0; i < n; ++i) o[i] = gd_drought_exceed_one(x[i], threshold);
            return;
        }
        hipLaunchKernelGGL(drought_exceed_kernel<T>, dim3(gd_stream_grid(n, DR_THREADS, 1L << 16)), dim3(DR_THREADS), 0, st, x, n, threshold, o);
    });
}

}  // namespace

// the checks an entry shares with its host twin
#define DROUGHT_CUBE_CHECKS(fn)                                                                        \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                    \
    GD_CHECK_ARG(T > 0 && T <= GD_DROUGHT_MAX_T, fn ": T outside 1..GD_DROUGHT_MAX_T");                \
    GD_CHECK_ARG(M > 0, fn ": M <= 0");                                                                \
    GD_CHECK_ARG(M < (1L << 31), fn ": too many series")
#define DROUGHT_CALENDAR_CHECKS(fn)                                                                    \
    GD_CHECK_ARG(period >= 1 && period <= GD_DROUGHT_MAX_PERIOD, fn ": period outside 1..GD_DROUGHT_MAX_PERIOD"); \
    GD_CHECK_ARG(phase >= 0 && phase < period, fn ": phase outside 0..period - 1")
#define DROUGHT_BASELINE_CHECKS(fn) \
    GD_CHECK_ARG(b0 >= 0 && b0 < b1 && b1 <= T, fn ": the baseline [b0, b1) is empty, reversed or outside [0, T]")

#define DROUGHT_CLIM_CHECKS(fn)                                                                        \
    GD_CHECK_ARG(x && clim, fn ": null pointer");                                                      \
    DROUGHT_CUBE_CHECKS(fn);                                                                           \
    DROUGHT_CALENDAR_CHECKS(fn);                                                                       \
    DROUGHT_BASELINE_CHECKS(fn);                                                                       \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(clim, 8), fn ": pointer not element aligned")

extern "C" int gd_drought_clim(const void* x, int dtype, long T, long M, int period, int phase, long b0, long b1,
                               const unsigned char* mask, double* clim, void* stream) {
    DROUGHT_CLIM_CHECKS("gd_drought_clim");
    clim_run(false, GD_S, x, dtype, M, period, phase, b0, b1, mask, clim);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_drought_clim_host(const void* x, int dtype, long T, long M, int period, int phase, long b0, long b1,
                                    const unsigned char* mask, double* clim) {
    DROUGHT_CLIM_CHECKS("gd_drought_clim_host");
    clim_run(true, nullptr, x, dtype, M, period, phase, b0, b1, mask, clim);
    return 0;
}

#define DROUGHT_INDEX_CHECKS(fn)                                                                                             \
    GD_CHECK_ARG(x && clim && out, fn ": null pointer");                                                                     \
    DROUGHT_CUBE_CHECKS(fn);                                                                                                 \
    DROUGHT_CALENDAR_CHECKS(fn);                                                                                             \
    GD_CHECK_ARG(kind == GD_DROUGHT_ANOMALY || kind == GD_DROUGHT_STANDARDIZED, fn ": kind is neither anomaly nor standardized"); \
    GD_CHECK_ARG(ddof == 0 || ddof == 1, fn ": ddof outside {0, 1}");                                                        \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_elem_aligned(out, dtype) && gd_aligned(clim, 8), fn ": pointer not element aligned")

extern "C" int gd_drought_index(const void* x, int dtype, long T, long M, const double* clim, int period, int phase, int kind, int ddof,
                                const unsigned char* mask, void* out, void* stream) {
    DROUGHT_INDEX_CHECKS("gd_drought_index");
    index_run(false, GD_S, x, dtype, T, M, clim, period, phase, kind, ddof, mask, out);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_drought_index_host(const void* x, int dtype, long T, long M, const double* clim, int period, int phase, int kind,
                                     int ddof, const unsigned char* mask, void* out) {
    DROUGHT_INDEX_CHECKS("gd_drought_index_host");
    index_run(true, nullptr, x, dtype, T, M, clim, period, phase, kind, ddof, mask, out);
    return 0;
}

#define DROUGHT_RANK_CHECKS(fn)                                                                                              \
    GD_CHECK_ARG(x && table && out, fn ": null pointer");                                                                    \
    DROUGHT_CUBE_CHECKS(fn);                                                                                                 \
    DROUGHT_CALENDAR_CHECKS(fn);                                                                                             \
    DROUGHT_BASELINE_CHECKS(fn);                                                                                             \
    GD_CHECK_ARG(nmax >= 1 && nmax <= GD_DROUGHT_MAX_N, fn ": nmax outside 1..GD_DROUGHT_MAX_N");                            \
    GD_CHECK_ARG((b1 - b0 + period - 1) / period + 1 <= nmax, fn ": nmax below ceil((b1 - b0) / period) + 1, the table is too small"); \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_elem_aligned(out, dtype) && gd_aligned(table, 8), fn ": pointer not element aligned")

extern "C" int gd_drought_rank(const void* x, int dtype, long T, long M, int period, int phase, long b0, long b1,
                               const unsigned char* mask, const double* table, int nmax, void* out, void* stream) {
    DROUGHT_RANK_CHECKS("gd_drought_rank");
    rank_run(false, GD_S, x, dtype, T, M, period, phase, b0, b1, mask, table, out);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_drought_rank_host(const void* x, int dtype, long T, long M, int period, int phase, long b0, long b1,
                                    const unsigned char* mask, const double* table, int nmax, void* out) {
    DROUGHT_RANK_CHECKS("gd_drought_rank_host");
    rank_run(true, nullptr, x, dtype, T, M, period, phase, b0, b1, mask, table, out);
    return 0;
}

#define DROUGHT_EVENTS_CHECKS(fn)                                                                                            \
    GD_CHECK_ARG(index && maps, fn ": null pointer");                                                                        \
    DROUGHT_CUBE_CHECKS(fn);                                                                                                 \
    GD_CHECK_ARG(threshold == threshold, fn ": the threshold is NaN");                                                       \
    GD_CHECK_ARG(min_duration >= 1, fn ": min_duration < 1");                                                                \
    GD_CHECK_ARG(which > 0 && which < (1 << GD_DROUGHT_EV_MAPS), fn ": no map selected or an unknown map");                  \
    GD_CHECK_ARG(gd_elem_aligned(index, dtype) && gd_aligned(maps, 8), fn ": pointer not element aligned")

extern "C" int gd_drought_events(const void* index, int dtype, long T, long M, double threshold, int min_duration, int which,
                                 const unsigned char* mask, double* maps, unsigned char* in_event, void* stream) {
    DROUGHT_EVENTS_CHECKS("gd_drought_events");
    events_run(false, GD_S, index, dtype, T, M, threshold, min_duration, which, mask, maps, in_event);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_drought_events_host(const void* index, int dtype, long T, long M, double threshold, int min_duration, int which,
                                      const unsigned char* mask, double* maps, unsigned char* in_event) {
    DROUGHT_EVENTS_CHECKS("gd_drought_events_host");
    events_run(true, nullptr, index, dtype, T, M, threshold, min_duration, which, mask, maps, in_event);
    return 0;
}

#define DROUGHT_EXCEED_CHECKS(fn)                                                                        \
    GD_CHECK_ARG(index && out, fn ": null pointer");                                                     \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                      \
    GD_CHECK_ARG(n > 0 && n < (1L << 53), fn ": n <= 0 or too many elements");                           \
    GD_CHECK_ARG(threshold == threshold, fn ": the threshold is NaN");                                   \
    GD_CHECK_ARG(gd_elem_aligned(index, dtype) && gd_elem_aligned(out, dtype), fn ": pointer not element aligned")

extern "C" int gd_drought_exceed(const void* index, int dtype, long n, double threshold, void* out, void* stream) {
    DROUGHT_EXCEED_CHECKS("gd_drought_exceed");
    exceed_run(false, GD_S, index, dtype, n, threshold, out);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_drought_exceed_host(const void* index, int dtype, long n, double threshold, void* out) {
    DROUGHT_EXCEED_CHECKS("gd_drought_exceed_host");
    exceed_run(true, nullptr, index, dtype, n, threshold, out);
    return 0;
}
