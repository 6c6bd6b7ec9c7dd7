// Drought analysis (include/gandanet.h, "Drought analysis"): the work on ONE series of a (T, M) cube -- calendar
// climatology, parametric and rank indices, the run-theory scan -- shared by the device kernels (drought.hip) and their
// host twins, so both perform the same operations in the same order.  All arithmetic fp64, every operation rounded on its
// own (no contraction into FMA); sqrt and the division are correctly rounded on both sides, and nothing transcendental is
// evaluated here (the rank index reads a table its caller built), so every output agrees bit for bit.
// A series is addressed as x[t * M] from its own column pointer; outputs likewise.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/gandanet.h"

// the first step t >= lo whose slot (t + phase) mod period is s
__host__ __device__ inline long gd_drought_first(long lo, int s, int period, int phase) {
    const long r = ((long)s - phase - lo) % period;
    return lo + (r < 0 ? r + period : r);
}

// ---- climatology: n, mean, M2 of every slot over the baseline steps that are not NaN, in time order ----------------------
// The recurrence is that of gd_series_push (series_core.h): with d = v - mean taken against the mean BEFORE the sample,
// mean += d / (n + 1) and M2 += d * d * (n / (n + 1)).  Slots in the outer loop: three accumulators, no array indexed by
// t mod period; every element of the baseline is read once.  An empty slot (and every slot of a series with live == false)
// has n = 0 and NaN mean and M2.  rec: the series' column of the (3, period, M) record.
template <typename T>
__host__ __device__ inline void gd_drought_clim_one(const T* __restrict__ x, long M, int period, int phase, long b0, long b1, bool live,
                                                    double* __restrict__ rec) {
#pragma clang fp contract(off)
    for (int s = 0; s < period; ++s) {
        double n = 0.0, mean = 0.0, m2 = 0.0;
        if (live) {
#pragma unroll 4
            for (long t = gd_drought_first(b0, s, period, phase); t < b1; t += period) {
                const double v = (double)x[t * M];
                const bool take = v == v;
                const double n1 = n + 1.0, inv = 1.0 / n1, f = n * inv, d = v - mean;
                const double mean1 = mean + d * inv, m21 = m2 + d * d * f;
                n = take ? n1 : n;
                mean = take ? mean1 : mean;
                m2 = take ? m21 : m2;
            }
        }
        const bool has = n > 0.0;
        rec[(long)s * M] = n;
        rec[((long)period + s) * M] = has ? mean : (double)NAN;
        rec[(2L * period + s) * M] = has ? m2 : (double)NAN;
    }
}

// ---- parametric indices: x - mean_s, or that over sqrt(M2_s / (n_s - ddof)), rounded once to the storage type ------------
template <typename T>
__host__ __device__ inline void gd_drought_index_one(const T* __restrict__ x, long Tn, long M, const double* __restrict__ rec, int period,
                                                     int phase, int kind, int ddof, bool live, T* __restrict__ out) {
#pragma clang fp contract(off)
    const double nan = (double)NAN;
    for (int s = 0; s < period; ++s) {
        const long t0 = gd_drought_first(0, s, period, phase);
        if (t0 >= Tn) continue;
        const double n = rec[(long)s * M];
        const double mean = (live && n > 0.0) ? rec[((long)period + s) * M] : nan;
        double sd = nan;
        if (kind == GD_DROUGHT_STANDARDIZED) {
            const double m2 = rec[(2L * period + s) * M], dof = n - (double)ddof;
            if (dof > 0.0 && m2 > 0.0) sd = sqrt(m2 / dof);
        }
#pragma unroll 4
        for (long t = t0; t < Tn; t += period) {
            const double a = (double)x[t * M] - mean;
            out[t * M] = (T)(kind == GD_DROUGHT_STANDARDIZED ? a / sd : a);
        }
    }
}

// ---- rank index: the table entry of the sample's midrank among the baseline samples of its slot --------------------------
// B = the baseline samples of the slot that are not NaN, and the sample itself when its step lies outside the baseline;
// n = |B|, k = 2 #{b < v} + #{b == v} (1 <= k <= 2 n - 1 as v is in B), out = table[(n - 1)^2 + (k - 1)].  n never exceeds
// ceil((b1 - b0) / period) + 1, which the entry points hold to nmax, so the index stays below nmax^2.
template <typename T>
__host__ __device__ inline void gd_drought_rank_one(const T* __restrict__ x, long Tn, long M, int period, int phase, long b0, long b1,
                                                    bool live, const double* __restrict__ table, T* __restrict__ out) {
    for (int s = 0; s < period; ++s) {
        const long tb0 = gd_drought_first(b0, s, period, phase);
        for (long t = gd_drought_first(0, s, period, phase); t < Tn; t += period) {
            const T v = x[t * M];
            if (!live || !(v == v)) {
                out[t * M] = (T)NAN;
                continue;
            }
            int n = 0, less = 0, eq = 0;
#pragma unroll 4
            for (long tb = tb0; tb < b1; tb += period) {
                const T b = x[tb * M];
                n += b == b;
                less += b < v;
                eq += b == v;
            }
            if (t < b0 || t >= b1) {
                ++n;
                ++eq;
            }
            const int k = 2 * less + eq;
            out[t * M] = (T)table[(long)(n - 1) * (n - 1) + (k - 1)];
        }
    }
}

// ---- events by run theory: one scan in time order --------------------------------------------------------------------------
// dry: v <= threshold (never for NaN).  An event is a maximal run of dry steps of length >= min_duration; its severity is
// sum (threshold - v) over its steps in time order.  o: the GD_DROUGHT_EV_MAPS maps in enum order.  ev: the series' column of
// the (T, M) in_event bytes or NULL; every byte of the column is written, 1 on the steps of events.
template <typename T>
__host__ __device__ inline void gd_drought_events_one(const T* __restrict__ x, long Tn, long M, double threshold, int min_duration,
                                                      bool live, double* o, unsigned char* __restrict__ ev) {
#pragma clang fp contract(off)
    const double nan = (double)NAN;
    if (!live) {
        for (int k = 0; k < GD_DROUGHT_EV_MAPS; ++k) o[k] = nan;
        o[GD_DROUGHT_EV_N_VALID] = o[GD_DROUGHT_EV_N_DRY] = o[GD_DROUGHT_EV_N_EVENTS] = o[GD_DROUGHT_EV_EVENT_STEPS] = 0.0;
        o[GD_DROUGHT_EV_MAX_DURATION] = o[GD_DROUGHT_EV_LAST_RUN] = 0.0;
        if (ev) {
            for (long t = 0; t < Tn; ++t) ev[t * M] = 0;
        }
        return;
    }
    long n_valid = 0, n_dry = 0, n_ev = 0, ev_steps = 0, max_dur = 0, run = 0, run_start = 0, longest_start = -1, worst_start = -1;
    double sev = 0.0, run_min = 0.0, max_sev = 0.0, total = 0.0, peak = nan;
    for (long t = 0; t <= Tn; ++t) {          // step Tn closes a run that is still open
        const double v = t < Tn ? (double)x[t * M] : nan;
        if (v <= threshold) {
            const double d = threshold - v;
            if (run == 0) {
                run_start = t;
                sev = d;
                run_min = v;
            } else {
                sev += d;
                run_min = v < run_min ? v : run_min;
            }
            ++run;
            ++n_dry;
        } else {
            if (t == Tn) o[GD_DROUGHT_EV_LAST_RUN] = (double)run;
            if (run >= min_duration) {
                ++n_ev;
                ev_steps += run;
                if (run > max_dur) {
                    max_dur = run;
                    longest_start = run_start;
                }
                if (n_ev == 1 || sev > max_sev) {
                    max_sev = sev;
                    worst_start = run_start;
                }
                total += sev;
                peak = (n_ev == 1 || run_min < peak) ? run_min : peak;
                if (ev) {
                    for (long u = run_start; u < t; ++u) ev[u * M] = 1;
                }
            }
            run = 0;
        }
        if (t < Tn) {
            n_valid += v == v;
            if (ev) ev[t * M] = 0;
        }
    }
    o[GD_DROUGHT_EV_N_VALID] = (double)n_valid;
    o[GD_DROUGHT_EV_N_DRY] = (double)n_dry;
    o[GD_DROUGHT_EV_N_EVENTS] = (double)n_ev;
    o[GD_DROUGHT_EV_EVENT_STEPS] = (double)ev_steps;
    o[GD_DROUGHT_EV_MAX_DURATION] = (double)max_dur;
    o[GD_DROUGHT_EV_MEAN_DURATION] = n_ev > 0 ? (double)ev_steps / (double)n_ev : nan;
    o[GD_DROUGHT_EV_MAX_SEVERITY] = max_sev;
    o[GD_DROUGHT_EV_TOTAL_SEVERITY] = total;
    o[GD_DROUGHT_EV_PEAK] = peak;
    o[GD_DROUGHT_EV_LONGEST_START] = (double)longest_start;
    o[GD_DROUGHT_EV_WORST_START] = (double)worst_start;
}

// the `which` maps of o to their planes, in enum order
__host__ __device__ inline void gd_drought_events_put(const double* o, int which, long M, double* __restrict__ maps) {
    long j = 0;
#pragma unroll
    for (int k = 0; k < GD_DROUGHT_EV_MAPS; ++k) {
        if (which >> k & 1) {
            maps[j * M] = o[k];
            ++j;
        }
    }
}

// ---- indicator: 1 where v <= threshold, 0 where not, NaN where v is NaN ----------------------------------------------------
template <typename T> __host__ __device__ inline T gd_drought_exceed_one(T v, double threshold) {
    return v == v ? (T)((double)v <= threshold ? 1.0 : 0.0) : v;
}
