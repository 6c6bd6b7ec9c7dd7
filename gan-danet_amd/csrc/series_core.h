// Per-pixel time series (include/gandanet.h, "Per-pixel time series"): the per-sample recurrences, the finalising of a
// record into skill maps, the normal-equation solver and the block mean, shared by the device kernels (series.hip) and
// their host twins so both perform the same operations in the same order.  All arithmetic fp64, every operation rounded on
// its own (no contraction into FMA); sqrt and the division are correctly rounded on both sides, so records, maps,
// coefficients, residual sums and block means agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// ---- the record of one series: n, mean_p, mean_t, M2_p, M2_t, C_pt, sum|p-t|, sum(p-t)^2 ---------------------------------
struct GdSeriesRec {
    double n, mp, mt, m2p, m2t, c, sae, sse;
};

__host__ __device__ inline GdSeriesRec gd_series_zero() { return GdSeriesRec{0, 0, 0, 0, 0, 0, 0, 0}; }

// One pair onto the record: the merge of "Evaluation" with a second record of one pair.  The increment of M2 is
// dp^2 n / (n + 1) with dp taken against the mean BEFORE the pair, so the rounding of the new mean does not enter it.
// Branch-free (the new record is selected at the end): the loads of an unrolled time loop are not held behind a branch.
__host__ __device__ inline void gd_series_push(GdSeriesRec& r, double p, double t, bool skip_nan) {
#pragma clang fp contract(off)
    const bool take = !skip_nan || (p == p && t == t);
    const double n1 = r.n + 1.0, inv = 1.0 / n1, f = r.n * inv;
    const double dp = p - r.mp, dt = t - r.mt, d = p - t;
    GdSeriesRec s;
    s.n = n1;
    s.mp = r.mp + dp * inv;
    s.mt = r.mt + dt * inv;
    s.m2p = r.m2p + dp * dp * f;
    s.m2t = r.m2t + dt * dt * f;
    s.c = r.c + dp * dt * f;
    s.sae = r.sae + fabs(d);
    s.sse = r.sse + d * d;
    if (take) r = s;
}

// The GD_SKILL_MAPS maps of a record, in the order of the GD_SKILL_* indices.
__host__ __device__ inline void gd_series_finalize(const GdSeriesRec& r, int ddof, double* o) {
#pragma clang fp contract(off)
    const double nan = (double)NAN;
    o[0] = r.n > 0 ? r.n : 0.0;
    if (!(r.n > 0)) {
        for (int k = 1; k < 12; ++k) o[k] = nan;
        return;
    }
    o[1] = r.mp;
    o[2] = r.mt;
    o[3] = r.mp - r.mt;
    o[4] = sqrt(r.sse / r.n);
    o[5] = r.sae / r.n;
    const double dof = r.n - (double)ddof;
    o[6] = dof > 0 ? sqrt(r.m2p / dof) : nan;
    o[7] = dof > 0 ? sqrt(r.m2t / dof) : nan;
    double cc = nan;
    if (r.m2p > 0 && r.m2t > 0) {
        cc = r.c / sqrt(r.m2p * r.m2t);
        cc = cc > 1.0 ? 1.0 : (cc < -1.0 ? -1.0 : cc);
    }
    o[8] = cc;
    // r2_score: 1 - SS_res / SS_tot; a constant truth scores 1 when the prediction is perfect, else 0; NaN stays NaN
    if (r.m2t > 0) o[9] = 1.0 - r.sse / r.m2t;
    else if (r.m2t == 0) o[9] = r.sse == 0 ? 1.0 : (r.sse > 0 ? 0.0 : nan);
    else o[9] = nan;
    if (cc == cc) {
        const double a = cc - 1.0, b = sqrt(r.m2p / r.m2t) - 1.0, g = r.mp / r.mt - 1.0;
        o[10] = 1.0 - sqrt(a * a + b * b + g * g);
    } else {
        o[10] = nan;
    }
    const double q = (r.m2p + r.m2t - 2.0 * r.c) / r.n;
    o[11] = q > 0 ? sqrt(q) : (q == q ? 0.0 : nan);
}

// ---- least squares against P basis columns -------------------------------------------------------------------------------
// the lower triangle of A^T A (entry (j, k), k <= j, at g[j (j + 1) / 2 + k]) and A^T y; every index is a compile-time
// constant once the loops are unrolled, so the 44 doubles at P = 8 stay in registers
template <int P> struct GdLsq {
    double g[P * (P + 1) / 2];
    double b[P];
    double n;
};

template <int P> __host__ __device__ inline void gd_lsq_zero(GdLsq<P>& s) {
#pragma unroll
    for (int i = 0; i < P * (P + 1) / 2; ++i) s.g[i] = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) s.b[i] = 0.0;
    s.n = 0.0;
}

// one sample y against the basis row a (P doubles); a NaN sample is left out
template <int P> __host__ __device__ inline void gd_lsq_add(GdLsq<P>& s, const double* __restrict__ a, double y) {
#pragma clang fp contract(off)
    if (!(y == y)) return;
    double r[P];
#pragma unroll
    for (int j = 0; j < P; ++j) r[j] = a[j];
#pragma unroll
    for (int j = 0; j < P; ++j) {
#pragma unroll
        for (int k = 0; k <= j; ++k) s.g[j * (j + 1) / 2 + k] += r[j] * r[k];
        s.b[j] += r[j] * y;
    }
    s.n += 1.0;
}

// Cholesky A^T A = L L^T in place, then L z = A^T y and L^T c = z.  false (c untouched) with fewer samples than columns or
// a pivot <= P 2^-52 times its diagonal entry.
template <int P> __host__ __device__ inline bool gd_lsq_solve(GdLsq<P>& s, double* c) {
#pragma clang fp contract(off)
    if (s.n < (double)P) return false;
    const double eps = (double)P * 2.220446049250313e-16;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double diag = s.g[j * (j + 1) / 2 + j];
        double d = diag;
#pragma unroll
        for (int k = 0; k < j; ++k) d -= s.g[j * (j + 1) / 2 + k] * s.g[j * (j + 1) / 2 + k];
        ok = ok && d > eps * diag;
        const double l = sqrt(d);
        s.g[j * (j + 1) / 2 + j] = l;
#pragma unroll
        for (int i = j + 1; i < P; ++i) {
            double v = s.g[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= s.g[i * (i + 1) / 2 + k] * s.g[j * (j + 1) / 2 + k];
            s.g[i * (i + 1) / 2 + j] = v / l;
        }
    }
    if (!ok) return false;
    double z[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        double v = s.b[j];
#pragma unroll
        for (int k = 0; k < j; ++k) v -= s.g[j * (j + 1) / 2 + k] * z[k];
        z[j] = v / s.g[j * (j + 1) / 2 + j];
    }
#pragma unroll
    for (int j = P - 1; j >= 0; --j) {
        double v = z[j];
#pragma unroll
        for (int k = j + 1; k < P; ++k) v -= s.g[k * (k + 1) / 2 + j] * c[k];
        c[j] = v / s.g[j * (j + 1) / 2 + j];
    }
    return true;
}

// the squared residual of one sample, y - sum_j a_j c_j with the sum in ascending j; 0 for a NaN sample
template <int P> __host__ __device__ inline double gd_lsq_resid2(const double* __restrict__ a, const double* c, double y) {
#pragma clang fp contract(off)
    if (!(y == y)) return 0.0;
    double fit = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) fit += a[j] * c[j];
    const double r = y - fit;
    return r * r;
}

// ---- block mean ----------------------------------------------------------------------------------------------------------
// the mean of the fy x fx block whose first element is x[0] (row stride W), members in row-major order; w: the weights of
// the same block (row stride W) or NULL
template <typename T>
__host__ __device__ inline double gd_block_mean_one(const T* __restrict__ x, const double* __restrict__ w, long W, int fy, int fx,
                                                    int min_count, int* count) {
#pragma clang fp contract(off)
    double sv = 0.0, sw = 0.0;
    int cnt = 0;
    for (int i = 0; i < fy; ++i) {
        for (int j = 0; j < fx; ++j) {
            const double v = (double)x[(long)i * W + j];
            if (!(v == v)) continue;
            if (w) {
                const double wi = w[(long)i * W + j];
                sv += wi * v;
                sw += wi;
            } else {
                sv += v;
                sw += 1.0;
            }
            ++cnt;
        }
    }
    *count = cnt;
    return (cnt >= min_count && cnt > 0 && sw != 0.0) ? sv / sw : (double)NAN;
}
