// Triple collocation (include/gandanet.h, "Triple collocation"): the listwise mean recurrence, the nine sums of one series
// or replicate, their finalising into the six covariances, the eight statistics and the flag word, and the mean / std
// recurrence over the replicates, shared by the device kernels (tcol.hip) and their host twins so both perform the same
// operations in the same order.  All arithmetic fp64, every operation rounded on its own (no contraction into FMA); the
// divisions and the sqrt are correctly rounded on both sides, so every output agrees bit for bit.  The running mean is
// gd_lag_mean_push of lagcorr_core.h; the quantiles of the replicates go through quantmap_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/gandanet.h"
#include "lagcorr_core.h"
#include "quantmap_core.h"

// the sums of one series or replicate over its counted steps: n, then Su Sv Sw Suu Svv Sww Suv Suw Svw
struct GdTcAcc {
    int n;
    double su, sv, sw, suu, svv, sww, suv, suw, svw;
};

__host__ __device__ inline GdTcAcc gd_tc_zero() { return GdTcAcc{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// One step onto the three running means: counted only if all three values are not NaN (gd_lag_mean_push leaves a NaN out,
// so a step that is not counted is handed over as three NaNs).  k: the counted steps so far.
__host__ __device__ inline void gd_tc_mean_push(int& k, double& mx, double& my, double& mz, double x, double y, double z) {
#pragma clang fp contract(off)
    const bool ok = x == x && y == y && z == z;
    const double nan = (double)NAN, inv = 1.0 / (double)(k + 1);
    int ky = k, kz = k;
    gd_lag_mean_push(k, mx, ok ? x : nan, inv);
    gd_lag_mean_push(ky, my, ok ? y : nan, inv);
    gd_lag_mean_push(kz, mz, ok ? z : nan, inv);
}

// The centred triple of one step, a NaN in any of the three making all three NaN: u == u is then the test for a counted step.
__host__ __device__ inline void gd_tc_centre(double x, double y, double z, double mx, double my, double mz, double& u, double& v, double& w) {
#pragma clang fp contract(off)
    const bool ok = x == x && y == y && z == z;
    const double nan = (double)NAN;
    u = ok ? x - mx : nan;
    v = ok ? y - my : nan;
    w = ok ? z - mz : nan;
}

// One centred triple onto the sums; a deleted step (u is NaN) adds +0.0 to every sum, which leaves a sum that started at
// +0.0 as it is.  Branch-free, the pattern of gd_lag_add.
__host__ __device__ inline void gd_tc_add(GdTcAcc& s, double u, double v, double w) {
#pragma clang fp contract(off)
    const bool ok = u == u;
    const double a = ok ? u : 0.0, b = ok ? v : 0.0, c = ok ? w : 0.0;
    s.n += ok ? 1 : 0;
    s.su += a;
    s.sv += b;
    s.sw += c;
    s.suu += a * a;
    s.svv += b * b;
    s.sww += c * c;
    s.suv += a * b;
    s.suw += a * c;
    s.svw += b * c;
}

// The six covariances (Qxx Qyy Qzz Qxy Qxz Qyz), the eight statistics and the flag word of the sums.  Below min_samples
// everything is NaN; with a cross-covariance that is not > 0 the statistics are NaN and the covariances stay.
__host__ __device__ inline int gd_tc_finish(const GdTcAcc& s, int min_samples, double* st, double* cov) {
#pragma clang fp contract(off)
    const double nan = (double)NAN;
#pragma unroll
    for (int k = 0; k < GD_TC_STATS; ++k) st[k] = nan;
#pragma unroll
    for (int k = 0; k < GD_TC_COVS; ++k) cov[k] = nan;
    if (s.n < min_samples) return GD_TC_FLAG_FEW;
    const double n = (double)s.n, n1 = (double)(s.n - 1);
    const double qxx = (s.suu - s.su * s.su / n) / n1, qyy = (s.svv - s.sv * s.sv / n) / n1, qzz = (s.sww - s.sw * s.sw / n) / n1;
    const double qxy = (s.suv - s.su * s.sv / n) / n1, qxz = (s.suw - s.su * s.sw / n) / n1, qyz = (s.svw - s.sv * s.sw / n) / n1;
    cov[0] = qxx, cov[1] = qyy, cov[2] = qzz, cov[3] = qxy, cov[4] = qxz, cov[5] = qyz;
    if (!(qxy > 0.0) || !(qxz > 0.0) || !(qyz > 0.0)) return GD_TC_FLAG_NONPOS;
    const double pyz = qxy * qxz, pxz = qxy * qyz, pxy = qxz * qyz;   // the products that estimate var(truth) Qyz, .. Qxz, .. Qxy
    st[GD_TC_ERR_VAR_X] = qxx - pyz / qyz;
    st[GD_TC_ERR_VAR_Y] = qyy - pxz / qxz;
    st[GD_TC_ERR_VAR_Z] = qzz - pxy / qxy;
    st[GD_TC_RHO2_X] = pyz / (qxx * qyz);
    st[GD_TC_RHO2_Y] = pxz / (qyy * qxz);
    st[GD_TC_RHO2_Z] = pxy / (qzz * qxy);
    st[GD_TC_BETA_Y] = qyz / qxz;
    st[GD_TC_BETA_Z] = qyz / qxy;
    int f = 0;
    f |= st[GD_TC_ERR_VAR_X] < 0.0 ? GD_TC_FLAG_NEG_X : 0;
    f |= st[GD_TC_ERR_VAR_Y] < 0.0 ? GD_TC_FLAG_NEG_Y : 0;
    f |= st[GD_TC_ERR_VAR_Z] < 0.0 ? GD_TC_FLAG_NEG_Z : 0;
    f |= (st[GD_TC_RHO2_X] > 1.0 || st[GD_TC_RHO2_Y] > 1.0 || st[GD_TC_RHO2_Z] > 1.0) ? GD_TC_FLAG_RHO2 : 0;
    return f;
}

// One replicate value onto the running mean and sum of squared deviations of a (pixel, statistic); NaN is left out.
__host__ __device__ inline void gd_tc_moment_push(int& k, double& m, double& m2, double v) {
#pragma clang fp contract(off)
    if (v == v) {
        k += 1;
        const double d = v - m;
        m = m + d * (1.0 / (double)k);
        m2 = m2 + d * (v - m);
    }
}

// mean and std (ddof 1) of the k values pushed: NaN below two
__host__ __device__ inline void gd_tc_moment_finish(int k, double m, double m2, double& mean, double& sd) {
#pragma clang fp contract(off)
    const double nan = (double)NAN;
    mean = k >= 2 ? m : nan;
    sd = k >= 2 ? sqrt(m2 / (double)(k - 1)) : nan;
}

// quantile j of n_ok >= 2 sorted keys (keys[0 .. n_ok - 1] ascending): numpy's node and _lerp
__host__ __device__ inline double gd_tc_quantile(const int64_t* keys, int n_ok, double q) {
    int prev, next;
    double g;
    gd_qm_node_index(n_ok, q, prev, next, g);
    return gd_qm_lerp(gd_qm_unkey(keys[prev]), gd_qm_unkey(keys[next]), g);
}
