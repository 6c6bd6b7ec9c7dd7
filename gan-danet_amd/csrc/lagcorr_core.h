// Lagged correlation (include/gandanet.h, "Lagged correlation"): the mean recurrence, the six sums of one (series, lag), their
// finalising into r or an autocorrelation, and the choice of the best lag, shared by the device kernel (lagcorr.hip) and its
// host twins so both perform the same operations in the same order.  All arithmetic fp64, every operation rounded on its
// own (no contraction into FMA); sqrt and the division are correctly rounded on both sides, so curves, counts and best-lag
// planes agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// the sums of one (series, lag) over its valid pairs: n, sum u, sum v, sum u^2, sum v^2, sum u v
struct GdLagAcc {
    int n;
    double su, sv, suu, svv, suv;
};

__host__ __device__ inline GdLagAcc gd_lag_zero() { return GdLagAcc{0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// One sample onto the running mean of a series: the mean_p lane of gd_series_push (series_core.h), m += (x - m) * (1 / n')
// with `inv` = 1 / (n + 1) handed in (the device reads it from a table of correctly rounded reciprocals).  NaN is left out.
__host__ __device__ inline void gd_lag_mean_push(int& n, double& m, double x, double inv) {
#pragma clang fp contract(off)
    const double s = m + (x - m) * inv;
    if (x == x) {
        m = s;
        n += 1;
    }
}

// One pair (u, v) of centred values onto the sums; a pair with a NaN on either side adds +0.0 to every sum, which leaves a
// sum that started at +0.0 as it is.  Branch-free.
__host__ __device__ inline void gd_lag_add(GdLagAcc& s, double u, double v) {
#pragma clang fp contract(off)
    const bool ok = u == u && v == v;
    const double a = ok ? u : 0.0, b = ok ? v : 0.0;
    s.n += ok ? 1 : 0;
    s.su += a;
    s.sv += b;
    s.suu += a * a;
    s.svv += b * b;
    s.suv += a * b;
}

// Pearson r of the sums: NaN below min_pairs pairs or at a variance <= 0, clipped to [-1, 1]
__host__ __device__ inline double gd_lag_r(const GdLagAcc& s, int min_pairs) {
#pragma clang fp contract(off)
    if (s.n < min_pairs) return (double)NAN;
    const double n = (double)s.n;
    const double va = s.suu - s.su * s.su / n, vb = s.svv - s.sv * s.sv / n, c = s.suv - s.su * s.sv / n;
    if (!(va > 0.0) || !(vb > 0.0)) return (double)NAN;
    const double r = c / sqrt(va * vb);
    return r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
}

// Box-Jenkins autocorrelation c_k / c_0 with c_k = suv / n0 and c_0 = suu0 / n0, n0 the valid samples of the series and
// suu0 their sum of squares (the sums of lag 0): NaN below min_pairs pairs or at c_0 <= 0
__host__ __device__ inline double gd_lag_acf(const GdLagAcc& s, int min_pairs, int n0, double suu0) {
#pragma clang fp contract(off)
    if (s.n < min_pairs || n0 <= 0) return (double)NAN;
    const double n = (double)n0;
    const double c0 = suu0 / n, ck = s.suv / n;
    if (!(c0 > 0.0)) return (double)NAN;
    return ck / c0;
}

// is r better than the best so far (NaN = none yet)?  select 0: larger |r|, 1: larger r, 2: smaller r; strictly, so that the
// lag visited first keeps a tie
__host__ __device__ inline bool gd_lag_better(int select, double r, double best) {
    if (!(r == r)) return false;
    if (!(best == best)) return true;
    if (select == 0) return fabs(r) > fabs(best);
    if (select == 1) return r > best;
    return r < best;
}

// The best lag of the curve get_r(k), get_n(k), k = 0 .. hi - lo (lag lo + k): the lags are visited in the order 0, +1, -1,
// +2, -2, ..., so a tie goes to the smaller |l| and then to the positive lag.  o: best_lag, best_r, best_n, r0.
template <class R, class N> __host__ __device__ inline void gd_lag_best(int lo, int hi, int select, R get_r, N get_n, double* o) {
    const double nan = (double)NAN;
    double bl = nan, br = nan, bn = 0.0;
    const int dmax = (hi > -lo ? hi : -lo);
    for (int d = 0; d <= dmax; ++d) {
        for (int sgn = 0; sgn < (d ? 2 : 1); ++sgn) {
            const int l = sgn ? -d : d;
            if (l < lo || l > hi) continue;
            const double r = get_r(l - lo);
            if (gd_lag_better(select, r, br)) {
                br = r;
                bl = (double)l;
                bn = (double)get_n(l - lo);
            }
        }
    }
    o[0] = bl;
    o[1] = br;
    o[2] = bn;
    o[3] = (lo <= 0 && hi >= 0) ? get_r(-lo) : nan;
}

// effective sample size and Fisher z of a correlation (Bretherton et al. 1999); p is left to the caller's erfc
__host__ __device__ inline void gd_corr_neff_z(double r, double n, double r1a, double r1b, double* neff, double* z) {
#pragma clang fp contract(off)
    const double nan = (double)NAN;
    *neff = nan;
    *z = nan;
    if (!(r == r) || !(n == n) || !(r1a == r1a) || !(r1b == r1b)) return;
    const double q = r1a * r1b;
    double ne = n * (1.0 - q) / (1.0 + q);
    if (!(ne == ne)) return;
    ne = ne < 0.0 ? 0.0 : (ne > n ? n : ne);
    *neff = ne;
    if (ne > 3.0) *z = atanh(r) * sqrt(ne - 3.0);
}
