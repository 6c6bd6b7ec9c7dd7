// Per-pixel trend tests (include/gandanet.h, "Per-pixel trend tests"): the arithmetic of one pair of samples, the monotone
// 64-bit key of a slope, and the formulas that turn the integer sums of a series into var_s, z, p, tau and the ranks of
// the confidence interval.  Shared by the device kernel (trend.hip) and its host twin so both perform the same operations
// in the same order.  All arithmetic fp64, every operation rounded on its own (no contraction into FMA); the division,
// sqrt and rint are correctly rounded on both sides, so every map but p (erfc is each side's library) agrees bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// sign(b - a) as an integer
__host__ __device__ inline int gd_trend_sign(double a, double b) { return (b > a) - (b < a); }

// the slope of the pair (t_i, y_i), (t_j, y_j), i < j: one subtraction over one subtraction, divided once; a zero of
// either sign becomes +0.0 so that all zeros share one key
__host__ __device__ inline double gd_trend_slope(double ti, double yi, double tj, double yj) {
#pragma clang fp contract(off)
    const double v = (yj - yi) / (tj - ti);
    return v == 0.0 ? 0.0 : v;
}

// the order of doubles as an order of unsigned 64-bit keys: negative values have all bits flipped, the others the sign bit
__host__ __device__ inline uint64_t gd_trend_key(double v) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__host__ __device__ inline double gd_trend_unkey(uint64_t k) {
    return __builtin_bit_cast(double, k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull));
}

// the median of an even or odd count from its two middle order statistics, as np.median forms it
__host__ __device__ inline double gd_trend_mid(double a, double b) {
#pragma clang fp contract(off)
    return (a + b) * 0.5;
}

__host__ __device__ inline double gd_trend_intercept(double med_y, double slope, double med_t) {
#pragma clang fp contract(off)
    return med_y - slope * med_t;
}

// The integer sums of one series (over its seasons, where it has them): n valid samples; s = sum of sign(y_j - y_i) over
// the counted pairs; k1 = sum over samples of (n_g - 1)(2 n_g + 5) = sum over seasons of n_g (n_g - 1)(2 n_g + 5); tie =
// sum over samples of (c_i - 1)(2 c_i + 5); tot2 = sum over samples of (n_g - 1) = 2 tot; ytie2 = sum of (c_i - 1) = 2 ytie
// (n_g: the samples of the sample's season, c_i: those of them equal to y_i).
struct GdTrendSums {
    long long n, s, k1, tie, tot2, ytie2;
};

struct GdTrendStats {
    double var_s, z, p, tau;
    long long nt;   // the number of slopes
};

__host__ __device__ inline GdTrendStats gd_trend_stats(const GdTrendSums& u, bool continuity) {
#pragma clang fp contract(off)
    const double nan = (double)NAN;
    GdTrendStats r;
    r.nt = u.tot2 / 2;
    if (u.n < 2) {
        r.var_s = r.z = r.p = r.tau = nan;
        return r;
    }
    r.var_s = (1.0 / 18.0) * (double)(u.k1 - u.tie);
    if (!(r.var_s > 0.0)) r.z = nan;
    else if (u.s == 0) r.z = 0.0;
    else r.z = (double)(continuity ? u.s - (u.s > 0 ? 1 : -1) : u.s) / sqrt(r.var_s);
    r.p = erfc(fabs(r.z) * 0.7071067811865476);
    const long long tot = u.tot2 / 2, ytie = u.ytie2 / 2;
    if (ytie == tot) {
        r.tau = nan;
    } else {
        const double tau = (double)u.s / sqrt((double)tot) / sqrt((double)(tot - ytie));
        r.tau = tau > 1.0 ? 1.0 : (tau < -1.0 ? -1.0 : tau);
    }
    return r;
}

// the ranks of the interval among nt >= 1 sorted slopes: Ru = min(rint((nt - zq sigma) / 2), nt - 1) and
// Rl = max(rint((nt + zq sigma) / 2) - 1, 0), rint to even; both are kept inside 0 .. nt - 1
__host__ __device__ inline void gd_trend_ranks(long long nt, double var_s, double zq, long long* rl, long long* ru) {
#pragma clang fp contract(off)
    const double sigma = sqrt(var_s);
    const double hi = rint(((double)nt - zq * sigma) / 2.0), lo = rint(((double)nt + zq * sigma) / 2.0);
    long long u = hi >= (double)(nt - 1) ? nt - 1 : (long long)hi;   // also the NaN-free form of min()
    long long l = lo - 1.0 <= 0.0 ? 0 : (long long)lo - 1;
    *ru = u < 0 ? 0 : u;
    *rl = l > nt - 1 ? nt - 1 : l;
}
