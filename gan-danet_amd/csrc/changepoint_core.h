// Per-pixel change points (include/gandanet.h, "Per-pixel change points"): the arithmetic of one sample joining the sums of
// one candidate break, the sequential CUSUM of a series, the rules that pick a break among the candidates, and the
// formulas that finish a family.  Shared by the device kernel (changepoint.hip) and its host twin so both perform the same
// operations in the same order.  All arithmetic fp64, every operation rounded on its own (no contraction into FMA); the
// division and sqrt are correctly rounded on both sides, so every map but pt_p and cs_p (exp is each side's library)
// agrees bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// sign(a - b) as an integer
__host__ __device__ inline int gd_cp_sign(double a, double b) { return (a > b) - (a < b); }

// the window of a series: begin clamped to 0 .. T, end to begin .. T
__host__ __device__ inline void gd_cp_window(int begin, int end, int T, int* b, int* e) {
    const int lo = begin < 0 ? 0 : (begin > T ? T : begin);
    *b = lo;
    *e = end < lo ? lo : (end > T ? T : end);
}

// ---- one sample joins the sums of a candidate: `before` says whether it lies at or before the candidate k (j <= k) --------
__host__ __device__ inline void gd_cp_add(double& s1, double& s2, bool before, double v) {
#pragma clang fp contract(off)
    if (before) s1 += v;
    else s2 += v;
}

__host__ __device__ inline double gd_cp_mean(double sum, int count) { return sum / (double)count; }

// STEP, second pass: the squared deviation from the mean of the sample's own side
__host__ __device__ inline void gd_cp_add_sq(double& r1, double& r2, bool before, double y, double m1, double m2) {
#pragma clang fp contract(off)
    const double d = y - (before ? m1 : m2);
    gd_cp_add(r1, r2, before, d * d);
}

// TREND: the line of one side, filled pass by pass: tbar, ybar after the first, b = sty / stt after the second
struct GdCpLine {
    double st, sy, tbar, ybar, stt, sty, b, rss;
};

__host__ __device__ inline void gd_cp_line_zero(GdCpLine& l) { l.st = l.sy = l.stt = l.sty = l.rss = 0.0; }

__host__ __device__ inline void gd_cp_line_pass1(GdCpLine& l1, GdCpLine& l2, bool before, double t, double y) {
    gd_cp_add(l1.st, l2.st, before, t);
    gd_cp_add(l1.sy, l2.sy, before, y);
}
__host__ __device__ inline void gd_cp_line_means(GdCpLine& l, int count) {
    l.tbar = gd_cp_mean(l.st, count);
    l.ybar = gd_cp_mean(l.sy, count);
}
__host__ __device__ inline void gd_cp_line_pass2(GdCpLine& l1, GdCpLine& l2, bool before, double t, double y) {
#pragma clang fp contract(off)
    const double dt = t - (before ? l1.tbar : l2.tbar), dy = y - (before ? l1.ybar : l2.ybar);
    gd_cp_add(l1.stt, l2.stt, before, dt * dt);
    gd_cp_add(l1.sty, l2.sty, before, dt * dy);
}
__host__ __device__ inline void gd_cp_line_slope(GdCpLine& l) { l.b = l.sty / l.stt; }
__host__ __device__ inline void gd_cp_line_pass3(GdCpLine& l1, GdCpLine& l2, bool before, double t, double y) {
#pragma clang fp contract(off)
    const double dt = t - (before ? l1.tbar : l2.tbar), dy = y - (before ? l1.ybar : l2.ybar);
    const double e = dy - (before ? l1.b : l2.b) * dt;
    gd_cp_add(l1.rss, l2.rss, before, e * e);
}
__host__ __device__ inline double gd_cp_intercept(double ybar, double b, double tbar) {
#pragma clang fp contract(off)
    return ybar - b * tbar;
}
// line 2 minus line 1 half way between the last sample before and the first after the break
__host__ __device__ inline double gd_cp_jump(double a1, double b1, double a2, double b2, double tk, double tk1) {
#pragma clang fp contract(off)
    const double tm = (tk + tk1) * 0.5;
    return (a2 + b2 * tm) - (a1 + b1 * tm);
}

__host__ __device__ inline double gd_cp_rss(double r1, double r2) { return r1 + r2; }

// ---- picking among candidates: is (v, k) ahead of (bv, bk)?  Smaller value (arg-min) or larger (arg-max) first, then the
// smaller k.  A NaN value is never ahead.
__host__ __device__ inline bool gd_cp_ahead_min(double v, int k, double bv, int bk) { return v < bv || (v == bv && k < bk); }
__host__ __device__ inline bool gd_cp_ahead_max(int v, int k, int bv, int bk) { return v > bv || (v == bv && k < bk); }

// ---- finishing formulas ---------------------------------------------------------------------------------------------------
// pt_p = min(1, 2 exp(-(6 K^2) / (n^3 + n^2))): the integers are exact in doubles at n <= 2048
__host__ __device__ inline double gd_cp_pettitt_p(int K, int n) {
#pragma clang fp contract(off)
    const double k = (double)K, nn = (double)n;
    const double p = 2.0 * exp(-(6.0 * k * k) / (nn * nn * nn + nn * nn));
    return p > 1.0 ? 1.0 : p;
}

// st_f = (rss0 - rss) / (rss / (n - 2)); tr_f = ((rss0 - rss) / 2) / (rss / (n - 4)), as IEEE division gives them
__host__ __device__ inline double gd_cp_f_step(double rss0, double rss, int n) {
#pragma clang fp contract(off)
    return (rss0 - rss) / (rss / (double)(n - 2));
}
__host__ __device__ inline double gd_cp_f_trend(double rss0, double rss, int n) {
#pragma clang fp contract(off)
    return ((rss0 - rss) / 2.0) / (rss / (double)(n - 4));
}

// The CUSUM of one series of n >= 1 samples y[0 .. n - 1], sequential in time order: q, r, p and the position k of the first
// maximum of |S_k| (-1 and NaN where sd is 0 or NaN)
struct GdCpCusum {
    double q, r, p;
    int k;
};

__host__ __device__ inline double gd_cp_cusum_p(double q) {
#pragma clang fp contract(off)
    if (!(q >= 0.3)) return q == q ? 1.0 : q;
    double s = 0.0;
    for (int j = 1; j <= 20; ++j) {
        const double e = exp(-2.0 * (double)(j * j) * q * q);
        if (j & 1) s += e;
        else s -= e;
    }
    const double p = 2.0 * s;
    return p > 1.0 ? 1.0 : (p < 0.0 ? 0.0 : p);
}

__host__ __device__ inline GdCpCusum gd_cp_cusum(const double* y, int n) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += y[i];
    const double ybar = gd_cp_mean(sum, n);
    double S = 0.0, ss = 0.0, amax = -1.0, smax = 0.0, smin = 0.0;
    int kmax = -1;
    for (int i = 0; i < n; ++i) {
        const double d = y[i] - ybar;
        S += d;
        ss += d * d;
        const double a = fabs(S);
        if (a > amax) {
            amax = a;
            kmax = i;
        }
        smax = S > smax ? S : smax;
        smin = S < smin ? S : smin;
    }
    const double sd = sqrt(ss / (double)n), rn = sqrt((double)n);
    GdCpCusum c;
    if (!(sd > 0.0) || kmax < 0) {
        c.q = c.r = c.p = (double)NAN;
        c.k = -1;
        return c;
    }
    c.q = (amax / sd) / rn;
    c.r = ((smax - smin) / sd) / rn;
    c.p = gd_cp_cusum_p(c.q);
    c.k = kmax;
    return c;
}
