// STL (Cleveland et al. 1990, as netlib's stl.f and its ports compute it) one output point at a time, shared by the device
// kernel (stl.hip) and its host twin gd_stl_decompose_host so both run the same arithmetic (include/gandanet.h, "STL
// decomposition", states the rules).  Positions are 1-based as in the Fortran; element i of a series is p[(i - 1) * st], so
// the same code walks a series of an interleaved LDS image (st = series per workgroup), a cycle-subseries of it (st times
// the period) and a plain host array (st = 1).  All arithmetic fp64, every operation rounded on its own (no FMA).
//
// stl.f keeps the window's weights in an array between its loops; here a thread has no such array, so every loop computes
// the weight of a tap again from (j, xs, h) -- the same operations on the same values, hence the same weight.  The moving
// averages are window sums per output instead of a running sum along the series (an output then depends on no other
// output): the one place where the order of additions differs from stl.f.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// a strided series: element i (1-based) is p[(i - 1) * st]
struct GdStlSeries {
    const double* p;
    long st;
    __host__ __device__ inline double at(int i) const { return p[(long)(i - 1) * st]; }
};

// the tricube weight of tap j for a fit at xs with half-width h (h9 = 0.999 h, h1 = 0.001 h), times rw_j under userw
__host__ __device__ inline double gd_stl_tap(int j, int xs, double h, double h9, double h1, bool userw, const GdStlSeries& rw) {
#pragma clang fp contract(off)
    const double r = fabs((double)(j - xs));
    double w = 0.0;
    if (r <= h9) {
        if (r <= h1) {
            w = 1.0;
        } else {
            const double q = r / h;
            const double u = 1.0 - q * q * q;
            w = u * u * u;
        }
        if (userw) w = w * rw.at(j);
    }
    return w;
}

// est of stl.f: one LOESS value at xs (0 .. n + 1) from y[nleft .. nright]; false (ys untouched) when no weight is positive
__host__ __device__ inline bool gd_stl_est(const GdStlSeries& y, int n, int len, int deg, int xs, int nleft, int nright, bool userw,
                                           const GdStlSeries& rw, double* ys) {
#pragma clang fp contract(off)
    int hi = xs - nleft > nright - xs ? xs - nleft : nright - xs;
    if (len > n) hi += (len - n) / 2;
    const double h = (double)hi, h9 = 0.999 * h, h1 = 0.001 * h;
    double a = 0.0;
    for (int j = nleft; j <= nright; ++j) a += gd_stl_tap(j, xs, h, h9, h1, userw, rw);
    if (!(a > 0.0)) return false;
    const double tot = a;
    bool slope = false;
    double b = 0.0;
    a = 0.0;
    if (h > 0.0 && deg > 0) {
        for (int j = nleft; j <= nright; ++j) a += gd_stl_tap(j, xs, h, h9, h1, userw, rw) / tot * (double)j;
        b = (double)xs - a;
        double c = 0.0;
        for (int j = nleft; j <= nright; ++j) {
            const double d = (double)j - a;
            c += gd_stl_tap(j, xs, h, h9, h1, userw, rw) / tot * d * d;
        }
        if (sqrt(c) > 0.001 * (double)(n - 1)) {
            b = b / c;
            slope = true;
        }
    }
    double s = 0.0;
    for (int j = nleft; j <= nright; ++j) {
        double w = gd_stl_tap(j, xs, h, h9, h1, userw, rw) / tot;
        if (slope) w = w * (b * ((double)j - a) + 1.0);
        s += w * y.at(j);
    }
    *ys = s;
    return true;
}

// the window ess of stl.f (jump 1) has reached at position i: it starts at [1, len] and moves right by one per position
// beyond nsh = (len + 1) / 2 until it touches n
__host__ __device__ inline void gd_stl_window(int n, int len, int i, int* nleft, int* nright) {
    if (len >= n) {
        *nleft = 1;
        *nright = n;
        return;
    }
    const int nsh = (len + 1) / 2;
    int shift = i - nsh;
    shift = shift < 0 ? 0 : (shift > n - len ? n - len : shift);
    *nleft = 1 + shift;
    *nright = len + shift;
}

// ess of stl.f at position i (1 .. n): the smoothed value, or y_i where est finds no positive weight
__host__ __device__ inline double gd_stl_ess_at(const GdStlSeries& y, int n, int len, int deg, int i, bool userw,
                                                const GdStlSeries& rw) {
    if (n < 2) return y.at(i);
    int nleft, nright;
    gd_stl_window(n, len, i, &nleft, &nright);
    double ys;
    return gd_stl_est(y, n, len, deg, i, nleft, nright, userw, rw, &ys) ? ys : y.at(i);
}

// Element q (0-based, 0 .. n + 2 np - 1) of the extended cycle-subseries image C: with c = q mod np and m = q / np it is
// position m (0 .. k + 1) of the smoothed subseries w_(c+1), w_(c+1+np), ... of length k = (n - 1 - c) / np + 1; the
// positions 0 and k + 1 are extrapolated by est and fall back on the neighbouring smoothed value.
__host__ __device__ inline double gd_stl_cycle_at(const GdStlSeries& w, int n, int np, int ns, int deg, int q, bool userw,
                                                  const GdStlSeries& rw) {
    const int c = q % np, m = q / np, k = (n - 1 - c) / np + 1;
    const GdStlSeries sub = {w.p + (long)c * w.st, w.st * np}, rsub = {rw.p + (long)c * rw.st, rw.st * np};
    double v;
    if (m == 0) {
        if (gd_stl_est(sub, k, ns, deg, 0, 1, ns < k ? ns : k, userw, rsub, &v)) return v;
        return gd_stl_ess_at(sub, k, ns, deg, 1, userw, rsub);
    }
    if (m == k + 1) {
        if (gd_stl_est(sub, k, ns, deg, k + 1, k - ns + 1 > 1 ? k - ns + 1 : 1, k, userw, rsub, &v)) return v;
        return gd_stl_ess_at(sub, k, ns, deg, k, userw, rsub);
    }
    return gd_stl_ess_at(sub, k, ns, deg, m, userw, rsub);
}

// the mean of x[i .. i + len - 1] (i 1-based), added in ascending order
__host__ __device__ inline double gd_stl_ma_at(const GdStlSeries& x, int len, int i) {
    double v = 0.0;
    for (int j = 0; j < len; ++j) v += x.at(i + j);
    return v / (double)len;
}

// the position (0 .. n - 1) of r_i in the ascending order of r_1 .. r_n, equal values in the order of their indices: the
// ranks are a permutation, so exactly one element holds each order statistic
__host__ __device__ inline int gd_stl_rank(const GdStlSeries& r, int n, int i) {
    const double v = r.at(i);
    int k = 0;
    for (int j = 1; j <= n; ++j) {
        const double u = r.at(j);
        k += (u < v || (u == v && j < i)) ? 1 : 0;
    }
    return k;
}

// the bisquare robustness weight of a residual of size r against cmad = 6 median|r|
__host__ __device__ inline double gd_stl_rweight(double r, double cmad) {
#pragma clang fp contract(off)
    if (r <= 0.001 * cmad) return 1.0;
    if (r <= 0.999 * cmad) {
        const double q = r / cmad;
        const double u = 1.0 - q * q;
        return u * u;
    }
    return 0.0;
}

// ---- the fit ----------------------------------------------------------------------------------------------------------------
struct GdStlParams {
    int n, np, ns, nt, nl;          // series length, period, seasonal / trend / low-pass windows
    int isdeg, itdeg, ildeg;        // their degrees, 0 or 1
    int ni, no;                     // inner passes per outer pass; outer passes = no + 1
};

// The working images of S series side by side, element (t, s) at [t * S + s] (t 0-based): y, trend and rw hold n rows,
// w1 .. w3 n + 2 np rows, sel 2 S doubles (the two order statistics of every series).
struct GdStlWork {
    double *y, *tr, *rw, *w1, *w2, *w3, *sel;
    int S;
};
__host__ __device__ constexpr long gd_stl_work_doubles(long n, long np, long S) { return (3 * n + 3 * (n + 2 * np) + 2) * S; }
__host__ __device__ inline void gd_stl_carve(double* base, long n, long np, int S, GdStlWork* A) {
    const long a = n * S, b = (n + 2 * np) * S;
    A->y = base;
    A->tr = A->y + a;
    A->rw = A->tr + a;
    A->w1 = A->rw + a;
    A->w2 = A->w1 + b;
    A->w3 = A->w2 + b;
    A->sel = A->w3 + b;
    A->S = S;
}

// The whole fit on images that hold y (tr = 0 and rw = 1 on entry); on return tr is the trend, w3 the seasonal component
// and rw the last robustness weights.  `ex.each(count, f)` runs f(0 .. count - 1) in any order and returns when all are
// done: every step below reads only what an earlier step wrote, and writes only element idx of its own image.
template <class Exec> __host__ __device__ inline void gd_stl_fit(const Exec& ex, const GdStlWork& A, const GdStlParams& P) {
    const int S = A.S, n = P.n, np = P.np, nc = n + 2 * np;
    bool userw = false;
    for (int outer = 0;; ++outer) {
        for (int it = 0; it < P.ni; ++it) {
            // 1: detrend
            ex.each(n * S, [&](int idx) { A.w1[idx] = A.y[idx] - A.tr[idx]; });
            // 2: the smoothed cycle-subseries, each extended by one position either way: C (n + 2 np) in w2
            ex.each(nc * S, [&](int idx) {
                const int q = idx / S, s = idx - q * S;
                A.w2[idx] = gd_stl_cycle_at({A.w1 + s, S}, n, np, P.ns, P.isdeg, q, userw, {A.rw + s, S});
            });
            // 3: low-pass filter of C: moving averages of np, np and 3, then LOESS; L (n) in w1
            ex.each((n + np + 1) * S, [&](int idx) {
                const int q = idx / S, s = idx - q * S;
                A.w3[idx] = gd_stl_ma_at({A.w2 + s, S}, np, q + 1);
            });
            ex.each((n + 2) * S, [&](int idx) {
                const int q = idx / S, s = idx - q * S;
                A.w1[idx] = gd_stl_ma_at({A.w3 + s, S}, np, q + 1);
            });
            ex.each(n * S, [&](int idx) {
                const int q = idx / S, s = idx - q * S;
                A.w3[idx] = gd_stl_ma_at({A.w1 + s, S}, 3, q + 1);
            });
            ex.each(n * S, [&](int idx) {
                const int q = idx / S, s = idx - q * S;
                A.w1[idx] = gd_stl_ess_at({A.w3 + s, S}, n, P.nl, P.ildeg, q + 1, false, {A.rw + s, S});
            });
            // 4: seasonal = C[np + i] - L into w3, and the deseasonalised series into w1
            ex.each(n * S, [&](int idx) {
                const double se = A.w2[idx + np * S] - A.w1[idx];
                A.w3[idx] = se;
                A.w1[idx] = A.y[idx] - se;
            });
            // 5: trend
            ex.each(n * S, [&](int idx) {
                const int q = idx / S, s = idx - q * S;
                A.tr[idx] = gd_stl_ess_at({A.w1 + s, S}, n, P.nt, P.itdeg, q + 1, userw, {A.rw + s, S});
            });
        }
        if (outer >= P.no) break;
        // robustness weights from r = |y - trend - seasonal| and cmad = 3 (r_(m1) + r_(m2))
        ex.each(n * S, [&](int idx) { A.w1[idx] = fabs(A.y[idx] - A.tr[idx] - A.w3[idx]); });
        ex.each(n * S, [&](int idx) {
            const int q = idx / S, s = idx - q * S, m1 = n / 2 + 1, m2 = n - m1 + 1;
            const int k = gd_stl_rank({A.w1 + s, S}, n, q + 1) + 1;
            if (k == m1) A.sel[2 * s] = A.w1[idx];
            if (k == m2) A.sel[2 * s + 1] = A.w1[idx];
        });
        ex.each(n * S, [&](int idx) {
            const int q = idx / S, s = idx - q * S;
            A.rw[idx] = gd_stl_rweight(A.w1[idx], 3.0 * (A.sel[2 * s] + A.sel[2 * s + 1]));
        });
        userw = true;
    }
}
