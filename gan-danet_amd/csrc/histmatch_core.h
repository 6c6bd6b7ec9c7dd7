// Histogram matching (include/gandanet.h, gd_hist_match): the key order, the two binary searches and the per-element
// quantile interpolation, shared by the device kernel (histmatch.hip) and its host twin so both perform the same IEEE double
// divisions, products and sums in the same order, every operation rounded on its own (no contraction into FMA).
//
// Key order: ascending by value with every NaN last, whatever its sign bit, as np.sort / np.unique order them.  A radix
// sort orders floats by their bit pattern, which puts a NaN whose sign bit is set in FRONT of -inf; the searches below
// would then walk into a NaN head (`a[mid] <= v` is false for NaN) and return wrong ranks for finite values.  So both
// twins sort gd_hm_key(v): every NaN becomes the one positive quiet NaN, every other value is kept bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

__host__ __device__ inline float gd_hm_key(float v) { return v != v ? __builtin_nanf("") : v; }

// strict weak order of the keys: a < b, NaNs after everything else and equal among themselves
__host__ __device__ inline bool gd_hm_less(float a, float b) { return a != a ? false : (b != b ? true : a < b); }

__host__ __device__ inline long gd_hm_upper_bound(const float* a, long n, float v) {   // first index with a[i] > v
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__host__ __device__ inline long gd_hm_lower_bound(const float* a, long n, float v) {   // first index with a[i] >= v
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The adjusted value of sorted source element i: skeys (ns) and tkeys (nt) ascending with NaNs last.  A NaN source key
// gives NaN (its rank is taken as 0, the matched value is finite, and (1 - weight) * NaN is NaN at every weight).
__host__ __device__ inline double gd_hm_element(const float* skeys, long ns, const float* tkeys, long nt, double weight, long i) {
#pragma clang fp contract(off)      // numpy rounds the product and the sum separately
    const float v = skeys[i];
    const double x = (double)gd_hm_upper_bound(skeys, ns, v) / (double)ns;          // s_q of this value
    // largest count c in [0, nt] with c / nt <= x
    long c = (long)floor(x * (double)nt);
    if (c > nt) c = nt;
    if (c < 0) c = 0;
    while (c < nt && (double)(c + 1) / (double)nt <= x) ++c;
    while (c > 0 && (double)c / (double)nt > x) --c;
    double matched;
    long e = 0;                                                               // largest run end <= c
    if (c > 0) {
        const float val = tkeys[c - 1];
        e = gd_hm_upper_bound(tkeys, nt, val) == c ? c : gd_hm_lower_bound(tkeys, nt, val);
    }
    if (e == 0) {
        matched = (double)tkeys[0];                                           // x < t_q[0]
    } else if (e == nt) {
        matched = (double)tkeys[nt - 1];                                      // last unique value
    } else {
        const double fpj = (double)tkeys[e - 1], xpj = (double)e / (double)nt;
        if (xpj == x) {
            matched = fpj;
        } else {
            const float nxt = tkeys[e];
            const double xpn = (double)gd_hm_upper_bound(tkeys, nt, nxt) / (double)nt;
            const double slope = ((double)nxt - fpj) / (xpn - xpj);
            matched = slope * (x - xpj) + fpj;
        }
    }
    const float t1 = (float)(1.0 - weight) * v;                       // float32 array times a Python scalar
    return (double)t1 + weight * matched;
}
