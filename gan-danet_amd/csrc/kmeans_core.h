// k-means on pixel series (include/gandanet.h, "Regionalisation"): the value of one sample, one term of a squared distance,
// the scan that keeps the nearest and the second nearest centroid, one weighted addend of a centroid sum, and the order of
// two (value, index) pairs of the farthest-point search, shared by the device kernels (kmeans.hip) and their host twins so
// both perform the same operations in the same order.  All arithmetic fp64, every operation rounded on its own (no
// contraction into FMA); only +, -, * occur here (the one division of gd_km_update is correctly rounded on both sides).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>

#include "../../include/gandanet.h"

// v = (x - shift) * scale.  Without a shift / scale vector the entry passes 0.0 / 1.0: x - 0.0 and v * 1.0 are exact, so the
// plain distance has the bits of the code without the two operations.
__host__ __device__ inline double gd_km_value(double x, double shift, double scale) {
#pragma clang fp contract(off)
    const double d = x - shift;
    return d * scale;
}

// false for NaN and for +-inf
__host__ __device__ inline bool gd_km_finite(double v) { return fabs(v) <= DBL_MAX; }

// one term of a squared distance: one subtraction, one square
__host__ __device__ inline double gd_km_term(double v, double c) {
#pragma clang fp contract(off)
    const double d = v - c;
    return d * d;
}

// acc += term, rounded on its own
__host__ __device__ inline void gd_km_add(double& acc, double term) {
#pragma clang fp contract(off)
    acc = acc + term;
}

// acc += w * v: one product, one addition
__host__ __device__ inline void gd_km_wadd(double& acc, double w, double v) {
#pragma clang fp contract(off)
    const double p = w * v;
    acc = acc + p;
}

// The distance d of centroid k onto the (nearest, second nearest) pair of a scan over ascending k that started from
// d1 = d2 = +inf, k1 = k2 = -1: `<` keeps the lower index on a tie, in both places.
__host__ __device__ inline void gd_km_pick(double d, int k, double& d1, int& k1, double& d2, int& k2) {
    const bool a = d < d1, b = d < d2;                                  // selects, not branches: the four stay in registers
    d2 = a ? d1 : (b ? d : d2);
    k2 = a ? k1 : (b ? k : k2);
    d1 = a ? d : d1;
    k1 = a ? k : k1;
}

// is the pair (v, i) ahead of (bv, bi) in the search for the largest value, the lowest index winning a tie?  "Nothing yet"
// is (-inf, INT_MAX), which every finite v is ahead of.  A total order on pairs with distinct i, so a reduction tree over
// it gives the same winner in any shape.
__host__ __device__ inline bool gd_km_ahead(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

// doubles of one partial slab (and of the running totals) of gd_km_update: the K * T centroid sums, then wsum, count and
// within, K each
__host__ __device__ inline long gd_km_slab_doubles(long T, int K) { return (long)K * T + 3L * K; }
