// EOF analysis (include/gandanet.h, "EOF analysis"): the per-series arithmetic shared by the device kernels (eof.hip) and
// their host twins, so both perform the same operations in the same order -- the validity and mean of a series, the
// weighted anomaly, the projection of a series on K coefficient columns and the rank-K reconstruction -- and the split
// geometry of the Gram kernel.  All arithmetic fp64, every operation rounded on its own (no contraction into FMA); sqrt and
// the division are correctly rounded on both sides, so means, validity bytes, pattern maps and reconstructions agree bit
// for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// ---- geometry of gd_eof_gram: a function of (T, M) alone, part of the result's bits -----------------------------------------
#define GD_EOF_CHUNK 32        // series a workgroup stages at a time
#define GD_EOF_SPLIT_MIN 8     // chunks a split holds at least (256 series)
#define GD_EOF_SPLIT_MAX 256   // splits at most: one workgroup per CU, and splits * nblk * 2 KiB of partial slabs
struct GdEofGeom {
    int nb;       // 16-row blocks: ceil(T / 16)
    int nblk;     // blocks on and above the diagonal: nb (nb + 1) / 2
    long chunks;  // ceil(M / GD_EOF_CHUNK)
    long per;     // chunks per split
    int splits;   // ceil(chunks / per), every split holds at least one chunk
};
static inline GdEofGeom gd_eof_geom(long T, long M) {
    GdEofGeom g;
    g.nb = (int)((T + 15) / 16);
    g.nblk = g.nb * (g.nb + 1) / 2;
    g.chunks = (M + GD_EOF_CHUNK - 1) / GD_EOF_CHUNK;
    long s = (g.chunks + GD_EOF_SPLIT_MIN - 1) / GD_EOF_SPLIT_MIN;
    s = s < 1 ? 1 : (s > GD_EOF_SPLIT_MAX ? GD_EOF_SPLIT_MAX : s);
    g.per = (g.chunks + s - 1) / s;
    g.splits = (int)((g.chunks + g.per - 1) / g.per);
    return g;
}

__host__ __device__ inline bool gd_eof_finite(double v) { return fabs(v) < (double)INFINITY; }   // false for NaN too

// ---- validity and mean of one series (stride M), samples in ascending t ------------------------------------------------------
template <typename T>
__host__ __device__ inline void gd_eof_prepare_one(const T* __restrict__ y, long Tn, long M, bool mask_ok, bool has_w, double w,
                                                   int center, double* mean, unsigned char* valid) {
#pragma clang fp contract(off)
    bool ok = mask_ok && (!has_w || (gd_eof_finite(w) && w > 0.0));
    double s = 0.0;
#pragma unroll 4
    for (long t = 0; t < Tn; ++t) {
        const double v = (double)y[t * M];
        ok = ok && gd_eof_finite(v);
        s += v;
    }
    *valid = ok ? 1 : 0;
    *mean = (ok && center) ? s / (double)Tn : 0.0;
}

// the weighted anomaly: a select, not a multiplication (NaN * 0 is NaN)
__host__ __device__ inline double gd_eof_anom(double v, double mean, double sw, bool ok) {
#pragma clang fp contract(off)
    const double a = sw * (v - mean);
    return ok ? a : 0.0;
}

// ---- projection of one series on KC coefficient columns (K <= KC of them live) ------------------------------------------------
// out[k] = s * sum_t coef[t * K + k] * (y[t] - mean), ascending t from +0.0; NaN for an invalid series
template <typename T, int KC>
__host__ __device__ inline void gd_eof_project_one(const T* __restrict__ y, long Tn, long M, double mean, bool ok, double s,
                                                   const double* __restrict__ coef, int K, double* __restrict__ out, long m) {
#pragma clang fp contract(off)
    double acc[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) acc[k] = 0.0;
#pragma unroll 2
    for (long t = 0; t < Tn; ++t) {
        const double d = (double)y[t * M] - mean;
        const double* c = coef + t * K;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            if (k < K) acc[k] += c[k] * d;
        }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        if (k < K) out[(long)k * M + m] = ok ? s * acc[k] : (double)NAN;
    }
}

// ---- rank-K reconstruction of one series -------------------------------------------------------------------------------------
// out[t] = mean + (sum_k pcs[t * K + k] * e[k]) / sw, ascending k from +0.0, one rounding to O; NaN for an invalid series
template <typename O, int KC>
__host__ __device__ inline void gd_eof_reconstruct_one(const double* __restrict__ eofs, const double* __restrict__ pcs, double mean, bool ok,
                                                       bool has_w, double sw, long Tn, long M, int K, O* __restrict__ out, long m) {
#pragma clang fp contract(off)
    double e[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) e[k] = k < K ? eofs[(long)k * M + m] : 0.0;
#pragma unroll 2
    for (long t = 0; t < Tn; ++t) {
        const double* p = pcs + t * K;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            if (k < K) s += p[k] * e[k];
        }
        if (has_w) s = s / sw;
        out[t * M + m] = ok ? (O)(mean + s) : (O)NAN;
    }
}
