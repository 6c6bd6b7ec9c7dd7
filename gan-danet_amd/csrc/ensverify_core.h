// Ensemble verification (include/gandanet.h, "Ensemble verification"): the arithmetic of ONE element -- the M differences
// d_i = x_i - y in ascending order in, its CRPS, rank bin, mean error, spread, Gaussian CRPS and coverage bits out -- the
// record's layout helpers and the launch grid.  Shared by the device kernel (ensverify.hip) and its host twin so both
// perform the same operations in the same order.  All arithmetic fp64, every operation rounded on its own (no contraction
// into FMA); division and sqrt are correctly rounded on both sides, so everything but crps_gauss (erf and exp are each
// side's library) agrees bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/gandanet.h"

constexpr int GD_ENSV_THREADS = 256;   // a workgroup of stage 1
constexpr int GD_ENSV_BLOCKS = 1024;   // stage-1 workgroups at most = partial records in the workspace
constexpr int GD_ENSV_SUMS = 5;        // the float sums GD_ENSV_CRPS .. GD_ENSV_S2, in the record's order

// Stage-1 grid (gx, gy): block (bx, by) takes the planes by, by + gy, ... and of each plane the elements bx * 256 + tid,
// + gx * 256, ...  Without a mask the caller passes the whole array as ONE plane.  A function of the shape alone: the
// partials' order is part of the result.
struct GdEnsvGrid {
    int gx, gy;
};
__host__ __device__ inline GdEnsvGrid gd_ensv_grid(long planes, long hw) {
    long gx = (hw + GD_ENSV_THREADS - 1) / GD_ENSV_THREADS;
    gx = gx < 1 ? 1 : (gx > GD_ENSV_BLOCKS ? GD_ENSV_BLOCKS : gx);
    long gy = GD_ENSV_BLOCKS / gx;
    gy = gy > planes ? planes : gy;
    return GdEnsvGrid{(int)gx, (int)(gy < 1 ? 1 : gy)};
}

// ascending bitonic network over N = 8 or 32 registers; the sorted VALUES do not depend on the network
template <int N> __host__ __device__ __forceinline__ void gd_ensv_sort(double (&d)[N]) {
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const double lo = fmin(d[i], d[l]), hi = fmax(d[i], d[l]);
                    const bool up = (i & k) == 0;
                    d[i] = up ? lo : hi;
                    d[l] = up ? hi : lo;
                }
            }
        }
    }
}

struct GdEnsvElem {
    double crps, crps_gauss, e, s;   // scaled
    double abs_e, e2, s2;            // scaled: |e|, e^2 and s^2 (the variance before its root, times scale^2)
    int bin, ties;                   // less + ties / 2, and #{d_i == 0}
    int cover;                       // bit k: |e| <= z_k s
};

// the z_k of the nominal levels 0.5, 0.6826894921370859 (one sigma), 0.9 and 0.95
#define GD_ENSV_Z0 0.674489750196082
#define GD_ENSV_Z1 1.0
#define GD_ENSV_Z2 1.644853626951472
#define GD_ENSV_Z3 1.959963984540054

// d: the M differences ascending in d[0 .. M - 1] (what lies behind them is not read).  Every sum starts from +0.0 and
// runs over the sorted values in ascending order.
template <int MMAX>
__host__ __device__ __forceinline__ void gd_ensv_elem(const double (&d)[MMAX], int M, bool fair, double scale, GdEnsvElem& r) {
#pragma clang fp contract(off)
    const double dm = (double)M;
    int less = 0, ties = 0;
    double sum = 0.0, sabs = 0.0, g = 0.0;
#pragma unroll
    for (int i = 0; i < MMAX; ++i) {
        if (i < M) {
            less += d[i] < 0.0;
            ties += d[i] == 0.0;
            sum += d[i];
            sabs += fabs(d[i]);
            g += (double)(2 * i - M + 1) * d[i];
        }
    }
    const double e = sum / dm;
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < MMAX; ++i) {
        if (i < M) {
            const double t = d[i] - e;
            q += t * t;
        }
    }
    const double s2 = M > 1 ? q / (double)(M - 1) : 0.0;
    const double s = sqrt(s2);
    const double a = sabs / dm;
    const double crps = a - g / (double)(fair ? M * (M - 1) : M * M);
    const double ae = fabs(e);
    double cg = ae;
    if (s > 0.0) {
        const double z = -e / s;
        const double phi = exp(-0.5 * (z * z)) * 0.3989422804014327;      // 1 / sqrt(2 pi)
        cg = s * (z * erf(z * 0.7071067811865476) + 2.0 * phi - 0.5641895835477563);   // 1 / sqrt(pi)
    }
    r.bin = less + ties / 2;
    r.ties = ties;
    r.cover = (ae <= GD_ENSV_Z0 * s ? 1 : 0) | (ae <= GD_ENSV_Z1 * s ? 2 : 0) | (ae <= GD_ENSV_Z2 * s ? 4 : 0) |
              (ae <= GD_ENSV_Z3 * s ? 8 : 0);
    r.crps = crps * scale;
    r.crps_gauss = cg * scale;
    r.e = e * scale;
    r.s = s * scale;
    r.abs_e = fabs(r.e);
    r.e2 = r.e * r.e;
    r.s2 = s2 * (scale * scale);
}
