// Spatial spectra (include/gandanet.h, "Spatial spectra"): the per-element arithmetic shared by the device kernels
// (spectra.hip) and their host twins -- validity, the detrended and tapered sample, the plane fit from its ten sums, the
// power and cross terms of one wavenumber -- and the tile geometry of the DFT kernel.  All arithmetic fp64, every operation
// rounded on its own (no contraction into FMA): Re/Im products of a field with itself cancel exactly.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/gandanet.h"

#define GD_SPEC_TILE 8   // real columns of a tile are 2 * GD_SPEC_TILE: 8 kx of one field, or 4 kx of each of two

enum { GD_SPEC_DETREND_NONE = 0, GD_SPEC_DETREND_MEAN = 1, GD_SPEC_DETREND_PLANE = 2 };

// kx = 0 .. W / 2
static inline long gd_spec_kx(long W) { return W / 2 + 1; }
// tiles of kx per field: nf = 1 (power) or 2 (cross)
static inline long gd_spec_tiles(long W, int nf) { return (gd_spec_kx(W) + GD_SPEC_TILE / nf - 1) / (GD_SPEC_TILE / nf); }

__host__ __device__ inline bool gd_spec_finite(double v) { return fabs(v) < (double)INFINITY; }   // false for NaN too

// the Hermitian weight of column kx
__host__ __device__ inline double gd_spec_hweight(int kx, int W) { return (kx == 0 || 2 * kx == W) ? 1.0 : 2.0; }

// centred coordinates: u = i - (H - 1) / 2, v = j - (W - 1) / 2, exact
__host__ __device__ inline double gd_spec_centre(int n) { return 0.5 * (double)(n - 1); }

// the detrended, tapered sample; exactly 0 for an invalid pixel (a select: the sample may be NaN)
__host__ __device__ inline double gd_spec_sample(double x, bool ok, double a, double b, double c, double u, double v, double wy,
                                                 double wx) {
#pragma clang fp contract(off)
    const double plane = (a + b * u) + c * v;
    const double d = ((x - plane) * wy) * wx;
    return ok ? d : 0.0;
}

// ---- the detrend coefficients of one field from its sums --------------------------------------------------------------------
// first pass: n, sum u, sum v, sum x, S = sum wy^2 wx^2 over the valid pixels
// second pass (about the means of the first): Suu, Svv, Suv, Sux, Svx
// plane: a + b u + c v by least squares; a rank-deficient fit (all valid pixels in one row, one column or on one line)
// keeps the slope that is determined (one row: c; one column: b) or none.
struct GdSpecMeans {
    double n, um, vm, xm;
};
__host__ __device__ inline GdSpecMeans gd_spec_means(double n, double su, double sv, double sx) {
#pragma clang fp contract(off)
    GdSpecMeans m;
    m.n = n;
    m.um = n > 0.0 ? su / n : 0.0;
    m.vm = n > 0.0 ? sv / n : 0.0;
    m.xm = n > 0.0 ? sx / n : 0.0;
    return m;
}
__host__ __device__ inline void gd_spec_solve(const GdSpecMeans& m, int detrend, double suu, double svv, double suv, double sux,
                                              double svx, double* coef) {
#pragma clang fp contract(off)
    double a = 0.0, b = 0.0, c = 0.0;
    if (m.n > 0.0 && detrend == GD_SPEC_DETREND_MEAN) a = m.xm;
    if (m.n > 0.0 && detrend == GD_SPEC_DETREND_PLANE) {
        const double det = suu * svv - suv * suv;
        if (suu > 0.0 && svv > 0.0 && det > 1e-12 * (suu * svv)) {
            b = (sux * svv - svx * suv) / det;
            c = (svx * suu - sux * suv) / det;
        } else if (suu > 0.0 && !(svv > 0.0)) {
            b = sux / suu;
        } else if (svv > 0.0 && !(suu > 0.0)) {
            c = svx / svv;
        }
        a = (m.xm - b * m.um) - c * m.vm;
    }
    coef[0] = a;
    coef[1] = b;
    coef[2] = c;
}

// ---- one wavenumber ------------------------------------------------------------------------------------------------------
// weight * |Z|^2, not yet divided by H W S
__host__ __device__ inline double gd_spec_pow(double zre, double zim, double w) {
#pragma clang fp contract(off)
    return w * (zre * zre + zim * zim);
}
// weight * Re(Za conj Zb) and weight * Im(Za conj Zb); for Za == Zb the second is exactly 0
__host__ __device__ inline double gd_spec_co(double are, double aim, double bre, double bim, double w) {
#pragma clang fp contract(off)
    return w * (are * bre + aim * bim);
}
__host__ __device__ inline double gd_spec_quad(double are, double aim, double bre, double bim, double w) {
#pragma clang fp contract(off)
    return w * (aim * bre - are * bim);
}
// a bin sum over its norm H W S; NaN for a field with no valid pixel
__host__ __device__ inline double gd_spec_norm(double sum, double hw, double s, bool any) {
#pragma clang fp contract(off)
    return any ? sum / (hw * s) : (double)NAN;
}
