// The containment rule of the basin analysis (include/gandanet.h, "Basin analysis"), shared by the device rasteriser and
// its host twin so both run the same arithmetic.  A zone is a set of rings (outer rings and holes of all its parts, any
// order, any orientation); a point is inside iff an odd number of ring edges count for it.  Edge (x0, y0)-(x1, y1) counts
// for the point (px, py) iff it straddles the point's row under the half-open rule and its crossing of that row lies
// strictly to the right of px.  Points exactly on a boundary are unspecified.
#pragma once
#include <hip/hip_runtime.h>

// half-open in y: a horizontal edge never counts and a ray through a vertex counts once
__host__ __device__ inline bool gd_zone_edge_straddles(double y0, double y1, double py) { return (y0 > py) != (y1 > py); }

// x of the edge at height py, in fp64; every operation rounded on its own (no FMA), on the host and on the device alike.
// Only called for a straddling edge, so y1 != y0.
__host__ __device__ inline double gd_zone_edge_intercept(double x0, double y0, double x1, double y1, double py) {
#pragma clang fp contract(off)
    const double num = (py - y0) * (x1 - x0);
    const double q = num / (y1 - y0);
    return x0 + q;
}

// the second half of the predicate: the crossing xi counts for the column at px
__host__ __device__ inline bool gd_zone_crossing_counts(double px, double xi) { return px < xi; }
