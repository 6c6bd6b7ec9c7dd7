// Connected components (include/gandanet.h, "Connected components"): what the device kernels (ccl.hip) and their host
// twins share -- the neighbourhood word, the foreground test, union-find over a parent array, and the fixed order of the
// fp64 sums of a track record and of a cluster's totals.
//
// Union-find.  parent[i] is -1 on background and an index of i's own component on foreground, and one invariant holds at
// every instant, in LDS and in global memory alike:
//     parent[i] <= i, and a stored parent is only ever LOWERED, by an integer atomic min.
// * find(x) follows parent until parent[x] == x.  Every step goes to a strictly smaller index, so it ends after at most x
//   steps whatever other threads do meanwhile.  A value it reads may be out of date; it is still a value that was stored
//   once, a member of the same component, so a stale read costs steps, never correctness.
// * union(a, b) takes the two roots, a > b, and does old = atomicMin(&parent[a], b).  old == a: a was a root and now hangs
//   below b, done.  Otherwise another thread lowered parent[a] to old < a first; whichever of old and b lost the min is no
//   longer recorded at a, so the thread goes on to unite old and b.  Each retry starts from a strictly smaller index than
//   the one before, so it ends.  The thread that overwrites a link re-creates it itself: no link is ever lost.
// * No thread waits for another thread or workgroup: there is no spin, no flag, no lock and no look-back anywhere.  Every
//   loop is bounded by the strictly descending index alone, so the kernels finish under any schedule, and a workgroup
//   that never runs concurrently with another still completes.
// * When all unions are done the trees are exactly the components of the graph (only neighbours inside one component are
//   ever united, and every neighbouring pair is).  The smallest index m of a component has parent[m] <= m inside the
//   component, so parent[m] == m: it is a root, and the one root.  After flattening, parent[i] is therefore the smallest
//   raster index of i's component -- a function of the input alone, whatever order the atomics landed in.
// Counts, bounds and sizes use integer atomic add / min / max, which are exact and commute.  There are no float atomics.
//
// fp64 sums.  A track record is summed by GD_CCL_TRACK_THREADS threads: thread j takes the pixels j, j + 256, ... of the
// cluster's bounding box in that plane (row-major inside the box), in ascending order; the 256 partial sums go through
// gd_block_sum_d (elem_util.h): inside each wave of 64 the butterfly v[l] += v[l ^ o], o = 32, 16, .. 1, then wave 0's
// total plus the totals of waves 1, 2, 3 in that order.  gd_ccl_block_sum_host is that order on the host.  A cluster's
// totals add its records in ascending t.  Every operation is rounded on its own (no contraction into FMA).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/gandanet.h"

#define GD_CCL_TRACK_THREADS 256
#define GD_CCL_TRACK_SUMS 5   // count, area, severity, sum a h, sum a w (the minimum is reduced apart)

// ---- the neighbourhood: bit k of the word is the backward offset (k / 9 - 1, k / 3 % 3 - 1, k % 3 - 1), k = 0 .. 12 --------
__host__ __device__ inline void gd_ccl_offset(int k, int& dt, int& dh, int& dw) {
    dt = k / 9 - 1;
    dh = k / 3 % 3 - 1;
    dw = k % 3 - 1;
}

// ---- foreground ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool gd_ccl_fg(float v, double thr) { return (double)v <= thr; }      // false for NaN
__host__ __device__ inline bool gd_ccl_fg(double v, double thr) { return v <= thr; }
__host__ __device__ inline bool gd_ccl_fg(unsigned char v, double) { return v != 0; }
template <typename X> struct gd_ccl_has_value { static constexpr bool value = true; };
template <> struct gd_ccl_has_value<unsigned char> { static constexpr bool value = false; };

// ---- union-find: `Mem` is how a parent is read and lowered (LDS, global memory, or a plain host array) --------------------
struct GdCclHostMem {
    static inline int load(const int* p) { return *p; }
    static inline int amin(int* p, int v) {
        const int old = *p;
        if (v < old) *p = v;
        return old;
    }
};
#if defined(__HIPCC__)
struct GdCclLdsMem {
    __device__ static __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ static __forceinline__ int amin(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct GdCclGlobalMem {
    __device__ static __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ static __forceinline__ int amin(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
#endif

// x is foreground.  Strictly downward: a value that is not below x (or is not an index at all) ends the walk.
template <class Mem> __host__ __device__ inline int gd_ccl_find(const int* p, int x) {
    for (;;) {
        const int y = Mem::load(p + x);
        if (y >= x || y < 0) return x;
        x = y;
    }
}

// a and b are foreground neighbours
template <class Mem> __host__ __device__ inline void gd_ccl_union(int* p, int a, int b) {
    for (;;) {
        a = gd_ccl_find<Mem>(p, a);
        b = gd_ccl_find<Mem>(p, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = Mem::amin(p + a, b);   // a > b
        if (old == a) return;                  // a was a root: it hangs below b now
        a = old;                               // old < a: unite what a pointed to with b
    }
}

// ---- track records ---------------------------------------------------------------------------------------------------------
// the partial sums of thread `tid`: the pixels tid, tid + 256, ... of the box [h0, h1] x [w0, w1] of one plane that carry
// `label`.  v: count, sum a, sum a (thr - x), sum a h, sum a w; mn: the smallest x.  Without values (uint8 input, or
// severity not asked) the severity and the minimum are not touched.
template <typename X>
__host__ __device__ inline void gd_ccl_track_thread(const X* __restrict__ x, const int* __restrict__ labels, long W, int label, int h0, int h1,
                                                    int w0, int w1, double thr, const double* __restrict__ weights, bool values, int tid,
                                                    double (&v)[GD_CCL_TRACK_SUMS], double& mn) {
#pragma clang fp contract(off)
    const long bw = (long)w1 - w0 + 1, npix = ((long)h1 - h0 + 1) * bw;
    for (long j = tid; j < npix; j += GD_CCL_TRACK_THREADS) {
        const long h = h0 + j / bw, w = w0 + j % bw, at = h * W + w;
        if (labels[at] != label) continue;
        const double a = weights ? weights[at] : 1.0;
        v[0] += 1.0;
        v[1] += a;
        v[3] += a * (double)h;
        v[4] += a * (double)w;
        if constexpr (gd_ccl_has_value<X>::value) {
            if (values) {
                const double xv = (double)x[at];
                v[2] += a * (thr - xv);
                mn = xv < mn ? xv : mn;
            }
        }
    }
}

// the order of gd_block_sum_d<GD_CCL_TRACK_SUMS, 4> over 256 partial sums, and the minimum (order-free)
inline void gd_ccl_block_sum_host(double (*part)[GD_CCL_TRACK_SUMS], const double* pmn, double* out, double& mn) {
#pragma clang fp contract(off)
    for (int q = 0; q < GD_CCL_TRACK_SUMS; ++q) {
        double tot = 0.0;
        for (int wv = 0; wv < GD_CCL_TRACK_THREADS / 64; ++wv) {
            double a[64], b[64];
            for (int l = 0; l < 64; ++l) a[l] = part[wv * 64 + l][q];
            for (int o = 32; o > 0; o >>= 1) {
                for (int l = 0; l < 64; ++l) b[l] = a[l] + a[l ^ o];
                for (int l = 0; l < 64; ++l) a[l] = b[l];
            }
            tot = wv == 0 ? a[0] : tot + a[0];
        }
        out[q] = tot;
    }
    mn = pmn[0];
    for (int j = 1; j < GD_CCL_TRACK_THREADS; ++j) mn = pmn[j] < mn ? pmn[j] : mn;
}

// the cluster of record r: the largest k with offsets[k] <= r (offsets is ascending, offsets[0] = 0, offsets[K] = R > r)
__host__ __device__ inline int gd_ccl_record_cluster(const int* offsets, int K, long r) {
    int lo = 0, hi = K;   // offsets[lo] <= r < offsets[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one record from its block sums
__host__ __device__ inline void gd_ccl_track_put(const double* v, double mn, bool values, double* rec) {
    const double nan = (double)NAN;
    rec[GD_CCL_TR_COUNT] = v[0];
    rec[GD_CCL_TR_AREA] = v[1];
    rec[GD_CCL_TR_SEVERITY] = values ? v[2] : nan;
    rec[GD_CCL_TR_SUM_H] = v[3];
    rec[GD_CCL_TR_SUM_W] = v[4];
    rec[GD_CCL_TR_MIN] = (values && v[0] > 0.0) ? mn : nan;
}

// ---- cluster totals: the records of cluster k in ascending t --------------------------------------------------------------
__host__ __device__ inline void gd_ccl_totals_one(long k, const double* __restrict__ tracks, const int* __restrict__ bounds,
                                                  const int* __restrict__ offsets, double* __restrict__ totals) {
#pragma clang fp contract(off)
    const int t0 = bounds[k * GD_CCL_BOUNDS + GD_CCL_B_T0];
    const long r0 = offsets[k], r1 = offsets[k + 1];
    double vol = 0.0, sev = 0.0, pa = -1.0, pstep = -1.0, st = 0.0, sh = 0.0, sw = 0.0;
    double pk = r1 > r0 ? tracks[r0 * GD_CCL_TRACK + GD_CCL_TR_MIN] : (double)NAN;
    for (long r = r0; r < r1; ++r) {
        const double* rec = tracks + r * GD_CCL_TRACK;
        const double a = rec[GD_CCL_TR_AREA], t = (double)(t0 + (r - r0)), m = rec[GD_CCL_TR_MIN];
        vol += a;
        sev += rec[GD_CCL_TR_SEVERITY];
        st += a * t;
        sh += rec[GD_CCL_TR_SUM_H];
        sw += rec[GD_CCL_TR_SUM_W];
        if (a > pa) {
            pa = a;
            pstep = t;
        }
        pk = m < pk ? m : pk;
    }
    double* o = totals + k * GD_CCL_TOTALS;
    o[GD_CCL_TO_VOLUME] = vol;
    o[GD_CCL_TO_SEVERITY] = sev;
    o[GD_CCL_TO_PEAK_AREA] = pa;
    o[GD_CCL_TO_PEAK_AREA_STEP] = pstep;
    o[GD_CCL_TO_PEAK] = pk;
    o[GD_CCL_TO_CENTROID_T] = st / vol;
    o[GD_CCL_TO_CENTROID_H] = sh / vol;
    o[GD_CCL_TO_CENTROID_W] = sw / vol;
}
