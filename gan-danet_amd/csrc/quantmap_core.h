// Bias correction (include/gandanet.h, "Bias correction"): the work on ONE sample or ONE element -- the order-preserving
// integer key of a double, the compare-exchange schedule of the bitonic sort, numpy's quantile node (index, weight and
// _lerp) and numpy's interp (bracket and expression) -- shared by the device kernels (quantmap.hip) and their host twins,
// so both perform the same operations in the same order.  All arithmetic fp64, every operation rounded on its own (no
// contraction into FMA: numpy's expressions are unfused); the division is correctly rounded on both sides and nothing
// transcendental is evaluated, so every output agrees bit for bit with the twin and with numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gandanet.h"

// the first step t >= lo whose slot (t + phase) mod period is s
__host__ __device__ inline long gd_qm_first(long lo, int s, int period, int phase) {
    const long r = ((long)s - phase - lo) % period;
    return lo + (r < 0 ? r + period : r);
}

// ---- keys: a double that is not NaN as an int64 that orders as the value does, -0.0 below +0.0 -----------------------------
// (the transform is its own inverse).  GD_QM_PAD sorts behind every key, +inf's included.
#define GD_QM_PAD INT64_MAX
__host__ __device__ inline int64_t gd_qm_key(double v) {
    const int64_t b = __builtin_bit_cast(int64_t, v);
    return b < 0 ? (b ^ INT64_MAX) : b;
}
__host__ __device__ inline double gd_qm_unkey(int64_t k) { return __builtin_bit_cast(double, k < 0 ? (k ^ INT64_MAX) : k); }

// ---- bitonic sort, ascending, over P = 2^r keys: stage k = 2, 4 .. P, step j = k/2 .. 1 ----------------------------------
// pair number `idx` (0 <= idx < P / 2) of step (k, j): positions i < l = i + j; up: the smaller key goes to i
__host__ __device__ inline void gd_qm_bitonic_pair(int idx, int k, int j, int& i, int& l, bool& up) {
    i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1));
    l = i | j;
    up = (i & k) == 0;
}
// the network over N registers (N a power of two, every index static after unrolling)
template <int N> __host__ __device__ __forceinline__ void gd_qm_sort_regs(int64_t (&d)[N]) {
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const bool sw = ((i & k) == 0) ? (d[l] < d[i]) : (d[i] < d[l]);
                    const int64_t a = d[i], b = d[l];
                    d[i] = sw ? b : a;
                    d[l] = sw ? a : b;
                }
            }
        }
    }
}

// ---- numpy's quantile node (method "linear") of n >= 1 sorted samples at probability q ------------------------------------
// v = (n - 1) q; i = floor(v), g = v - i; where v >= n - 1 numpy sets both indices to -1 (the last sample) and takes g
// against that -1: g = v + 1.  The indices are held to [0, n - 1] so that a q outside [0, 1] reads nothing else.
__host__ __device__ inline void gd_qm_node_index(int n, double q, int& prev, int& next, double& g) {
#pragma clang fp contract(off)
    const double last = (double)(n - 1), v = last * q;
    if (v >= last) {
        prev = next = n - 1;
        g = v - (-1.0);
    } else {
        const double fl = floor(v);
        int i = (int)fl;
        i = i < 0 ? 0 : i;
        prev = i > n - 1 ? n - 1 : i;
        next = i + 1 > n - 1 ? n - 1 : i + 1;
        g = v - fl;
    }
}
// numpy's _lerp: a + (b - a) g, replaced by b - (b - a) (1 - g) where g >= 0.5
__host__ __device__ inline double gd_qm_lerp(double a, double b, double g) {
#pragma clang fp contract(off)
    const double d = b - a;
    const double lo = a + d * g;
    const double hi = b - d * (1.0 - g);
    return g >= 0.5 ? hi : lo;
}

// ---- numpy's interp over a table of Q >= 2 ascending nodes ----------------------------------------------------------------
// a strided column of doubles as a function of the node number
struct GdQmCol {
    const double* p;
    long stride;
    __host__ __device__ double operator()(int j) const { return p[(long)j * stride]; }
};

// the last j with xp(j) <= x, for xp(0) <= x (numpy's binary_search_with_guess returns that j for ascending nodes)
template <class XP> __host__ __device__ inline int gd_qm_bracket(double x, int Q, const XP& xp) {
    int lo = 1, hi = Q;   // xp(0) <= x is known
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (x >= xp(mid)) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// numpy.interp's value for the bracket j of x (arr_interp of compiled_base.c): fp(j) at the last node and on a node, else
// slope (x - xp(j)) + fp(j) with slope = (fp(j+1) - fp(j)) / (xp(j+1) - xp(j)); a NaN (infinite nodes) is retried from the
// right node, then replaced by fp(j) where both ends agree
template <class XP, class FP> __host__ __device__ inline double gd_qm_interp_at(double x, int j, int Q, const XP& xp, const FP& fp) {
#pragma clang fp contract(off)
    const double x0 = xp(j), y0 = fp(j);
    if (j >= Q - 1 || x0 == x) return y0;
    const double x1 = xp(j + 1), y1 = fp(j + 1);
    const double slope = (y1 - y0) / (x1 - x0);
    double r = slope * (x - x0) + y0;
    if (r != r) {
        r = slope * (x - x1) + y1;
        if (r != r && y0 == y1) r = y0;
    }
    return r;
}

// ---- one element of gd_qm_apply ---------------------------------------------------------------------------------------------
// mq, oq: the model and observation nodes of the element's slot and parent pixel; own: those of the element's own series
// (GD_QM_QDM only); p: the node probabilities (GD_QM_QDM only)
__host__ __device__ inline double gd_qm_apply_one(double x, int Q, const GdQmCol& mq, const GdQmCol& oq, const GdQmCol& own, const double* p,
                                                  int kind, int extrapolate) {
#pragma clang fp contract(off)
    const double nan = (double)NAN;
    const double m0 = mq(0), o0 = oq(0);
    if (x != x || m0 != m0 || o0 != o0) return nan;
    if (kind == GD_QM_EQM) {
        if (x < m0) return extrapolate == GD_QM_CLIP ? o0 : x + (o0 - m0);
        const double m1 = mq(Q - 1);
        if (x > m1) {
            const double o1 = oq(Q - 1);
            return extrapolate == GD_QM_CLIP ? o1 : x + (o1 - m1);
        }
        if (m1 != m1) return nan;
        return gd_qm_interp_at(x, gd_qm_bracket(x, Q, mq), Q, mq, oq);
    }
    // x is a sample of its own series, so own(0) <= x <= own(Q - 1); anything else (a foreign table) gives NaN
    const double w0 = own(0), w1 = own(Q - 1);
    if (!(w0 <= x && x <= w1)) return nan;
    const GdQmCol pc{p, 1};
    const double tau = gd_qm_interp_at(x, gd_qm_bracket(x, Q, own), Q, own, pc);
    if (!(tau >= 0.0 && tau <= 1.0)) return nan;
    const int j = gd_qm_bracket(tau, Q, pc);
    const double o = gd_qm_interp_at(tau, j, Q, pc, oq), m = gd_qm_interp_at(tau, j, Q, pc, mq);
    return x + (o - m);
}
