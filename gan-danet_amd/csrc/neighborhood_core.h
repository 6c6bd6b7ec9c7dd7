// Neighbourhood verification (include/gandanet.h, "Neighbourhood verification"): the per-pixel work of the fractions skill
// score -- the packed indicator word of a voxel, the clipped four-corner window lookup in a summed-area table, the three sums
// of a centre pixel in either normalisation, the fraction of one pixel -- and the order of the block sum, shared by the device
// kernels (neighborhood.hip) and their host twins, so both perform the same operations in the same order.
//
// The word.  H W <= 2^20, so a count of pixels of a plane is at most 2^20 and fits GD_NBR_FIELD = 21 bits.  A table entry
// holds three counts in one 64-bit word: valid in bits 0..20, I_f in bits 21..41, I_o in bits 42..62.  A prefix sum of words
// is the word of the prefix sums (no field ever exceeds 2^20, so nothing carries from one field into the next), and the
// four-corner value D - B - C + A, taken mod 2^64, is the word of the three window counts: the expression is linear in the
// fields, its true value has every field in [0, 2^20], and that value is below 2^63.
//
// The table of a plane is (H + 1) x (W + 1) words with a zero leading row and column: entry (r, c) counts the pixels of rows
// < r and columns < c, so the window rows i - h .. i + h clipped to the domain are r0 = max(i - h, 0), r1 = min(i + h + 1, H)
// and the lookup needs no branch.
//
// Sums.  window: A = sum (cf - co)^2, B = sum cf^2, C = sum co^2 as unsigned 64-bit integers (every term <= 2^40, at most
// 2^20 terms: exact, whatever the order).  valid: pf = cf / cv, po = co / cv and the fp64 sums of (pf - po)^2, pf^2, po^2,
// every operation rounded on its own (no contraction into FMA), in this order: thread j of workgroup b takes the pixels
// b GD_NBR_TILE + j + q GD_NBR_THREADS, q = 0 .. GD_NBR_ITEMS - 1, ascending; the GD_NBR_THREADS partial sums go through
// gd_block_sum_d (elem_util.h): the butterfly v[l] += v[l ^ o], o = 32 .. 1, inside every wave, then wave 0's total plus
// those of waves 1, 2, 3 in that order; the workgroups of a plane are added ascending onto 0.  gd_nbr_block_sum_host is
// that order on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/gandanet.h"

#define GD_NBR_THREADS 256
#define GD_NBR_ITEMS 4
#define GD_NBR_TILE (GD_NBR_THREADS * GD_NBR_ITEMS)   // centre pixels of one workgroup of the score kernel
#define GD_NBR_FIELD 21
#define GD_NBR_FMASK ((1ull << GD_NBR_FIELD) - 1ull)

typedef unsigned long long gd_nbr_word;

__host__ __device__ inline long gd_nbr_valid_of(gd_nbr_word w) { return (long)(w & GD_NBR_FMASK); }
__host__ __device__ inline long gd_nbr_f_of(gd_nbr_word w) { return (long)(w >> GD_NBR_FIELD & GD_NBR_FMASK); }
__host__ __device__ inline long gd_nbr_o_of(gd_nbr_word w) { return (long)(w >> (2 * GD_NBR_FIELD) & GD_NBR_FMASK); }

// ---- the indicator word of one voxel: comparisons in fp64 (the widening of fp32 is exact), never an event for NaN ----------
__host__ __device__ inline bool gd_nbr_event(double v, double thr, int below) { return below ? v <= thr : v >= thr; }

template <typename T>
__host__ __device__ inline gd_nbr_word gd_nbr_indicator(T fv, T ov, bool live, double thr_f, double thr_o, int below) {
    const bool valid = live && fv == fv && ov == ov;
    const gd_nbr_word ef = valid && gd_nbr_event((double)fv, thr_f, below), eo = valid && gd_nbr_event((double)ov, thr_o, below);
    return (gd_nbr_word)valid | ef << GD_NBR_FIELD | eo << (2 * GD_NBR_FIELD);
}

// ---- the three counts of the window of half width h around (i, j), clipped to the domain ---------------------------------
__host__ __device__ inline gd_nbr_word gd_nbr_window(const gd_nbr_word* __restrict__ tab, long H, long W, long i, long j, long h) {
    const long W1 = W + 1;
    const long r0 = i - h > 0 ? i - h : 0, r1 = i + h + 1 < H ? i + h + 1 : H;
    const long c0 = j - h > 0 ? j - h : 0, c1 = j + h + 1 < W ? j + h + 1 : W;
    return tab[r1 * W1 + c1] - tab[r0 * W1 + c1] - tab[r1 * W1 + c0] + tab[r0 * W1 + c0];
}

// is the centre pixel valid: the 1 x 1 window's count of valid pixels
__host__ __device__ inline bool gd_nbr_centre(const gd_nbr_word* __restrict__ tab, long H, long W, long i, long j) {
    return gd_nbr_valid_of(gd_nbr_window(tab, H, W, i, j, 0)) != 0;
}

// ---- one valid centre pixel onto the three sums ------------------------------------------------------------------------------
__host__ __device__ inline void gd_nbr_add(gd_nbr_word w, unsigned long long* s) {
    const long cf = gd_nbr_f_of(w), co = gd_nbr_o_of(w), d = cf - co;
    s[0] += (unsigned long long)(d * d);
    s[1] += (unsigned long long)(cf * cf);
    s[2] += (unsigned long long)(co * co);
}

__host__ __device__ inline void gd_nbr_add(gd_nbr_word w, double* s) {
#pragma clang fp contract(off)
    const double cv = (double)gd_nbr_valid_of(w);   // >= 1: the centre itself is valid
    const double pf = (double)gd_nbr_f_of(w) / cv, po = (double)gd_nbr_o_of(w) / cv, d = pf - po;
    s[0] += d * d;
    s[1] += pf * pf;
    s[2] += po * po;
}

// the sums of thread j of workgroup b of the score kernel: its GD_NBR_ITEMS pixels in ascending order
template <typename A>
__host__ __device__ inline void gd_nbr_thread_sums(const gd_nbr_word* __restrict__ tab, long H, long W, long b, int j, long h, A* s) {
    s[0] = s[1] = s[2] = (A)0;
    for (int q = 0; q < GD_NBR_ITEMS; ++q) {
        const long idx = b * GD_NBR_TILE + j + (long)q * GD_NBR_THREADS;
        if (idx >= H * W) break;
        const long pi = idx / W, pj = idx - pi * W;
        if (gd_nbr_centre(tab, H, W, pi, pj)) gd_nbr_add(gd_nbr_window(tab, H, W, pi, pj, h), s);
    }
}

// the order of gd_block_sum_d<3, GD_NBR_THREADS / 64> over the GD_NBR_THREADS partial sums (integers: any order)
template <typename A> inline void gd_nbr_block_sum_host(A (*part)[3], A* out) {
#pragma clang fp contract(off)
    for (int c = 0; c < 3; ++c) {
        A tot = (A)0;
        for (int wv = 0; wv < GD_NBR_THREADS / 64; ++wv) {
            A a[64], b[64];
            for (int l = 0; l < 64; ++l) a[l] = part[wv * 64 + l][c];
            for (int o = 32; o > 0; o >>= 1) {
                for (int l = 0; l < 64; ++l) b[l] = a[l] + a[l ^ o];
                for (int l = 0; l < 64; ++l) a[l] = b[l];
            }
            tot = wv == 0 ? a[0] : tot + a[0];
        }
        out[c] = tot;
    }
}

// one pixel of a map at one step: the sums continue from `s` (steps ascending)
template <typename A>
__host__ __device__ inline void gd_nbr_map_step(const gd_nbr_word* __restrict__ tab, long H, long W, long pi, long pj, long h, A* s) {
    if (gd_nbr_centre(tab, H, W, pi, pj)) gd_nbr_add(gd_nbr_window(tab, H, W, pi, pj, h), s);
}

// ---- the fraction field: one division of exact integers, NaN at an invalid centre ------------------------------------------
// n2 = (double)n * (double)n, exact for n < 2^26 (a window wider than 2 max(H, W) + 1 <= 2^21 + 1 counts nothing more)
__host__ __device__ inline double gd_nbr_fraction_one(const gd_nbr_word* __restrict__ tab, long H, long W, long pi, long pj, long h, double n2,
                                                      int normalize) {
    if (!gd_nbr_centre(tab, H, W, pi, pj)) return (double)NAN;
    const gd_nbr_word w = gd_nbr_window(tab, H, W, pi, pj, h);
    return (double)gd_nbr_f_of(w) / (normalize == GD_NBR_VALID ? (double)gd_nbr_valid_of(w) : n2);
}

// ---- sizes -----------------------------------------------------------------------------------------------------------------
__host__ __device__ inline long gd_nbr_plane_words(long H, long W) { return (H + 1) * (W + 1); }
__host__ __device__ inline long gd_nbr_blocks(long H, long W) { return (H * W + GD_NBR_TILE - 1) / GD_NBR_TILE; }
