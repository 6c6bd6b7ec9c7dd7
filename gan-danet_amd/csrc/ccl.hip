// Connected components (include/gandanet.h, "Connected components"): 3-D labelling of the dry voxels of a (T, H, W) cube,
// the size filter, canonical labels, and the bounds, track and totals tables of the clusters.  Union-find, the neighbourhood
// word and the order of the fp64 sums are ccl_core.h, shared with the host twins; the argument why no thread ever waits
// and why the result does not depend on the order of the atomics is at the top of that file.
//
// label: (1) a workgroup of 256 threads owns a tile of GD_CCL_TILE_T x _H x _W voxels: it builds the foreground, unites
// the neighbours inside the tile in LDS (ds atomic min) and writes the tile-local roots as raster indices; (2) a thread
// per voxel on a tile border unites it with its backward neighbours in OTHER tiles, in global memory (agent-scope atomic
// min; parents are read with agent-scope relaxed loads, so every value read is one that was stored); (3) a thread per
// voxel replaces its parent by its root.  Three launches: the launch boundary is the only ordering between the stages.
// filter / bounds: integer atomics, one per distinct root among the first lanes of a wave instead of one per lane (a giant
// cluster would otherwise send 64 atomics per wave to one address).  relabel / offsets: a three-pass exclusive scan (block
// sums, one workgroup over the block sums, add).  tracks: one workgroup per record, gd_block_sum_d.  totals: gd_for_items.
// From elem_util.h: gd_aligned, gd_elem_aligned, gd_with_dtype, gd_for_items, gd_block_sum_d, GD_S.
#include <limits.h>

#include <vector>

#include "elem_util.h"
#include "ccl_core.h"

namespace {

constexpr int TT = GD_CCL_TILE_T, TH = GD_CCL_TILE_H, TW = GD_CCL_TILE_W;
constexpr int TILE = TT * TH * TW;
constexpr int CCL_THREADS = 256;
constexpr int SCAN_PER_THREAD = 8, SCAN_BLOCK = CCL_THREADS * SCAN_PER_THREAD;
constexpr int TOP_THREADS = 1024;
constexpr int AGG_ROUNDS = 2;   // distinct roots of a wave that get one aggregated atomic; the lanes left add on their own
static_assert(TH * TW == CCL_THREADS, "a thread owns one (h, w) column of the tile");

struct Geo {
    int T, H, W;
};

// f(X{}) with X the element type of the tag, uint8 included
template <class F> inline auto with_ccl_dtype(int dtype, F&& f) {
    if (dtype == GD_CCL_U8) return f((unsigned char)0);
    return gd_with_dtype(dtype, f);
}

template <typename X> __host__ __device__ inline bool foreground(const X* x, const unsigned char* mask, long i, long hw, double thr) {
    if constexpr (gd_ccl_has_value<X>::value) {
        if (mask && mask[hw] == 0) return false;
    }
    return gd_ccl_fg(x[i], thr);
}

// ---- label -------------------------------------------------------------------------------------------------------------------
template <typename X>
__global__ __launch_bounds__(CCL_THREADS) void ccl_tile_kernel(const X* __restrict__ x, Geo g, double thr, const unsigned char* __restrict__ mask,
                                                               int structure, int ntw, int nth, long ntiles, int* __restrict__ parent) {
    __shared__ int lp[TILE];
    const int tid = threadIdx.x, lh = tid / TW, lw = tid % TW;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int w0 = (int)(tile % ntw) * TW, h0 = (int)(tile / ntw % nth) * TH, t0 = (int)(tile / ((long)ntw * nth)) * TT;
        const int gh = h0 + lh, gw = w0 + lw;
        const bool col = gh < g.H && gw < g.W;
        unsigned mine = 0;
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            const int gt = t0 + j;
            bool fg = false;
            if (col && gt < g.T) {
                const long hw = (long)gh * g.W + gw;
                fg = foreground(x, mask, (long)gt * g.H * g.W + hw, hw, thr);
            }
            mine |= (unsigned)fg << j;
            lp[j * CCL_THREADS + tid] = fg ? j * CCL_THREADS + tid : -1;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            if (!(mine >> j & 1)) continue;
            const int l = j * CCL_THREADS + tid;
#pragma unroll
            for (int k = 0; k < GD_CCL_STRUCT_BITS; ++k) {
                if (!(structure >> k & 1)) continue;
                int dt, dh, dw;
                gd_ccl_offset(k, dt, dh, dw);
                const int nt = j + dt, nh = lh + dh, nw = lw + dw;
                if (nt < 0 || nh < 0 || nh >= TH || nw < 0 || nw >= TW) continue;   // another tile's: the border kernel
                const int nl = (nt * TH + nh) * TW + nw;
                if (GdCclLdsMem::load(lp + nl) >= 0) gd_ccl_union<GdCclLdsMem>(lp, l, nl);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            const int gt = t0 + j;
            if (!col || gt >= g.T) continue;
            const long i = ((long)gt * g.H + gh) * g.W + gw;
            int out = -1;
            if (mine >> j & 1) {
                const int r = gd_ccl_find<GdCclLdsMem>(lp, j * CCL_THREADS + tid);
                out = (int)(((long)(t0 + r / CCL_THREADS) * g.H + h0 + r / TW % TH) * g.W + w0 + r % TW);
            }
            parent[i] = out;
        }
        __syncthreads();   // lp is rebuilt by the next tile
    }
}

template <typename X>
__global__ __launch_bounds__(CCL_THREADS) void ccl_init_kernel(const X* __restrict__ x, long n, long HW, double thr,
                                                               const unsigned char* __restrict__ mask, int* __restrict__ parent) {
    const long i = (long)blockIdx.x * CCL_THREADS + threadIdx.x;
    if (i < n) parent[i] = foreground(x, mask, i, i % HW, thr) ? (int)i : -1;
}

// ALL = false: only the pairs that straddle two tiles (the tile kernel united the others); ALL = true: every pair
template <bool ALL> __global__ __launch_bounds__(CCL_THREADS) void ccl_merge_kernel(Geo g, long n, int structure, int* parent) {
    const long i = (long)blockIdx.x * CCL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int w = (int)(i % g.W), h = (int)(i / g.W % g.H), t = (int)(i / ((long)g.W * g.H));
    if (!ALL) {
        const int lt = t % TT, lh = h % TH, lw = w % TW;
        if (lt > 0 && lh > 0 && lh < TH - 1 && lw > 0 && lw < TW - 1) return;   // no backward neighbour outside the tile
    }
    if (parent[i] < 0) return;   // the sign never changes
#pragma unroll
    for (int k = 0; k < GD_CCL_STRUCT_BITS; ++k) {
        if (!(structure >> k & 1)) continue;
        int dt, dh, dw;
        gd_ccl_offset(k, dt, dh, dw);
        const int nt = t + dt, nh = h + dh, nw = w + dw;
        if (nt < 0 || nh < 0 || nh >= g.H || nw < 0 || nw >= g.W) continue;
        if (!ALL && nt / TT == t / TT && nh / TH == h / TH && nw / TW == w / TW) continue;
        const long nb = ((long)nt * g.H + nh) * g.W + nw;   // nb < i
        if (GdCclGlobalMem::load(parent + nb) >= 0) gd_ccl_union<GdCclGlobalMem>(parent, (int)i, (int)nb);
    }
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_flatten_kernel(long n, int* parent) {
    const long i = (long)blockIdx.x * CCL_THREADS + threadIdx.x;
    if (i >= n || parent[i] < 0) return;
    // roots are fixed by now; a parent another thread has already flattened is as good as the one it replaced
    __hip_atomic_store(parent + i, gd_ccl_find<GdCclGlobalMem>(parent, (int)i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename X> void label_host(const X* x, Geo g, double thr, const unsigned char* mask, int structure, int* parent) {
    const long HW = (long)g.H * g.W, n = HW * g.T;
    for (long i = 0; i < n; ++i) parent[i] = foreground(x, mask, i, i % HW, thr) ? (int)i : -1;
    for (long i = 0; i < n; ++i) {
        if (parent[i] < 0) continue;
        const int w = (int)(i % g.W), h = (int)(i / g.W % g.H), t = (int)(i / HW);
        for (int k = 0; k < GD_CCL_STRUCT_BITS; ++k) {
            if (!(structure >> k & 1)) continue;
            int dt, dh, dw;
            gd_ccl_offset(k, dt, dh, dw);
            const int nt = t + dt, nh = h + dh, nw = w + dw;
            if (nt < 0 || nh < 0 || nh >= g.H || nw < 0 || nw >= g.W) continue;
            const long nb = ((long)nt * g.H + nh) * g.W + nw;
            if (parent[nb] >= 0) gd_ccl_union<GdCclHostMem>(parent, (int)i, (int)nb);
        }
    }
    for (long i = 0; i < n; ++i)
        if (parent[i] >= 0) parent[i] = gd_ccl_find<GdCclHostMem>(parent, (int)i);
}

void label_run(bool host, hipStream_t st, const void* xv, int dtype, Geo g, double thr, const unsigned char* mask, int structure, int flags,
               int* parent) {
    const long HW = (long)g.H * g.W, n = HW * g.T;
    with_ccl_dtype(dtype, [&](auto zero) {
        using X = decltype(zero);
        const X* x = (const X*)xv;
        if (host) {
            label_host(x, g, thr, mask, structure, parent);
            return;
        }
        const int grid = gd_cdiv(n, CCL_THREADS);
        if (flags & GD_CCL_NO_TILES) {
            hipLaunchKernelGGL(ccl_init_kernel<X>, dim3(grid), dim3(CCL_THREADS), 0, st, x, n, HW, thr, mask, parent);
            hipLaunchKernelGGL(ccl_merge_kernel<true>, dim3(grid), dim3(CCL_THREADS), 0, st, g, n, structure, parent);
        } else {
            const int ntw = gd_cdiv(g.W, TW), nth = gd_cdiv(g.H, TH), ntt = gd_cdiv(g.T, TT);
            const long ntiles = (long)ntw * nth * ntt;
            hipLaunchKernelGGL(ccl_tile_kernel<X>, dim3((unsigned)(ntiles < (1L << 22) ? ntiles : (1L << 22))), dim3(CCL_THREADS), 0, st, x, g, thr,
                               mask, structure, ntw, nth, ntiles, parent);
            hipLaunchKernelGGL(ccl_merge_kernel<false>, dim3(grid), dim3(CCL_THREADS), 0, st, g, n, structure, parent);
        }
        hipLaunchKernelGGL(ccl_flatten_kernel, dim3(grid), dim3(CCL_THREADS), 0, st, n, parent);
    });
}

// ---- wave helpers --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ int wave_incl_scan_i(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}
// exclusive scan of one int per thread over a block of NT threads (all call it); total: the block's sum.  red: NT / 64 + 1 ints of LDS
template <int NT> __device__ __forceinline__ int block_excl_scan_i(int v, int* red, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int incl = wave_incl_scan_i(v);
    __syncthreads();   // red may still be read from an earlier call
    if (lane == 63) red[wv] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int q = 0; q < NT / 64; ++q) {
        const int s = red[q];
        base += q < wv ? s : 0;
        tot += s;
    }
    total = tot;
    return base + incl - v;
}

// ---- size filter -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CCL_THREADS) void ccl_count_kernel(const int* __restrict__ parent, long n, int* __restrict__ cnt) {
    const long i = (long)blockIdx.x * CCL_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int r = i < n ? parent[i] : -1;
    bool active = r >= 0 && r < n;   // never an address outside cnt
    // the whole wave walks this loop together: `rem` is the same in every lane
    unsigned long long rem = __ballot(active);
    for (int round = 0; round < AGG_ROUNDS && rem; ++round) {
        const int leader = __ffsll((long long)rem) - 1;
        const int lr = __shfl(r, leader, 64);
        const bool match = active && r == lr;
        const unsigned long long m = __ballot(match);
        if (lane == leader) atomicAdd(cnt + lr, __popcll(m));
        active = active && !match;
        rem &= ~m;
    }
    if (active) atomicAdd(cnt + r, 1);
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_drop_kernel(int* __restrict__ parent, long n, const int* __restrict__ cnt, int min_size) {
    const long i = (long)blockIdx.x * CCL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int r = parent[i];
    if (r >= 0 && r < n && cnt[r] < min_size) parent[i] = -1;
}

// ---- exclusive scan in three passes: block sums, one workgroup over the block sums, add ---------------------------------------------
struct RootFlag {   // 1 at the first voxel of every component
    const int* parent;
    __host__ __device__ int operator()(long i) const { return parent[i] == (int)i; }
};
struct Duration {   // t1 - t0 + 1 of every cluster
    const int* bounds;
    __host__ __device__ int operator()(long k) const { return bounds[k * GD_CCL_BOUNDS + GD_CCL_B_T1] - bounds[k * GD_CCL_BOUNDS + GD_CCL_B_T0] + 1; }
};

template <class V> __global__ __launch_bounds__(CCL_THREADS) void scan_sums_kernel(V val, long n, int* __restrict__ bsum) {
    __shared__ int red[CCL_THREADS / 64 + 1];
    const long i0 = (long)blockIdx.x * SCAN_BLOCK + (long)threadIdx.x * SCAN_PER_THREAD;
    int s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_PER_THREAD; ++j)
        if (i0 + j < n) s += val(i0 + j);
    int total;
    block_excl_scan_i<CCL_THREADS>(s, red, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(TOP_THREADS) void scan_top_kernel(int* __restrict__ bsum, long nb, int* __restrict__ total) {
    __shared__ int red[TOP_THREADS / 64 + 1];
    int carry = 0;
    for (long base = 0; base < nb; base += TOP_THREADS) {
        const long j = base + threadIdx.x;
        const int v = j < nb ? bsum[j] : 0;
        int tot;
        const int ex = block_excl_scan_i<TOP_THREADS>(v, red, tot);
        if (j < nb) bsum[j] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

template <class V> __global__ __launch_bounds__(CCL_THREADS) void scan_add_kernel(V val, long n, const int* __restrict__ bsum, int* __restrict__ out) {
    __shared__ int red[CCL_THREADS / 64 + 1];
    const long i0 = (long)blockIdx.x * SCAN_BLOCK + (long)threadIdx.x * SCAN_PER_THREAD;
    int v[SCAN_PER_THREAD], s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_PER_THREAD; ++j) {
        v[j] = i0 + j < n ? val(i0 + j) : 0;
        s += v[j];
    }
    int total;
    int run = bsum[blockIdx.x] + block_excl_scan_i<CCL_THREADS>(s, red, total);
#pragma unroll
    for (int j = 0; j < SCAN_PER_THREAD; ++j) {
        if (i0 + j < n) out[i0 + j] = run;
        run += v[j];
    }
}

// out[i] = sum of val(j), j < i; *total = the sum of all n.  bsum: gd_cdiv(n, SCAN_BLOCK) ints
template <class V> void scan_run(hipStream_t st, V val, long n, int* out, int* bsum, int* total) {
    const int nb = gd_cdiv(n, SCAN_BLOCK);
    hipLaunchKernelGGL(scan_sums_kernel<V>, dim3(nb), dim3(CCL_THREADS), 0, st, val, n, bsum);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(TOP_THREADS), 0, st, bsum, (long)nb, total);
    hipLaunchKernelGGL(scan_add_kernel<V>, dim3(nb), dim3(CCL_THREADS), 0, st, val, n, (const int*)bsum, out);
}
template <class V> void scan_host(V val, long n, int* out, int* total) {
    int run = 0;
    for (long i = 0; i < n; ++i) {
        const int v = val(i);
        out[i] = run;
        run += v;
    }
    *total = run;
}

// labels may be parent: a thread reads its own parent and the scan of its root, and writes its own label
__global__ __launch_bounds__(CCL_THREADS) void ccl_labels_kernel(const int* parent, long n, const int* __restrict__ scan, int* labels) {
    const long i = (long)blockIdx.x * CCL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int r = parent[i];
    labels[i] = (r < 0 || r >= n) ? 0 : scan[r] + 1;
}

// ---- bounds ------------------------------------------------------------------------------------------------------------------------
struct BoundsInit {
    int* bounds;
    __host__ __device__ void operator()(long k) const {
        int* b = bounds + k * GD_CCL_BOUNDS;
        b[GD_CCL_B_N] = 0;
        b[GD_CCL_B_T0] = b[GD_CCL_B_H0] = b[GD_CCL_B_W0] = INT_MAX;
        b[GD_CCL_B_T1] = b[GD_CCL_B_H1] = b[GD_CCL_B_W1] = -1;
    }
};

__device__ __forceinline__ void bounds_put(int* b, int n, int t0, int t1, int h0, int h1, int w0, int w1) {
    atomicAdd(b + GD_CCL_B_N, n);
    atomicMin(b + GD_CCL_B_T0, t0);
    atomicMax(b + GD_CCL_B_T1, t1);
    atomicMin(b + GD_CCL_B_H0, h0);
    atomicMax(b + GD_CCL_B_H1, h1);
    atomicMin(b + GD_CCL_B_W0, w0);
    atomicMax(b + GD_CCL_B_W1, w1);
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_bounds_kernel(const int* __restrict__ labels, Geo g, long n, int K, int* __restrict__ bounds) {
    const long i = (long)blockIdx.x * CCL_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int lab = i < n ? labels[i] : 0;
    if (lab > K) lab = 0;   // not a label of this table: never an address outside it
    const long ic = i < n ? i : 0;
    const int w = (int)(ic % g.W), h = (int)(ic / g.W % g.H), t = (int)(ic / ((long)g.W * g.H));
    bool active = lab > 0;
    unsigned long long rem = __ballot(active);   // the same in every lane: the wave walks the loop together
    for (int round = 0; round < AGG_ROUNDS && rem; ++round) {
        const int leader = __ffsll((long long)rem) - 1;
        const int ll = __shfl(lab, leader, 64);
        const bool match = active && lab == ll;
        const unsigned long long m = __ballot(match);
        const int t0 = wave_min_i(match ? t : INT_MAX), t1 = wave_max_i(match ? t : -1);
        const int h0 = wave_min_i(match ? h : INT_MAX), h1 = wave_max_i(match ? h : -1);
        const int w0 = wave_min_i(match ? w : INT_MAX), w1 = wave_max_i(match ? w : -1);
        if (lane == leader) bounds_put(bounds + (long)(ll - 1) * GD_CCL_BOUNDS, __popcll(m), t0, t1, h0, h1, w0, w1);
        active = active && !match;
        rem &= ~m;
    }
    if (active) bounds_put(bounds + (long)(lab - 1) * GD_CCL_BOUNDS, 1, t, t, h, h, w, w);
}

void bounds_host(const int* labels, Geo g, int K, int* bounds) {
    const long n = (long)g.T * g.H * g.W;
    for (long i = 0; i < n; ++i) {
        const int lab = labels[i];
        if (lab <= 0 || lab > K) continue;
        int* b = bounds + (long)(lab - 1) * GD_CCL_BOUNDS;
        const int w = (int)(i % g.W), h = (int)(i / g.W % g.H), t = (int)(i / ((long)g.W * g.H));
        b[GD_CCL_B_N] += 1;
        b[GD_CCL_B_T0] = t < b[GD_CCL_B_T0] ? t : b[GD_CCL_B_T0];
        b[GD_CCL_B_T1] = t > b[GD_CCL_B_T1] ? t : b[GD_CCL_B_T1];
        b[GD_CCL_B_H0] = h < b[GD_CCL_B_H0] ? h : b[GD_CCL_B_H0];
        b[GD_CCL_B_H1] = h > b[GD_CCL_B_H1] ? h : b[GD_CCL_B_H1];
        b[GD_CCL_B_W0] = w < b[GD_CCL_B_W0] ? w : b[GD_CCL_B_W0];
        b[GD_CCL_B_W1] = w > b[GD_CCL_B_W1] ? w : b[GD_CCL_B_W1];
    }
}

// ---- tracks ------------------------------------------------------------------------------------------------------------------------
// a box that is not inside the plane (a table that does not belong to these labels) is an empty one: no address outside
__host__ __device__ inline bool track_box(const int* b, Geo g, long r, long r0, int& t, int& h0, int& h1, int& w0, int& w1) {
    t = b[GD_CCL_B_T0] + (int)(r - r0);
    h0 = b[GD_CCL_B_H0], h1 = b[GD_CCL_B_H1], w0 = b[GD_CCL_B_W0], w1 = b[GD_CCL_B_W1];
    return t >= 0 && t < g.T && h0 >= 0 && h0 <= h1 && h1 < g.H && w0 >= 0 && w0 <= w1 && w1 < g.W;
}

template <typename X>
__global__ __launch_bounds__(GD_CCL_TRACK_THREADS) void ccl_tracks_kernel(const X* __restrict__ x, Geo g, double thr, const int* __restrict__ labels,
                                                                          const int* __restrict__ bounds, const int* __restrict__ offsets, int K,
                                                                          long R, const double* __restrict__ weights, bool values,
                                                                          double* __restrict__ tracks, int* __restrict__ index) {
    constexpr int NW = GD_CCL_TRACK_THREADS / 64;
    __shared__ double red[NW][GD_CCL_TRACK_SUMS];
    __shared__ double redm[NW];
    const int tid = threadIdx.x;
    const long HW = (long)g.H * g.W;
    for (long r = blockIdx.x; r < R; r += gridDim.x) {
        const int k = gd_ccl_record_cluster(offsets, K, r);
        int t, h0, h1, w0, w1;
        const bool ok = track_box(bounds + (long)k * GD_CCL_BOUNDS, g, r, offsets[k], t, h0, h1, w0, w1);
        double v[GD_CCL_TRACK_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0}, mn = (double)INFINITY;
        if (ok) gd_ccl_track_thread<X>(x ? x + t * HW : x, labels + t * HW, g.W, k + 1, h0, h1, w0, w1, thr, weights, values, tid, v, mn);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double u = __shfl_xor(mn, o, 64);
            mn = u < mn ? u : mn;
        }
        __syncthreads();   // thread 0 may still read the previous record's sums
        if ((tid & 63) == 0) redm[tid >> 6] = mn;
        gd_block_sum_d<GD_CCL_TRACK_SUMS, NW>(v, red);
        if (tid == 0) {
            for (int q = 1; q < NW; ++q) mn = redm[q] < mn ? redm[q] : mn;
            gd_ccl_track_put(v, mn, values, tracks + r * GD_CCL_TRACK);
            index[2 * r] = k;
            index[2 * r + 1] = t;
        }
    }
}

template <typename X>
void tracks_host(const X* x, Geo g, double thr, const int* labels, const int* bounds, const int* offsets, int K, long R, const double* weights,
                 bool values, double* tracks, int* index) {
    const long HW = (long)g.H * g.W;
    std::vector<double> part(GD_CCL_TRACK_THREADS * GD_CCL_TRACK_SUMS), pmn(GD_CCL_TRACK_THREADS);
    double(*p)[GD_CCL_TRACK_SUMS] = (double(*)[GD_CCL_TRACK_SUMS])part.data();
    for (long r = 0; r < R; ++r) {
        const int k = gd_ccl_record_cluster(offsets, K, r);
        int t, h0, h1, w0, w1;
        const bool ok = track_box(bounds + (long)k * GD_CCL_BOUNDS, g, r, offsets[k], t, h0, h1, w0, w1);
        for (int tid = 0; tid < GD_CCL_TRACK_THREADS; ++tid) {
            double v[GD_CCL_TRACK_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0}, mn = (double)INFINITY;
            if (ok) gd_ccl_track_thread<X>(x ? x + t * HW : x, labels + t * HW, g.W, k + 1, h0, h1, w0, w1, thr, weights, values, tid, v, mn);
            for (int q = 0; q < GD_CCL_TRACK_SUMS; ++q) p[tid][q] = v[q];
            pmn[tid] = mn;
        }
        double v[GD_CCL_TRACK_SUMS], mn;
        gd_ccl_block_sum_host(p, pmn.data(), v, mn);
        gd_ccl_track_put(v, mn, values, tracks + r * GD_CCL_TRACK);
        index[2 * r] = k;
        index[2 * r + 1] = t;
    }
}

struct TotalsBody {
    const double* tracks;
    const int* bounds;
    const int* offsets;
    double* totals;
    __host__ __device__ void operator()(long k) const { gd_ccl_totals_one(k, tracks, bounds, offsets, totals); }
};

size_t ws_ints(long n) { return (size_t)n + (size_t)gd_cdiv(n, SCAN_BLOCK) + 4; }

}  // namespace

extern "C" size_t gd_ccl_ws_bytes(long n) { return n > 0 ? ws_ints(n) * sizeof(int) : 0; }

#define CCL_CUBE_CHECKS(fn)                                                              \
    GD_CHECK_ARG(T > 0 && H > 0 && W > 0, fn ": T, H or W <= 0");                        \
    GD_CHECK_ARG(T < (1L << 31) && H < (1L << 31) && W < (1L << 31) && (double)T * (double)H * (double)W < 2147483648.0, \
                 fn ": too many voxels, T H W >= 2^31")

#define CCL_LABEL_CHECKS(fn)                                                                                                  \
    GD_CHECK_ARG(x && parent, fn ": null pointer");                                                                           \
    GD_CHECK_ARG(gd_dtype_ok(dtype) || dtype == GD_CCL_U8, fn ": dtype outside {0, 1, 2}");                                   \
    CCL_CUBE_CHECKS(fn);                                                                                                      \
    GD_CHECK_ARG(dtype == GD_CCL_U8 || threshold == threshold, fn ": the threshold is NaN");                                  \
    GD_CHECK_ARG(structure >= 0 && structure < (1 << GD_CCL_STRUCT_BITS), fn ": structure has bits above the 13 backward offsets"); \
    GD_CHECK_ARG((flags & ~GD_CCL_NO_TILES) == 0, fn ": unknown flags");                                                      \
    GD_CHECK_ARG((dtype == GD_CCL_U8 || gd_elem_aligned(x, dtype)) && gd_aligned(parent, 4), fn ": pointer not element aligned")

extern "C" int gd_ccl_label(const void* x, int dtype, long T, long H, long W, double threshold, const unsigned char* mask, int structure,
                            int flags, int* parent, void* stream) {
    CCL_LABEL_CHECKS("gd_ccl_label");
    label_run(false, GD_S, x, dtype, Geo{(int)T, (int)H, (int)W}, threshold, mask, structure, flags, parent);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_ccl_label_host(const void* x, int dtype, long T, long H, long W, double threshold, const unsigned char* mask, int structure,
                                 int flags, int* parent) {
    CCL_LABEL_CHECKS("gd_ccl_label_host");
    label_run(true, nullptr, x, dtype, Geo{(int)T, (int)H, (int)W}, threshold, mask, structure, flags, parent);
    return 0;
}

#define CCL_N_CHECKS(fn) GD_CHECK_ARG(n > 0 && n < (1L << 31), fn ": n <= 0 or n >= 2^31")
#define CCL_WS_CHECKS(fn, count)                                                          \
    GD_CHECK_ARG(ws && gd_aligned(ws, 4), fn ": the workspace is null or not aligned");   \
    GD_CHECK_ARG(ws_bytes >= gd_ccl_ws_bytes(count), fn ": the workspace is smaller than gd_ccl_ws_bytes")

#define CCL_FILTER_CHECKS(fn)                          \
    GD_CHECK_ARG(parent, fn ": null pointer");         \
    CCL_N_CHECKS(fn);                                  \
    GD_CHECK_ARG(min_size >= 1, fn ": min_size < 1");  \
    GD_CHECK_ARG(gd_aligned(parent, 4), fn ": pointer not element aligned")

extern "C" int gd_ccl_filter(int* parent, long n, int min_size, void* ws, size_t ws_bytes, void* stream) {
    CCL_FILTER_CHECKS("gd_ccl_filter");
    CCL_WS_CHECKS("gd_ccl_filter", n);
    int* cnt = (int*)ws;
    const int grid = gd_cdiv(n, CCL_THREADS);
    if (hipMemsetAsync(cnt, 0, (size_t)n * sizeof(int), GD_S) != hipSuccess) {
        gd_set_error("gd_ccl_filter: hipMemsetAsync failed");
        return -2;
    }
    hipLaunchKernelGGL(ccl_count_kernel, dim3(grid), dim3(CCL_THREADS), 0, GD_S, (const int*)parent, n, cnt);
    hipLaunchKernelGGL(ccl_drop_kernel, dim3(grid), dim3(CCL_THREADS), 0, GD_S, parent, n, (const int*)cnt, min_size);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_ccl_filter_host(int* parent, long n, int min_size) {
    CCL_FILTER_CHECKS("gd_ccl_filter_host");
    std::vector<int> cnt(n, 0);
    for (long i = 0; i < n; ++i)
        if (parent[i] >= 0 && parent[i] < n) cnt[parent[i]] += 1;
    for (long i = 0; i < n; ++i)
        if (parent[i] >= 0 && parent[i] < n && cnt[parent[i]] < min_size) parent[i] = -1;
    return 0;
}

#define CCL_RELABEL_CHECKS(fn)                                     \
    GD_CHECK_ARG(parent && labels && count, fn ": null pointer");  \
    CCL_N_CHECKS(fn);                                              \
    GD_CHECK_ARG(gd_aligned(parent, 4) && gd_aligned(labels, 4) && gd_aligned(count, 4), fn ": pointer not element aligned")

extern "C" int gd_ccl_relabel(const int* parent, long n, int* labels, int* count, void* ws, size_t ws_bytes, void* stream) {
    CCL_RELABEL_CHECKS("gd_ccl_relabel");
    CCL_WS_CHECKS("gd_ccl_relabel", n);
    int* scan = (int*)ws;
    scan_run(GD_S, RootFlag{parent}, n, scan, scan + n, count);
    hipLaunchKernelGGL(ccl_labels_kernel, dim3(gd_cdiv(n, CCL_THREADS)), dim3(CCL_THREADS), 0, GD_S, parent, n, (const int*)scan, labels);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_ccl_relabel_host(const int* parent, long n, int* labels, int* count) {
    CCL_RELABEL_CHECKS("gd_ccl_relabel_host");
    std::vector<int> scan(n);
    scan_host(RootFlag{parent}, n, scan.data(), count);
    for (long i = 0; i < n; ++i) labels[i] = (parent[i] < 0 || parent[i] >= n) ? 0 : scan[parent[i]] + 1;
    return 0;
}

#define CCL_K_CHECKS(fn) GD_CHECK_ARG(K > 0, fn ": K <= 0")

#define CCL_BOUNDS_CHECKS(fn)                               \
    GD_CHECK_ARG(labels && bounds, fn ": null pointer");    \
    CCL_CUBE_CHECKS(fn);                                    \
    CCL_K_CHECKS(fn);                                       \
    GD_CHECK_ARG(gd_aligned(labels, 4) && gd_aligned(bounds, 4), fn ": pointer not element aligned")

extern "C" int gd_ccl_bounds(const int* labels, long T, long H, long W, int K, int* bounds, void* stream) {
    CCL_BOUNDS_CHECKS("gd_ccl_bounds");
    const Geo g{(int)T, (int)H, (int)W};
    const long n = T * H * W;
    gd_for_items<CCL_THREADS>(false, K, GD_S, BoundsInit{bounds});
    hipLaunchKernelGGL(ccl_bounds_kernel, dim3(gd_cdiv(n, CCL_THREADS)), dim3(CCL_THREADS), 0, GD_S, labels, g, n, K, bounds);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_ccl_bounds_host(const int* labels, long T, long H, long W, int K, int* bounds) {
    CCL_BOUNDS_CHECKS("gd_ccl_bounds_host");
    gd_for_items<CCL_THREADS>(true, K, nullptr, BoundsInit{bounds});
    bounds_host(labels, Geo{(int)T, (int)H, (int)W}, K, bounds);
    return 0;
}

#define CCL_OFFSETS_CHECKS(fn)                               \
    GD_CHECK_ARG(bounds && offsets, fn ": null pointer");    \
    CCL_K_CHECKS(fn);                                        \
    GD_CHECK_ARG(gd_aligned(bounds, 4) && gd_aligned(offsets, 4), fn ": pointer not element aligned")

extern "C" int gd_ccl_offsets(const int* bounds, int K, int* offsets, void* ws, size_t ws_bytes, void* stream) {
    CCL_OFFSETS_CHECKS("gd_ccl_offsets");
    CCL_WS_CHECKS("gd_ccl_offsets", K);
    scan_run(GD_S, Duration{bounds}, (long)K, offsets, (int*)ws, offsets + K);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_ccl_offsets_host(const int* bounds, int K, int* offsets) {
    CCL_OFFSETS_CHECKS("gd_ccl_offsets_host");
    scan_host(Duration{bounds}, (long)K, offsets, offsets + K);
    return 0;
}

#define CCL_TRACKS_CHECKS(fn)                                                                                                 \
    GD_CHECK_ARG(labels && bounds && offsets && tracks && index, fn ": null pointer");                                        \
    GD_CHECK_ARG(gd_dtype_ok(dtype) || dtype == GD_CCL_U8, fn ": dtype outside {0, 1, 2}");                                   \
    CCL_CUBE_CHECKS(fn);                                                                                                      \
    CCL_K_CHECKS(fn);                                                                                                         \
    GD_CHECK_ARG(R >= K && (double)R <= (double)T * (double)H * (double)W, fn ": R outside K .. T H W");                      \
    GD_CHECK_ARG((flags & ~GD_CCL_SEVERITY) == 0, fn ": unknown flags");                                                      \
    GD_CHECK_ARG(!(flags & GD_CCL_SEVERITY) || dtype != GD_CCL_U8, fn ": severity asked of a uint8 cube, which has no values"); \
    GD_CHECK_ARG(!(flags & GD_CCL_SEVERITY) || x, fn ": severity asked without x");                                           \
    GD_CHECK_ARG(!(flags & GD_CCL_SEVERITY) || threshold == threshold, fn ": the threshold is NaN");                          \
    GD_CHECK_ARG((dtype == GD_CCL_U8 || !x || gd_elem_aligned(x, dtype)) && gd_aligned(labels, 4) && gd_aligned(bounds, 4) &&  \
                     gd_aligned(offsets, 4) && gd_aligned(index, 4) && gd_aligned(tracks, 8) && gd_aligned(weights, 8),        \
                 fn ": pointer not element aligned")

extern "C" int gd_ccl_tracks(const void* x, int dtype, long T, long H, long W, double threshold, const int* labels, const int* bounds,
                             const int* offsets, int K, long R, const double* weights, int flags, double* tracks, int* index, void* stream) {
    CCL_TRACKS_CHECKS("gd_ccl_tracks");
    const Geo g{(int)T, (int)H, (int)W};
    const bool values = (flags & GD_CCL_SEVERITY) != 0;
    with_ccl_dtype(dtype, [&](auto zero) {
        using X = decltype(zero);
        hipLaunchKernelGGL(ccl_tracks_kernel<X>, dim3((unsigned)(R < (1L << 20) ? R : (1L << 20))), dim3(GD_CCL_TRACK_THREADS), 0, GD_S,
                           (const X*)x, g, threshold, labels, bounds, offsets, K, R, weights, values, tracks, index);
    });
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_ccl_tracks_host(const void* x, int dtype, long T, long H, long W, double threshold, const int* labels, const int* bounds,
                                  const int* offsets, int K, long R, const double* weights, int flags, double* tracks, int* index) {
    CCL_TRACKS_CHECKS("gd_ccl_tracks_host");
    const Geo g{(int)T, (int)H, (int)W};
    const bool values = (flags & GD_CCL_SEVERITY) != 0;
    with_ccl_dtype(dtype, [&](auto zero) {
        using X = decltype(zero);
        tracks_host((const X*)x, g, threshold, labels, bounds, offsets, K, R, weights, values, tracks, index);
    });
    return 0;
}

#define CCL_TOTALS_CHECKS(fn)                                                   \
    GD_CHECK_ARG(tracks && bounds && offsets && totals, fn ": null pointer");   \
    CCL_K_CHECKS(fn);                                                           \
    GD_CHECK_ARG(gd_aligned(tracks, 8) && gd_aligned(totals, 8) && gd_aligned(bounds, 4) && gd_aligned(offsets, 4), fn ": pointer not element aligned")

extern "C" int gd_ccl_totals(const double* tracks, const int* bounds, const int* offsets, int K, double* totals, void* stream) {
    CCL_TOTALS_CHECKS("gd_ccl_totals");
    gd_for_items<CCL_THREADS>(false, K, GD_S, TotalsBody{tracks, bounds, offsets, totals});
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_ccl_totals_host(const double* tracks, const int* bounds, const int* offsets, int K, double* totals) {
    CCL_TOTALS_CHECKS("gd_ccl_totals_host");
    gd_for_items<CCL_THREADS>(true, K, nullptr, TotalsBody{tracks, bounds, offsets, totals});
    return 0;
}
