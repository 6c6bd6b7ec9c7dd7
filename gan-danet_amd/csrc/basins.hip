// Basin analysis (include/gandanet.h, "Basin analysis"): the loop body of Basin_TWSA_Comparison_GRACE_Downscaled.ipynb,
// cell 5, on the device.  gd_zone_rasterize replaces `polygon.contains(Point(x, y))` per grid point by an even-odd scan
// of the polygon's edges against a rectilinear grid, up to 32 zones into one word per grid point; gd_zone_mean replaces
// `np.nanmean(data[:, mask], axis=1)` per basin by one pass over the product for all zones.  The containment rule is
// zones.h, shared with the host twin gd_zone_rasterize_host.  No global atomics; every reduction runs in an order fixed
// by the shape, so the same input gives the same bits.  All index arithmetic on the grid is 64-bit.
// From elem_util.h: gd_head_of, gd_vec16, gd_plane_gx, gd_dtype_ok, gd_elem_aligned, gd_aligned, GD_S.
#include "elem_util.h"
#include "zones.h"

#include <math.h>

#include <vector>

namespace {

constexpr int ZN_THREADS = 256;
constexpr int ZN_ROWS = ZN_THREADS / GD_WAVE;   // grid rows one workgroup owns: one wave per row
constexpr int ZN_COLS = 1024;                   // columns of a row one workgroup owns
constexpr int ZN_CHUNK = GD_ZONE_EDGE_CHUNK;    // edges per pass = capacity of a row's crossing list

// edge_off of the call, by value in the kernel arguments (E < 2^30)
struct ZoneOffsets {
    int off[GD_ZONE_MAX + 1];
};

// ---- rasteriser ---------------------------------------------------------------------------------------------------------
// Workgroup (blockIdx.x, blockIdx.y) owns the rows [blockIdx.x * 4, + 4) and the columns [blockIdx.y * 1024, + 1024) of
// the grid, for all zones.  All points of a row share py, so the straddle test and the crossing belong to (row, edge): per
// zone the edges are taken in chunks of ZN_CHUNK; every thread tests its edges of the chunk against the four rows and
// appends the crossings of the straddling ones to that row's list in LDS (an LDS counter hands out the slots: the order
// of a list varies from run to run, the number of its entries right of a column does not).  Then wave w walks the columns
// of row w and flips bit z of the column's word, kept in LDS, when an odd number of the list's crossings lies right of it.
// Parity adds up over the chunks.  Most (row, chunk) pairs have no crossing and skip the column walk: O(E + W k) per row,
// k the crossings of the row.  The words are zeroed here and every one of them is stored, with plain vector stores.
// The two counter sets alternate between passes, so the set of the next pass is cleared while this one is read.
__global__ __launch_bounds__(ZN_THREADS) void zone_rasterize_kernel(const double* __restrict__ edges, ZoneOffsets zo, int Z,
                                                                    const double* __restrict__ xs, long W,
                                                                    const double* __restrict__ ys, long H,
                                                                    unsigned int* __restrict__ bits) {
    __shared__ double xint[ZN_ROWS][ZN_CHUNK];
    __shared__ unsigned int word[ZN_ROWS][ZN_COLS];
    __shared__ int cnt[2][ZN_ROWS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long r0 = (long)blockIdx.x * ZN_ROWS, c0 = (long)blockIdx.y * ZN_COLS;
    const int nrows = H - r0 < ZN_ROWS ? (int)(H - r0) : ZN_ROWS;
    const int tw = W - c0 < ZN_COLS ? (int)(W - c0) : ZN_COLS;
    double py[ZN_ROWS];
#pragma unroll
    for (int r = 0; r < ZN_ROWS; ++r) py[r] = r < nrows ? ys[r0 + r] : 0.0;
    for (int i = tid; i < ZN_ROWS * ZN_COLS; i += ZN_THREADS) (&word[0][0])[i] = 0u;
    if (tid < 2 * ZN_ROWS) (&cnt[0][0])[tid] = 0;
    __syncthreads();
    int pass = 0;
    for (int z = 0; z < Z; ++z) {
        const int e1 = zo.off[z + 1];
        for (int e0 = zo.off[z]; e0 < e1; e0 += ZN_CHUNK, ++pass) {
            int* cur = cnt[pass & 1];
            const int eend = e1 - e0 < ZN_CHUNK ? e1 : e0 + ZN_CHUNK;
            for (int e = e0 + tid; e < eend; e += ZN_THREADS) {
                const double* p = edges + 4L * e;
                const double x0 = p[0], y0 = p[1], x1 = p[2], y1 = p[3];
#pragma unroll
                for (int r = 0; r < ZN_ROWS; ++r) {
                    if (r < nrows && gd_zone_edge_straddles(y0, y1, py[r])) {
                        const int k = atomicAdd(&cur[r], 1);   // LDS; k < ZN_CHUNK: a chunk appends at most one entry per edge
                        xint[r][k] = gd_zone_edge_intercept(x0, y0, x1, y1, py[r]);
                    }
                }
            }
            __syncthreads();
            const int n = cur[wave];   // 0 for a row past the grid
            if (tid < ZN_ROWS) cnt[(pass + 1) & 1][tid] = 0;
            if (n > 0) {
                for (int j = lane; j < tw; j += GD_WAVE) {
                    const double px = xs[c0 + j];
                    unsigned int c = 0;
                    for (int k = 0; k < n; ++k) c += gd_zone_crossing_counts(px, xint[wave][k]) ? 1u : 0u;
                    word[wave][j] ^= (c & 1u) << z;
                }
            }
            __syncthreads();
        }
    }
    if (wave < nrows) {
        unsigned int* o = bits + (r0 + wave) * W + c0;
        for (int j = lane; j < tw; j += GD_WAVE) o[j] = word[wave][j];
    }
}

// ---- zonal means -----------------------------------------------------------------------------------------------------------
// one pixel into the ZM accumulator triples of a thread: the zone loop is unrolled and every update is a select, so the
// arrays are indexed by constants only and stay in registers
template <int ZM, bool WT>
__device__ __forceinline__ void zone_acc(double (&s)[ZM], double (&sw)[WT ? ZM : 1], unsigned int (&c)[ZM], double v,
                                         unsigned int b, double w) {
    const unsigned int live = v == v ? b : 0u;   // a NaN pixel contributes to no zone
    const double t = WT ? v * w : v;
#pragma unroll
    for (int z = 0; z < ZM; ++z) {
        const bool in = (live >> z) & 1u;
        s[z] += in ? t : 0.0;
        if (WT) sw[z] += in ? w : 0.0;
        c[z] += in ? 1u : 0u;
    }
}

// grid (gx, planes): the partial (sum of w v, sum of w, count) of every zone over the pixels one workgroup takes of one
// plane, ws[((plane * gx + bx) * Z + z) * 3].  16-byte loads from the first 16-byte boundary of the plane; workgroup 0 also
// takes the elements in front of it and behind the last whole load.  Without weights the weight sum is the count.
template <typename T, int ZM, bool WT>
__global__ __launch_bounds__(ZN_THREADS) void zone_sum_kernel(const T* __restrict__ x, long hw, const unsigned int* __restrict__ bits,
                                                              const double* __restrict__ wts, int Z, double* __restrict__ ws) {
    constexpr int VW = gd_vec16<T>::W;
    __shared__ double red[ZN_THREADS / GD_WAVE][ZM * 3];
    const int tid = threadIdx.x;
    const T* p = x + (long)blockIdx.y * hw;
    long head = gd_head_of(p);
    if (head > hw) head = hw;             // a plane shorter than its head: all of it is 'rest'
    const long nv = (hw - head) / VW;
    double s[ZM], sw[WT ? ZM : 1];
    unsigned int c[ZM];
#pragma unroll
    for (int z = 0; z < ZM; ++z) {
        s[z] = 0.0;
        c[z] = 0u;
    }
#pragma unroll
    for (int z = 0; z < (WT ? ZM : 1); ++z) sw[z] = 0.0;
    for (long v = (long)blockIdx.x * ZN_THREADS + tid; v < nv; v += (long)gridDim.x * ZN_THREADS) {
        const long i = head + v * VW;
        double e[VW];
        gd_vec16<T>::load(p + i, e);
#pragma unroll
        for (int j = 0; j < VW; ++j) zone_acc<ZM, WT>(s, sw, c, e[j], bits[i + j], WT ? wts[i + j] : 1.0);
    }
    if (blockIdx.x == 0) {
        const long body_end = head + nv * VW, rest = hw - nv * VW;
        for (long r = tid; r < rest; r += ZN_THREADS) {
            const long i = r < head ? r : body_end + (r - head);
            zone_acc<ZM, WT>(s, sw, c, (double)p[i], bits[i], WT ? wts[i] : 1.0);
        }
    }
#pragma unroll
    for (int z = 0; z < ZM; ++z) {
        if (z < Z) {
            const double a = gd_wave_sum_d(s[z]), n = gd_wave_sum_d((double)c[z]);
            const double b = WT ? gd_wave_sum_d(sw[WT ? z : 0]) : n;
            if ((tid & 63) == 0) {
                red[tid >> 6][z * 3 + 0] = a;
                red[tid >> 6][z * 3 + 1] = b;
                red[tid >> 6][z * 3 + 2] = n;
            }
        }
    }
    __syncthreads();
    if (tid < Z * 3) {
        double a = red[0][tid];
        for (int w = 1; w < ZN_THREADS / GD_WAVE; ++w) a += red[w][tid];
        ws[((long)blockIdx.y * gridDim.x + blockIdx.x) * Z * 3 + tid] = a;
    }
}

// one thread per (plane, zone) adds the gx partials in ascending order; no contributing pixel, or a weight sum of zero,
// gives NaN and count 0 (np.nanmean of an empty selection)
__global__ void zone_mean_final_kernel(const double* __restrict__ ws, int gx, long planes, int Z, double* __restrict__ mean,
                                       long long* __restrict__ count) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= planes * Z) return;
    const long pl = i / Z;
    const int z = (int)(i - pl * Z);
    double a = 0.0, b = 0.0, n = 0.0;
    for (int k = 0; k < gx; ++k) {
        const double* s = ws + ((pl * gx + k) * Z + z) * 3;
        a += s[0];
        b += s[1];
        n += s[2];
    }
    const bool ok = n > 0 && b != 0.0;
    mean[i] = ok ? a / b : (double)NAN;
    count[i] = ok ? (long long)n : 0;
}

// workgroups per plane: a function of the shape alone (the partials' order is part of the result)
static int zone_gx(long planes, long hw) { return gd_plane_gx(planes, hw, ZN_THREADS * 8); }

template <typename T, int ZM>
static void zone_sum_launch(const T* x, long planes, long hw, const unsigned int* bits, const double* wts, int Z, double* ws, int gx,
                            hipStream_t st) {
    const dim3 grid((unsigned)gx, (unsigned)planes);
    if (wts)
        hipLaunchKernelGGL((zone_sum_kernel<T, ZM, true>), grid, dim3(ZN_THREADS), 0, st, x, hw, bits, wts, Z, ws);
    else
        hipLaunchKernelGGL((zone_sum_kernel<T, ZM, false>), grid, dim3(ZN_THREADS), 0, st, x, hw, bits, wts, Z, ws);
}

template <typename T>
static void zone_sum_dispatch(const T* x, long planes, long hw, const unsigned int* bits, const double* wts, int Z, double* ws, int gx,
                              hipStream_t st) {
    if (Z <= 8) zone_sum_launch<T, 8>(x, planes, hw, bits, wts, Z, ws, gx, st);
    else if (Z <= 16) zone_sum_launch<T, 16>(x, planes, hw, bits, wts, Z, ws, gx, st);
    else zone_sum_launch<T, 32>(x, planes, hw, bits, wts, Z, ws, gx, st);
}

static bool offsets_ok(const long* off, int Z, long E) {
    if (off[0] != 0 || off[Z] != E) return false;
    for (int z = 0; z < Z; ++z)
        if (off[z + 1] < off[z]) return false;
    return true;
}

}  // namespace

// the checks gd_zone_rasterize and its host twin share
#define ZN_RASTER_CHECKS(fn)                                                                                              \
    GD_CHECK_ARG(edges && edge_off && xs && ys && bits, fn ": null pointer");                                           \
    GD_CHECK_ARG(Z >= 1 && Z <= GD_ZONE_MAX, fn ": Z outside 1..32");                                                    \
    GD_CHECK_ARG(E > 0 && W > 0 && H > 0, fn ": E <= 0, W <= 0 or H <= 0");                                               \
    GD_CHECK_ARG(E <= (1L << 30), fn ": more than 2^30 edges");                                                          \
    GD_CHECK_ARG(offsets_ok(edge_off, Z, E), fn ": offsets must start at 0, never decrease and end at E");               \
    GD_CHECK_ARG(gd_aligned(edges, 8) && gd_aligned(xs, 8) && gd_aligned(ys, 8) && gd_aligned(bits, 4),                   \
                 fn ": pointer not element aligned")

extern "C" int gd_zone_rasterize(const double* edges, long E, const long* edge_off, int Z, const double* xs, long W, const double* ys,
                                 long H, unsigned int* bits, void* stream) {
    ZN_RASTER_CHECKS("gd_zone_rasterize");
    const long gr = (H + ZN_ROWS - 1) / ZN_ROWS, gc = (W + ZN_COLS - 1) / ZN_COLS;
    GD_CHECK_ARG(gr < (1L << 31) && gc <= 65535 && H < (1L << 53) / W, "gd_zone_rasterize: grid too large");
    ZoneOffsets zo;
    for (int z = 0; z <= GD_ZONE_MAX; ++z) zo.off[z] = (int)edge_off[z < Z ? z : Z];
    hipLaunchKernelGGL(zone_rasterize_kernel, dim3((unsigned)gr, (unsigned)gc), dim3(ZN_THREADS), 0, GD_S, edges, zo, Z, xs, W, ys, H,
                       bits);
    GD_LAUNCH_CHECK();
    return 0;
}

// Host only, no GPU call: plain loops over the predicate of zones.h, every pointer in HOST memory.
extern "C" int gd_zone_rasterize_host(const double* edges, long E, const long* edge_off, int Z, const double* xs, long W,
                                      const double* ys, long H, unsigned int* bits) {
    ZN_RASTER_CHECKS("gd_zone_rasterize_host");
    std::vector<double> xi;
    for (long i = 0; i < H; ++i) {
        const double py = ys[i];
        unsigned int* row = bits + i * W;
        for (long j = 0; j < W; ++j) row[j] = 0u;
        for (int z = 0; z < Z; ++z) {
            xi.clear();
            for (long e = edge_off[z]; e < edge_off[z + 1]; ++e) {
                const double* p = edges + 4 * e;
                if (gd_zone_edge_straddles(p[1], p[3], py)) xi.push_back(gd_zone_edge_intercept(p[0], p[1], p[2], p[3], py));
            }
            if (xi.empty()) continue;
            for (long j = 0; j < W; ++j) {
                unsigned int c = 0;
                for (double x : xi) c += gd_zone_crossing_counts(xs[j], x) ? 1u : 0u;
                row[j] |= (c & 1u) << z;
            }
        }
    }
    return 0;
}

extern "C" size_t gd_zone_mean_ws_bytes(long planes, long hw, int Z) {
    if (planes <= 0 || hw <= 0 || Z < 1 || Z > GD_ZONE_MAX) return 0;
    return (size_t)planes * (size_t)zone_gx(planes, hw) * (size_t)Z * 3 * sizeof(double);
}

extern "C" int gd_zone_mean(const void* x, int dtype, long planes, long hw, const unsigned int* bits, int Z, const double* weights,
                            double* mean, long long* count, void* ws, size_t ws_bytes, void* stream) {
    GD_CHECK_ARG(x && bits && mean && count && ws, "gd_zone_mean: null pointer");
    GD_CHECK_ARG(gd_dtype_ok(dtype), "gd_zone_mean: dtype outside {0, 1}");
    GD_CHECK_ARG(Z >= 1 && Z <= GD_ZONE_MAX, "gd_zone_mean: Z outside 1..32");
    GD_CHECK_ARG(planes > 0 && hw > 0, "gd_zone_mean: planes <= 0 or hw <= 0");
    GD_CHECK_ARG(planes <= 65535, "gd_zone_mean: more than 65535 planes in one call");
    GD_CHECK_ARG(hw < (1L << 53) / planes, "gd_zone_mean: tensor too large");
    GD_CHECK_ARG(ws_bytes >= gd_zone_mean_ws_bytes(planes, hw, Z), "gd_zone_mean: workspace smaller than gd_zone_mean_ws_bytes");
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(bits, 4) && gd_aligned(weights, 8) && gd_aligned(mean, 8) &&
                     gd_aligned(count, 8) && gd_aligned(ws, 8),
                 "gd_zone_mean: pointer not element aligned");
    const int gx = zone_gx(planes, hw);
    if (dtype == GD_FILTER_F64) zone_sum_dispatch((const double*)x, planes, hw, bits, weights, Z, (double*)ws, gx, GD_S);
    else zone_sum_dispatch((const float*)x, planes, hw, bits, weights, Z, (double*)ws, gx, GD_S);
    hipLaunchKernelGGL(zone_mean_final_kernel, dim3(gd_cdiv(planes * Z, 256)), dim3(256), 0, GD_S, (const double*)ws, gx, planes, Z,
                       mean, count);
    GD_LAUNCH_CHECK();
    return 0;
}
