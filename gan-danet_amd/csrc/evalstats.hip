// On-device evaluation (include/gandanet.h, "evaluation"): streaming regression statistics of a prediction against its
// target, masked per-plane means and statistics over an ensemble's member axis.  All HBM-bound: every input byte is read
// once, 16 bytes per lane where the pointers allow it, with a scalar head / tail for ragged sizes and for pointers that
// are only element aligned (channel and batch slices).  Reductions are two-stage in a fixed order (no atomics), in fp64,
// as co-moments: a thread shifts its sums by the first valid pair it meets (norm.hip does the same for BatchNorm), and
// everything above a thread is merged with Chan's pairwise formulas -- raw sums of squares are never formed.
// From elem_util.h: gd_head_of, gd_vec16, gd_plane_gx, gd_block_sum_d, gd_shfl_down_d, gd_aligned, gd_elem_aligned,
// GD_S.
#include "elem_util.h"

#include <math.h>

#include <string>

namespace {

constexpr int EV_BLOCKS = 1024;  // stage-1 workgroups at most = partial records in the workspace
constexpr int EV_THREADS = 256;

// ---- the record: n, mean_p, mean_t, M2_p, M2_t, C_pt, sum|p-t|, sum(p-t)^2 ------------------------------------------
struct Rec {
    double n, mp, mt, m2p, m2t, c, sae, sse;
};

// Chan et al.: statistics of A followed by B.  A record with n == 0 is neutral whatever else it holds.
__host__ __device__ inline Rec rec_merge(const Rec& a, const Rec& b) {
    if (!(b.n > 0)) return a;
    if (!(a.n > 0)) return b;
    Rec r;
    r.n = a.n + b.n;
    const double dp = b.mp - a.mp, dt = b.mt - a.mt;
    const double fb = b.n / r.n, w = a.n * fb;
    r.mp = a.mp + dp * fb;
    r.mt = a.mt + dt * fb;
    r.m2p = a.m2p + b.m2p + dp * dp * w;
    r.m2t = a.m2t + b.m2t + dt * dt * w;
    r.c = a.c + b.c + dp * dt * w;
    r.sae = a.sae + b.sae;
    r.sse = a.sse + b.sse;
    return r;
}

__host__ __device__ inline Rec rec_zero() { return Rec{0, 0, 0, 0, 0, 0, 0, 0}; }

// lane l ends with the merge of lanes l .. 63 in ascending order along a fixed tree; lane 0 holds the wave's record
__device__ __forceinline__ Rec rec_wave_merge(Rec r) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        Rec b;
        b.n = gd_shfl_down_d(r.n, o);
        b.mp = gd_shfl_down_d(r.mp, o);
        b.mt = gd_shfl_down_d(r.mt, o);
        b.m2p = gd_shfl_down_d(r.m2p, o);
        b.m2t = gd_shfl_down_d(r.m2t, o);
        b.c = gd_shfl_down_d(r.c, o);
        b.sae = gd_shfl_down_d(r.sae, o);
        b.sse = gd_shfl_down_d(r.sse, o);
        if (((threadIdx.x & 63) & (2 * o - 1)) == 0) r = rec_merge(r, b);   // lanes that own a block of 2*o lanes
    }
    return r;
}

__device__ __forceinline__ void rec_store(double* dst, const Rec& r) {
    dst[0] = r.n; dst[1] = r.mp; dst[2] = r.mt; dst[3] = r.m2p;
    dst[4] = r.m2t; dst[5] = r.c; dst[6] = r.sae; dst[7] = r.sse;
}
__host__ __device__ inline Rec rec_load(const double* s) { return Rec{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]}; }

// ---- a thread's running sums, shifted by its first valid pair ---------------------------------------------------------
struct Acc {
    double sp, st;                              // the shift
    double s1p, s1t, s2p, s2t, spt, sae, sse;   // sums of (p - sp), (t - st), their squares and product, |p-t|, (p-t)^2
    unsigned int cnt;
    bool have;
};

template <bool AFF, bool SKIPNAN>
__device__ __forceinline__ void acc_add(Acc& A, double p, double t, bool valid, double a, double b) {
    if (AFF) {
        p = p * a + b;
        t = t * a + b;
    }
    if (SKIPNAN) valid = valid && p == p && t == t;
    if (valid && !A.have) {   // after a thread's first pair this is not taken again
        A.sp = p;
        A.st = t;
        A.have = true;
    }
    const double dp = valid ? p - A.sp : 0.0, dt = valid ? t - A.st : 0.0, d = valid ? p - t : 0.0;
    A.s1p += dp;
    A.s1t += dt;
    A.s2p = fma(dp, dp, A.s2p);
    A.s2t = fma(dt, dt, A.s2t);
    A.spt = fma(dp, dt, A.spt);
    A.sae += fabs(d);
    A.sse = fma(d, d, A.sse);
    A.cnt += valid ? 1u : 0u;
}

__device__ __forceinline__ Rec acc_finish(const Acc& A) {
    if (A.cnt == 0) return rec_zero();
    Rec r;
    r.n = (double)A.cnt;
    const double ip = A.s1p / r.n, it = A.s1t / r.n;
    r.mp = A.sp + ip;
    r.mt = A.st + it;
    r.m2p = fmax(A.s2p - A.s1p * ip, 0.0);
    r.m2t = fmax(A.s2t - A.s1t * it, 0.0);
    r.c = A.spt - A.s1p * it;
    r.sae = A.sae;
    r.sse = A.sse;
    return r;
}

// Stage 1.  grid (gx, gy): block (bx, by) takes the planes by, by + gy, ... and of each plane the 16-byte vectors
// bx * 256 + tid, + gx * 256, ...; block bx == 0 also takes the plane's unaligned head and its tail.  Without a mask the
// host passes the whole tensor as ONE plane.  One partial record per block at ws[by * gx + bx].
template <typename T, bool MASK, bool AFF, bool SKIPNAN>
__global__ __launch_bounds__(EV_THREADS) void eval_stats_kernel(const T* __restrict__ pred, const T* __restrict__ truth,
                                                                long planes, long hw,
                                                                const unsigned char* __restrict__ mask, double a, double b,
                                                                double* __restrict__ ws) {
    typedef typename gd_vec16<T>::type V;
    constexpr int W = gd_vec16<T>::W;
    __shared__ double red[EV_THREADS / 64][8];
    Acc A;
    A.sp = A.st = A.s1p = A.s1t = A.s2p = A.s2t = A.spt = A.sae = A.sse = 0.0;
    A.cnt = 0;
    A.have = false;
    const int tid = threadIdx.x;
    for (long pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const T* p = pred + pl * hw;
        const T* t = truth + pl * hw;
        const long head = gd_head_of(p);
        if (head != gd_head_of(t) || head > hw) {   // the two pointers never meet a 16-byte boundary together: scalar sweep
            for (long i = (long)blockIdx.x * EV_THREADS + tid; i < hw; i += (long)gridDim.x * EV_THREADS) {
                const bool valid = MASK ? mask[i] != 0 : true;
                acc_add<AFF, SKIPNAN>(A, (double)p[i], (double)t[i], valid, a, b);
            }
            continue;
        }
        const long nv = (hw - head) / W;
        const V* p4 = reinterpret_cast<const V*>(p + head);
        const V* t4 = reinterpret_cast<const V*>(t + head);
        for (long v = (long)blockIdx.x * EV_THREADS + tid; v < nv; v += (long)gridDim.x * EV_THREADS) {
            const V pv = p4[v], tv = t4[v];
            double pe[W], te[W];
            gd_vec16<T>::unpack(pv, pe);
            gd_vec16<T>::unpack(tv, te);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const bool valid = MASK ? mask[head + v * W + j] != 0 : true;
                acc_add<AFF, SKIPNAN>(A, pe[j], te[j], valid, a, b);
            }
        }
        if (blockIdx.x == 0) {   // head [0, head) and tail [head + nv * W, hw): fewer than 2 * W elements
            const long body_end = head + nv * W, rest = hw - nv * W;
            for (long r = tid; r < rest; r += EV_THREADS) {
                const long i = r < head ? r : body_end + (r - head);
                const bool valid = MASK ? mask[i] != 0 : true;
                acc_add<AFF, SKIPNAN>(A, (double)p[i], (double)t[i], valid, a, b);
            }
        }
    }
    Rec r = rec_wave_merge(acc_finish(A));
    if ((tid & 63) == 0) rec_store(red[tid >> 6], r);
    __syncthreads();
    if (tid == 0) {
        Rec s = rec_load(red[0]);
        for (int w = 1; w < EV_THREADS / 64; ++w) s = rec_merge(s, rec_load(red[w]));
        rec_store(ws + 8 * ((long)blockIdx.y * gridDim.x + blockIdx.x), s);
    }
}

// Stage 2 (one wave): lane l merges its contiguous run of partial records in ascending order, then the lanes are merged
// in ascending order along the same fixed tree as inside a wave of stage 1.
__global__ __launch_bounds__(64) void eval_stats_final_kernel(const double* __restrict__ ws, int nparts,
                                                              double* __restrict__ rec) {
    const int lane = threadIdx.x, per = (nparts + 63) / 64;
    Rec r = rec_zero();
    for (int i = lane * per; i < (lane + 1) * per && i < nparts; ++i) r = rec_merge(r, rec_load(ws + 8 * (long)i));
    r = rec_wave_merge(r);
    if (lane == 0) rec_store(rec, r);
}

struct EvGrid {
    int gx, gy;
};
// without a mask the tensor is one plane of n elements
static EvGrid eval_grid(long planes, long hw) {
    long gx = (hw + EV_THREADS * 4 - 1) / (EV_THREADS * 4);
    gx = gx < 1 ? 1 : (gx > EV_BLOCKS ? EV_BLOCKS : gx);
    long gy = EV_BLOCKS / gx;
    gy = gy > planes ? planes : gy;
    return EvGrid{(int)gx, (int)(gy < 1 ? 1 : gy)};
}

// ---- masked plane means -------------------------------------------------------------------------------------------
// grid (gx, planes): partial (sum, count) of the valid pixels of one plane per block, ws[(plane * gx + bx) * 2].  16-byte
// loads from the plane's first 16-byte boundary; block 0 also takes the elements in front of it and behind the last whole
// load.  SKIPNAN: a NaN pixel counts as invalid (gd_masked_plane_mean_f64); without it a NaN at a valid pixel makes the
// plane's sum NaN (gd_masked_plane_mean).
template <typename T, bool SKIPNAN>
__global__ __launch_bounds__(EV_THREADS) void plane_sum_kernel(const T* __restrict__ x, long hw,
                                                               const unsigned char* __restrict__ mask,
                                                               double* __restrict__ ws) {
    constexpr int W = gd_vec16<T>::W;
    __shared__ double red[EV_THREADS / 64][2];
    const int tid = threadIdx.x;
    const T* p = x + (long)blockIdx.y * hw;
    long head = gd_head_of(p);
    if (head > hw) head = hw;             // a plane shorter than its head: all of it is 'rest'
    const long nv = (hw - head) / W;
    double s = 0.0;
    unsigned int cnt = 0;
    for (long v = (long)blockIdx.x * EV_THREADS + tid; v < nv; v += (long)gridDim.x * EV_THREADS) {
        T e[W];
        gd_vec16<T>::load(p + head + v * W, e);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            bool valid = mask ? mask[head + v * W + j] != 0 : true;
            if (SKIPNAN) valid = valid && e[j] == e[j];
            s += valid ? (double)e[j] : 0.0;
            cnt += valid ? 1u : 0u;
        }
    }
    if (blockIdx.x == 0) {
        const long body_end = head + nv * W, rest = hw - nv * W;
        for (long r = tid; r < rest; r += EV_THREADS) {
            const long i = r < head ? r : body_end + (r - head);
            bool valid = mask ? mask[i] != 0 : true;
            if (SKIPNAN) valid = valid && p[i] == p[i];
            s += valid ? (double)p[i] : 0.0;
            cnt += valid ? 1u : 0u;
        }
    }
    double sc[2] = {s, (double)cnt};
    gd_block_sum_d<2, EV_THREADS / 64>(sc, red);
    if (tid == 0) {
        double* o = ws + 2 * ((long)blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = sc[0];
        o[1] = sc[1];
    }
}
// one thread per plane adds the plane's gx partials in ascending order; no valid pixel -> NaN (np.nanmean)
__global__ void plane_mean_final_kernel(const double* __restrict__ ws, int gx, long planes, double* __restrict__ mean,
                                        long long* __restrict__ count) {
    const long pl = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pl >= planes) return;
    double s = 0.0, c = 0.0;
    for (int i = 0; i < gx; ++i) {
        s += ws[2 * (pl * gx + i)];
        c += ws[2 * (pl * gx + i) + 1];
    }
    mean[pl] = c > 0 ? s / c : (double)NAN;
    count[pl] = (long long)c;
}
static int plane_gx(long planes, long hw) { return gd_plane_gx(planes, hw, EV_THREADS * 4); }

// the two exported plane means: `fn` is the entry's name, for its messages
template <typename T>
static int plane_mean_launch(const char* fn, const T* x, long planes, long hw, const unsigned char* mask, double* mean,
                             long long* count, void* ws, size_t ws_bytes, hipStream_t st) {
    const std::string f(fn);
#define PM_CHECK(cond, what) GD_CHECK_ARG(cond, (f + what).c_str())
    PM_CHECK(x && mean && count && ws, ": null pointer");
    PM_CHECK(planes > 0 && hw > 0, ": n <= 0");
    PM_CHECK(planes <= 65535, ": more than 65535 planes in one call");
    PM_CHECK(ws_bytes >= gd_masked_plane_mean_ws_bytes(planes, hw), ": workspace smaller than " + f + "_ws_bytes");
    PM_CHECK(gd_aligned(x, sizeof(T)) && gd_aligned(mean, 8) && gd_aligned(count, 8) && gd_aligned(ws, 8),
             ": pointer not element aligned");
#undef PM_CHECK
    const int gx = plane_gx(planes, hw);
    // SKIPNAN with the dtype: the fp64 entry leaves NaN pixels out, the fp32 entry does not
    hipLaunchKernelGGL((plane_sum_kernel<T, sizeof(T) == 8>), dim3(gx, (unsigned)planes), dim3(EV_THREADS), 0, st, x, hw, mask,
                       (double*)ws);
    hipLaunchKernelGGL(plane_mean_final_kernel, dim3(gd_cdiv(planes, 256)), dim3(256), 0, st, (const double*)ws, gx, planes,
                       mean, count);
    GD_LAUNCH_CHECK();
    return 0;
}

// ---- statistics over the member axis ----------------------------------------------------------------------------------
// One lane owns VW consecutive elements (one 16-byte load per member when VW > 1) and keeps all M members of them in
// registers (fp32 members widen exactly; nothing spills to scratch at M = 32 in either dtype): mean = v0 + sum(v_m - v0) / M, then
// sum (v_m - mean)^2 over the same registers, all arithmetic in fp64, rounded once on the store.  Shifting by member 0
// makes identical members give exactly (v0, 0).  Items below `skip_from` map to themselves, the others to item +
// skip_len: the scalar instance covers the head and the tail around a vector body.  MMAX = 8 or 32 bounds the unrolled
// member loops; both have a 16-byte and a scalar instance.
template <typename T, int MMAX, int VW>
__global__ __launch_bounds__(EV_THREADS) void ensemble_stats_kernel(const T* __restrict__ x, int M, long mstride, long items,
                                                                    long skip_from, long skip_len, T* __restrict__ mean,
                                                                    T* __restrict__ sd) {
    const double inv = 1.0 / (double)M;
    for (long it = (long)blockIdx.x * EV_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * EV_THREADS) {
        const long e = (it < skip_from ? it : it + skip_len) * VW;
        T v[MMAX][VW];
#pragma unroll
        for (int m = 0; m < MMAX; ++m) {
            if (m < M) {
                if constexpr (VW > 1) {
                    gd_vec16<T>::load(x + (long)m * mstride + e, v[m]);
                } else {
                    v[m][0] = x[(long)m * mstride + e];
                }
            }
        }
        double mu[VW], sq[VW];
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            double s = 0.0;
#pragma unroll
            for (int m = 1; m < MMAX; ++m)
                if (m < M) s += (double)v[m][j] - (double)v[0][j];
            mu[j] = (double)v[0][j] + s * inv;
            double q = 0.0;
#pragma unroll
            for (int m = 0; m < MMAX; ++m)
                if (m < M) {
                    const double d = (double)v[m][j] - mu[j];
                    q = fma(d, d, q);
                }
            sq[j] = sqrt(q * inv);
        }
        if constexpr (VW > 1) {
            gd_vec16<T>::store(mean + e, mu);
            gd_vec16<T>::store(sd + e, sq);
        } else {
            mean[e] = (T)mu[0];
            sd[e] = (T)sq[0];
        }
    }
}

static int ens_grid(long items) {
    long g = (items + EV_THREADS - 1) / EV_THREADS;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

template <typename T, int MMAX>
static void ensemble_launch_m(const T* x, int M, long mstride, long n, long head, long nv, T* mean, T* sd, hipStream_t s) {
    constexpr int VW = gd_vec16<T>::W;
    if (nv > 0)
        hipLaunchKernelGGL((ensemble_stats_kernel<T, MMAX, VW>), dim3(ens_grid(nv)), dim3(EV_THREADS), 0, s, x + head, M,
                           mstride, nv, nv, 0L, mean + head, sd + head);
    const long rest = n - nv * VW;
    if (rest > 0)
        hipLaunchKernelGGL((ensemble_stats_kernel<T, MMAX, 1>), dim3(ens_grid(rest)), dim3(EV_THREADS), 0, s, x, M, mstride,
                           rest, head, nv * VW, mean, sd);
}

template <typename T>
static void ensemble_launch(const T* x, int M, long mstride, long n, T* mean, T* sd, hipStream_t s) {
    // 16-byte path: every member row, and both outputs, reach a 16-byte boundary after the same `head` elements (a
    // single member has no stride to satisfy); otherwise every element goes through the scalar instance
    long head = gd_head_of(x), nv = 0;
    const bool same = head == gd_head_of(mean) && head == gd_head_of(sd) && (M == 1 || (mstride * (long)sizeof(T)) % 16 == 0);
    if (same && head <= n) nv = (n - head) / gd_vec16<T>::W;
    else head = 0;
    if (M <= 8) ensemble_launch_m<T, 8>(x, M, mstride, n, head, nv, mean, sd, s);
    else ensemble_launch_m<T, 32>(x, M, mstride, n, head, nv, mean, sd, s);
}

template <typename T, bool MASK>
static void eval_launch(const T* pred, const T* truth, long planes, long hw, const unsigned char* mask, double a, double b,
                        int flags, double* ws, EvGrid g, hipStream_t s) {
    const bool aff = !(a == 1.0 && b == 0.0), skip = (flags & GD_EVAL_SKIP_NAN) != 0;
    const dim3 grid(g.gx, g.gy), blk(EV_THREADS);
#define EV_GO(AFF, SKIP) \
    hipLaunchKernelGGL((eval_stats_kernel<T, MASK, AFF, SKIP>), grid, blk, 0, s, pred, truth, planes, hw, mask, a, b, ws)
    if (aff && skip) EV_GO(true, true);
    else if (aff) EV_GO(true, false);
    else if (skip) EV_GO(false, true);
    else EV_GO(false, false);
#undef EV_GO
}

}  // namespace

extern "C" size_t gd_eval_stats_ws_bytes(long n) {
    if (n <= 0) return 0;
    // the partial count depends on how the planes are cut; EV_BLOCKS records cover every cut
    return (size_t)EV_BLOCKS * 8 * sizeof(double);
}

extern "C" int gd_eval_stats(const void* pred, const void* truth, long planes, long hw, const unsigned char* mask, double a,
                             double b, int flags, double* rec, void* ws, size_t ws_bytes, void* stream) {
    GD_CHECK_ARG(pred && truth && rec && ws, "gd_eval_stats: null pointer");
    GD_CHECK_ARG(planes > 0 && hw > 0, "gd_eval_stats: n <= 0");
    GD_CHECK_ARG((flags & ~(GD_EVAL_F64 | GD_EVAL_SKIP_NAN)) == 0, "gd_eval_stats: unknown flag");
    GD_CHECK_ARG(a == a && b == b, "gd_eval_stats: the affine is NaN");
    GD_CHECK_ARG(ws_bytes >= gd_eval_stats_ws_bytes(planes * hw), "gd_eval_stats: workspace smaller than gd_eval_stats_ws_bytes");
    const int f64 = flags & GD_EVAL_F64;
    GD_CHECK_ARG(gd_elem_aligned(pred, f64) && gd_elem_aligned(truth, f64) && gd_aligned(rec, 8) && gd_aligned(ws, 8),
                 "gd_eval_stats: pointer not element aligned");
    if (!mask) {   // nothing repeats per plane: one plane of n elements
        hw *= planes;
        planes = 1;
    }
    const EvGrid g = eval_grid(planes, hw);
    double* w = (double*)ws;
    if (flags & GD_EVAL_F64) {
        if (mask) eval_launch<double, true>((const double*)pred, (const double*)truth, planes, hw, mask, a, b, flags, w, g, GD_S);
        else eval_launch<double, false>((const double*)pred, (const double*)truth, planes, hw, mask, a, b, flags, w, g, GD_S);
    } else {
        if (mask) eval_launch<float, true>((const float*)pred, (const float*)truth, planes, hw, mask, a, b, flags, w, g, GD_S);
        else eval_launch<float, false>((const float*)pred, (const float*)truth, planes, hw, mask, a, b, flags, w, g, GD_S);
    }
    hipLaunchKernelGGL(eval_stats_final_kernel, dim3(1), dim3(64), 0, GD_S, w, g.gx * g.gy, rec);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t gd_masked_plane_mean_ws_bytes(long planes, long hw) {
    if (planes <= 0 || hw <= 0) return 0;
    return (size_t)planes * plane_gx(planes, hw) * 2 * sizeof(double);
}

extern "C" int gd_masked_plane_mean(const float* x, long planes, long hw, const unsigned char* mask, double* mean,
                                    long long* count, void* ws, size_t ws_bytes, void* stream) {
    return plane_mean_launch("gd_masked_plane_mean", x, planes, hw, mask, mean, count, ws, ws_bytes, GD_S);
}

extern "C" size_t gd_masked_plane_mean_f64_ws_bytes(long planes, long hw) { return gd_masked_plane_mean_ws_bytes(planes, hw); }

extern "C" int gd_masked_plane_mean_f64(const double* x, long planes, long hw, const unsigned char* mask, double* mean,
                                        long long* count, void* ws, size_t ws_bytes, void* stream) {
    return plane_mean_launch("gd_masked_plane_mean_f64", x, planes, hw, mask, mean, count, ws, ws_bytes, GD_S);
}

extern "C" int gd_ensemble_stats(const void* x, int M, long member_stride, long n, int f64, void* mean, void* std_out,
                                 void* stream) {
    GD_CHECK_ARG(x && mean && std_out, "gd_ensemble_stats: null pointer");
    GD_CHECK_ARG(n > 0, "gd_ensemble_stats: n <= 0");
    GD_CHECK_ARG(M >= 1 && M <= 32, "gd_ensemble_stats: M outside 1..32");
    GD_CHECK_ARG(M == 1 || member_stride >= n, "gd_ensemble_stats: member stride smaller than n");
    GD_CHECK_ARG(gd_elem_aligned(x, f64) && gd_elem_aligned(mean, f64) && gd_elem_aligned(std_out, f64),
                 "gd_ensemble_stats: pointer not element aligned");
    if (f64) ensemble_launch<double>((const double*)x, M, member_stride, n, (double*)mean, (double*)std_out, GD_S);
    else ensemble_launch<float>((const float*)x, M, member_stride, n, (float*)mean, (float*)std_out, GD_S);
    GD_LAUNCH_CHECK();
    return 0;
}

// Host only.  Merges k records in the given order (the same rec_merge as the kernels) and derives the metrics.
extern "C" int gd_eval_merge_host(const double* recs, long k, double* rec_out, double* metrics) {
    GD_CHECK_ARG(metrics, "gd_eval_merge_host: null pointer");
    GD_CHECK_ARG(k >= 0 && (recs || k == 0), "gd_eval_merge_host: k records but no pointer");
    Rec r = rec_zero();
    for (long i = 0; i < k; ++i) r = rec_merge(r, rec_load(recs + 8 * i));
    if (!(r.n > 0)) r = rec_zero();
    if (rec_out) {
        rec_out[0] = r.n; rec_out[1] = r.mp; rec_out[2] = r.mt; rec_out[3] = r.m2p;
        rec_out[4] = r.m2t; rec_out[5] = r.c; rec_out[6] = r.sae; rec_out[7] = r.sse;
    }
    if (!(r.n > 0)) {
        metrics[0] = metrics[1] = metrics[2] = metrics[3] = NAN;
        return 0;
    }
    metrics[0] = r.sse / r.n;                                   // mean_squared_error
    metrics[1] = r.sae / r.n;                                   // mean_absolute_error
    // r2_score defaults: 1 - SS_res / SS_tot; a constant truth scores 1 when the prediction is perfect, else 0
    metrics[2] = r.m2t > 0 ? 1.0 - r.sse / r.m2t : (r.sse == 0 ? 1.0 : 0.0);
    // np.corrcoef(...)[0, 1]: 0 / 0 = NaN for a constant series; clipped to [-1, 1] as numpy does
    if (r.m2p > 0 && r.m2t > 0) {
        const double cc = r.c / (sqrt(r.m2p) * sqrt(r.m2t));
        metrics[3] = cc > 1.0 ? 1.0 : (cc < -1.0 ? -1.0 : cc);
    } else {
        metrics[3] = NAN;
    }
    return 0;
}
