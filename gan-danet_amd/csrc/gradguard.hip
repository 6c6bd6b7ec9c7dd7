// Guarded optimiser step (include/gandanet.h, "guarded step"): the squared norm of a whole list of gradient tensors, the
// clip / skip decision as one record in device memory, and an AdamW pass that reads that record -- the host never learns
// whether a step was applied until it asks.  All HBM-bound: the norm reads every gradient once with 16-byte loads where
// the pointer allows it (scalar head / tail otherwise, as in evalstats.hip), the update moves the 28 bytes per element of
// adamw_kernel (pointwise.hip) plus 8 when an averaged copy of the weights (EMA) rides along.  Reductions are two-stage in
// a fixed order, in fp64, without atomics.  From elem_util.h: gd_head_of, gd_block_sum_d, gd_aligned, GD_S.
#include "elem_util.h"

#include <math.h>

namespace {

constexpr int GG_THREADS = 256;
constexpr long GG_CHUNK = GD_GUARD_CHUNK;   // elements of one tensor per workgroup = per partial slot
constexpr int GG_TENSORS = 48;              // (pointer, n) pairs that travel by value in one launch's arguments

// One launch's slice of the tensor list.  first[t] = the block of this launch at which tensor t starts; first[count] =
// the launch's grid.  Passed by value: no pointer table in device memory, nothing a replayed graph could read stale.
struct NormArgs {
    const float* ptr[GG_TENSORS];
    long n[GG_TENSORS];
    int first[GG_TENSORS + 1];
    int count;
};

__device__ __forceinline__ double sq4(const float4& q, double acc) {
    acc = fma((double)q.x, (double)q.x, acc);
    acc = fma((double)q.y, (double)q.y, acc);
    acc = fma((double)q.z, (double)q.z, acc);
    return fma((double)q.w, (double)q.w, acc);
}

// Stage 1.  Block b of the launch owns chunk (b - first[t]) of tensor t: elements [c * GG_CHUNK, min(n, (c + 1) * GG_CHUNK)).
// Its partial sum of squares, times gscale^2, goes to ws[slot0 + b]: the slot is fixed by (tensor, chunk of tensor) alone.
__global__ __launch_bounds__(GG_THREADS) void grad_sqnorm_kernel(const NormArgs a, double gscale2, double* __restrict__ ws) {
    __shared__ double red[GG_THREADS / 64][1];
    const int b = blockIdx.x, tid = threadIdx.x;
    int t = 0;
    while (t + 1 < a.count && b >= a.first[t + 1]) ++t;   // uniform over the block
    const long lo = (long)(b - a.first[t]) * GG_CHUNK;
    long len = a.n[t] - lo;
    len = len > GG_CHUNK ? GG_CHUNK : len;
    const float* p = a.ptr[t] + lo;
    long head = gd_head_of(p);
    head = head > len ? len : head;
    const long nv = (len - head) / 4;
    const float4* p4 = reinterpret_cast<const float4*>(p + head);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    long v = tid;
    for (; v + 3 * GG_THREADS < nv; v += 4 * GG_THREADS) {   // four independent 16-byte loads in flight per lane
        const float4 q0 = p4[v], q1 = p4[v + GG_THREADS], q2 = p4[v + 2 * GG_THREADS], q3 = p4[v + 3 * GG_THREADS];
        s0 = sq4(q0, s0);
        s1 = sq4(q1, s1);
        s2 = sq4(q2, s2);
        s3 = sq4(q3, s3);
    }
    for (; v < nv; v += GG_THREADS) s0 = sq4(p4[v], s0);
    // head [0, head) and tail [head + 4 nv, len): fewer than 8 elements
    const long body_end = head + nv * 4, rest = len - nv * 4;
    if (tid < rest) {
        const double e = (double)p[tid < head ? tid : body_end + (tid - head)];
        s1 = fma(e, e, s1);
    }
    double s[1] = {(s0 + s1) + (s2 + s3)};
    gd_block_sum_d<1, GG_THREADS / 64>(s, red);
    if (tid == 0) ws[b] = s[0] * gscale2;
}

// Stage 2 (one block): thread i adds its contiguous run of slots in ascending order, then the threads are added in
// ascending order along a fixed tree.  sqnorm = (accumulate ? sqnorm : 0) + sum.
__global__ __launch_bounds__(GG_THREADS) void grad_sqnorm_final_kernel(const double* __restrict__ ws, long nslots, int accumulate,
                                                                      double* __restrict__ rec) {
    __shared__ double red[GG_THREADS];
    const int tid = threadIdx.x;
    const long per = (nslots + GG_THREADS - 1) / GG_THREADS;
    double s = 0.0;
    for (long i = tid * per; i < (tid + 1) * per && i < nslots; ++i) s += ws[i];
    red[tid] = s;
    __syncthreads();
    for (int o = 1; o < GG_THREADS; o <<= 1) {
        if ((tid & (2 * o - 1)) == 0) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) rec[GD_GUARD_SQNORM] = (accumulate ? rec[GD_GUARD_SQNORM] : 0.0) + red[0];
}

__global__ void guard_finalize_kernel(double* __restrict__ rec, double max_norm, int skip_nonfinite) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double norm = sqrt(rec[GD_GUARD_SQNORM]);
    const bool ok = skip_nonfinite ? isfinite(norm) : true;
    double coef = 1.0;
    if (max_norm > 0.0) {
        coef = max_norm / (norm + 1e-6);
        coef = coef < 1.0 ? coef : 1.0;   // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1)
    }
    rec[GD_GUARD_NORM] = norm;
    rec[GD_GUARD_COEF] = coef;
    rec[GD_GUARD_OK] = ok ? 1.0 : 0.0;
    if (ok) rec[GD_GUARD_APPLIED] += 1.0;
    else rec[GD_GUARD_SKIPPED] += 1.0;
}

// the arithmetic of adamw_kernel (pointwise.hip), term for term; gs = gscale * coef
struct AdamC {
    float lr, beta1, beta2, eps, wd, gs, inv_bc1, inv_sqrt_bc2, decay;
};
template <bool EMA>
__device__ __forceinline__ void adamw_one(const AdamC& c, float& p, float g, float& m, float& v, float& e) {
    // every product and sum rounded on its own: which pairs the compiler fuses into an fma depends on what else uses the
    // value, and the weights must come out the same bits with and without the EMA, on the vector and on the scalar path
#pragma clang fp contract(off)
    const float gi = g * c.gs;
    float pi = p * (1.f - c.lr * c.wd);
    const float mi = c.beta1 * m + (1.f - c.beta1) * gi;
    const float vi = c.beta2 * v + (1.f - c.beta2) * gi * gi;
    const float denom = sqrtf(vi) * c.inv_sqrt_bc2 + c.eps;
    pi -= (c.lr * c.inv_bc1) * (mi / denom);
    p = pi;
    m = mi;
    v = vi;
    if (EMA) e = c.decay * e + (1.f - c.decay) * pi;
}

// `head` scalar elements, then nv 16-byte vectors, then the scalar tail; the host passes head = nv = 0 when the pointers
// do not reach a 16-byte boundary together, and every element then takes the scalar loop.  Nothing is written when the
// record says the step is skipped; the scaled gradient is never written at all.
template <bool EMA>
__global__ __launch_bounds__(GG_THREADS) void adamw_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v,
                                                                  float* __restrict__ ema, long n, long head, long nv,
                                                                  const double* __restrict__ rec, float lr, float beta1,
                                                                  float beta2, float eps, float wd, float gscale,
                                                                  float decay) {
    if (rec[GD_GUARD_OK] == 0.0) return;
    const double step = rec[GD_GUARD_APPLIED];   // already counts this step (gd_guard_finalize)
    AdamC c;
    c.lr = lr; c.beta1 = beta1; c.beta2 = beta2; c.eps = eps; c.wd = wd; c.decay = decay;
    c.gs = gscale * (float)rec[GD_GUARD_COEF];
    c.inv_bc1 = (float)(1.0 / (1.0 - pow((double)beta1, step)));
    c.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, step)));
    const long gtid = (long)blockIdx.x * GG_THREADS + threadIdx.x, gstride = (long)gridDim.x * GG_THREADS;
    float4* p4 = reinterpret_cast<float4*>(p + head);
    const float4* g4 = reinterpret_cast<const float4*>(g + head);
    float4* m4 = reinterpret_cast<float4*>(m + head);
    float4* v4 = reinterpret_cast<float4*>(v + head);
    float4* e4 = reinterpret_cast<float4*>(ema + head);
    for (long i = gtid; i < nv; i += gstride) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i], ee = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 gg = g4[i];
        if (EMA) ee = e4[i];
        adamw_one<EMA>(c, pp.x, gg.x, mm.x, vv.x, ee.x);
        adamw_one<EMA>(c, pp.y, gg.y, mm.y, vv.y, ee.y);
        adamw_one<EMA>(c, pp.z, gg.z, mm.z, vv.z, ee.z);
        adamw_one<EMA>(c, pp.w, gg.w, mm.w, vv.w, ee.w);
        p4[i] = pp;
        m4[i] = mm;
        v4[i] = vv;
        if (EMA) e4[i] = ee;
    }
    const long body_end = head + nv * 4, rest = n - nv * 4;
    for (long r = gtid; r < rest; r += gstride) {
        const long i = r < head ? r : body_end + (r - head);
        float pi = p[i], mi = m[i], vi = v[i], ei = EMA ? ema[i] : 0.f;
        adamw_one<EMA>(c, pi, g[i], mi, vi, ei);
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
        if (EMA) ema[i] = ei;
    }
}

static long chunks_of(long n) { return (n + GG_CHUNK - 1) / GG_CHUNK; }

}  // namespace

extern "C" size_t gd_grad_sqnorm_ws_bytes(long total_chunks) {
    return total_chunks > 0 ? (size_t)total_chunks * sizeof(double) : 0;
}

extern "C" int gd_grad_sqnorm(const float* const* grads, const long* ns, int count, float gscale, int accumulate, double* rec,
                              void* ws, size_t ws_bytes, void* stream) {
    GD_CHECK_ARG(grads && ns && rec && ws, "gd_grad_sqnorm: null pointer");
    GD_CHECK_ARG(count > 0, "gd_grad_sqnorm: n <= 0 (empty tensor list)");
    GD_CHECK_ARG(gd_aligned(rec, 8) && gd_aligned(ws, 8), "gd_grad_sqnorm: record or workspace not 8-byte aligned");
    long total = 0;
    for (int t = 0; t < count; ++t) {
        GD_CHECK_ARG(grads[t], "gd_grad_sqnorm: null pointer in the tensor list");
        GD_CHECK_ARG(ns[t] > 0, "gd_grad_sqnorm: n <= 0 in the tensor list");
        GD_CHECK_ARG(gd_aligned(grads[t], 4), "gd_grad_sqnorm: pointer not element aligned");
        // one launch's grid is an int: a tensor of more than 2^31 - 1 chunks (1.4e14 elements) does not fit one
        GD_CHECK_ARG(chunks_of(ns[t]) <= 0x7fffffffL, "gd_grad_sqnorm: tensor longer than 2^31 - 1 chunks");
        total += chunks_of(ns[t]);
    }
    GD_CHECK_ARG(ws_bytes >= gd_grad_sqnorm_ws_bytes(total), "gd_grad_sqnorm: workspace smaller than gd_grad_sqnorm_ws_bytes");
    long slot0 = 0;
    int t = 0;
    while (t < count) {   // argument chunks: up to GG_TENSORS tensors and 2^31 - 1 blocks each
        NormArgs a;
        long blocks = 0;
        int k = 0;
        while (t + k < count && k < GG_TENSORS && blocks + chunks_of(ns[t + k]) <= 0x7fffffffL) {
            a.ptr[k] = grads[t + k];
            a.n[k] = ns[t + k];
            a.first[k] = (int)blocks;
            blocks += chunks_of(ns[t + k]);
            ++k;
        }
        for (int j = k; j < GG_TENSORS; ++j) {
            a.ptr[j] = nullptr;
            a.n[j] = 0;
            a.first[j] = (int)blocks;
        }
        a.first[GG_TENSORS] = (int)blocks;
        a.count = k;
        hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)blocks), dim3(GG_THREADS), 0, GD_S, a,
                           (double)gscale * (double)gscale, (double*)ws + slot0);
        slot0 += blocks;
        t += k;
    }
    hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(GG_THREADS), 0, GD_S, (const double*)ws, total, accumulate, rec);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_guard_finalize(double* rec, double max_norm, int skip_nonfinite, void* stream) {
    GD_CHECK_ARG(rec, "gd_guard_finalize: null pointer");
    GD_CHECK_ARG(gd_aligned(rec, 8), "gd_guard_finalize: record not 8-byte aligned");
    GD_CHECK_ARG(max_norm == max_norm, "gd_guard_finalize: max_norm is NaN");
    hipLaunchKernelGGL(guard_finalize_kernel, dim3(1), dim3(64), 0, GD_S, rec, max_norm, skip_nonfinite);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_adamw_guarded(float* p, const float* g, float* m, float* v, float* ema, long n, const double* rec, float lr,
                                float beta1, float beta2, float eps, float weight_decay, float grad_scale, float ema_decay,
                                void* stream) {
    GD_CHECK_ARG(p && g && m && v && rec, "gd_adamw_guarded: null pointer");
    GD_CHECK_ARG(n > 0, "gd_adamw_guarded: n <= 0");
    GD_CHECK_ARG(gd_aligned(p, 4) && gd_aligned(g, 4) && gd_aligned(m, 4) && gd_aligned(v, 4) &&
                     gd_aligned(ema, 4) && gd_aligned(rec, 8), "gd_adamw_guarded: pointer not element aligned");
    GD_CHECK_ARG(!ema || (ema_decay >= 0.f && ema_decay <= 1.f), "gd_adamw_guarded: ema_decay outside [0, 1]");
    long head = gd_head_of(p), nv = 0;
    const bool same = head == gd_head_of(g) && head == gd_head_of(m) && head == gd_head_of(v) && (!ema || head == gd_head_of(ema));
    if (same && head <= n) nv = (n - head) / 4;
    else head = 0;
    long grid = (nv + (n - nv * 4) + GG_THREADS - 1) / GG_THREADS;   // one vector or one scalar element per thread ...
    grid = grid > 8192 ? 8192 : grid;                                // ... up to 8192 blocks, a grid-stride loop beyond
    if (ema)
        hipLaunchKernelGGL(adamw_guarded_kernel<true>, dim3((unsigned)grid), dim3(GG_THREADS), 0, GD_S, p, g, m, v, ema, n, head,
                           nv, rec, lr, beta1, beta2, eps, weight_decay, grad_scale, ema_decay);
    else
        hipLaunchKernelGGL(adamw_guarded_kernel<false>, dim3((unsigned)grid), dim3(GG_THREADS), 0, GD_S, p, g, m, v, ema, n, head,
                           nv, rec, lr, beta1, beta2, eps, weight_decay, grad_scale, ema_decay);
    GD_LAUNCH_CHECK();
    return 0;
}
