// Bias correction (include/gandanet.h, "Bias correction"): the quantile nodes of every (calendar slot, pixel) sample of a
// (T, M) cube, and the per-element table search that maps a cube through two such tables (empirical quantile mapping and
// quantile delta mapping).  The per-sample arithmetic is quantmap_core.h, shared with the host twins.
//
// gd_qm_quantiles, register route (no slot has more than GD_QM_SMALL_N baseline steps: 181 months / 12 gives 16): one
// thread per (slot, pixel), lanes along the pixels, so every step is one coalesced row read.  The sample goes into 16 or
// 32 int64 keys in registers (every index static), a bitonic network sorts them, and each node picks its two neighbours
// with a select chain.  No LDS, no scratch, no atomics.
// LDS route (up to GD_QM_MAX_N steps per slot): one wave (a 64-thread workgroup) per (slot, pixel); the keys go to LDS
// padded to a power of two, a bitonic sort runs there, and the lanes emit the nodes.  No atomics.
// Both routes sort the same keys, so the nodes do not depend on the route.
// gd_qm_apply: one thread per element; the tables are (period, Q, H, W), so neighbouring lanes read neighbouring words of
// one node plane at every step of the binary search.
// From elem_util.h: gd_dtype_ok, gd_elem_aligned, gd_aligned, gd_with_dtype, gd_for_items, GD_S.
#include <vector>

#include "elem_util.h"
#include "quantmap_core.h"

namespace {

constexpr int QM_THREADS = 256;

struct QmArgs {
    long M, b0, b1, sj, ss;   // sj, ss: the strides of the node and slot axes of `quant`
    const double* q;
    const unsigned char* mask;
    double* quant;
    int* n;
    int Q, period, phase, min_samples;
};

// ---- register route ---------------------------------------------------------------------------------------------------------
template <typename T, int CAP> struct QuantSmallBody {
    const T* x;
    const T* x2;
    QmArgs a;
    __host__ __device__ void operator()(long i) const {
        const int s = (int)(i / a.M);
        const long m = i - (long)s * a.M;
        const bool live = !a.mask || a.mask[m] != 0;
        int64_t key[CAP];
        int n = 0;
        const long t0 = gd_qm_first(a.b0, s, a.period, a.phase);
#pragma unroll
        for (int k = 0; k < CAP; ++k) {
            const long t = t0 + (long)k * a.period;
            bool ok = live && t < a.b1;
            double v = 0.0;
            if (ok) {
                v = (double)x[t * a.M + m];
                ok = v == v;
                if (x2) {
                    const double w = (double)x2[t * a.M + m];
                    ok = ok && w == w;
                }
            }
            key[k] = ok ? gd_qm_key(v) : GD_QM_PAD;
            n += ok;
        }
        gd_qm_sort_regs<CAP>(key);
        double v[CAP];
#pragma unroll
        for (int k = 0; k < CAP; ++k) v[k] = gd_qm_unkey(key[k]);
        a.n[(long)s * a.M + m] = n;
        double* out = a.quant + (long)s * a.ss + m;
        const bool has = n >= (a.min_samples > 1 ? a.min_samples : 1);
        for (int j = 0; j < a.Q; ++j) {
            double r = (double)NAN;
            if (has) {
                int prev, next;
                double g;
                gd_qm_node_index(n, a.q[j], prev, next, g);
                double lo = v[0], hi = v[0];
#pragma unroll
                for (int k = 1; k < CAP; ++k) {
                    lo = k == prev ? v[k] : lo;
                    hi = k == next ? v[k] : hi;
                }
                r = gd_qm_lerp(lo, hi, g);
            }
            out[(long)j * a.sj] = r;
        }
    }
};

// ---- LDS route ----------------------------------------------------------------------------------------------------------------
// one 64-thread workgroup per (slot, pixel); P: the power of two >= 64 that holds the longest slot; dynamic LDS: P keys
template <typename T>
__global__ __launch_bounds__(64) void qm_quant_long_kernel(const T* __restrict__ x, const T* __restrict__ x2, QmArgs a, int P) {
    extern __shared__ int64_t qm_keys[];
    const int lane = threadIdx.x;
    const long i = blockIdx.x;
    const int s = (int)(i / a.M);
    const long m = i - (long)s * a.M;
    const bool live = !a.mask || a.mask[m] != 0;
    const long t0 = gd_qm_first(a.b0, s, a.period, a.phase);
    int cnt = 0;
    for (int k = lane; k < P; k += 64) {
        const long t = t0 + (long)k * a.period;
        bool ok = live && t < a.b1;
        double v = 0.0;
        if (ok) {
            v = (double)x[t * a.M + m];
            ok = v == v;
            if (x2) {
                const double w = (double)x2[t * a.M + m];
                ok = ok && w == w;
            }
        }
        qm_keys[k] = ok ? gd_qm_key(v) : GD_QM_PAD;
        cnt += ok;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = lane; idx < (P >> 1); idx += 64) {
                int lo, hi;
                bool up;
                gd_qm_bitonic_pair(idx, k, j, lo, hi, up);
                const int64_t ka = qm_keys[lo], kb = qm_keys[hi];
                if (up ? kb < ka : ka < kb) {
                    qm_keys[lo] = kb;
                    qm_keys[hi] = ka;
                }
            }
            __syncthreads();
        }
    }
    const int n = cnt;
    if (lane == 0) a.n[(long)s * a.M + m] = n;
    double* out = a.quant + (long)s * a.ss + m;
    const bool has = n >= (a.min_samples > 1 ? a.min_samples : 1);
    for (int j = lane; j < a.Q; j += 64) {
        double r = (double)NAN;
        if (has) {
            int prev, next;
            double g;
            gd_qm_node_index(n, a.q[j], prev, next, g);
            r = gd_qm_lerp(gd_qm_unkey(qm_keys[prev]), gd_qm_unkey(qm_keys[next]), g);
        }
        out[(long)j * a.sj] = r;
    }
}

// the same schedule on the calling thread
template <typename T> void quant_long_host(const T* x, const T* x2, const QmArgs& a, int P) {
    std::vector<int64_t> keys((size_t)P);
    for (long i = 0; i < (long)a.period * a.M; ++i) {
        const int s = (int)(i / a.M);
        const long m = i - (long)s * a.M;
        const bool live = !a.mask || a.mask[m] != 0;
        const long t0 = gd_qm_first(a.b0, s, a.period, a.phase);
        int n = 0;
        for (int k = 0; k < P; ++k) {
            const long t = t0 + (long)k * a.period;
            bool ok = live && t < a.b1;
            double v = 0.0;
            if (ok) {
                v = (double)x[t * a.M + m];
                ok = v == v;
                if (x2) {
                    const double w = (double)x2[t * a.M + m];
                    ok = ok && w == w;
                }
            }
            keys[k] = ok ? gd_qm_key(v) : GD_QM_PAD;
            n += ok;
        }
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int idx = 0; idx < (P >> 1); ++idx) {
                    int lo, hi;
                    bool up;
                    gd_qm_bitonic_pair(idx, k, j, lo, hi, up);
                    const int64_t ka = keys[lo], kb = keys[hi];
                    if (up ? kb < ka : ka < kb) {
                        keys[lo] = kb;
                        keys[hi] = ka;
                    }
                }
            }
        }
        a.n[(long)s * a.M + m] = n;
        double* out = a.quant + (long)s * a.ss + m;
        const bool has = n >= (a.min_samples > 1 ? a.min_samples : 1);
        for (int j = 0; j < a.Q; ++j) {
            double r = (double)NAN;
            if (has) {
                int prev, next;
                double g;
                gd_qm_node_index(n, a.q[j], prev, next, g);
                r = gd_qm_lerp(gd_qm_unkey(keys[prev]), gd_qm_unkey(keys[next]), g);
            }
            out[(long)j * a.sj] = r;
        }
    }
}

// the longest slot of the baseline, and the route it takes
inline long qm_slot_steps(long b0, long b1, int period) { return (b1 - b0 + period - 1) / period; }

void quantiles_run(bool host, hipStream_t st, const void* x, const void* x2, int dtype, long M, const double* q, int Q, int period,
                   int phase, long b0, long b1, const unsigned char* mask, int min_samples, int layout, int route, double* quant, int* n) {
    QmArgs a;
    a.M = M, a.b0 = b0, a.b1 = b1;
    a.sj = layout == GD_QM_LAYOUT_QSM ? (long)period * M : M;
    a.ss = layout == GD_QM_LAYOUT_QSM ? M : (long)Q * M;
    a.q = q, a.mask = mask, a.quant = quant, a.n = n;
    a.Q = Q, a.period = period, a.phase = phase, a.min_samples = min_samples;
    const long steps = qm_slot_steps(b0, b1, period), items = (long)period * M;
    const bool small = route == GD_QM_ROUTE_SMALL || (route == GD_QM_ROUTE_AUTO && steps <= GD_QM_SMALL_N);
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        const T* xa = (const T*)x;
        const T* xb = (const T*)x2;
        if (small) {
            if (steps <= 16) gd_for_items<QM_THREADS>(host, items, st, QuantSmallBody<T, 16>{xa, xb, a});
            else gd_for_items<QM_THREADS>(host, items, st, QuantSmallBody<T, 32>{xa, xb, a});
            return;
        }
        int P = 64;
        while (P < steps) P <<= 1;
        if (host) {
            quant_long_host<T>(xa, xb, a, P);
            return;
        }
        hipLaunchKernelGGL(qm_quant_long_kernel<T>, dim3((unsigned)items), dim3(64), (size_t)P * sizeof(int64_t), st, xa, xb, a, P);
    });
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------
template <typename T> struct ApplyBody {
    const T* x;
    T* out;
    const double* model_q;
    const double* obs_q;
    const double* own_q;
    const double* p;
    long Hx, Wx, W, Mtab;   // the grid of x, the width and the pixels of the table grid
    int f, Q, period, phase, kind, extrapolate;
    __host__ __device__ void operator()(long i) const {
        const long mx = Hx * Wx, t = i / mx, pix = i - t * mx, h = pix / Wx, w = pix - h * Wx;
        const int s = (int)((t + phase) % period);
        const long parent = (h / f) * W + w / f, base = (long)s * Q * Mtab + parent;
        const GdQmCol mq{model_q + base, Mtab}, oq{obs_q + base, Mtab};
        const GdQmCol own{kind == GD_QM_QDM ? own_q + (long)s * Q * mx + pix : own_q, mx};
        out[i] = (T)gd_qm_apply_one((double)x[i], Q, mq, oq, own, p, kind, extrapolate);
    }
};

void apply_run(bool host, hipStream_t st, const void* x, int dtype, long Tn, long H, long W, int f, const double* model_q, const double* obs_q,
               const double* own_q, const double* p, int Q, int period, int phase, int kind, int extrapolate, void* out) {
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        const long Hx = H * f, Wx = W * f;
        gd_for_items<QM_THREADS>(host, Tn * Hx * Wx, st,
                                 ApplyBody<T>{(const T*)x, (T*)out, model_q, obs_q, own_q, p, Hx, Wx, W, H * W, f, Q, period, phase, kind, extrapolate});
    });
}

}  // namespace

// the checks an entry shares with its host twin
#define QM_QUANT_CHECKS(fn)                                                                                                  \
    GD_CHECK_ARG(x && q && quant && n, fn ": null pointer");                                                                 \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                          \
    GD_CHECK_ARG(T > 0 && T <= GD_QM_MAX_T, fn ": T outside 1..GD_QM_MAX_T");                                                \
    GD_CHECK_ARG(M > 0, fn ": M <= 0");                                                                                      \
    GD_CHECK_ARG(Q >= 1 && Q <= GD_QM_MAX_Q, fn ": Q outside 1..GD_QM_MAX_Q");                                               \
    GD_CHECK_ARG(period >= 1 && period <= GD_QM_MAX_PERIOD, fn ": period outside 1..GD_QM_MAX_PERIOD");                      \
    GD_CHECK_ARG(phase >= 0 && phase < period, fn ": phase outside 0..period - 1");                                          \
    GD_CHECK_ARG((long)period * M < (1L << 31), fn ": too many (slot, series) samples");                                     \
    GD_CHECK_ARG(b0 >= 0 && b0 < b1 && b1 <= T, fn ": the baseline [b0, b1) is empty, reversed or outside [0, T]");          \
    GD_CHECK_ARG(qm_slot_steps(b0, b1, period) <= GD_QM_MAX_N, fn ": more than GD_QM_MAX_N baseline steps per slot");        \
    GD_CHECK_ARG(min_samples >= 0, fn ": min_samples < 0");                                                                  \
    GD_CHECK_ARG(layout == GD_QM_LAYOUT_QSM || layout == GD_QM_LAYOUT_SQM, fn ": unknown layout");                           \
    GD_CHECK_ARG(route >= GD_QM_ROUTE_AUTO && route <= GD_QM_ROUTE_LONG, fn ": unknown route");                              \
    GD_CHECK_ARG(route != GD_QM_ROUTE_SMALL || qm_slot_steps(b0, b1, period) <= GD_QM_SMALL_N,                               \
                 fn ": the register route takes at most GD_QM_SMALL_N baseline steps per slot");                            \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_elem_aligned(x2, dtype) && gd_aligned(q, 8) && gd_aligned(quant, 8) && gd_aligned(n, 4), \
                 fn ": pointer not element aligned")

extern "C" int gd_qm_quantiles(const void* x, const void* x2, int dtype, long T, long M, const double* q, int Q, int period, int phase,
                               long b0, long b1, const unsigned char* mask, int min_samples, int layout, int route, double* quant, int* n,
                               void* stream) {
    QM_QUANT_CHECKS("gd_qm_quantiles");
    quantiles_run(false, GD_S, x, x2, dtype, M, q, Q, period, phase, b0, b1, mask, min_samples, layout, route, quant, n);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_qm_quantiles_host(const void* x, const void* x2, int dtype, long T, long M, const double* q, int Q, int period, int phase,
                                    long b0, long b1, const unsigned char* mask, int min_samples, int layout, int route, double* quant,
                                    int* n) {
    QM_QUANT_CHECKS("gd_qm_quantiles_host");
    for (int j = 0; j < Q; ++j) GD_CHECK_ARG(q[j] >= 0.0 && q[j] <= 1.0, "gd_qm_quantiles_host: a probability is NaN or outside [0, 1]");
    quantiles_run(true, nullptr, x, x2, dtype, M, q, Q, period, phase, b0, b1, mask, min_samples, layout, route, quant, n);
    return 0;
}

#define QM_APPLY_CHECKS(fn)                                                                                                  \
    GD_CHECK_ARG(x && model_q && obs_q && out, fn ": null pointer");                                                         \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                          \
    GD_CHECK_ARG(T > 0 && H > 0 && W > 0, fn ": empty cube");                                                                \
    GD_CHECK_ARG(f >= 1 && f <= GD_QM_MAX_F, fn ": f outside 1..GD_QM_MAX_F");                                               \
    GD_CHECK_ARG(Q >= 2 && Q <= GD_QM_MAX_Q, fn ": Q outside 2..GD_QM_MAX_Q");                                               \
    GD_CHECK_ARG(period >= 1 && period <= GD_QM_MAX_PERIOD, fn ": period outside 1..GD_QM_MAX_PERIOD");                      \
    GD_CHECK_ARG(phase >= 0 && phase < period, fn ": phase outside 0..period - 1");                                          \
    GD_CHECK_ARG(H * W < (1L << 31) / (f * f) && T < (1L << 53) / (H * W * f * f), fn ": too many elements");                \
    GD_CHECK_ARG(kind == GD_QM_EQM || kind == GD_QM_QDM, fn ": kind is neither eqm nor qdm");                                \
    GD_CHECK_ARG(extrapolate == GD_QM_CONSTANT || extrapolate == GD_QM_CLIP, fn ": extrapolate is neither constant nor clip"); \
    GD_CHECK_ARG(kind != GD_QM_QDM || (own_q && p), fn ": qdm needs own_q and p");                                           \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_elem_aligned(out, dtype) && gd_aligned(model_q, 8) && gd_aligned(obs_q, 8) && \
                     gd_aligned(own_q, 8) && gd_aligned(p, 8),                                                               \
                 fn ": pointer not element aligned")

extern "C" int gd_qm_apply(const void* x, int dtype, long T, long H, long W, int f, const double* model_q, const double* obs_q,
                           const double* own_q, const double* p, int Q, int period, int phase, int kind, int extrapolate, void* out,
                           void* stream) {
    QM_APPLY_CHECKS("gd_qm_apply");
    apply_run(false, GD_S, x, dtype, T, H, W, f, model_q, obs_q, own_q, p, Q, period, phase, kind, extrapolate, out);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_qm_apply_host(const void* x, int dtype, long T, long H, long W, int f, const double* model_q, const double* obs_q,
                                const double* own_q, const double* p, int Q, int period, int phase, int kind, int extrapolate, void* out) {
    QM_APPLY_CHECKS("gd_qm_apply_host");
    apply_run(true, nullptr, x, dtype, T, H, W, f, model_q, obs_q, own_q, p, Q, period, phase, kind, extrapolate, out);
    return 0;
}
