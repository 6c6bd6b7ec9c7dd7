// Singular spectrum analysis (include/gandanet.h, "Singular spectrum analysis"): the lag covariance, its eigen-decomposition
// by cyclic Jacobi, the reconstructed components and the iterative gap filling of Kondrashov & Ghil (2006), for every series
// of a (T, P) cube.  The per-element arithmetic is ssa_core.h.
//
// One wave owns one series (a workgroup is one wave).  The centred series y, the partial reconstruction R, one principal
// component, the covariance A and the eigenvector matrix V sit in dynamic LDS sized by the actual T and M (ssa_lds_bytes).
// The whole algorithm of a series is ONE function, ssa_series, written over "lane loops" (for i = lane; i < n; i += stride):
// the device runs it with 64 lanes and a barrier where a phase ends, the host twin with one lane and no barrier.  Every item
// of a lane loop writes only what it owns and reads only what earlier phases left, and the two reductions (did any pair
// rotate; the largest change) do not depend on an order, so both give the same bits.
//   covariance   a lane owns the entries (i, j), i <= j, and writes the mirror;
//   Jacobi       a set of the round robin is M / 2 disjoint pairs: lanes own the pairs for the rotation parameters (from the
//                matrix as the set found it), then the 2 x 2 blocks of two pairs (column rotation, then row rotation, the
//                mirror block copied) and the rows of V; two barriers per set;
//   components   lanes own the K entries of a principal component, then the time steps of its diagonal average.
// No atomics, no cross-wave waiting; every loop is bounded by T, M, GD_SSA_MAX_SWEEPS, rank and max_iter, which both entry
// points validate.  The pixels are walked GD_SSA_CHUNK series per launch.
#include <vector>

#include "elem_util.h"
#include "ssa_core.h"

namespace {

constexpr int SSA_LANES = 64;

struct SsaArgs {
    int T, M, rank, method, fill, max_iter, min_valid;
    double tol;
};

// the lanes of one series: 64 on the device, one on the host
template <bool DEV> struct SsaLanes {
    int lane, stride;
    __host__ __device__ inline void sync() const {
#if defined(__HIP_DEVICE_COMPILE__)
        if (DEV) __syncthreads();
#endif
    }
    __host__ __device__ inline bool any(bool v) const {
#if defined(__HIP_DEVICE_COMPILE__)
        if (DEV) return __any(v ? 1 : 0) != 0;
#endif
        return v;
    }
    __host__ __device__ inline double max(double v) const {
#if defined(__HIP_DEVICE_COMPILE__)
        if (DEV) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double u = __shfl_xor(v, o, 64);
                v = u > v ? u : v;
            }
        }
#endif
        return v;
    }
};

// ---- the LDS (host: heap) of one series ---------------------------------------------------------------------------------------
struct SsaMem {
    double *y, *R, *pc, *A, *V, *lam, *sgn;
    GdSsaRot* rot;
    int *perm, *pp, *qq;
    unsigned char* gap;
};
static inline size_t ssa_lds_bytes(long T, long M) {
    const long K = T - M + 1, nh = (M + 1) / 2;
    return sizeof(double) * (size_t)(2 * T + K + 2 * M * M + 2 * M) + sizeof(GdSsaRot) * (size_t)nh + sizeof(int) * (size_t)(M + 2 * nh) + (size_t)T;
}
__host__ __device__ inline SsaMem ssa_carve(void* base, int T, int M) {
    const int K = T - M + 1, nh = (M + 1) / 2;
    SsaMem s;
    s.y = reinterpret_cast<double*>(base);
    s.R = s.y + T;
    s.pc = s.R + T;
    s.A = s.pc + K;
    s.V = s.A + M * M;
    s.lam = s.V + M * M;
    s.sgn = s.lam + M;
    s.rot = reinterpret_cast<GdSsaRot*>(s.sgn + M);
    s.perm = reinterpret_cast<int*>(s.rot + nh);
    s.pp = s.perm + M;
    s.qq = s.pp + nh;
    s.gap = reinterpret_cast<unsigned char*>(s.qq + nh);
    return s;
}

// item e of the n (n + 1) / 2 pairs i <= j < n, folded so that no item is idle: row r and row n - 1 - r share n + 1 columns
__host__ __device__ inline bool ssa_upper(int e, int n, int* i, int* j) {
    const int r = e / (n + 1), c = e % (n + 1);
    if (c < n - r) {
        *i = r;
        *j = r + c;
        return true;
    }
    if (n - 1 - r == r) return false;   // the middle row of an odd n has no partner
    *i = n - 1 - r;
    *j = *i + (c - (n - r));
    return true;
}
__host__ __device__ inline int ssa_upper_items(int n) { return ((n + 1) / 2) * (n + 1); }

// ---- C of the current series into A, V = I ------------------------------------------------------------------------------------
template <bool DEV> __host__ __device__ inline void ssa_covariance(const SsaLanes<DEV>& L, const SsaMem& s, int T, int M, int method) {
    const int K = T - M + 1;
    if (method == GD_SSA_BK) {
        for (int e = L.lane; e < ssa_upper_items(M); e += L.stride) {
            int i, j;
            if (!ssa_upper(e, M, &i, &j)) continue;
            double c = 0.0;
            for (int k = 0; k < K; ++k) c = gd_ssa_mac(c, s.y[k + i], s.y[k + j]);
            c = c / (double)K;
            s.A[i * M + j] = c;
            s.A[j * M + i] = c;
        }
    } else {
        for (int l = L.lane; l < M; l += L.stride) {   // c(l) into the component buffer (K >= M)
            double c = 0.0;
            for (int t = 0; t < T - l; ++t) c = gd_ssa_mac(c, s.y[t], s.y[t + l]);
            s.pc[l] = c / (double)(T - l);
        }
        L.sync();
        for (int e = L.lane; e < M * M; e += L.stride) {
            const int i = e / M, j = e % M;
            s.A[e] = s.pc[i > j ? i - j : j - i];
        }
    }
    for (int e = L.lane; e < M * M; e += L.stride) s.V[e] = (e / M == e % M) ? 1.0 : 0.0;
    L.sync();
}

// ---- cyclic Jacobi on A (V accumulates the rotations), then the order and signs of the eigenpairs -------------------------------
// returns the sweeps run; *capped: the last of GD_SSA_MAX_SWEEPS sweeps still rotated
template <bool DEV> __host__ __device__ inline int ssa_jacobi(const SsaLanes<DEV>& L, const SsaMem& s, int M, bool* capped, double* trace) {
    const int nh = (M + 1) / 2, sets = 2 * nh - 1;
    double dmax = 0.0;
    for (int i = 0; i < M; ++i) {
        const double d = fabs(s.A[i * M + i]);
        dmax = d > dmax ? d : dmax;
    }
    const double thr = GD_SSA_JTOL * dmax;
    int sweeps = 0;
    bool rotated = true;
    while (sweeps < GD_SSA_MAX_SWEEPS && rotated) {
        bool mine = false;
        for (int set = 0; set < sets; ++set) {
            for (int a = L.lane; a < nh; a += L.stride) {
                int p, q;
                gd_ssa_pair(M, set, a, &p, &q);
                s.pp[a] = p;
                s.qq[a] = q;
                s.rot[a] = q < 0 ? gd_ssa_rotation(0.0, 0.0, 0.0, 0.0) : gd_ssa_rotation(s.A[p * M + p], s.A[q * M + q], s.A[p * M + q], thr);
                mine = mine || s.rot[a].rotated;
            }
            L.sync();
            for (int e = L.lane; e < ssa_upper_items(nh); e += L.stride) {
                int a, b;
                if (!ssa_upper(e, nh, &a, &b)) continue;
                gd_ssa_block(s.A, M, a == b, s.pp[a], s.qq[a], s.rot[a], s.pp[b], s.qq[b], s.rot[b]);
            }
            for (int e = L.lane; e < nh * M; e += L.stride) {
                const int a = e / M;
                gd_ssa_vrow(s.V, M, e % M, s.pp[a], s.qq[a], s.rot[a]);
            }
            L.sync();
        }
        ++sweeps;
        rotated = L.any(mine);
    }
    *capped = rotated;
    // a diagonal that overflowed to NaN ranks every index 0: perm starts as the identity so that it always holds indices;
    // such a series has a trace that is not finite, and the caller flags it
    for (int i = L.lane; i < M; i += L.stride) {
        s.perm[i] = i;
        s.lam[i] = (double)NAN;
    }
    L.sync();
    for (int i = L.lane; i < M; i += L.stride) {
        const int r = gd_ssa_rank(s.A, M, i);
        s.perm[r] = i;
        s.lam[r] = s.A[i * M + i];
    }
    L.sync();
    for (int k = L.lane; k < M; k += L.stride) s.sgn[k] = gd_ssa_sign(s.V, M, s.perm[k]);
    L.sync();
    double tr = 0.0;
    for (int k = 0; k < M; ++k) tr += s.lam[k];
    *trace = tr;
    return sweeps;
}

// entry j of eigenvector k (sorted, signed)
__host__ __device__ inline double ssa_e(const SsaMem& s, int M, int j, int k) { return s.sgn[k] * s.V[j * M + s.perm[k]]; }

// the principal component k of the current series into s.pc
template <bool DEV> __host__ __device__ inline void ssa_pc(const SsaLanes<DEV>& L, const SsaMem& s, int T, int M, int k) {
    const int K = T - M + 1;
    for (int i = L.lane; i < K; i += L.stride) {
        double a = 0.0;
        for (int j = 0; j < M; ++j) a = gd_ssa_mac(a, s.y[i + j], ssa_e(s, M, j, k));
        s.pc[i] = a;
    }
    L.sync();
}
// RC_k[t] from s.pc
__host__ __device__ inline double ssa_rc(const SsaMem& s, int T, int M, int k, int t) {
    int j0, j1;
    gd_ssa_diag_range(t, M, T - M + 1, &j0, &j1);
    double a = 0.0;
    for (int j = j0; j <= j1; ++j) a = gd_ssa_mac(a, s.pc[t - j], ssa_e(s, M, j, k));
    return gd_ssa_diag_mean(a, j1 - j0 + 1);
}

// ---- one series ---------------------------------------------------------------------------------------------------------------
template <bool DEV, typename Tx>
__host__ __device__ inline void ssa_series(const SsaLanes<DEV>& L, const Tx* __restrict__ x, long P, long m, bool masked, const SsaArgs& a,
                                           void* mem, double* __restrict__ eig, double* __restrict__ maps, double* __restrict__ rc,
                                           double* __restrict__ evec, double* __restrict__ filled) {
#pragma clang fp contract(off)
    const int T = a.T, M = a.M;
    const double nan = (double)NAN;
    const SsaMem s = ssa_carve(mem, T, M);
    int n = 0, flags = 0;
    double mean = nan, sd = nan;
    if (masked) {
        flags = GD_SSA_FLAG_MASKED;
    } else {
        for (int t = L.lane; t < T; t += L.stride) s.y[t] = (double)x[(long)t * P + m];
        L.sync();
        // every lane walks the series itself: the sums are sequential in time by definition
        double sum = 0.0;
        bool inf = false;
        for (int t = 0; t < T; ++t) {
            const double v = s.y[t];
            if (v == v) {
                ++n;
                sum += v;
                inf = inf || gd_ssa_is_inf(v);
            }
        }
        if (inf) {
            flags |= GD_SSA_FLAG_NONFINITE;
        } else if (n >= 1) {
            mean = sum / (double)n;
            double ss = 0.0;
            for (int t = 0; t < T; ++t) {
                const double v = s.y[t];
                if (v == v) ss = gd_ssa_sq_dev(ss, v, mean);
            }
            sd = gd_ssa_sd(ss, n);
            if (!(sd > 0.0)) flags |= GD_SSA_FLAG_CONSTANT;
        }
        if (a.fill ? n < a.min_valid : n < T) flags |= a.fill ? GD_SSA_FLAG_FEW : GD_SSA_FLAG_GAPS;
    }
    const int n_gaps = masked ? 0 : T - n;
    double trace = nan, last_change = nan, sweeps = nan, iterations = nan;
    if (flags == 0) {
        L.sync();
        for (int t = L.lane; t < T; t += L.stride) {
            const double v = s.y[t];
            const bool g = !(v == v);
            s.gap[t] = g ? 1 : 0;
            s.y[t] = g ? 0.0 : v - mean;
        }
        L.sync();
        bool capped = false;
        if (!a.fill || n_gaps == 0) {
            ssa_covariance(L, s, T, M, a.method);
            sweeps = (double)ssa_jacobi(L, s, M, &capped, &trace);
            if (capped) flags |= GD_SSA_FLAG_SWEEPS;
            if (!(trace - trace == 0.0)) flags |= GD_SSA_FLAG_NONFINITE;   // the squares overflowed: the same verdict in every lane
            iterations = 0.0;
            last_change = 0.0;
            if (evec && !(flags & GD_SSA_FLAG_NONFINITE)) {
                for (int e = L.lane; e < a.rank * M; e += L.stride) evec[(long)e * P + m] = ssa_e(s, M, e % M, e / M);
            }
            if (rc && !(flags & GD_SSA_FLAG_NONFINITE)) {
                for (int k = 0; k < a.rank; ++k) {
                    ssa_pc(L, s, T, M, k);
                    for (int t = L.lane; t < T; t += L.stride) rc[((long)k * T + t) * P + m] = ssa_rc(s, T, M, k, t);
                    L.sync();
                }
            }
        } else {
            int iters = 0;
            for (int q = 1; q <= a.rank && !(flags & GD_SSA_FLAG_NONFINITE); ++q) {
                bool done = false;
                for (int it = 0; it < a.max_iter && !done; ++it) {
                    ssa_covariance(L, s, T, M, a.method);
                    sweeps = (double)ssa_jacobi(L, s, M, &capped, &trace);
                    if (capped) flags |= GD_SSA_FLAG_SWEEPS;
                    if (!(trace - trace == 0.0)) {   // the squares overflowed: the same verdict in every lane
                        flags |= GD_SSA_FLAG_NONFINITE;
                        break;
                    }
                    for (int t = L.lane; t < T; t += L.stride) s.R[t] = 0.0;   // a lane keeps its steps through all k
                    for (int k = 0; k < q; ++k) {
                        ssa_pc(L, s, T, M, k);
                        for (int t = L.lane; t < T; t += L.stride)
                            if (s.gap[t]) s.R[t] = s.R[t] + ssa_rc(s, T, M, k, t);
                        L.sync();
                    }
                    double change = 0.0;
                    for (int t = L.lane; t < T; t += L.stride) {
                        if (!s.gap[t]) continue;
                        change = gd_ssa_change(change, s.R[t], s.y[t]);
                        s.y[t] = s.R[t];
                    }
                    change = L.max(change);
                    L.sync();
                    ++iters;
                    last_change = change;
                    done = gd_ssa_converged(change, a.tol, sd);
                }
                if (!done && !(flags & GD_SSA_FLAG_NONFINITE)) flags |= GD_SSA_FLAG_ITER;
            }
            iterations = (double)iters;
        }
    }
    const bool bad = (flags & (GD_SSA_FLAG_MASKED | GD_SSA_FLAG_FEW | GD_SSA_FLAG_CONSTANT | GD_SSA_FLAG_NONFINITE | GD_SSA_FLAG_GAPS)) != 0;
    for (int k = L.lane; k < a.rank; k += L.stride) eig[(long)k * P + m] = bad ? nan : s.lam[k];
    if (bad && rc) {
        for (long e = L.lane; e < (long)a.rank * T; e += L.stride) rc[e * P + m] = nan;
    }
    if (bad && evec) {
        for (int e = L.lane; e < a.rank * M; e += L.stride) evec[(long)e * P + m] = nan;
    }
    if (bad) trace = sweeps = iterations = last_change = nan;
    if (filled) {
        for (int t = L.lane; t < T; t += L.stride)
            filled[(long)t * P + m] = bad ? nan : (s.gap[t] ? mean + s.y[t] : (double)x[(long)t * P + m]);
    }
    if (L.lane == 0) {
        maps[GD_SSA_N * P + m] = (double)n;
        maps[GD_SSA_N_GAPS * P + m] = (double)n_gaps;
        maps[GD_SSA_MEAN * P + m] = mean;
        maps[GD_SSA_SD * P + m] = sd;
        maps[GD_SSA_TRACE * P + m] = trace;
        maps[GD_SSA_SWEEPS * P + m] = sweeps;
        maps[GD_SSA_ITERATIONS * P + m] = iterations;
        maps[GD_SSA_LAST_CHANGE * P + m] = last_change;
        maps[GD_SSA_FLAGS * P + m] = (double)flags;
    }
}

template <typename Tx>
__global__ __launch_bounds__(SSA_LANES) void ssa_kernel(const Tx* __restrict__ x, long P, long p0, const unsigned char* __restrict__ mask,
                                                        SsaArgs a, double* __restrict__ eig, double* __restrict__ maps,
                                                        double* __restrict__ rc, double* __restrict__ evec,
                                                        double* __restrict__ filled) {
    extern __shared__ double ssa_smem[];
    const long m = p0 + blockIdx.x;
    const SsaLanes<true> L{(int)threadIdx.x, SSA_LANES};
    ssa_series<true, Tx>(L, x, P, m, mask && mask[m] == 0, a, ssa_smem, eig, maps, rc, evec, filled);
}

template <typename Tx>
static int ssa_launch(const Tx* x, long P, const unsigned char* mask, const SsaArgs& a, double* eig, double* maps, double* rc, double* evec,
                      double* filled, hipStream_t st) {
    const size_t bytes = ssa_lds_bytes(a.T, a.M);
    if (bytes > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ssa_kernel<Tx>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)bytes);
        if (e != hipSuccess) {
            gd_set_error(hipGetErrorString(e));
            return -2;
        }
    }
    for (long p0 = 0; p0 < P; p0 += GD_SSA_CHUNK) {
        const long np = P - p0 < GD_SSA_CHUNK ? P - p0 : GD_SSA_CHUNK;
        hipLaunchKernelGGL((ssa_kernel<Tx>), dim3((unsigned)np), dim3(SSA_LANES), bytes, st, x, P, p0, mask, a, eig, maps, rc, evec,
                           filled);
    }
    return 0;
}

template <typename Tx>
static void ssa_host(const Tx* x, long P, const unsigned char* mask, const SsaArgs& a, double* eig, double* maps, double* rc, double* evec,
                     double* filled) {
    std::vector<double> mem(ssa_lds_bytes(a.T, a.M) / sizeof(double) + 1);
    const SsaLanes<false> L{0, 1};
    for (long m = 0; m < P; ++m) ssa_series<false, Tx>(L, x, P, m, mask && mask[m] == 0, a, mem.data(), eig, maps, rc, evec, filled);
}

}  // namespace

// the checks an entry shares with its host twin
#define SSA_CHECKS(fn)                                                                                                              \
    GD_CHECK_ARG(x && eig && maps, fn ": null pointer");                                                                          \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                                                                \
    GD_CHECK_ARG(window >= 2 && window <= GD_SSA_MAX_M, fn ": window outside 2..GD_SSA_MAX_M");                                    \
    GD_CHECK_ARG(T >= 2L * window - 1 && T <= GD_SSA_MAX_T, fn ": T outside 2 window - 1..GD_SSA_MAX_T");                          \
    GD_CHECK_ARG(M_pixels > 0 && M_pixels < (1L << 31), fn ": M_pixels <= 0 or too many series");                                 \
    GD_CHECK_ARG(rank >= 1 && rank <= window && rank <= GD_SSA_MAX_RANK, fn ": rank outside 1..min(window, GD_SSA_MAX_RANK)");      \
    GD_CHECK_ARG(method == GD_SSA_BK || method == GD_SSA_VG, fn ": unknown method");                                              \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(eig, 8) && gd_aligned(maps, 8), fn ": pointer not element aligned")
#define SSA_FILL_CHECKS(fn)                                                                                                         \
    GD_CHECK_ARG(filled, fn ": null pointer");                                                                                    \
    GD_CHECK_ARG(gd_aligned(filled, 8), fn ": pointer not element aligned");                                                      \
    GD_CHECK_ARG(tol - tol == 0.0 && tol > 0.0, fn ": tol is not finite and > 0");                                                \
    GD_CHECK_ARG(max_iter >= 1 && max_iter <= GD_SSA_MAX_ITER, fn ": max_iter outside 1..GD_SSA_MAX_ITER");                        \
    GD_CHECK_ARG(min_valid >= 2 && min_valid <= GD_SSA_MAX_T, fn ": min_valid outside 2..GD_SSA_MAX_T")

static SsaArgs ssa_args(long T, int window, int rank, int method, int fill, double tol, int max_iter, int min_valid) {
    SsaArgs a;
    a.T = (int)T;
    a.M = window;
    a.rank = rank;
    a.method = method;
    a.fill = fill;
    a.tol = tol;
    a.max_iter = max_iter;
    a.min_valid = min_valid;
    return a;
}

extern "C" int gd_ssa_decompose(const void* x, int dtype, long T, long M_pixels, int window, int rank, int method, const unsigned char* mask,
                                double* eig, double* maps, double* rc, double* evec, void* stream) {
    SSA_CHECKS("gd_ssa_decompose");
    GD_CHECK_ARG(gd_aligned(rc, 8) && gd_aligned(evec, 8), "gd_ssa_decompose: pointer not element aligned");
    const SsaArgs a = ssa_args(T, window, rank, method, 0, 1.0, 1, 2);
    const int r = gd_with_dtype(dtype, [&](auto zero) { return ssa_launch((const decltype(zero)*)x, M_pixels, mask, a, eig, maps, rc, evec, nullptr, GD_S); });
    if (r) return r;
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_ssa_decompose_host(const void* x, int dtype, long T, long M_pixels, int window, int rank, int method,
                                     const unsigned char* mask, double* eig, double* maps, double* rc, double* evec) {
    SSA_CHECKS("gd_ssa_decompose_host");
    GD_CHECK_ARG(gd_aligned(rc, 8) && gd_aligned(evec, 8), "gd_ssa_decompose_host: pointer not element aligned");
    const SsaArgs a = ssa_args(T, window, rank, method, 0, 1.0, 1, 2);
    gd_with_dtype(dtype, [&](auto zero) { ssa_host((const decltype(zero)*)x, M_pixels, mask, a, eig, maps, rc, evec, nullptr); });
    return 0;
}

extern "C" int gd_ssa_fill(const void* x, int dtype, long T, long M_pixels, int window, int rank, int method, const unsigned char* mask,
                           double tol, int max_iter, int min_valid, double* filled, double* eig, double* maps, void* stream) {
    SSA_CHECKS("gd_ssa_fill");
    SSA_FILL_CHECKS("gd_ssa_fill");
    const SsaArgs a = ssa_args(T, window, rank, method, 1, tol, max_iter, min_valid);
    const int r = gd_with_dtype(dtype, [&](auto zero) { return ssa_launch((const decltype(zero)*)x, M_pixels, mask, a, eig, maps, nullptr, nullptr, filled, GD_S); });
    if (r) return r;
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_ssa_fill_host(const void* x, int dtype, long T, long M_pixels, int window, int rank, int method, const unsigned char* mask,
                                double tol, int max_iter, int min_valid, double* filled, double* eig, double* maps) {
    SSA_CHECKS("gd_ssa_fill_host");
    SSA_FILL_CHECKS("gd_ssa_fill_host");
    const SsaArgs a = ssa_args(T, window, rank, method, 1, tol, max_iter, min_valid);
    gd_with_dtype(dtype, [&](auto zero) { ssa_host((const decltype(zero)*)x, M_pixels, mask, a, eig, maps, nullptr, nullptr, filled); });
    return 0;
}
