// EOF analysis (include/gandanet.h, "EOF analysis"): validity and mean of every series of a (T, M) cube, the T x T Gram
// matrix of its weighted anomalies on the fp64 matrix pipe, the projection of every series on K coefficient columns (the
// pattern maps) and the rank-K reconstruction.  The per-series arithmetic is eof_core.h, shared with the host twins.
//
// prepare, project and reconstruct are of the family of series.hip: one thread per series, t ascending, every time step one
// coalesced row read, coefficient rows at a wave-uniform address.
//
// gram: the weighted anomalies of GD_EOF_CHUNK = 32 series for all Tp = 16 nb rows are staged in LDS as fp64, row t at
// t * EOF_STRIDE doubles; padded rows, invalid series and series beyond M are zeros.  A row fragment of
// v_mfma_f64_16x16x4_f64 -- lane l holds a[16 b + (l & 15)][4 ks + (l >> 4)] -- is the A operand of block row b and the B
// operand of block column b alike, so a wave reads the fragments of the row blocks its 16 x 16 blocks touch once per k-step
// and feeds each of its blocks from two of them.  With EOF_STRIDE = 34 the 32 lanes of a ds_read_b64 group (16 rows x 2
// series) fall on 32 different bank pairs.  The nblk = nb (nb + 1) / 2 blocks on and above the diagonal, numbered row by
// row, are dealt to the 8 waves in contiguous runs of floor((w + 1) nblk / 8) - floor(w nblk / 8); the run of a wave is a
// compile-time list, so its accumulators (4 doubles per block and lane) are registers with static indices.  The next
// chunk's samples are loaded into registers ahead of the MFMAs of the current one.  A workgroup owns a contiguous run of
// chunks (gd_eof_geom) and writes its accumulators as one slab [nblk][4][64]; a second launch adds the slabs in ascending
// order and writes both triangles of G from the upper one.  No atomics; the geometry depends on (T, M) alone.
#include <type_traits>
#include <vector>

#include "elem_util.h"
#include "eof_core.h"

namespace {

constexpr int EOF_THREADS = 256;                    // prepare, project, reconstruct
constexpr int EOF_WAVES = 8;                        // gram: waves per workgroup
constexpr int EOF_GTHREADS = EOF_WAVES * 64;
constexpr int EOF_STRIDE = GD_EOF_CHUNK + 2;        // doubles per LDS row: 2 * 34 = 4 (mod 64) dwords from row to row
constexpr int EOF_KSTEPS = GD_EOF_CHUNK / 4;
static_assert(GD_EOF_MAX_T % 16 == 0 && EOF_GTHREADS / GD_EOF_CHUNK == 16, "a thread stages one row of every 16-row block");

typedef double f64x4_t __attribute__((ext_vector_type(4)));

constexpr int eof_nblk(int nb) { return nb * (nb + 1) / 2; }
constexpr int eof_lo(int nb, int w) { return w * eof_nblk(nb) / EOF_WAVES; }
constexpr int eof_per_wave(int nb) { return (eof_nblk(nb) + EOF_WAVES - 1) / EOF_WAVES; }
// bit b: a block numbered in [lo, hi) lies in block row b or block column b
constexpr unsigned eof_need(int nb, int lo, int hi) {
    unsigned m = 0;
    int idx = 0;
    for (int bi = 0; bi < nb; ++bi) {
        for (int bj = bi; bj < nb; ++bj, ++idx) {
            if (idx >= lo && idx < hi) m |= (1u << bi) | (1u << bj);
        }
    }
    return m;
}

// the MFMAs of wave W over 4 staged series; frag: the lane's element of row block 0 at this k-step
template <int NB, int W>
__device__ __forceinline__ void gram_kstep(const double* __restrict__ frag, f64x4_t (&acc)[eof_per_wave(NB)]) {
    constexpr int LO = eof_lo(NB, W), HI = eof_lo(NB, W + 1);
    constexpr unsigned NEED = eof_need(NB, LO, HI);
    double f[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) f[b] = (NEED >> b & 1) ? frag[b * 16 * EOF_STRIDE] : 0.0;
    int idx = 0;
#pragma unroll
    for (int bi = 0; bi < NB; ++bi) {
#pragma unroll
        for (int bj = bi; bj < NB; ++bj, ++idx) {
            if (idx >= LO && idx < HI) acc[idx - LO] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[bi], f[bj], acc[idx - LO], 0, 0, 0);
        }
    }
}

// ... over one staged chunk.  The k-steps are not unrolled: a wave holds one set of fragments at a time, which keeps the
// widest forms free of scratch, and the fragment reads stay single ds_read_b64 (two neighbouring k-steps would be merged
// into ds_read2_b64, which runs at half the rate and maps rows r and r + 8 to one bank at this stride).  The second wave of
// the SIMD covers the wait for the fragments.
template <int NB, int W>
__device__ __forceinline__ void gram_wave(const double* __restrict__ frag, f64x4_t (&acc)[eof_per_wave(NB)]) {
    if constexpr (eof_lo(NB, W + 1) > eof_lo(NB, W)) {
#pragma nounroll
        for (int ks = 0; ks < EOF_KSTEPS; ++ks) gram_kstep<NB, W>(frag + ks * 4, acc);
    }
}

template <typename T, int NB>
__global__ __launch_bounds__(EOF_GTHREADS) void eof_gram_kernel(const T* __restrict__ x, int Tn, long M, const double* __restrict__ mean,
                                                                const unsigned char* __restrict__ valid,
                                                                const double* __restrict__ weight, long per, long chunks,
                                                                double* __restrict__ ws) {
    constexpr int PER = eof_per_wave(NB), NBLK = eof_nblk(NB);
    __shared__ double lds[NB * 16 * EOF_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = tid & (GD_EOF_CHUNK - 1), r = tid >> 5;   // the thread stages series s of the chunk, row r of every block
    const long c0 = (long)blockIdx.x * per, c1 = c0 + per < chunks ? c0 + per : chunks;
    const double* frag = lds + (lane & 15) * EOF_STRIDE + (lane >> 4);

    f64x4_t acc[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) acc[j] = f64x4_t{0.0, 0.0, 0.0, 0.0};

    // the samples of the next chunk, as stored, and what turns them into anomalies; every address is clamped into the
    // cube, what lies outside is replaced by zero when the chunk is written
    // (only the last block has rows beyond T: 16 (nb - 1) < T)
    T v[NB];
    double mu, sw;
    bool ok;
    const int tl = 16 * (NB - 1) + r;
    const T* xr = x + (long)r * M;
    const T* xl = x + (long)(tl < Tn ? tl : Tn - 1) * M;
    auto fetch = [&](long c) {
        const long m = c * GD_EOF_CHUNK + s, mc = m < M ? m : M - 1;
        ok = m < M && valid[mc] != 0;
        mu = mean[mc];
        sw = weight ? sqrt(weight[mc]) : 1.0;
#pragma unroll
        for (int j = 0; j < NB - 1; ++j) v[j] = xr[(long)(16 * j) * M + mc];
        v[NB - 1] = xl[mc];
    };
    fetch(c0);
    for (long c = c0; c < c1; ++c) {
        __syncthreads();   // the MFMAs of the chunk before have read their fragments
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int t = 16 * j + r;
            lds[t * EOF_STRIDE + s] = gd_eof_anom((double)v[j], mu, sw, ok && t < Tn);
        }
        __syncthreads();
        if (c + 1 < c1) fetch(c + 1);
        switch (wave) {   // wave-uniform: every wave runs the list of its own blocks
            case 0: gram_wave<NB, 0>(frag, acc); break;
            case 1: gram_wave<NB, 1>(frag, acc); break;
            case 2: gram_wave<NB, 2>(frag, acc); break;
            case 3: gram_wave<NB, 3>(frag, acc); break;
            case 4: gram_wave<NB, 4>(frag, acc); break;
            case 5: gram_wave<NB, 5>(frag, acc); break;
            case 6: gram_wave<NB, 6>(frag, acc); break;
            default: gram_wave<NB, 7>(frag, acc); break;
        }
    }
    // slab [block][register][lane]
    const int lo = wave * NBLK / EOF_WAVES, cnt = (wave + 1) * NBLK / EOF_WAVES - lo;
    double* slab = ws + (long)blockIdx.x * (NBLK * 256);
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (j < cnt) {
#pragma unroll
            for (int q = 0; q < 4; ++q) slab[(lo + j) * 256 + q * 64 + lane] = acc[j][q];
        }
    }
}

// one thread per accumulator element: the slabs in ascending order, then G[row][col] and its mirror image.  C/D of the
// f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * register.  Of a diagonal block only row <= col is written.
__global__ __launch_bounds__(256) void eof_gram_reduce_kernel(const double* __restrict__ ws, int splits, int nb, int Tn,
                                                             double* __restrict__ G) {
    const int slab = nb * (nb + 1) / 2 * 256;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= slab) return;
    double v = ws[i];
    for (int sp = 1; sp < splits; ++sp) v += ws[(long)sp * slab + i];
    int bi = 0, rem = i >> 8;
    while (rem >= nb - bi) {
        rem -= nb - bi;
        ++bi;
    }
    const int bj = bi + rem, lane = i & 63, q = (i >> 6) & 3;
    const int row = 16 * bi + (lane >> 4) + 4 * q, col = 16 * bj + (lane & 15);
    if (row < Tn && col < Tn && row <= col) {
        G[(long)row * Tn + col] = v;
        G[(long)col * Tn + row] = v;
    }
}

template <typename T, int NB>
static void gram_go(const T* x, int Tn, long M, const double* mean, const unsigned char* valid, const double* weight, const GdEofGeom& g,
                    double* ws, hipStream_t st) {
    hipLaunchKernelGGL((eof_gram_kernel<T, NB>), dim3(g.splits), dim3(EOF_GTHREADS), 0, st, x, Tn, M, mean, valid, weight, g.per, g.chunks,
                       ws);
}

template <typename T>
static void gram_dispatch(const T* x, int Tn, long M, const double* mean, const unsigned char* valid, const double* weight,
                          const GdEofGeom& g, double* ws, hipStream_t st) {
    switch (g.nb) {
#define GRAM_CASE(n) case n: gram_go<T, n>(x, Tn, M, mean, valid, weight, g, ws, st); break
        GRAM_CASE(1); GRAM_CASE(2); GRAM_CASE(3); GRAM_CASE(4); GRAM_CASE(5); GRAM_CASE(6); GRAM_CASE(7); GRAM_CASE(8);
        GRAM_CASE(9); GRAM_CASE(10); GRAM_CASE(11); GRAM_CASE(12); GRAM_CASE(13); GRAM_CASE(14); GRAM_CASE(15); GRAM_CASE(16);
#undef GRAM_CASE
    }
    static_assert(GD_EOF_MAX_T == 256, "one case per nb");
}

// the host twin: every entry on and above the diagonal is the sum over m in ascending order
template <typename T>
static void gram_host(const T* x, long Tn, long M, const double* mean, const unsigned char* valid, const double* weight, double* G) {
    for (long i = 0; i < Tn * Tn; ++i) G[i] = 0.0;
    std::vector<double> a((size_t)Tn);
    for (long m = 0; m < M; ++m) {
        if (!valid[m]) continue;
        const double sw = weight ? sqrt(weight[m]) : 1.0;
        for (long t = 0; t < Tn; ++t) a[t] = gd_eof_anom((double)x[t * M + m], mean[m], sw, true);
        for (long t = 0; t < Tn; ++t) {
            for (long u = t; u < Tn; ++u) G[t * Tn + u] += a[t] * a[u];
        }
    }
    for (long t = 0; t < Tn; ++t) {
        for (long u = t + 1; u < Tn; ++u) G[u * Tn + t] = G[t * Tn + u];
    }
}

// ---- prepare -------------------------------------------------------------------------------------------------------------
// One Body per entry (gd_for_items): operator() is the per-series call of the device kernel and of the host twin alike.
// Each *_run is called by the device entry (host = false) and by its host twin (host = true, st unused).
template <typename T> struct PrepareBody {
    const T* x;
    long Tn, M;
    const unsigned char* mask;
    const double* weight;
    int center;
    double* mean;
    unsigned char* valid;
    __host__ __device__ void operator()(long m) const {
        gd_eof_prepare_one(x + m, Tn, M, !mask || mask[m] != 0, weight != nullptr, weight ? weight[m] : 1.0, center, mean + m, valid + m);
    }
};

void prepare_run(bool host, hipStream_t st, const void* x, int dtype, long Tn, long M, const unsigned char* mask, const double* weight,
                 int center, double* mean, unsigned char* valid) {
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        gd_for_items<EOF_THREADS>(host, M, st, PrepareBody<T>{(const T*)x, Tn, M, mask, weight, center, mean, valid});
    });
}

// ---- project -------------------------------------------------------------------------------------------------------------
// K accumulators in registers: f(KC) for the instance with KC = 1, 4 or 16 of them that holds K
template <class F> void with_kc(int K, F&& f) {
    if (K <= 1) f(std::integral_constant<int, 1>{});
    else if (K <= 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 16>{});
    static_assert(GD_EOF_MAX_K == 16, "the widest instance holds GD_EOF_MAX_K");
}

template <typename T, int KC> struct ProjectBody {
    const T* x;
    long Tn, M;
    const double* mean;
    const unsigned char* valid;
    const double *weight, *coef;
    int K;
    double* out;
    __host__ __device__ void operator()(long m) const {
        gd_eof_project_one<T, KC>(x + m, Tn, M, mean[m], valid[m] != 0, weight ? sqrt(weight[m]) : 1.0, coef, K, out, m);
    }
};

void project_run(bool host, hipStream_t st, const void* x, int dtype, long Tn, long M, const double* mean, const unsigned char* valid,
                 const double* weight, const double* coef, int K, double* out) {
    gd_with_dtype(dtype, [&](auto zero) {
        using T = decltype(zero);
        with_kc(K, [&](auto kc) {
            gd_for_items<EOF_THREADS>(host, M, st, ProjectBody<T, decltype(kc)::value>{(const T*)x, Tn, M, mean, valid, weight, coef, K, out});
        });
    });
}

// ---- reconstruct ---------------------------------------------------------------------------------------------------------
template <typename O, int KC> struct ReconstructBody {
    const double *eofs, *pcs, *mean;
    const unsigned char* valid;
    const double* weight;
    long Tn, M;
    int K;
    O* out;
    __host__ __device__ void operator()(long m) const {
        gd_eof_reconstruct_one<O, KC>(eofs, pcs, mean[m], valid[m] != 0, weight != nullptr, weight ? sqrt(weight[m]) : 1.0, Tn, M, K, out, m);
    }
};

void reconstruct_run(bool host, hipStream_t st, const double* eofs, const double* pcs, const double* mean, const unsigned char* valid,
                     const double* weight, long Tn, long M, int K, void* out, int out_dtype) {
    gd_with_dtype(out_dtype, [&](auto zero) {
        using O = decltype(zero);
        with_kc(K, [&](auto kc) {
            gd_for_items<EOF_THREADS>(host, M, st, ReconstructBody<O, decltype(kc)::value>{eofs, pcs, mean, valid, weight, Tn, M, K, (O*)out});
        });
    });
}

}  // namespace

// the checks an entry shares with its host twin
#define EOF_CUBE_CHECKS(fn)                                                                   \
    GD_CHECK_ARG(gd_dtype_ok(dtype), fn ": dtype outside {0, 1}");                            \
    GD_CHECK_ARG(T > 0 && M > 0, fn ": T <= 0 or M <= 0");                                     \
    GD_CHECK_ARG(M < (1L << 31) && M < (1L << 53) / T, fn ": too many series")

#define EOF_PREPARE_CHECKS(fn)                                                                             \
    GD_CHECK_ARG(x && mean && valid, fn ": null pointer");                                                \
    EOF_CUBE_CHECKS(fn);                                                                                   \
    GD_CHECK_ARG(center == 0 || center == 1, fn ": center outside {0, 1}");                                \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(weight, 8) && gd_aligned(mean, 8), fn ": pointer not element aligned")

extern "C" int gd_eof_prepare(const void* x, int dtype, long T, long M, const unsigned char* mask, const double* weight, int center,
                              double* mean, unsigned char* valid, void* stream) {
    EOF_PREPARE_CHECKS("gd_eof_prepare");
    prepare_run(false, GD_S, x, dtype, T, M, mask, weight, center, mean, valid);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_eof_prepare_host(const void* x, int dtype, long T, long M, const unsigned char* mask, const double* weight, int center,
                                   double* mean, unsigned char* valid) {
    EOF_PREPARE_CHECKS("gd_eof_prepare_host");
    prepare_run(true, nullptr, x, dtype, T, M, mask, weight, center, mean, valid);
    return 0;
}

extern "C" size_t gd_eof_gram_ws_bytes(long T, long M) {
    if (T < 2 || T > GD_EOF_MAX_T || M <= 0 || M >= (1L << 31)) return 0;
    const GdEofGeom g = gd_eof_geom(T, M);
    return (size_t)g.splits * g.nblk * 256 * sizeof(double);
}

#define EOF_GRAM_CHECKS(fn)                                                                                       \
    GD_CHECK_ARG(x && mean && valid && G, fn ": null pointer");                                                  \
    EOF_CUBE_CHECKS(fn);                                                                                          \
    GD_CHECK_ARG(T >= 2 && T <= GD_EOF_MAX_T, fn ": T outside 2..GD_EOF_MAX_T");                                  \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(weight, 8) && gd_aligned(mean, 8) && gd_aligned(G, 8),   \
                 fn ": pointer not element aligned")

extern "C" int gd_eof_gram(const void* x, int dtype, long T, long M, const double* mean, const unsigned char* valid, const double* weight,
                           double* G, void* ws, size_t ws_bytes, void* stream) {
    EOF_GRAM_CHECKS("gd_eof_gram");
    GD_CHECK_ARG(ws && gd_aligned(ws, 8) && ws_bytes >= gd_eof_gram_ws_bytes(T, M), "gd_eof_gram: workspace missing, misaligned or too small");
    const GdEofGeom g = gd_eof_geom(T, M);
    gd_with_dtype(dtype, [&](auto zero) { gram_dispatch((const decltype(zero)*)x, (int)T, M, mean, valid, weight, g, (double*)ws, GD_S); });
    GD_LAUNCH_CHECK();
    hipLaunchKernelGGL(eof_gram_reduce_kernel, dim3(gd_cdiv((long)g.nblk * 256, 256)), dim3(256), 0, GD_S, (const double*)ws, g.splits, g.nb,
                       (int)T, G);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_eof_gram_host(const void* x, int dtype, long T, long M, const double* mean, const unsigned char* valid,
                                const double* weight, double* G) {
    EOF_GRAM_CHECKS("gd_eof_gram_host");
    gd_with_dtype(dtype, [&](auto zero) { gram_host((const decltype(zero)*)x, T, M, mean, valid, weight, G); });
    return 0;
}

#define EOF_PROJECT_CHECKS(fn)                                                                                          \
    GD_CHECK_ARG(x && mean && valid && coef && out, fn ": null pointer");                                              \
    EOF_CUBE_CHECKS(fn);                                                                                                \
    GD_CHECK_ARG(K >= 1 && K <= GD_EOF_MAX_K, fn ": K outside 1..GD_EOF_MAX_K");                                        \
    GD_CHECK_ARG(use_weight == 0 || (use_weight == 1 && weight), fn ": use_weight outside {0, 1} or without weights"); \
    GD_CHECK_ARG(gd_elem_aligned(x, dtype) && gd_aligned(weight, 8) && gd_aligned(mean, 8) && gd_aligned(coef, 8) &&    \
                     gd_aligned(out, 8),                                                                                \
                 fn ": pointer not element aligned")

extern "C" int gd_eof_project(const void* x, int dtype, long T, long M, const double* mean, const unsigned char* valid,
                              const double* weight, int use_weight, const double* coef, int K, double* out, void* stream) {
    EOF_PROJECT_CHECKS("gd_eof_project");
    project_run(false, GD_S, x, dtype, T, M, mean, valid, use_weight ? weight : nullptr, coef, K, out);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_eof_project_host(const void* x, int dtype, long T, long M, const double* mean, const unsigned char* valid,
                                   const double* weight, int use_weight, const double* coef, int K, double* out) {
    EOF_PROJECT_CHECKS("gd_eof_project_host");
    project_run(true, nullptr, x, dtype, T, M, mean, valid, use_weight ? weight : nullptr, coef, K, out);
    return 0;
}

#define EOF_RECONSTRUCT_CHECKS(fn)                                                                                      \
    GD_CHECK_ARG(eofs && pcs && mean && valid && out, fn ": null pointer");                                            \
    GD_CHECK_ARG(gd_dtype_ok(out_dtype), fn ": dtype outside {0, 1}");                                                  \
    GD_CHECK_ARG(T > 0 && M > 0, fn ": T <= 0 or M <= 0");                                                               \
    GD_CHECK_ARG(M < (1L << 31) && M < (1L << 53) / T, fn ": too many series");                                          \
    GD_CHECK_ARG(K >= 1 && K <= GD_EOF_MAX_K, fn ": K outside 1..GD_EOF_MAX_K");                                        \
    GD_CHECK_ARG(gd_elem_aligned(out, out_dtype) && gd_aligned(weight, 8) && gd_aligned(mean, 8) && gd_aligned(eofs, 8) && \
                     gd_aligned(pcs, 8),                                                                                \
                 fn ": pointer not element aligned")

extern "C" int gd_eof_reconstruct(const double* eofs, const double* pcs, const double* mean, const unsigned char* valid,
                                  const double* weight, long T, long M, int K, void* out, int out_dtype, void* stream) {
    EOF_RECONSTRUCT_CHECKS("gd_eof_reconstruct");
    reconstruct_run(false, GD_S, eofs, pcs, mean, valid, weight, T, M, K, out, out_dtype);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_eof_reconstruct_host(const double* eofs, const double* pcs, const double* mean, const unsigned char* valid,
                                       const double* weight, long T, long M, int K, void* out, int out_dtype) {
    EOF_RECONSTRUCT_CHECKS("gd_eof_reconstruct_host");
    reconstruct_run(true, nullptr, eofs, pcs, mean, valid, weight, T, M, K, out, out_dtype);
    return 0;
}
