// PAM attention probe: what the N x N attention matrix P = softmax_j(q_i . k_j) of the fused PAM kernels looks like,
// without ever forming it.  Sweeps of the kind pam_f32.hip runs for S = K Q^T, on the same operand contract: q, k
// (B, r, Npad) fp32 planes, Npad a multiple of 256, columns >= N zero, every product a v_mfma_f32_32x32x2_f32.  The logits
// are s_ij = logit_scale * (q_i . k_j) in nats: 1 for the projections as they are, ln 2 for planes that hold the 16-bit
// routes' operands (q log2 e and k rounded to bf16 / fp16 by gd_round_to_16), so one code path serves both.
//
//   stats     query-parallel, 4 waves x 32 queries, key tiles of 64 through the LDS-DMA ring (the forward's layout, no V).
//             Per query, online: m = running maximum, l = sum e^(s - m), u = sum e^(s - m) (s - m)   (every term <= 0).
//             When m rises by d:  u <- e^-d (u - d l),  l <- e^-d l.
//             lse = m + ln l;  entropy = ln l - u / l  (= -sum_j P_ij ln P_ij, nats);  peak = 1 / l  (= max_j P_ij).
//   received  key-parallel, 32 keys per wave, queries streamed in 32-column tiles (the dV kernel's layout, no dO):
//             received_j = sum_{i < N} exp(s_ij - lse_i); its mean over j is 1.
//   rows      the stats sweep on S gathered queries (padded to groups of 32: the same S tile, the same order of sums, so
//             lse_rows equals the stats' lse bit for bit), then a second sweep that writes P through an LDS transpose:
//             lanes along the keys, 16-byte stores where N % 4 == 0.
// No atomics, no scratch, no N x N or N x tile global buffer; every output element is summed by one wave in a fixed order.
#include <stdint.h>

#include "pam_common.h"
#include "../../include/gandanet.h"

namespace {

using pam::LOG2E;
using gd::acc_row;
using namespace pam::f32;

// K region of key tile t -> ``base`` (four waves share the pieces; the forward's K staging)
__device__ __forceinline__ void dma_k_tile(const float* kb, int R, int nks, int ld, int t, float* base, int wave, int lane) {
    const int kpiece = (2 * nks * F_RCH + 63) >> 6;
    const long col = (long)t * F_KT;
    for (int p = wave; p < kpiece; p += 4) {
        const int c = p * 64 + lane;
        const int row = c / F_RCH, part = c - row * F_RCH;
        dma16(kb + (long)min(row, R - 1) * ld + col + min(part, F_RCH - 2) * 4, base + p * 256);
    }
}

// S^T of key tile t against the wave's 32 queries, in nats: register e of half ``sub`` <-> key t 64 + sub 32 + acc_row(e, h)
__device__ __forceinline__ void logits_tile(f32x16_t (&s)[2], const float* Ks, int r, int h, int nks, const float (&qf)[MAXKS],
                                            float logit_scale) {
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
        zero16(s[sub]);
        s_tile<F_LD>(s[sub], Ks, sub * 32 + r, h, nks, qf);
#pragma unroll
        for (int e = 0; e < 16; ++e) s[sub][e] *= logit_scale;
    }
}

constexpr int ROW_LD = 36;     // P staging of one 32-key half: [32 queries][32 keys + 4 pad floats], 16-byte accesses

// ROWS = false: queries blockIdx.x 128 + wave 32 + r, maps lse / entropy / peak (B, N).
// ROWS = true : queries idx[blockIdx.x 128 + wave 32 + r] (clamped to [0, N)), lse (B, S) and rows (B, S, N).
template <bool ROWS>
__global__ __launch_bounds__(256) void pam_attn_sweep_kernel(const float* __restrict__ q, long q_bs, const float* __restrict__ k,
                                                             long k_bs, const int* __restrict__ idx, int S, int N, int ld, int R,
                                                             float logit_scale, float* __restrict__ lse,
                                                             float* __restrict__ entropy, float* __restrict__ peak,
                                                             float* __restrict__ rows) {
    constexpr int TILE = F_KPIECE * 256;      // floats per ring slot
    __shared__ __attribute__((aligned(16))) float ring[2 * TILE];
    __shared__ __attribute__((aligned(16))) float stage[ROWS ? 4 * 32 * ROW_LD : 4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int slot0 = blockIdx.x * 128 + wave * 32;     // first query slot of this wave
    const int nq = ROWS ? S : N;                        // slots that produce output
    const int nks = (R + 1) >> 1;
    const float* qb = q + (long)b * q_bs;
    const float* kb = k + (long)b * k_bs;

    int qi = slot0 + r;      // < Npad; the padded queries are zero columns
    if (ROWS) qi = slot0 + r < S ? min(max(idx[slot0 + r], 0), N - 1) : 0;

    float qf[MAXKS];
#pragma unroll
    for (int s = 0; s < MAXKS; ++s) qf[s] = (2 * s + h) < R ? qb[(long)(2 * s + h) * ld + qi] : 0.f;

    float m = -MASKED, l = 0.f, u = 0.f;
    const int nkt = (N + F_KT - 1) / F_KT;

    dma_k_tile(kb, R, nks, ld, 0, ring, wave, lane);
    for (int t = 0; t < nkt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of tile t has landed
        __syncthreads();                                   // ... and everyone's; tile t - 1 has been consumed
        if (t + 1 < nkt) dma_k_tile(kb, R, nks, ld, t + 1, ring + ((t + 1) & 1) * TILE, wave, lane);

        f32x16_t s[2];
        logits_tile(s, ring + (t & 1) * TILE, r, h, nks, qf, logit_scale);
        if ((t + 1) * F_KT > N) {
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (t * F_KT + sub * 32 + acc_row(e, h) >= N) s[sub][e] = -MASKED;
        }
        float mloc = s[0][0];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int e = 0; e < 16; ++e) mloc = fmaxf(mloc, s[sub][e]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        if (__any(mloc > m)) {
            const float m_new = fmaxf(m, mloc);
            const float d = m - m_new;                     // <= 0
            const float alpha = gd_exp2_fast(d * LOG2E);
            u = alpha * fmaf(d, l, u);
            l *= alpha;
            m = m_new;
        }
        float lsum = 0.f, usum = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float d = s[sub][e] - m;             // masked keys: p = 0, p d = -0
                const float p = gd_exp2_fast(d * LOG2E);
                lsum += p;
                usum = fmaf(p, d, usum);
            }
        lsum += __shfl_xor(lsum, 32, 64);
        usum += __shfl_xor(usum, 32, 64);
        l += lsum;
        u += usum;
    }

    const int slot = slot0 + r;
    const float ln_l = logf(l);
    if (slot < nq && h == 0) {
        if (lse) lse[(long)b * nq + slot] = m + ln_l;
        if (!ROWS) {
            if (entropy) entropy[(long)b * N + slot] = ln_l - u / l;
            if (peak) peak[(long)b * N + slot] = 1.f / l;
        }
    }

    if constexpr (ROWS) {
        // second sweep: P = e^(s - m) / l, staged per 32-key half as [query][key] so that the stores run along the keys
        const float inv_l = 1.f / l;
        float* st = stage + wave * 32 * ROW_LD;
        float* out = rows + ((long)b * S + slot0) * N;
        const bool vec = (N & 3) == 0 && ((uintptr_t)rows & 15u) == 0;
        __syncthreads();                                   // every wave is done with the ring's last tile
        dma_k_tile(kb, R, nks, ld, 0, ring, wave, lane);
        for (int t = 0; t < nkt; ++t) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (t + 1 < nkt) dma_k_tile(kb, R, nks, ld, t + 1, ring + ((t + 1) & 1) * TILE, wave, lane);

            f32x16_t s[2];
            logits_tile(s, ring + (t & 1) * TILE, r, h, nks, qf, logit_scale);
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {              // registers 4 g .. 4 g + 3 = keys 8 g + 4 h + 0 .. 3 of query r
                    f32x4_t p;
#pragma unroll
                    for (int j = 0; j < 4; ++j) p[j] = gd_exp2_fast((s[sub][4 * g + j] - m) * LOG2E) * inv_l;
                    *reinterpret_cast<f32x4_t*>(st + r * ROW_LD + 8 * g + 4 * h) = p;
                }
                __builtin_amdgcn_wave_barrier();           // the staging tile is this wave's own: LDS runs its accesses in order
                const int key = t * F_KT + sub * 32 + (lane & 7) * 4;
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int row = it * 8 + (lane >> 3);
                    const f32x4_t p = *reinterpret_cast<const f32x4_t*>(st + row * ROW_LD + (lane & 7) * 4);
                    if (slot0 + row < S) {
                        float* dst = out + (long)row * N + key;
                        if (vec) {
                            if (key < N) *reinterpret_cast<f32x4_t*>(dst) = p;     // N % 4 == 0: all four in or all out
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (key + j < N) dst[j] = p[j];
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
}

// owners = keys (32 per wave, 128 per workgroup); queries streamed in 32-column tiles with their lse
__global__ __launch_bounds__(256) void pam_attn_received_kernel(const float* __restrict__ q, long q_bs, const float* __restrict__ k,
                                                                long k_bs, const float* __restrict__ lse, int N, int ld, int R,
                                                                float logit_scale, float* __restrict__ received) {
    constexpr int SLOT = B_RREG + 64;
    __shared__ __attribute__((aligned(16))) float ring[2 * SLOT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int j0 = blockIdx.x * 128 + wave * 32;
    const int nks = (R + 1) >> 1;
    const float* qb = q + (long)b * q_bs;
    const float* kb = k + (long)b * k_bs;
    const float* lse_b = lse + (long)b * N;

    float kf[MAXKS];
#pragma unroll
    for (int s = 0; s < MAXKS; ++s) kf[s] = (2 * s + h) < R ? kb[(long)(2 * s + h) * ld + j0 + r] : 0.f;

    auto load_stat = [&](int t) {     // lse of tile t's queries (MASKED past N: P = 0 there)
        const int i = t * 32 + tid;
        return (tid < 32 && i < N) ? lse_b[i] : MASKED;
    };

    float acc = 0.f;
    const int nqt = (N + 31) / 32;

    bwd_dma_r(qb, R, nks, ld, 0, ring, wave, lane);
    if (tid < 32) ring[B_RREG + tid] = load_stat(0);
    for (int t = 0; t < nqt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        float stat_next = 0.f;
        if (t + 1 < nqt) {
            bwd_dma_r(qb, R, nks, ld, (t + 1) * 32, ring + ((t + 1) & 1) * SLOT, wave, lane);
            stat_next = load_stat(t + 1);
        }
        const float* Qs = ring + (t & 1) * SLOT;
        const float* Ls = Qs + B_RREG;

        f32x16_t p;    // S, then P: query acc_row(e, h) on the rows, key j0 + r on the lane
        zero16(p);
        s_tile<B_RLD>(p, Qs, r, h, nks, kf);
        float tsum = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) tsum += gd_exp2_fast((p[e] * logit_scale - Ls[acc_row(e, h)]) * LOG2E);
        acc += tsum;
        if (t + 1 < nqt && tid < 32) ring[((t + 1) & 1) * SLOT + B_RREG + tid] = stat_next;
    }
    acc += __shfl_xor(acc, 32, 64);

    const int j = j0 + r;
    if (j < N && h == 0) received[(long)b * N + j] = acc;
}

__global__ __launch_bounds__(256) void round_to_16_kernel(const float* __restrict__ x, float* __restrict__ y, long n, float scale,
                                                          int f16) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = x[i] * scale;
        y[i] = f16 ? (float)(_Float16)v : gd_bf2f(gd_f2bf(v));
    }
}

int probe_check(const float* q, long q_bs, const float* k, long k_bs, int B, int N, int Npad, int r) {
    GD_CHECK_ARG(q && k, "gd_pam_attn: null pointer (q / k)");
    GD_CHECK_ARG(B > 0 && B <= 65535, "gd_pam_attn: B must be in 1..65535");
    GD_CHECK_ARG(N > 0 && Npad >= N && Npad % 256 == 0, "gd_pam_attn: Npad must be a multiple of 256 >= N");
    GD_CHECK_ARG(r >= 1 && r <= 63, "gd_pam_attn: r (query / key channels) must be in 1..63");
    GD_CHECK_ARG(q_bs >= 0 && k_bs >= 0, "gd_pam_attn: negative batch stride");
    GD_CHECK_ARG(aligned16(q) && aligned16(k) && q_bs % 4 == 0 && k_bs % 4 == 0,
                 "gd_pam_attn: unaligned plane (q / k must be 16-byte aligned with batch strides that are multiples of 4)");
    return 0;
}

}  // namespace

extern "C" int gd_pam_attn_stats(const float* q, long q_bs, const float* k, long k_bs, int B, int N, int Npad, int r,
                                 float logit_scale, float* lse, float* entropy, float* peak, void* stream) {
    if (probe_check(q, q_bs, k, k_bs, B, N, Npad, r)) return -1;
    GD_CHECK_ARG(lse, "gd_pam_attn_stats: null pointer (lse)");
    hipLaunchKernelGGL((pam_attn_sweep_kernel<false>), dim3(Npad / 128, B), dim3(256), 0, (hipStream_t)stream, q, q_bs, k, k_bs,
                       (const int*)nullptr, 0, N, Npad, r, logit_scale, lse, entropy, peak, (float*)nullptr);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_pam_attn_received(const float* q, long q_bs, const float* k, long k_bs, const float* lse, int B, int N, int Npad,
                                    int r, float logit_scale, float* received, void* stream) {
    if (probe_check(q, q_bs, k, k_bs, B, N, Npad, r)) return -1;
    GD_CHECK_ARG(lse && received, "gd_pam_attn_received: null pointer (lse / received)");
    hipLaunchKernelGGL(pam_attn_received_kernel, dim3(Npad / 128, B), dim3(256), 0, (hipStream_t)stream, q, q_bs, k, k_bs, lse, N,
                       Npad, r, logit_scale, received);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_pam_attn_rows(const float* q, long q_bs, const float* k, long k_bs, const int* idx, int S, int B, int N,
                                int Npad, int r, float logit_scale, float* rows, float* lse_rows, void* stream) {
    if (probe_check(q, q_bs, k, k_bs, B, N, Npad, r)) return -1;
    GD_CHECK_ARG(idx && rows, "gd_pam_attn_rows: null pointer (idx / rows)");
    GD_CHECK_ARG(S >= 1 && S <= 256, "gd_pam_attn_rows: S (selected queries) must be in 1..256");
    hipLaunchKernelGGL((pam_attn_sweep_kernel<true>), dim3((S + 127) / 128, B), dim3(256), 0, (hipStream_t)stream, q, q_bs, k,
                       k_bs, idx, S, N, Npad, r, logit_scale, lse_rows, (float*)nullptr, (float*)nullptr, rows);
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_round_to_16(const float* x, float* y, long n, float scale, int f16, void* stream) {
    GD_CHECK_ARG(x && y, "gd_round_to_16: null pointer");
    GD_CHECK_ARG(n > 0, "gd_round_to_16: n <= 0");
    GD_CHECK_ARG(f16 == 0 || f16 == 1, "gd_round_to_16: f16 must be 0 (bf16) or 1 (fp16)");
    const long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(round_to_16_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, x, y,
                       n, scale, f16);
    GD_LAUNCH_CHECK();
    return 0;
}
