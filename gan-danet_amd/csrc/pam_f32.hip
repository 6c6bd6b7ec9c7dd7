// Fused (flash-style) PAM on EXACT fp32 operands (generator.py:115-122 and its autograd): the parity mode's attention
// without the reference's N x N matrices.  Every product is a v_mfma_f32_32x32x2_f32 (operands one fp32 per lane,
// A[row l&31][k = l>>5], B[k = l>>5][col l&31]); nothing is rounded to 16 bits.
//
// Operand contract: q, k (B, r, Npad) and v, gdo (B, C, Npad) are the projections' own fp32 planes (channel-major, row
// length Npad = N rounded up to 256, columns >= N zero): with N % 256 == 0 the 1x1 convs' outputs go in as they are.
// The channel-major planes ARE the MFMA operand layout (one channel pair per k-step, 32 consecutive positions per
// lane group), so no transposed copy exists.  r is padded to the k-step only (r + (r & 1)); channel rows past r / C are
// never read (row indices are clamped, the other operand is zero there).
//
// Accumulator as operand: register e of a 32x32 accumulator holds row 8 (e / 4) + e % 4 in lanes 0..31 and that row + 4 in
// lanes 32..63 = the row pair of ONE k-step of the next product's B operand.  The A operand of that k-step is read from
// the LDS tile at column acc_row(e, h); four consecutive e are one 16-byte LDS read.
//
// Forward: query-parallel, 4 waves x 32 queries; K / V tiles of 64 keys streamed through a two-slot LDS ring by LDS-DMA.
//   S^T = K Q^T (keys on accumulator rows), online softmax (running maximum with rescale, fp32), O^T += V P^T.
//   One launch per chunk of <= 192 value channels; every chunk recomputes S in the same order, chunk 0 writes the LSE.
// Backward: no atomics, no scratch.  Owners (32 per wave, 128 per workgroup) keep their accumulators for the whole sweep;
//   the other side is streamed through LDS in 32-column tiles:
//     dv  (owners = keys, one launch per V chunk): P from q, k and the LSE, dV^T += dO P
//     dkq (owners = keys -> dK, owners = queries -> dQ; the same kernel with the operand roles swapped):
//         S, dP over all C channels (the owner's C-vector lives in registers as the B operand), dS = P (dP - delta),
//         dOwn^T += Other^T dS.
//   Every output element is summed by one wave in a fixed order: two runs agree bit for bit.
#include <stdint.h>
#include <stdlib.h>

#include "pam_common.h"
#include "../../include/gandanet.h"

namespace {

using pam::LOG2E;
using gd::acc_row;
using namespace pam::f32;     // s_tile, the LDS-DMA helpers and the tile geometry shared with pam_probe.hip

// =====================================================================================================
// forward
// =====================================================================================================
template <int CT>
__global__ __launch_bounds__(256) void pam_f32_fwd_kernel(const float* __restrict__ q, long q_bs, const float* __restrict__ k,
                                                          long k_bs, const float* __restrict__ v, long v_bs, int c0, int N,
                                                          int ld, int C, int R, const float* __restrict__ gamma,
                                                          const float* __restrict__ x, long x_bs, float* __restrict__ out,
                                                          long out_bs, float* __restrict__ o_attn, float* __restrict__ lse) {
    constexpr int NW = 4, CP = CT * 32;       // one wave per SIMD: up to 512 registers, and the 64-cycle MFMAs leave no gap to fill
    constexpr int VCH = CP * F_RCH;
    constexpr int VPIECE = (VCH + 63) / 64;
    constexpr int TILE = (F_KPIECE + VPIECE) * 256;      // floats per ring slot
    __shared__ __attribute__((aligned(16))) float ring[2 * TILE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * (NW * 32) + wave * 32;
    const int nks = (R + 1) >> 1;
    const int kpiece = (2 * nks * F_RCH + 63) >> 6;
    const float* qb = q + (long)b * q_bs;
    const float* kb = k + (long)b * k_bs;
    const float* vb = v + (long)b * v_bs;

    // Q^T fragment: channel 2 s + h of query q0 + r (zero past r: the clamped K rows meet a zero there)
    float qf[MAXKS];
#pragma unroll
    for (int s = 0; s < MAXKS; ++s) qf[s] = (2 * s + h) < R ? qb[(long)(2 * s + h) * ld + q0 + r] : 0.f;

    auto dma_tile = [&](int t, int slot) {
        float* base = ring + slot * TILE;
        const long col = (long)t * F_KT;
        for (int p = wave; p < kpiece; p += NW) {
            const int c = p * 64 + lane;
            const int row = c / F_RCH, part = c - row * F_RCH;
            dma16(kb + (long)min(row, R - 1) * ld + col + min(part, F_RCH - 2) * 4, base + p * 256);
        }
#pragma unroll
        for (int p0 = 0; p0 < VPIECE; p0 += NW) {
            const int p = p0 + wave;
            const int c = p * 64 + lane;
            if (p < VPIECE && c < VCH) {
                const int row = c / F_RCH, part = c - row * F_RCH;
                dma16(vb + (long)min(c0 + row, C - 1) * ld + col + min(part, F_RCH - 2) * 4, base + (F_KPIECE + p) * 256);
            }
        }
    };

    f32x16_t o[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) zero16(o[ct]);
    float m = -MASKED, l = 0.f;
    const int nkt = (N + F_KT - 1) / F_KT;

    dma_tile(0, 0);
    for (int t = 0; t < nkt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of tile t has landed
        __syncthreads();                                   // ... and everyone's; tile t - 1 has been consumed
        if (t + 1 < nkt) dma_tile(t + 1, (t + 1) & 1);
        const float* Ks = ring + (t & 1) * TILE;
        const float* Vs = Ks + F_KPIECE * 256;

        f32x16_t sacc[2];    // S^T: keys on rows (register e <-> key acc_row(e, h) of the 32-key half), query r on the lane
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            zero16(sacc[sub]);
            s_tile<F_LD>(sacc[sub], Ks, sub * 32 + r, h, nks, qf);
        }
        if ((t + 1) * F_KT > N) {
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (t * F_KT + sub * 32 + acc_row(e, h) >= N) sacc[sub][e] = -MASKED;
        }
        float mloc = sacc[0][0];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int e = 0; e < 16; ++e) mloc = fmaxf(mloc, sacc[sub][e]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        if (__any(mloc > m)) {
            const float m_new = fmaxf(m, mloc);
            const float alpha = gd_exp2_fast((m - m_new) * LOG2E);
            l *= alpha;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int e = 0; e < 16; ++e) o[ct][e] *= alpha;
            m = m_new;
        }
        float lsum = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                sacc[sub][e] = gd_exp2_fast((sacc[sub][e] - m) * LOG2E);
                lsum += sacc[sub][e];
            }
        lsum += __shfl_xor(lsum, 32, 64);
        l += lsum;

        // O^T += V P^T: k-step e of half ``sub`` is the key pair (acc_row(e, 0), acc_row(e, 1)) = register e of P^T
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4_t vf[CT];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    vf[ct] = *reinterpret_cast<const f32x4_t*>(Vs + (ct * 32 + r) * F_LD + sub * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) o[ct] = mfma_f32(vf[ct][j], sacc[sub][4 * g + j], o[ct]);
            }
    }

    const int qi = q0 + r;
    if (qi < N) {
        const float inv_l = 1.f / l;
        const float g = *gamma;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int c = c0 + ct * 32 + acc_row(e, h);
                if (c < C) {
                    const float val = o[ct][e] * inv_l;
                    o_attn[((long)b * C + c) * N + qi] = val;
                    out[(long)b * out_bs + (long)c * N + qi] = fmaf(g, val, x[(long)b * x_bs + (long)c * N + qi]);
                }
            }
        if (c0 == 0 && h == 0) lse[(long)b * N + qi] = m + logf(l);
    }
}

// =====================================================================================================
// backward: streamed 32-column tiles.  Slot = [r region: 64 rows x 36 floats (8 data chunks + 1 pad chunk per row)]
//                                             [C region: rows of CLD floats][lse 32][delta 32]
// =====================================================================================================
// -----------------------------------------------------------------------------------------------------
// dV^T of one channel chunk (CT x 32 channels from c0); owners = keys
// -----------------------------------------------------------------------------------------------------
template <int CT>
__global__ __launch_bounds__(256) void pam_f32_dv_kernel(const float* __restrict__ q, long q_bs, const float* __restrict__ k,
                                                         long k_bs, const float* __restrict__ gdo, long gdo_bs, int c0,
                                                         const float* __restrict__ lse, int N, int ld, int C, int R,
                                                         float* __restrict__ dv) {
    constexpr int CP = CT * 32, CLD = 36, CCH = CP * 9;
    constexpr int CPIECE = (CCH + 63) / 64;
    constexpr int SLOT = B_RREG + CPIECE * 256 + 64;
    __shared__ __attribute__((aligned(16))) float ring[2 * SLOT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int j0 = blockIdx.x * 128 + wave * 32;
    const int nks = (R + 1) >> 1;
    const float* qb = q + (long)b * q_bs;
    const float* kb = k + (long)b * k_bs;
    const float* db = gdo + (long)b * gdo_bs;
    const float* lse_b = lse + (long)b * N;

    float kf[MAXKS];
#pragma unroll
    for (int s = 0; s < MAXKS; ++s) kf[s] = (2 * s + h) < R ? kb[(long)(2 * s + h) * ld + j0 + r] : 0.f;

    auto dma_tile = [&](int t, int slot) {
        float* base = ring + slot * SLOT;
        bwd_dma_r(qb, R, nks, ld, t * 32, base, wave, lane);
#pragma unroll
        for (int p0 = 0; p0 < CPIECE; p0 += 4) {
            const int p = p0 + wave;
            const int c = p * 64 + lane;
            if (p < CPIECE && c < CCH) {
                const int row = c / 9, part = c - row * 9;
                dma16(db + (long)min(c0 + row, C - 1) * ld + t * 32 + min(part, 7) * 4, base + B_RREG + p * 256);
            }
        }
    };
    auto load_stat = [&](int t) {     // lse of tile t's queries (MASKED past N: P = 0 there)
        const int i = t * 32 + tid;
        return (tid < 32 && i < N) ? lse_b[i] : MASKED;
    };

    f32x16_t acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) zero16(acc[ct]);
    const int nqt = (N + 31) / 32;

    dma_tile(0, 0);
    if (tid < 32) ring[B_RREG + CPIECE * 256 + tid] = load_stat(0);
    for (int t = 0; t < nqt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        float stat_next = 0.f;
        if (t + 1 < nqt) {
            dma_tile(t + 1, (t + 1) & 1);
            stat_next = load_stat(t + 1);
        }
        const float* Qs = ring + (t & 1) * SLOT;
        const float* dOs = Qs + B_RREG;
        const float* Ls = dOs + CPIECE * 256;

        f32x16_t p;    // S, then P: query acc_row(e, h) on the rows, key j0 + r on the lane
        zero16(p);
        s_tile<B_RLD>(p, Qs, r, h, nks, kf);
#pragma unroll
        for (int e = 0; e < 16; ++e) p[e] = gd_exp2_fast((p[e] - Ls[acc_row(e, h)]) * LOG2E);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4_t a[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) a[ct] = *reinterpret_cast<const f32x4_t*>(dOs + (ct * 32 + r) * CLD + 8 * g + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma_f32(a[ct][j], p[4 * g + j], acc[ct]);
        }
        if (t + 1 < nqt && tid < 32) ring[((t + 1) & 1) * SLOT + B_RREG + CPIECE * 256 + tid] = stat_next;
    }

    const int j = j0 + r;
    if (j < N) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int c = c0 + ct * 32 + acc_row(e, h);
                if (c < C) dv[((long)b * C + c) * N + j] = acc[ct][e];
            }
    }
}

// -----------------------------------------------------------------------------------------------------
// dOwn^T (R rows) over all C channels.  QSIDE = false: owners = keys (own = k, v; streamed = q, gdo; result dK);
// QSIDE = true: owners = queries (own = q, gdo; streamed = k, v; result dQ).  CTMAX x 32 >= C.
// -----------------------------------------------------------------------------------------------------
template <int CTMAX, bool QSIDE>
__global__ __launch_bounds__(256) void pam_f32_dkq_kernel(const float* __restrict__ own_r, long own_r_bs,
                                                          const float* __restrict__ own_c, long own_c_bs,
                                                          const float* __restrict__ str_r, long str_r_bs,
                                                          const float* __restrict__ str_c, long str_c_bs,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          int N, int ld, int C, int R, float* __restrict__ d_own) {
    constexpr int CLD = 32;                          // C rows unpadded: only read as [channel pair][32 lanes]
    constexpr int NCS = CTMAX * 16;                  // k-steps of the dP product
    constexpr int SLOT = B_RREG + CTMAX * 32 * CLD + 64;
    __shared__ __attribute__((aligned(16))) float ring[2 * SLOT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int x0 = blockIdx.x * 128 + wave * 32;
    const int nks = (R + 1) >> 1;
    const int ncp = (C + 7) >> 3;                    // 8-row pieces (= groups of four k-steps) of the C region
    const float* orb = own_r + (long)b * own_r_bs;
    const float* ocb = own_c + (long)b * own_c_bs;
    const float* srb = str_r + (long)b * str_r_bs;
    const float* scb = str_c + (long)b * str_c_bs;
    const float* lse_b = lse + (long)b * N;
    const float* delta_b = delta + (long)b * N;

    float rf[MAXKS];
#pragma unroll
    for (int s = 0; s < MAXKS; ++s) rf[s] = (2 * s + h) < R ? orb[(long)(2 * s + h) * ld + x0 + r] : 0.f;
    float cf[NCS];     // the owner's C-vector: the B operand of dP over all channels
#pragma unroll
    for (int s = 0; s < NCS; ++s) cf[s] = (2 * s + h) < C ? ocb[(long)(2 * s + h) * ld + x0 + r] : 0.f;

    float own_lse = 0.f, own_delta = 0.f;
    if (QSIDE && x0 + r < N) {
        own_lse = lse_b[x0 + r];
        own_delta = delta_b[x0 + r];
    }

    auto dma_tile = [&](int t, int slot) {
        float* base = ring + slot * SLOT;
        bwd_dma_r(srb, R, nks, ld, t * 32, base, wave, lane);
        for (int p = wave; p < ncp; p += 4)
            dma16(scb + (long)min(8 * p + (lane >> 3), C - 1) * ld + t * 32 + (lane & 7) * 4, base + B_RREG + p * 256);
    };
    auto load_stat = [&](int t) {     // streamed queries: lse (lanes 0..31; MASKED past N) and delta (lanes 32..63)
        const int i = t * 32 + (tid & 31);
        if (tid < 32) return i < N ? lse_b[i] : MASKED;
        return (tid < 64 && i < N) ? delta_b[i] : 0.f;
    };
    constexpr int STAT = B_RREG + CTMAX * 32 * CLD;

    f32x16_t acc[2];
    zero16(acc[0]);
    zero16(acc[1]);
    const int nt = (N + 31) / 32;
    const int last_row = 2 * nks - 1;

    dma_tile(0, 0);
    if (!QSIDE && tid < 64) ring[STAT + tid] = load_stat(0);
    for (int t = 0; t < nt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        float stat_next = 0.f;
        if (t + 1 < nt) {
            dma_tile(t + 1, (t + 1) & 1);
            if (!QSIDE) stat_next = load_stat(t + 1);
        }
        const float* Yr = ring + (t & 1) * SLOT;
        const float* Yc = Yr + B_RREG;
        const float* Ls = Yr + STAT;

        f32x16_t s, dp0, dp1;     // streamed position acc_row(e, h) on the rows, owner x0 + r on the lane
        zero16(s);
        zero16(dp0);
        zero16(dp1);
        s_tile<B_RLD>(s, Yr, r, h, nks, rf);
#pragma unroll
        for (int g = 0; g < CTMAX * 4; ++g) {
            if (g < ncp) {
                float a[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = Yc[(8 * g + 2 * j + h) * CLD + r];
                dp0 = mfma_f32(a[0], cf[4 * g + 0], dp0);
                dp1 = mfma_f32(a[1], cf[4 * g + 1], dp1);
                dp0 = mfma_f32(a[2], cf[4 * g + 2], dp0);
                dp1 = mfma_f32(a[3], cf[4 * g + 3], dp1);
            }
        }
        // dS = P (dP - delta)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float ls = QSIDE ? own_lse : Ls[acc_row(e, h)];
            const float dl = QSIDE ? own_delta : Ls[32 + acc_row(e, h)];
            float p = gd_exp2_fast((s[e] - ls) * LOG2E);
            if (QSIDE && t * 32 + acc_row(e, h) >= N) p = 0.f;     // padded keys
            s[e] = p * ((dp0[e] + dp1[e]) - dl);
        }
        // dOwn^T[d][x] += Other^T[d][y] dS[y][x]
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            if (dt == 0 || R > 32) {
                const float* row = Yr + min(dt * 32 + r, last_row) * B_RLD + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(row + 8 * g);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[dt] = mfma_f32(a[j], s[4 * g + j], acc[dt]);
                }
            }
        }
        if (!QSIDE && t + 1 < nt && tid < 64) ring[((t + 1) & 1) * SLOT + STAT + tid] = stat_next;
    }

    const int xi = x0 + r;
    if (xi < N) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int d = dt * 32 + acc_row(e, h);
                if (d < R) d_own[((long)b * R + d) * N + xi] = acc[dt][e];
            }
    }
}

}  // namespace

#define PAM_F32_DISPATCH_ALL(TILES_, ...)                                    \
    do {                                                                     \
        if ((TILES_) <= 3) { constexpr int CTMAX = 3; __VA_ARGS__; }         \
        else if ((TILES_) <= 6) { constexpr int CTMAX = 6; __VA_ARGS__; }    \
        else if ((TILES_) <= 8) { constexpr int CTMAX = 8; __VA_ARGS__; }    \
        else if ((TILES_) <= 12) { constexpr int CTMAX = 12; __VA_ARGS__; }  \
        else { constexpr int CTMAX = 16; __VA_ARGS__; }                      \
    } while (0)

static int pam_f32_check(int B, int N, int Npad, int C, int r) {
    GD_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && Npad >= N && Npad % 256 == 0, "gd_pam_f32: Npad must be a multiple of 256 >= N");
    GD_CHECK_ARG(C >= 1 && C <= 511, "gd_pam_f32: C (value channels) must be in 1..511");
    GD_CHECK_ARG(r >= 1 && r <= 63, "gd_pam_f32: r (query / key channels) must be in 1..63");
    return 0;
}

extern "C" int gd_pam_f32_fwd(const float* q, long q_bs, const float* k, long k_bs, const float* v, long v_bs, int B, int N,
                              int Npad, int C, int r, const float* gamma, const float* x, long x_bs, float* out, long out_bs,
                              float* o_attn, float* lse, void* stream) {
    GD_CHECK_ARG(q && k && v && gamma && x && out && o_attn && lse, "gd_pam_f32_fwd: null pointer");
    if (pam_f32_check(B, N, Npad, C, r)) return -1;
    GD_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && q_bs % 4 == 0 && k_bs % 4 == 0 && v_bs % 4 == 0,
                 "gd_pam_f32_fwd: q / k / v must be 16-byte aligned with batch strides that are multiples of 4");
    hipStream_t s = (hipStream_t)stream;
    const pam::Chunks ch((C + 31) / 32);
    const dim3 grid(Npad / 128, B), block(256);
    for (int i = 0; i < ch.n; ++i) {
        PAM_DISPATCH_CT(ch.ct[i], {
            hipLaunchKernelGGL((pam_f32_fwd_kernel<CT>), grid, block, 0, s, q, q_bs, k, k_bs, v, v_bs, ch.c0[i], N, Npad, C, r,
                               gamma, x, x_bs, out, out_bs, o_attn, lse);
        });
    }
    GD_LAUNCH_CHECK();
    return 0;
}

extern "C" int gd_pam_f32_bwd(const float* q, long q_bs, const float* k, long k_bs, const float* v, long v_bs, const float* gdo,
                              long gdo_bs, const float* lse, const float* delta, int B, int N, int Npad, int C, int r,
                              float* dq, float* dk, float* dv, void* stream) {
    GD_CHECK_ARG(q && k && v && gdo && lse && delta && dq && dk && dv, "gd_pam_f32_bwd: null pointer");
    if (pam_f32_check(B, N, Npad, C, r)) return -1;
    GD_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(gdo) && q_bs % 4 == 0 && k_bs % 4 == 0 &&
                     v_bs % 4 == 0 && gdo_bs % 4 == 0,
                 "gd_pam_f32_bwd: q / k / v / gdo must be 16-byte aligned with batch strides that are multiples of 4");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(Npad / 128, B), block(256);
    const pam::Chunks ch((C + 31) / 32);
    for (int i = 0; i < ch.n; ++i) {
        PAM_DISPATCH_CT(ch.ct[i], {
            hipLaunchKernelGGL((pam_f32_dv_kernel<CT>), grid, block, 0, s, q, q_bs, k, k_bs, gdo, gdo_bs, ch.c0[i], lse, N, Npad,
                               C, r, dv);
        });
    }
    PAM_F32_DISPATCH_ALL((C + 31) / 32, {
        hipLaunchKernelGGL((pam_f32_dkq_kernel<CTMAX, false>), grid, block, 0, s, k, k_bs, v, v_bs, q, q_bs, gdo, gdo_bs, lse,
                           delta, N, Npad, C, r, dk);
        hipLaunchKernelGGL((pam_f32_dkq_kernel<CTMAX, true>), grid, block, 0, s, q, q_bs, gdo, gdo_bs, k, k_bs, v, v_bs, lse,
                           delta, N, Npad, C, r, dq);
    });
    GD_LAUNCH_CHECK();
    return 0;
}
