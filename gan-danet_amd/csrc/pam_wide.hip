// Fused (flash-style) PAM for attention widths past the narrow kernels' 192 value channels: 193 <= C <= 511
// (generator.py:115-122 at the widths FlexibleUpsamplingModule reaches with a larger growth_rate / num_layers_per_block).
//
// Same operand contract as pam.hip (q pre-scaled by log2 e, S tiles in the log2 domain, fp32 softmax statistics), with
//   * q / k padded to D = 32 (r <= 31) or D = 64 (32 <= r <= 63) slots; k carries 1.0 in the spare slot D - 1, through
//     which the forward feeds its running maximum (-m in the Q fragment);
//   * V split along its channels into chunks of at most 192 (the narrow forward's register ceiling).
// Forward: one launch per V chunk, each the LDS-DMA running-maximum sweep of pam_fwd_dma_kernel over ALL keys for its
//   channels.  Every chunk recomputes S and the softmax in the same order, so m and l agree in every chunk; chunk 0
//   writes the LSE.  The denominator is a VALU row sum (a chunk has no spare padded channel for a ones row).
// Backward: two key-parallel kernels, 4 waves x 32 keys per workgroup, queries swept in 32-row tiles:
//   dkq : dP = dO V^T over all Cp channels (this wave's V rows live in registers as the MFMA B operand, the dO tile
//         is staged in LDS), dS = P (dP - delta), dK^T += Q^T dS, dQ^T part = K^T dS^T per workgroup -> fp32 atomics,
//         or (deterministic) bf16 parts per key block summed by pam_dq_reduce_kernel.
//   dv  : one launch per V chunk: P recomputed from q, k and the LSE, dV^T += dO^T P with the chunk of dV^T in the
//         accumulation registers.  No dP, no dS.
// No N x N buffer anywhere: memory is O(N (D + Cp)) per image.
#include <stdlib.h>

#include "pam_common.h"
#include "../../include/gandanet.h"

namespace {

using namespace pam;

// =====================================================================================================
// forward: one V chunk of CT x 32 channels (chunk origin c0 inside the padded Cp rows of v)
// =====================================================================================================
template <int CT, int D, int KT, bool F16>
__global__ __launch_bounds__(512, 2) void pam_wide_fwd_kernel(const unsigned short* __restrict__ qt,
                                                             const unsigned short* __restrict__ kt,
                                                             const unsigned short* __restrict__ v, long v_bs, int c0,
                                                             int N, int Npad, int C, const float* __restrict__ gamma,
                                                             const float* __restrict__ x, long x_bs,
                                                             float* __restrict__ out, long out_bs,
                                                             float* __restrict__ o_attn, float* __restrict__ lse) {
    constexpr int NW = 8;
    constexpr int CP = CT * 32;
    constexpr int NKS = D / 16;                     // 16-wide k-steps of an S tile
    constexpr int KROWCH = D / 8 + 1;               // 16-byte chunks per K row in LDS (data + 1 pad)
    constexpr int KLD = D + 8;
    constexpr int NSUB = KT / 32;
    constexpr int VROWCH = KT / 8 + 1;
    constexpr int VLD = KT + 8;
    constexpr int KCH = KT * KROWCH;
    constexpr int NCH = KCH + CP * VROWCH;
    constexpr int NPIECE = (NCH + 63) / 64;
    constexpr int PPW = (NPIECE + NW - 1) / NW;
    constexpr int TILE = NPIECE * 64 * 8;
    static_assert(KCH % 64 == 0, "a DMA piece must be all-K or all-V");
    __shared__ __attribute__((aligned(16))) unsigned short ring[2 * TILE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * (NW * 32) + wave * 32;
    const unsigned short* ktb = kt + (long)b * Npad * D;
    const unsigned short* vb = v + (long)b * v_bs + (long)c0 * Npad;

    bf16x8_t qf[NKS];
#pragma unroll
    for (int s = 0; s < NKS; ++s)
        qf[s] = *reinterpret_cast<const bf16x8_t*>(qt + ((long)b * Npad + q0 + r) * D + s * 16 + 8 * h);

    // DMA plan: byte offset of this lane's chunk inside the tile's K / V source (see pam_fwd_dma_kernel)
    unsigned int voff[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int piece = wave + NW * i;
        const int c = piece * 64 + lane;
        if (piece * 64 < KCH) {
            const int row = c / KROWCH, part = c - row * KROWCH;
            voff[i] = (unsigned int)(row * D + (part < D / 8 ? part : D / 8 - 1) * 8) * 2u;
        } else {
            const int c2 = (c < NCH ? c : NCH - 1) - KCH;
            const int row = c2 / VROWCH, part = c2 - row * VROWCH;
            voff[i] = ((unsigned int)row * (unsigned int)Npad + (unsigned int)(part < KT / 8 ? part : KT / 8 - 1) * 8u) * 2u;
        }
    }
    auto dma_tile = [&](int t, int slot) {
        const char* kbase = reinterpret_cast<const char*>(ktb + (long)t * (KT * D));
        const char* vbase = reinterpret_cast<const char*>(vb + (long)t * KT);
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int piece = wave + NW * i;
            if (piece < NPIECE && piece * 64 + lane < NCH) {
                unsigned short* dst = ring + slot * TILE + piece * 512;
                const char* base = piece * 64 < KCH ? kbase : vbase;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + voff[i]),
                                                 (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
            }
        }
    };

    f32x16_t o[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[ct][e] = 0.f;
    float m = 0.f, l = 0.f;
    const int nkt = (N + KT - 1) / KT;

    dma_tile(0, 0);
    for (int t = 0; t < nkt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the DMA wait is ours to place (see pam_fwd_dma_kernel)
        __syncthreads();
        if (t + 1 < nkt) dma_tile(t + 1, (t + 1) & 1);
        const unsigned short* Ks = ring + (t & 1) * TILE;
        const unsigned short* Vs = Ks + KCH * 8;

        f32x16_t sacc[NSUB];
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
#pragma unroll
            for (int e = 0; e < 16; ++e) sacc[sub][e] = 0.f;
#pragma unroll
            for (int s = 0; s < NKS; ++s) {
                const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(Ks + (sub * 32 + r) * KLD + s * 16 + 8 * h);
                sacc[sub] = mfma16<F16>(kf, qf[s], sacc[sub]);
            }
        }
        if ((t + 1) * KT > N) {
#pragma unroll
            for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if ((t * KT + sub * 32 + acc_row(e, h)) >= N) sacc[sub][e] = -1e30f;
        }
        float mloc = sacc[0][0];
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
            for (int e = 0; e < 16; ++e) mloc = fmaxf(mloc, sacc[sub][e]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        float shift = 0.f;
        if (t == 0 || __any(mloc > 0.f)) {
            // new maximum, rounded UP to the operand type so that it passes through the Q fragment exactly
            const float want = m + (t == 0 ? mloc : fmaxf(mloc, 0.f));
            float m_new;
            unsigned short m_neg16;
            if constexpr (F16) {
                _Float16 hm = (_Float16)want;
                unsigned short hb = __builtin_bit_cast(unsigned short, hm);
                if ((float)hm < want) hb = (hb & 0x8000u) ? (unsigned short)(hb - 1) : (unsigned short)(hb + 1);
                m_new = (float)__builtin_bit_cast(_Float16, hb);
                m_neg16 = hb ^ 0x8000u;
            } else {
                const unsigned int wb = __builtin_bit_cast(unsigned int, want);
                m_new = __builtin_bit_cast(float, want > 0.f ? (wb + 0xFFFFu) & 0xFFFF0000u : wb & 0xFFFF0000u);
                m_neg16 = (unsigned short)(__builtin_bit_cast(unsigned int, -m_new) >> 16);
            }
            shift = m_new - m;
            if (t != 0) {
                const float alpha = gd_exp2_fast(-shift);
                l *= alpha;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int e = 0; e < 16; ++e) o[ct][e] *= alpha;
            }
            m = m_new;
            if (h) qf[NKS - 1][7] = (short)m_neg16;   // slot d = D - 1 lives in lane half 1
        }
        float lsum = 0.f;
        bf16x8_t pf[NSUB][2];     // P^T tile as the B operand of O^T += V P^T
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                sacc[sub][e] = gd_exp2_fast(sacc[sub][e] - shift);
                lsum += sacc[sub][e];
            }
            pf[sub][0] = pam::pack_frag<F16>(sacc[sub], 0);
            pf[sub][1] = pam::pack_frag<F16>(sacc[sub], 1);
        }
        lsum += __shfl_xor(lsum, 32, 64);
        l += lsum;

#pragma unroll
        for (int ks = 0; ks < 2 * NSUB; ++ks) {
            const int sub = ks >> 1, s2 = ks & 1;
            bf16x8_t vf[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                vf[ct] = *reinterpret_cast<const bf16x8_t*>(Vs + (ct * 32 + r) * VLD + sub * 32 + s2 * 16 + 8 * h);
            __builtin_amdgcn_sched_group_barrier(0x100, CT, 0);   // DS reads
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) o[ct] = mfma16<F16>(vf[ct], pf[sub][s2], o[ct]);
            __builtin_amdgcn_sched_group_barrier(0x008, CT, 0);   // MFMAs
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
        if (c0 == 0 && h == 0) lse[(long)b * N + qi] = (m + log2f(l)) * LN2;   // natural-log LSE of the UNSCALED energies
    }
}

// =====================================================================================================
// backward staging shared by both kernels: the 32-query Q tile [i][D] and a 32-query dO tile of CP channels from
// column c0 of dot_ (row length ld) go global -> registers (one tile ahead) -> LDS, with -LSE (log2 domain) and
// -delta for the 32 queries.  Chunk k of thread tid is tile chunk tid + 256 k: the first QCH chunks are Q, then dO.
// =====================================================================================================
template <int D, int CP, bool SWZ>
struct Stage {
    static constexpr int NT = 256;
    static constexpr int QLD = D + 8;                        // odd number of 16-byte units per row
    static constexpr int DOLD = SWZ ? CP + 32 : CP + 8;      // SWZ: pam.hip's chunk-swizzled image (transpose reads)
    static constexpr int QCH = 32 * D / 8, DCH = 32 * CP / 8, NCHUNK = QCH + DCH;
    static constexpr int NPRE = (NCHUNK + NT - 1) / NT;
    u32x4_t pre[NPRE];
    float pre_s;

    __device__ __forceinline__ void load(const unsigned short* qt, const unsigned short* dot_, long ld, int c0, long nb,
                                         int i0, const float* lse_b, const float* delta_b, int N, int tid) {
#pragma unroll
        for (int k = 0; k < NPRE; ++k) {
            const int c = tid + k * NT;
            if (NCHUNK % NT == 0 || c < NCHUNK) {
                const unsigned short* src;
                if (c < QCH) {
                    src = qt + (nb + i0 + c / (D / 8)) * D + (c % (D / 8)) * 8;
                } else {
                    const int c2 = c - QCH, i = c2 / (CP / 8), ch = c2 - i * (CP / 8);
                    src = dot_ + (nb + i0 + i) * ld + c0 + ch * 8;
                }
                pre[k] = *reinterpret_cast<const u32x4_t*>(src);
            }
        }
        pre_s = 0.f;
        if (tid < 64) {
            const int i = i0 + (tid & 31);
            if (i < N) pre_s = tid < 32 ? -lse_b[i] * LOG2E : (delta_b ? -delta_b[i] : 0.f);
        }
    }
    __device__ __forceinline__ void store(unsigned short* Qs, unsigned short* dOs, float* Ls, float* Ds, int tid) const {
#pragma unroll
        for (int k = 0; k < NPRE; ++k) {
            const int c = tid + k * NT;
            if (NCHUNK % NT == 0 || c < NCHUNK) {
                unsigned short* dst;
                if (c < QCH) {
                    dst = Qs + (c / (D / 8)) * QLD + (c % (D / 8)) * 8;
                } else {
                    const int c2 = c - QCH, i = c2 / (CP / 8), ch = c2 - i * (CP / 8);
                    dst = dOs + (SWZ ? do_off(i, ch, DOLD) : i * DOLD + ch * 8);
                }
                *reinterpret_cast<u32x4_t*>(dst) = pre[k];
            }
        }
        if (tid < 32) Ls[tid] = pre_s;
        else if (tid < 64) Ds[tid - 32] = pre_s;
    }
};

// =====================================================================================================
// backward (a): dK^T and dQ over all Cp = CT x 32 channels; 4 waves x 32 keys, one wave per SIMD (the wave's V rows
// take up to 128 registers)
// =====================================================================================================
template <int CT, int D, bool F16>
__global__ __launch_bounds__(256, 1) void pam_wide_bwd_dkq_kernel(
    const unsigned short* __restrict__ qt, const unsigned short* __restrict__ kt, const unsigned short* __restrict__ kn,
    const unsigned short* __restrict__ vt, const unsigned short* __restrict__ dot_, const float* __restrict__ lse,
    const float* __restrict__ delta, int N, int Npad, float* __restrict__ dkn, float* __restrict__ dqn,
    unsigned short* __restrict__ dq_part) {
    constexpr int NW = 4, KEYS = 128;
    constexpr int CP = CT * 32, NKS = D / 16, DT = D / 32;
    using St = Stage<D, CP, false>;
    constexpr int XLD = 36;                         // dS^T rows [key][32 queries] (72 B: conflict-free 8-byte writes)
    constexpr int YLD = D + 1;                      // fp32 dQ part rows [query][D]
    __shared__ __attribute__((aligned(16))) unsigned short Qs[32 * St::QLD];
    __shared__ __attribute__((aligned(16))) unsigned short dOs[32 * St::DOLD];
    __shared__ __attribute__((aligned(16))) unsigned short Xs[NW * 32 * XLD];
    __shared__ float Ys[NW * 32 * YLD];
    __shared__ float Ls[32], Ds[32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int j0 = blockIdx.x * KEYS + wave * 32;
    const long nb = (long)b * Npad;

    bf16x8_t kfB[NKS];
#pragma unroll
    for (int s = 0; s < NKS; ++s) kfB[s] = *reinterpret_cast<const bf16x8_t*>(kt + (nb + j0 + r) * D + s * 16 + 8 * h);
    // K^T rows d of this wave's keys: the A operand of dQ^T[d][i] += K^T[d][j] dS^T[j][i] (kn is perm16 along the keys)
    bf16x8_t knA[DT][2];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int s = 0; s < 2; ++s)
            knA[dt][s] = *reinterpret_cast<const bf16x8_t*>(kn + ((long)b * D + 32 * dt + r) * Npad + j0 + s * 16 + 8 * h);
    // V rows of this wave's keys: the B operand of dP[i][j] = sum_c dO[i][c] V[j][c], all Cp channels
    bf16x8_t vf[2 * CT];
#pragma unroll
    for (int s = 0; s < 2 * CT; ++s) vf[s] = *reinterpret_cast<const bf16x8_t*>(vt + (nb + j0 + r) * CP + s * 16 + 8 * h);

    f32x16_t dkacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) dkacc[dt][e] = 0.f;

    const bool key_ok = (j0 + r) < N;
    const bool need_mask = (int)(blockIdx.x + 1) * KEYS > N;
    const int nqt = (N + 31) / 32;
    const float* lse_b = lse + (long)b * N;
    const float* delta_b = delta + (long)b * N;
    unsigned short* Xw = Xs + wave * 32 * XLD;
    float* Yw = Ys + wave * 32 * YLD;
    const int KB = Npad / KEYS;

    St st;
    st.load(qt, dot_, CP, 0, nb, 0, lse_b, delta_b, N, tid);
    st.store(Qs, dOs, Ls, Ds, tid);
    __syncthreads();

    for (int qtile = 0; qtile < nqt; ++qtile) {
        const int i0 = qtile * 32;
        if (qtile + 1 < nqt) st.load(qt, dot_, CP, 0, nb, i0 + 32, lse_b, delta_b, N, tid);

        f32x16_t sacc, dpacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            sacc[e] = Ls[acc_row(e, h)];
            dpacc[e] = Ds[acc_row(e, h)];
        }
#pragma unroll
        for (int s = 0; s < NKS; ++s)
            sacc = mfma16<F16>(*reinterpret_cast<const bf16x8_t*>(Qs + r * St::QLD + s * 16 + 8 * h), kfB[s], sacc);
        constexpr int FB = 8;   // dO fragments read in batches ahead of their MFMAs
#pragma unroll
        for (int s0 = 0; s0 < 2 * CT; s0 += FB) {
            bf16x8_t da[FB];
#pragma unroll
            for (int i = 0; i < FB; ++i)
                if (s0 + i < 2 * CT) da[i] = *reinterpret_cast<const bf16x8_t*>(dOs + r * St::DOLD + (s0 + i) * 16 + 8 * h);
#pragma unroll
            for (int i = 0; i < FB; ++i)
                if (s0 + i < 2 * CT) dpacc = mfma16<F16>(da[i], vf[s0 + i], dpacc);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) sacc[e] = gd_exp2_fast(sacc[e]);   // P (-lse log2 e was the accumulator input)
        if (need_mask || i0 + 32 > N) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (!(key_ok && (i0 + acc_row(e, h)) < N)) sacc[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) dpacc[e] *= sacc[e];   // dS
        bf16x8_t dsf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) dsf[s] = pam::pack_frag<F16>(dpacc, s);
        // dS tile [query rows][key lanes] -> X[key][query] (wave-private), read back transposed for dQ^T
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const u32x4_t w = __builtin_bit_cast(u32x4_t, dsf[s]);
            const u32x2_t lo = {w.x, w.y}, hi = {w.z, w.w};
            *reinterpret_cast<u32x2_t*>(Xw + r * XLD + 16 * s + 4 * h) = lo;
            *reinterpret_cast<u32x2_t*>(Xw + r * XLD + 16 * s + 8 + 4 * h) = hi;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                dkacc[dt] = mfma16<F16>(read_tr_frag(Qs, St::QLD, s, 32 * dt, lane), dsf[s], dkacc[dt]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            f32x16_t dqp;
#pragma unroll
            for (int e = 0; e < 16; ++e) dqp[e] = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s) dqp = mfma16<F16>(knA[dt][s], read_tr_frag(Xw, XLD, s, 0, lane), dqp);
            // this wave's dQ^T part [d rows][query lanes] -> Y[query][d] (fp32)
#pragma unroll
            for (int e = 0; e < 16; ++e) Yw[r * YLD + 32 * dt + acc_row(e, h)] = dqp[e];
        }
        __syncthreads();
        // the NW waves' parts summed; item = (d, query), consecutive threads on consecutive queries
        for (int it = tid; it < 32 * D; it += 256) {
            const int q = it & 31, d = it >> 5;
            float acc = 0.f;
#pragma unroll
            for (int w4 = 0; w4 < NW; ++w4) acc += Ys[(w4 * 32 + q) * YLD + d];
            if (dq_part)
                dq_part[((((long)b * DT + (d >> 5)) * KB + blockIdx.x) * Npad + i0 + q) * 32 + (d & 31)] = gd_f2bf(acc);
            else if (i0 + q < N)
                atomicAdd(dqn + ((long)b * D + d) * Npad + i0 + q, acc);
        }
        if (qtile + 1 < nqt) st.store(Qs, dOs, Ls, Ds, tid);
        __syncthreads();
    }

    const int j = j0 + r;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e)
            dkn[((long)b * D + 32 * dt + acc_row(e, h)) * Npad + j] = dkacc[dt][e] * LN2;   // Q^T was q * log2 e
}

// =====================================================================================================
// backward (b): dV^T of one channel chunk (CT x 32 channels from c0); 4 waves x 32 keys, P recomputed from the LSE
// =====================================================================================================
template <int CT, int D, bool F16>
__global__ __launch_bounds__(256, 2) void pam_wide_bwd_dv_kernel(
    const unsigned short* __restrict__ qt, const unsigned short* __restrict__ kt, const unsigned short* __restrict__ dot_,
    int Cp_all, int c0, const float* __restrict__ lse, int N, int Npad, float* __restrict__ dv) {
    constexpr int KEYS = 128;
    constexpr int NKS = D / 16;
    using St = Stage<D, CT * 32, true>;
    __shared__ __attribute__((aligned(16))) unsigned short Qs[32 * St::QLD];
    __shared__ __attribute__((aligned(16))) unsigned short dOs[32 * St::DOLD];
    __shared__ float Ls[32], Ds[32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int j0 = blockIdx.x * KEYS + wave * 32;
    const long nb = (long)b * Npad;

    bf16x8_t kfB[NKS];
#pragma unroll
    for (int s = 0; s < NKS; ++s) kfB[s] = *reinterpret_cast<const bf16x8_t*>(kt + (nb + j0 + r) * D + s * 16 + 8 * h);
    f32x16_t dvacc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) dvacc[ct][e] = 0.f;

    const bool key_ok = (j0 + r) < N;
    const bool need_mask = (int)(blockIdx.x + 1) * KEYS > N;
    const int nqt = (N + 31) / 32;
    const float* lse_b = lse + (long)b * N;

    St st;
    st.load(qt, dot_, Cp_all, c0, nb, 0, lse_b, nullptr, N, tid);
    st.store(Qs, dOs, Ls, Ds, tid);
    __syncthreads();

    for (int qtile = 0; qtile < nqt; ++qtile) {
        const int i0 = qtile * 32;
        if (qtile + 1 < nqt) st.load(qt, dot_, Cp_all, c0, nb, i0 + 32, lse_b, nullptr, N, tid);
        f32x16_t sacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) sacc[e] = Ls[acc_row(e, h)];
#pragma unroll
        for (int s = 0; s < NKS; ++s)
            sacc = mfma16<F16>(*reinterpret_cast<const bf16x8_t*>(Qs + r * St::QLD + s * 16 + 8 * h), kfB[s], sacc);
#pragma unroll
        for (int e = 0; e < 16; ++e) sacc[e] = gd_exp2_fast(sacc[e]);
        if (need_mask || i0 + 32 > N) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (!(key_ok && (i0 + acc_row(e, h)) < N)) sacc[e] = 0.f;
        }
        bf16x8_t pf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) pf[s] = pam::pack_frag<F16>(sacc, s);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                dvacc[ct] = mfma16<F16>(read_tr_frag_sw(dOs, St::DOLD, s, ct, lane), pf[s], dvacc[ct]);
        __syncthreads();
        if (qtile + 1 < nqt) {
            st.store(Qs, dOs, Ls, Ds, tid);
            __syncthreads();
        }
    }

    const int j = j0 + r;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) dv[((long)b * Cp_all + c0 + ct * 32 + acc_row(e, h)) * Npad + j] = dvacc[ct][e];
}

}  // namespace

#define PAM_WIDE_DISPATCH_D(D_, ...)                            \
    do {                                                        \
        if ((D_) == 32) { constexpr int D = 32; __VA_ARGS__; }  \
        else { constexpr int D = 64; __VA_ARGS__; }             \
    } while (0)
#define PAM_WIDE_DISPATCH_ALL(CT_, ...)                          \
    switch (CT_) {                                               \
        case 7: { constexpr int CT = 7; __VA_ARGS__; } break;    \
        case 8: { constexpr int CT = 8; __VA_ARGS__; } break;    \
        case 9: { constexpr int CT = 9; __VA_ARGS__; } break;    \
        case 10: { constexpr int CT = 10; __VA_ARGS__; } break;  \
        case 11: { constexpr int CT = 11; __VA_ARGS__; } break;  \
        case 12: { constexpr int CT = 12; __VA_ARGS__; } break;  \
        case 13: { constexpr int CT = 13; __VA_ARGS__; } break;  \
        case 14: { constexpr int CT = 14; __VA_ARGS__; } break;  \
        case 15: { constexpr int CT = 15; __VA_ARGS__; } break;  \
        default: { constexpr int CT = 16; __VA_ARGS__; } break;  \
    }

static int pam_wide_check(int B, int N, int Npad, int Cp, int D) {
    GD_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && Npad >= N && Npad % 256 == 0, "gd_pam_wide: Npad must be a multiple of 256 >= N");
    GD_CHECK_ARG(Cp % 32 == 0 && Cp > 192 && Cp <= 512, "gd_pam_wide: Cp must be a multiple of 32, 192 < Cp <= 512");
    GD_CHECK_ARG(D == 32 || D == 64, "gd_pam_wide: D (q / k slots) must be 32 or 64");
    return 0;
}

extern "C" int gd_pam_wide_fwd(const void* qt, const void* kt, const void* v, int B, int N, int Npad, int C, int Cp, int D,
                               int f16, const float* gamma, const float* x, long x_bs, float* out, long out_bs,
                               float* o_attn, float* lse, void* stream) {
    GD_CHECK_ARG(qt && kt && v && gamma && x && out && o_attn && lse, "gd_pam_wide_fwd: null pointer");
    if (pam_wide_check(B, N, Npad, Cp, D)) return -1;
    GD_CHECK_ARG(C > Cp - 32 && C <= Cp, "gd_pam_wide_fwd: Cp must be C rounded up to a multiple of 32");
    hipStream_t s = (hipStream_t)stream;
    const Chunks ch(Cp / 32);
    const dim3 grid(Npad / 256, B), block(512);
    const unsigned short *q16 = (const unsigned short*)qt, *k16 = (const unsigned short*)kt, *v16 = (const unsigned short*)v;
    const long v_bs = (long)Cp * Npad;
    for (int i = 0; i < ch.n; ++i) {
        // 64-key tiles: at D = 64 and 6 channel tiles the 128-key form leaves no registers for the S tiles
#define PAM_WIDE_FWD_ARGS q16, k16, v16, v_bs, ch.c0[i], N, Npad, C, gamma, x, x_bs, out, out_bs, o_attn, lse
        PAM_WIDE_DISPATCH_D(D, PAM_DISPATCH_CT(ch.ct[i], if constexpr (CT >= 3) {
            if (f16) hipLaunchKernelGGL((pam_wide_fwd_kernel<CT, D, 64, true>), grid, block, 0, s, PAM_WIDE_FWD_ARGS);
            else hipLaunchKernelGGL((pam_wide_fwd_kernel<CT, D, 64, false>), grid, block, 0, s, PAM_WIDE_FWD_ARGS);
        }));
#undef PAM_WIDE_FWD_ARGS
    }
    GD_LAUNCH_CHECK();
    return 0;
}

// deterministic dQ: bf16 parts (D / 32, Npad / 128 key blocks, Npad, 32) per image
extern "C" size_t gd_pam_wide_scratch_bytes(int Npad, int D, int deterministic) {
    if (!deterministic) return 0;
    return (size_t)(D / 32) * (size_t)(Npad / 128) * (size_t)Npad * 32 * sizeof(unsigned short);
}

extern "C" int gd_pam_wide_bwd(const void* qt, const void* kt, const void* kn, const void* vt, const void* dot_,
                               const float* lse, const float* delta, int B, int N, int Npad, int Cp, int D, int f16,
                               int deterministic, float* dqn, float* dkn, float* dv, void* scratch, size_t scratch_bytes,
                               void* stream) {
    GD_CHECK_ARG(qt && kt && kn && vt && dot_ && lse && delta && dqn && dkn && dv, "gd_pam_wide_bwd: null pointer");
    if (pam_wide_check(B, N, Npad, Cp, D)) return -1;
    hipStream_t s = (hipStream_t)stream;
    const unsigned short *q = (const unsigned short*)qt, *k = (const unsigned short*)kt, *kT = (const unsigned short*)kn;
    const unsigned short *v = (const unsigned short*)vt, *dO = (const unsigned short*)dot_;
    const size_t per_image = gd_pam_wide_scratch_bytes(Npad, D, deterministic);
    int slice = B;
    if (deterministic) {
        GD_CHECK_ARG(scratch && scratch_bytes >= per_image, "gd_pam_wide_bwd: scratch smaller than gd_pam_wide_scratch_bytes (one image)");
        slice = (int)(scratch_bytes / per_image < (size_t)B ? scratch_bytes / per_image : (size_t)B);
    } else {
        GD_CHECK_ARG(hipMemsetAsync(dqn, 0, (size_t)B * D * Npad * sizeof(float), s) == hipSuccess, "gd_pam_wide_bwd: memset failed");
    }
    for (int b0 = 0; b0 < B; b0 += slice) {   // the batch is walked in slices that fit the caller's scratch
        const int nb = B - b0 < slice ? B - b0 : slice;
        const long oD = (long)b0 * Npad * D, oc = (long)b0 * Npad * Cp, on = (long)b0 * N;
        unsigned short* part = deterministic ? (unsigned short*)scratch : nullptr;
        PAM_WIDE_DISPATCH_D(D, PAM_WIDE_DISPATCH_ALL(Cp / 32, {
            if (f16)
                hipLaunchKernelGGL((pam_wide_bwd_dkq_kernel<CT, D, true>), dim3(Npad / 128, nb), dim3(256), 0, s, q + oD, k + oD,
                                   kT + oD, v + oc, dO + oc, lse + on, delta + on, N, Npad, dkn + oD, dqn + oD, part);
            else
                hipLaunchKernelGGL((pam_wide_bwd_dkq_kernel<CT, D, false>), dim3(Npad / 128, nb), dim3(256), 0, s, q + oD, k + oD,
                                   kT + oD, v + oc, dO + oc, lse + on, delta + on, N, Npad, dkn + oD, dqn + oD, part);
        }));
        if (deterministic) gd_pam_dq_reduce_launch(part, Npad / 128, Npad, nb * (D / 32), dqn + oD, stream);
    }
    const Chunks ch(Cp / 32);
    for (int i = 0; i < ch.n; ++i) {
        PAM_WIDE_DISPATCH_D(D, PAM_DISPATCH_CT(ch.ct[i], if constexpr (CT >= 3) {
            if (f16)
                hipLaunchKernelGGL((pam_wide_bwd_dv_kernel<CT, D, true>), dim3(Npad / 128, B), dim3(256), 0, s, q, k, dO, Cp,
                                   ch.c0[i], lse, N, Npad, dv);
            else
                hipLaunchKernelGGL((pam_wide_bwd_dv_kernel<CT, D, false>), dim3(Npad / 128, B), dim3(256), 0, s, q, k, dO, Cp,
                                   ch.c0[i], lse, N, Npad, dv);
        }));
    }
    GD_LAUNCH_CHECK();
    return 0;
}
