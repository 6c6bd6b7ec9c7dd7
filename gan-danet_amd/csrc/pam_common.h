// Helpers shared by the PAM kernels (pam*.hip): 16-bit MFMA wrappers for both operand types
// (bf16 = the training default, f16 = BASELINE config 5), accumulator-as-operand packing, LDS transpose reads.
#pragma once
#include "common.h"
#include "tile_mma.h"

namespace pam {

using gd::acc_row;
using gd::bf16x8_native_t;

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));   // staging registers: first-class vectors, never
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));   // demoted to scratch like arrays of uint4 structs
typedef _Float16 f16x8_native_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_native_t __attribute__((ext_vector_type(2)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// D = A B + C on 32x32x16 tiles; operands are 8 x 16-bit per lane (bf16 or f16 bit patterns in a short8)
template <bool F16>
__device__ __forceinline__ f32x16_t mfma16(bf16x8_t a, bf16x8_t b, f32x16_t c) {
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_native_t, a),
                                                      __builtin_bit_cast(f16x8_native_t, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_native_t, a),
                                                       __builtin_bit_cast(bf16x8_native_t, b), c, 0, 0, 0);
}

// two floats -> one dword of two 16-bit values (lo in bits 0..15), round to nearest even
template <bool F16>
__device__ __forceinline__ unsigned int pack2(float lo, float hi) {
    if constexpr (F16) {
        const gd_f32x2_t v = {lo, hi};
        return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, f16x2_native_t));
    } else {
        return gd_pack_bf2(lo, hi);
    }
}
template <bool F16>
__device__ __forceinline__ float unpack_lo(unsigned int w) {
    if constexpr (F16) return (float)__builtin_bit_cast(f16x2_native_t, w)[0];
    else return gd_bf2f((unsigned short)(w & 0xFFFFu));
}
template <bool F16>
__device__ __forceinline__ float unpack_hi(unsigned int w) {
    if constexpr (F16) return (float)__builtin_bit_cast(f16x2_native_t, w)[1];
    else return gd_bf2f((unsigned short)(w >> 16));
}

// registers 8s..8s+7 of a 32x32 accumulator -> the 16-bit fragment of k-step s (k = accumulator ROW index,
// element j of lane half h <-> row 16s + 8(j>>2) + 4h + (j&3))
template <bool F16>
__device__ __forceinline__ bf16x8_t pack_frag(const f32x16_t& a, int s) {
    const u32x4_t w = {pack2<F16>(a[8 * s + 0], a[8 * s + 1]), pack2<F16>(a[8 * s + 2], a[8 * s + 3]),
                       pack2<F16>(a[8 * s + 4], a[8 * s + 5]), pack2<F16>(a[8 * s + 6], a[8 * s + 7])};
    return __builtin_bit_cast(bf16x8_t, w);
}

__device__ __forceinline__ s16x4_t lds_tr16(const unsigned short* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
}
// A fragment (row = column c of X, k = accumulator-row-ordered query index) of k-step s from X[i][c] (LDS, ld):
// element j of lane half h <-> query 16s + 8(j>>2) + 4h + (j&3)
__device__ __forceinline__ bf16x8_t read_tr_frag(const unsigned short* X, int ld, int s, int ccol, int lane) {
    const int li = lane & 15, hh = lane >> 5;
    const unsigned short* p = X + (16 * s + 4 * hh + (li >> 2)) * ld + ccol + 16 * ((lane >> 4) & 1) + 4 * (li & 3);
    const s16x4_t lo = lds_tr16(p);             // queries 16s + 4h + 0..3
    const s16x4_t hi = lds_tr16(p + 8 * ld);    // queries 16s + 8 + 4h + 0..3
    const bf16x8_t f = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return f;
}

// dO tile image: rows of DOLD = CP + 32 elements (448 B at CP = 192: 28 sixteen-byte units, 28 = 12 mod 16) with the
// 16-byte chunk index XOR-swizzled by (row >> 2) & 3.  Both ways the tile is read are then bank-conflict free:
//   plain 16-byte reads, 16 rows x one chunk per pass : units {0,12,8,4} (row & 3) + {c^0..c^3} (row >> 2) -> 16 distinct;
//   transpose reads, 4 rows x 4 chunks per 32-lane pass: units {0,12,8,4} + {g..g+3}              -> 16 distinct
// (with plain 400-byte rows the transpose reads ran 2-way conflicted on half the banks: PMC SQ_LDS_BANK_CONFLICT).
__device__ __forceinline__ int do_off(int row, int chunk, int ld) { return row * ld + ((chunk ^ ((row >> 2) & 3)) << 3); }
__device__ __forceinline__ bf16x8_t read_tr_frag_sw(const unsigned short* X, int ld, int s, int ct, int lane) {
    const int li = lane & 15, hh = lane >> 5;
    const int row = 16 * s + 4 * hh + (li >> 2);
    const int chunk = 4 * ct + 2 * ((lane >> 4) & 1) + ((li & 3) >> 1), sub = 4 * (li & 1);
    const s16x4_t lo = lds_tr16(X + do_off(row, chunk, ld) + sub);          // queries 16s + 4h + 0..3
    const s16x4_t hi = lds_tr16(X + do_off(row + 8, chunk, ld) + sub);      // queries 16s + 8 + 4h + 0..3
    const bf16x8_t f = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return f;
}

constexpr int B_QLD = 40;   // Q tile rows [i][32 d] (80 B): 16-B reads

// ---- exact-fp32 operands (pam_f32.hip, pam_probe.hip): v_mfma_f32_32x32x2_f32 on channel-major (rows, Npad) planes ----
namespace f32 {

__device__ __forceinline__ f32x16_t mfma_f32(float a, float b, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// one LDS-DMA wave-instruction: lane l's 16 bytes land at dst + 16 l (dst is wave-uniform)
__device__ __forceinline__ void dma16(const float* src, float* dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

__device__ __forceinline__ void zero16(f32x16_t& a) {
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = 0.f;
}

constexpr float MASKED = 1e30f;
constexpr int MAXKS = 32;          // k-steps of the q.k product: r <= 63 -> (r + 1) / 2 <= 32

// S tile: acc += A_tile^T-rows x own fragment, A read from an LDS region of rows [d][ld floats] at column ``col``; k-steps in
// groups of four (reads first, then the MFMAs); rows past the last k-step are clamped (their B operand is zero or unused)
template <int LD>
__device__ __forceinline__ void s_tile(f32x16_t& acc, const float* rows, int col, int h, int nks, const float (&own)[MAXKS]) {
    const int last = 2 * nks - 1;
#pragma unroll
    for (int g = 0; g < MAXKS / 4; ++g) {
        if (4 * g < nks) {
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = rows[min(2 * (4 * g + j) + h, last) * LD + col];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * g + j < nks) acc = mfma_f32(a[j], own[4 * g + j], acc);
        }
    }
}

// key tiles of the query-parallel sweeps: 64 keys per tile, rows [channel][F_LD floats]
constexpr int F_KT = 64;            // keys per tile
constexpr int F_LD = 68;            // LDS row: 64 keys + 4 pad floats (17 sixteen-byte chunks, the last a repeat)
constexpr int F_RCH = 17;
constexpr int F_KPIECE = 17;        // 1 KiB DMA pieces of the K region (64 rows x 17 chunks / 64)

// streamed 32-column tiles of the owner-parallel sweeps: r region of 64 rows x 36 floats (8 data chunks + 1 pad chunk per row)
constexpr int B_RLD = 36, B_RCH = 9;
constexpr int B_RREG = 9 * 256;       // floats of the r region (64 rows x 9 chunks = 9 pieces)

__device__ __forceinline__ void bwd_dma_r(const float* src, int R, int nks, int ld, int y0, float* slot, int wave, int lane) {
    const int npiece = (2 * nks * B_RCH + 63) >> 6;
    for (int p = wave; p < npiece; p += 4) {
        const int c = p * 64 + lane;
        const int row = c / B_RCH, part = c - row * B_RCH;
        dma16(src + (long)min(row, R - 1) * ld + y0 + min(part, B_RCH - 2) * 4, slot + p * 256);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace f32

// ---- host side ----
// V channel chunks: `tiles` 32-channel tiles split into the fewest chunks of at most 6 tiles (the forward's register
// ceiling), as even as possible
struct Chunks {
    int n, ct[3], c0[3];
    explicit Chunks(int tiles) {
        n = (tiles + 5) / 6;
        int c = 0;
        for (int i = 0; i < n; ++i) {
            ct[i] = tiles / n + (i < tiles % n ? 1 : 0);
            c0[i] = c;
            c += ct[i] * 32;
        }
    }
};

}  // namespace pam

// runs the statement(s) with `constexpr int CT` = the number of 32-channel tiles of one launch, 1..6
#define PAM_DISPATCH_CT(CT_, ...)                                \
    switch (CT_) {                                               \
        case 1: { constexpr int CT = 1; __VA_ARGS__; } break;    \
        case 2: { constexpr int CT = 2; __VA_ARGS__; } break;    \
        case 3: { constexpr int CT = 3; __VA_ARGS__; } break;    \
        case 4: { constexpr int CT = 4; __VA_ARGS__; } break;    \
        case 5: { constexpr int CT = 5; __VA_ARGS__; } break;    \
        case 6: { constexpr int CT = 6; __VA_ARGS__; } break;    \
        default: gd_set_error("pam: Cp must be 32..192"); return -1; \
    }

// entry points that one PAM translation unit calls in another
extern "C" void gd_pam_dq_reduce_launch(const void* part, int KB, int Npad, int nb, float* dqn, void* stream);   // pam_bwd64.hip
extern "C" size_t gd_pam_bwd64_scratch_bytes(int Npad, int deterministic);                                       // pam_bwd64.hip
extern "C" int gd_pam_bwd64_slice(const void* qt, const void* kt, const void* kn, const void* vt, const void* dot_,
                                  const float* lse, const float* delta, int nb, int N, int Npad, int Cp, int f16,
                                  int deterministic, float* dqn, float* dkn, float* dv, long out_bs,
                                  void* scratch, void* stream);                                                  // pam_bwd64.hip
