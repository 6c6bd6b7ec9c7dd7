// Shared device helpers for the GAN-DANet gfx950 kernels (CDNA4, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GD_WAVE 64

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;   // 8 bf16 = 4 VGPR (MFMA A/B fragment)
typedef __attribute__((ext_vector_type(4))) short bf16x4_t;   // 4 bf16 = 2 VGPR
typedef __attribute__((ext_vector_type(16))) float f32x16_t;  // 32x32 accumulator fragment
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// ---- bf16 <-> f32 ---------------------------------------------------------------------------
// round-to-nearest-even; NaN stays NaN (plain cast lowers to v_cvt_pk_bf16_f32 on gfx950)
__device__ __forceinline__ unsigned short gd_f2bf(float f) {
    __bf16 h = (__bf16)f;
    return __builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float gd_bf2f(unsigned short h) {
    return __builtin_bit_cast(float, ((unsigned int)h) << 16);
}
typedef float gd_f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 gd_bf16x2_t __attribute__((ext_vector_type(2)));
// two floats -> one dword of two bf16 (lo in bits 0..15): a vector convert lowers to ONE v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned int gd_pack_bf2(float lo, float hi) {
    const gd_f32x2_t v = {lo, hi};
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, gd_bf16x2_t));
}
// split-bf16 ("x3" operands, set_precision("mixed")): v = hi + lo with hi = bf16(v), lo = bf16(v - hi): 16 mantissa bits.
// Two values per dword like gd_pack_bf2.  A product of two split operands is hi*hi + lo*hi + hi*lo (+ 2^-16 relative).
__device__ __forceinline__ void gd_split_bf2(float a, float b, unsigned int& hi, unsigned int& lo) {
    hi = gd_pack_bf2(a, b);
    lo = gd_pack_bf2(a - __builtin_bit_cast(float, hi << 16), b - __builtin_bit_cast(float, hi & 0xffff0000u));
}
__device__ __forceinline__ void gd_split_bf(float a, unsigned short& hi, unsigned short& lo) {
    hi = gd_f2bf(a);
    lo = gd_f2bf(a - gd_bf2f(hi));
}
// raw v_exp_f32 (2^x) without the denormal-range fix-up sequence exp2f() expands to; callers pass x <= ~0
__device__ __forceinline__ float gd_exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

// ---- wave / block reductions ----------------------------------------------------------------
__device__ __forceinline__ float gd_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float gd_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double gd_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum of one float; `red` = LDS scratch of >= blockDim/64 floats; result valid in ALL threads
__device__ __forceinline__ float gd_block_sum(float v, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = gd_wave_sum(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < nw; ++i) r += red[i];
    return r;
}
__device__ __forceinline__ float gd_block_max(float v, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = gd_wave_max(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < nw; ++i) r = fmaxf(r, red[i]);
    return r;
}

// ---- error plumbing for the C ABI -------------------------------------------------------------
extern "C" void gd_set_error(const char* msg);
extern "C" int gd_get_deterministic(void);   // api.hip: 1 = no order-dependent (atomic) reductions
extern "C" int gd_get_det_reduce(void);      // api.hip: 1 = "ordered" (split partial slabs + ordered sum) while deterministic
// det_reduce.hip: out[b * c_bs + m * ldc + n] (+)= sum over the `splits` dense [B][M][N] slabs of `part`, ascending, + bias[n]
int gd_det_reduce_launch(const float* part, int splits, float* out, int B, int M, int N, long c_bs, long ldc,
                         const float* bias, int accumulate, hipStream_t s);
// slabs [split][Ci][Co][10] -> dw (Co, Ci, 3, 3), db (Co) or NULL
int gd_det_reduce_stem_launch(const float* part, int splits, int Ci, int Co, float* dw, float* db, hipStream_t s);
// true when a split reduction may use the ordered form with this workspace
static inline bool gd_det_ordered(const void* ws) { return ws && gd_get_deterministic() && gd_get_det_reduce() == 1; }
// Outside deterministic mode (api.hip): 0 = the default, partial slabs in the library's own workspace + the ordered sum;
// 1 = fp32 atomics onto the zeroed output.
extern "C" int gd_get_split_reduce(void);
// true when a split reduction outside deterministic mode takes the slab form
static inline bool gd_split_own() { return !gd_get_deterministic() && gd_get_split_reduce() == 0; }
// det_reduce.hip: the library's slab workspace of the current device and this stream, grown to the largest request and
// kept (16-byte aligned; NULL when the allocation fails).  Uses on one stream are stream-ordered; two streams never share.
void* gd_split_ws(size_t bytes, hipStream_t s);
// a default-mode reduction takes at most this many bytes of slabs; its split count is clamped to fit (as a caller's
// workspace clamps the deterministic ordered form: 256 MiB is that mode's default too, so the two agree bit for bit)
static const size_t GD_SPLIT_WS_CAP = (size_t)256 << 20;
#define GD_CHECK_ARG(cond, msg)          \
    do {                                 \
        if (!(cond)) {                   \
            gd_set_error(msg);           \
            return -1;                   \
        }                                \
    } while (0)
#define GD_LAUNCH_CHECK()                                   \
    do {                                                    \
        hipError_t e_ = hipGetLastError();                  \
        if (e_ != hipSuccess) {                             \
            gd_set_error(hipGetErrorString(e_));            \
            return -2;                                      \
        }                                                   \
    } while (0)

static inline int gd_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
