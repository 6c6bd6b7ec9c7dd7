// Shared device and host plumbing of the pixel-major (NHWC) 16-bit activation kernels (nhwc.hip: the VGG19 feature stack
// of the perceptual term; disc_nhwc.hip: the Discriminator1 trunk): channel-octet (16-byte) access with the split
// [hi | lo | hi] layout, launch-grid sizing, and what the two 3x3 stem convolutions (fp32 NCHW image -> NHWC bf16) have in
// common -- the forward kernel and the first phase of the data gradient.  All HBM-bound, no MFMA.
#pragma once
#include "common.h"
#include "../../include/gandanet.h"

#define NS(s) ((hipStream_t)(s))

namespace {

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void unpack8(const u32x4_t v, float* f) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[2 * k] = gd_bf2f((unsigned short)(v[k] & 0xFFFFu));
        f[2 * k + 1] = gd_bf2f((unsigned short)(v[k] >> 16));
    }
}
__device__ __forceinline__ u32x4_t pack8(const float* f) {
    const u32x4_t v = {gd_pack_bf2(f[0], f[1]), gd_pack_bf2(f[2], f[3]), gd_pack_bf2(f[4], f[5]), gd_pack_bf2(f[6], f[7])};
    return v;
}
// bf16 > 0  <=>  sign clear and magnitude non-zero
__device__ __forceinline__ bool bf_pos(unsigned int h) { return (h & 0x7FFFu) && !(h & 0x8000u); }

// Split activations (set_precision("mixed"), operand mode "x3"; gd_pack_16_split makes the same layout): a pixel's C logical
// channels are stored as the 3 C bf16 [hi | lo | hi] with hi = bf16(v), lo = bf16(v - hi) -- the operand the pixel-major
// conv kernels take against weights split [hi ; hi ; lo] along the contraction axis.  store8 / load8 are the only readers
// and writers of that layout in these kernels.  `row` = the pixel's first element, c8 = the channel octet's first channel.
__device__ __forceinline__ void store8(unsigned short* row, int C, int c8, const float* v, int split) {
    const u32x4_t hi = pack8(v);
    *reinterpret_cast<u32x4_t*>(row + c8) = hi;
    if (split) {
        float r[8];
        unpack8(hi, r);
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = v[k] - r[k];
        *reinterpret_cast<u32x4_t*>(row + C + c8) = pack8(r);
        *reinterpret_cast<u32x4_t*>(row + 2 * C + c8) = hi;
    }
}
__device__ __forceinline__ void load8(const unsigned short* row, int C, int c8, float* v, int split) {
    unpack8(*reinterpret_cast<const u32x4_t*>(row + c8), v);
    if (split) {
        float l[8];
        unpack8(*reinterpret_cast<const u32x4_t*>(row + C + c8), l);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += l[k];
    }
}

static inline int grid_n(long n, int cap = 16384) {
    long g = (n + 255) / 256;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// ---- the stem convolutions: 3x3, pad 1, Ci <= 4 image channels, weights w (Co, Ci, 3, 3) fp32 ------------------------------
// the LDS image of the weights, [ci][tap][co] (an output-channel octet of one tap is contiguous); 256 threads, no barrier
__device__ __forceinline__ void stage_stem_weights(float* wl, const float* __restrict__ w, int Ci, int Co) {
    for (int i = threadIdx.x; i < Ci * 9 * Co; i += 256) {
        const int co = i % Co, t = (i / Co) % 9, ci = i / (9 * Co);
        wl[i] = w[((long)co * Ci + ci) * 9 + t];
    }
}

// LEAKY: LeakyReLU(slope); else ReLU where relu != 0
template <bool LEAKY> __device__ __forceinline__ void stem_act(float* acc, int relu, float slope) {
    if (LEAKY) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = acc[k] > 0.f ? acc[k] : acc[k] * slope;
    } else if (relu) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = fmaxf(acc[k], 0.f);
    }
}

// forward: img (B, Ci, H, W) fp32 -> act(conv3x3 stride STRIDE + bias) as (B, Ho, Wo, Co) bf16, Ho = (H - 1) / STRIDE + 1.
// <1, false> is the VGG stem (ReLU flag), <2, true> the Discriminator1 stem (LeakyReLU slope); the other argument is unused.
// thread = (output pixel, output-channel octet); npix_total = B * Ho * Wo
template <int STRIDE, bool LEAKY>
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ img, int Ci, int H, int W,
                                                      const float* __restrict__ w, const float* __restrict__ bias, int Co,
                                                      int relu, float slope, unsigned short* __restrict__ y, long npix_total,
                                                      int split) {
    extern __shared__ float wl[];                       // Ci * 9 * Co
    const int RS = split ? 3 * Co : Co;                 // elements per output pixel
    stage_stem_weights(wl, w, Ci, Co);
    __syncthreads();
    const int oct = Co / 8;
    const int Ho = (H - 1) / STRIDE + 1, Wo = (W - 1) / STRIDE + 1;
    const long HW = (long)H * W, HWo = (long)Ho * Wo;
    if (Ci == 1 && Co == 64) {
        // the common case (single-channel image, 64 filters): a thread's octet is fixed over the grid stride
        // (256 * gridDim.x is a multiple of 8), so its 9 x 8 weights and 8 biases live in registers -- the LDS-resident
        // form below spends 18 16-byte LDS reads per 16 bytes stored
        const int o8 = (threadIdx.x & 7) * 8;
        float wr[9][8], br[8];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int k = 0; k < 8; ++k) wr[t][k] = wl[t * 64 + o8 + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) br[k] = bias ? bias[o8 + k] : 0.f;
        for (long p = ((long)blockIdx.x * 256 + threadIdx.x) >> 3; p < npix_total; p += ((long)gridDim.x * 256) >> 3) {
            const long b = p / HWo;
            const int rem = (int)(p - b * HWo);
            const int py = rem / Wo, px = rem - py * Wo;
            const float* plane = img + b * HW;
            float acc[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = br[k];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = STRIDE * py + t / 3 - 1, ix = STRIDE * px + t % 3 - 1;
                const float v = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? plane[(long)iy * W + ix] : 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] = fmaf(v, wr[t][k], acc[k]);
            }
            stem_act<LEAKY>(acc, relu, slope);
            store8(y + p * RS, 64, o8, acc, split);
        }
        return;
    }
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < npix_total * oct; idx += (long)gridDim.x * 256) {
        const long p = idx / oct;
        const int o8 = (int)(idx - p * oct) * 8;
        const long b = p / HWo;
        const int rem = (int)(p - b * HWo);
        const int py = rem / Wo, px = rem - py * Wo;
        float acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = bias ? bias[o8 + k] : 0.f;
        for (int ci = 0; ci < Ci; ++ci) {
            const float* plane = img + (b * Ci + ci) * HW;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = STRIDE * py + t / 3 - 1, ix = STRIDE * px + t % 3 - 1;
                if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
                const float v = plane[(long)iy * W + ix];
                const float* wp = wl + (ci * 9 + t) * Co + o8;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] = fmaf(v, wp[k], acc[k]);
            }
        }
        stem_act<LEAKY>(acc, relu, slope);
        store8(y + p * RS, Co, o8, acc, split);
    }
}

// LDS bytes of a stem data-gradient kernel whose haloed tile is HT x HT pixels: the weights, then the T planes
static inline size_t stem_dgrad_lds(int Ci, int Co, int HT) { return ((size_t)Ci * 9 * Co + (size_t)Ci * 9 * HT * HT) * sizeof(float); }

// Phase 1 of both stem data gradients.  A workgroup (256 threads) owns a tile of gradient pixels plus a halo, HT x HT pixels
// with the first at (qy0, qx0) of image b of g (B, Hg, Wg, Co) bf16.  Every haloed pixel reads its Co gradient values ONCE
// and reduces them against the 9 Ci weight vectors into the LDS planes T[ci * 9 + tap][pixel] = sum_co g[pixel][co]
// w[co][ci][tap]; pixels outside the image give zeros.  smem = weights [ci][tap][co], then T (stem_dgrad_lds bytes);
// returns T, ready to read (a barrier has passed).  Phase 2, the gather over T, is the caller's.
template <int HT>
__device__ __forceinline__ const float* stem_dgrad_phase1(float* smem, const unsigned short* __restrict__ g,
                                                          const float* __restrict__ w, int b, int Hg, int Wg, int qy0, int qx0,
                                                          int Ci, int Co, int split) {
    constexpr int NH = HT * HT;
    const int RS = split ? 3 * Co : Co;
    float* wl = smem;
    float* T = smem + Ci * 9 * Co;
    stage_stem_weights(wl, w, Ci, Co);
    __syncthreads();
    for (int hp = threadIdx.x; hp < NH; hp += 256) {
        const int hy = hp / HT, hx = hp - hy * HT;
        const int qy = qy0 + hy, qx = qx0 + hx;
        const bool inside = qy >= 0 && qy < Hg && qx >= 0 && qx < Wg;
        for (int ci = 0; ci < Ci; ++ci) {
            float t[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) t[k] = 0.f;
            if (inside) {
                const unsigned short* gp = g + (((long)b * Hg + qy) * Wg + qx) * RS;
                for (int o8 = 0; o8 < Co; o8 += 8) {
                    float f[8];
                    load8(gp, Co, o8, f, split);
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        const float* wp = wl + (ci * 9 + k) * Co + o8;      // uniform address: LDS broadcast
#pragma unroll
                        for (int j = 0; j < 8; ++j) t[k] = fmaf(f[j], wp[j], t[k]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) T[(ci * 9 + k) * NH + hp] = t[k];
        }
    }
    __syncthreads();
    return T;
}

}  // namespace
