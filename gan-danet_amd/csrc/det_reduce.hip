// Ordered reduction of split partials: the default form of every split reduction outside PAM, and the "ordered"
// deterministic mode (gd_set_det_reduce(1)).
//
// A split kernel (3x3 weight gradient, split-K NT GEMM, Discriminator1's stem weight gradient, the NHWC -> NCHW
// transposer's channel sums) writes the partial result of split s with plain stores into slab s of a caller-owned
// workspace; the kernels here add the slabs in ascending split order, in fp32, one thread per output element (or per
// four contiguous ones), and write -- or, with accumulate, add onto -- the real output.  No atomics, no hand-offs: the
// second stream-ordered launch is the whole synchronisation, and the order of the additions is a function of the
// shapes alone.  HBM-bound: every partial is read once.  The output is never read unless the caller accumulates, so it
// needs no zero-fill.
//
// Outside deterministic mode the slabs live in a workspace the library owns (gd_split_ws): one allocation per device and
// stream, grown to the largest request and kept.
#include "common.h"

#include <map>
#include <mutex>
#include <utility>

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// contiguous output of `total` floats (total % 4 == 0, 16-byte aligned slabs and output); bias[n], n = index % N, N % 4 == 0.
// One wave per workgroup and 1 KiB of contiguous output: the slabs are small (135 KB for a 184 x 184 weight gradient,
// summed over 340 splits), so a 256-thread block left most CUs without work and four loads per thread in flight left the
// others waiting on HBM latency.  A wave keeps VEC_U 16-byte loads per lane in flight (16 KiB) and adds them in ascending
// split order: the same chain of fp32 additions as one adder per element.
constexpr int VEC_T = 64, VEC_U = 16;
__global__ __launch_bounds__(VEC_T) void det_reduce_vec_kernel(const float* __restrict__ part, int splits, long slab,
                                                              float* __restrict__ out, long total, const float* __restrict__ bias,
                                                              int N, int accumulate) {
    const long i = ((long)blockIdx.x * VEC_T + threadIdx.x) * 4;
    if (i >= total) return;
    const float* p = part + i;
    f32x4_t v = *reinterpret_cast<const f32x4_t*>(p);
    int s = 1;
    for (; s + VEC_U <= splits; s += VEC_U) {
        f32x4_t t[VEC_U];
#pragma unroll
        for (int u = 0; u < VEC_U; ++u) t[u] = *reinterpret_cast<const f32x4_t*>(p + (long)(s + u) * slab);
#pragma unroll
        for (int u = 0; u < VEC_U; ++u) v += t[u];
    }
    for (; s + 3 < splits; s += 4) {                    // four loads in flight, added in ascending order
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p + (long)s * slab);
        const f32x4_t b = *reinterpret_cast<const f32x4_t*>(p + (long)(s + 1) * slab);
        const f32x4_t c = *reinterpret_cast<const f32x4_t*>(p + (long)(s + 2) * slab);
        const f32x4_t d = *reinterpret_cast<const f32x4_t*>(p + (long)(s + 3) * slab);
        v += a; v += b; v += c; v += d;
    }
    for (; s < splits; ++s) v += *reinterpret_cast<const f32x4_t*>(p + (long)s * slab);
    if (bias) v += *reinterpret_cast<const f32x4_t*>(bias + (int)(i % N));
    if (accumulate) v += *reinterpret_cast<const f32x4_t*>(out + i);
    *reinterpret_cast<f32x4_t*>(out + i) = v;
}

// general form: dense [split][B][M][N] slabs -> out[b * c_bs + m * ldc + n]
__global__ __launch_bounds__(256) void det_reduce_strided_kernel(const float* __restrict__ part, int splits, long slab,
                                                                float* __restrict__ out, int B, int M, int N, long c_bs,
                                                                long ldc, const float* __restrict__ bias, int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= slab) return;
    const int n = (int)(i % N);
    const long t = i / N;
    const int m = (int)(t % M);
    const int b = (int)(t / M);
    float v = part[i];
    for (int s = 1; s < splits; ++s) v += part[(long)s * slab + i];
    if (bias) v += bias[n];
    float* o = out + (long)b * c_bs + (long)m * ldc + n;
    if (accumulate) v += *o;
    *o = v;
}

// Discriminator1's stem: slabs [split][ci][co][10] (nine taps + the plain sum) -> dw[co][ci][tap], db[co] (from ci == 0)
__global__ __launch_bounds__(256) void det_reduce_stem_kernel(const float* __restrict__ part, int splits, int Ci, int Co,
                                                             float* __restrict__ dw, float* __restrict__ db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int slab = Ci * Co * 10;
    if (i >= slab) return;
    const int t = i % 10, co = (i / 10) % Co, ci = i / (10 * Co);
    float v = part[i];
    for (int s = 1; s < splits; ++s) v += part[(long)s * slab + i];
    if (t < 9) dw[((long)co * Ci + ci) * 9 + t] = v;
    else if (ci == 0 && db) db[co] = v;
}

struct SplitWs { void* p = nullptr; size_t bytes = 0; };
std::mutex g_ws_mutex;
std::map<std::pair<int, hipStream_t>, SplitWs> g_ws;      // (device, stream) -> slabs

}  // namespace

void* gd_split_ws(size_t bytes, hipStream_t s) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    SplitWs& w = g_ws[std::make_pair(dev, s)];
    if (w.bytes < bytes) {
        if (w.p) (void)hipFree(w.p);                      // waits for the kernels that still use it
        w.p = nullptr; w.bytes = 0;
        if (hipMalloc(&w.p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            w.p = nullptr;
            return nullptr;
        }
        w.bytes = bytes;
    }
    return w.p;
}

// bytes of slab workspace the library holds, over all devices and streams
extern "C" size_t gd_split_ws_bytes(void) {
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    size_t n = 0;
    for (const auto& kv : g_ws) n += kv.second.bytes;
    return n;
}

int gd_det_reduce_launch(const float* part, int splits, float* out, int B, int M, int N, long c_bs, long ldc,
                         const float* bias, int accumulate, hipStream_t s) {
    const long slab = (long)B * M * N;
    const bool dense = ldc == N && (B == 1 || c_bs == (long)M * N);
    if (dense && slab % 4 == 0 && (!bias || N % 4 == 0) && ((uintptr_t)part % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
        (!bias || ((uintptr_t)bias % 16) == 0)) {
        const long blocks = (slab / 4 + VEC_T - 1) / VEC_T;
        hipLaunchKernelGGL(det_reduce_vec_kernel, dim3((unsigned)blocks), dim3(VEC_T), 0, s, part, splits, slab, out, slab, bias, N,
                           accumulate);
    } else {
        const long blocks = (slab + 255) / 256;
        hipLaunchKernelGGL(det_reduce_strided_kernel, dim3((unsigned)blocks), dim3(256), 0, s, part, splits, slab, out, B, M, N,
                           c_bs, ldc, bias, accumulate);
    }
    GD_LAUNCH_CHECK();
    return 0;
}

int gd_det_reduce_stem_launch(const float* part, int splits, int Ci, int Co, float* dw, float* db, hipStream_t s) {
    hipLaunchKernelGGL(det_reduce_stem_kernel, dim3((Ci * Co * 10 + 255) / 256), dim3(256), 0, s, part, splits, Ci, Co, dw, db);
    GD_LAUNCH_CHECK();
    return 0;
}
