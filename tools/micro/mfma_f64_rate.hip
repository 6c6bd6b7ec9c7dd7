// Register-only v_mfma_f64_16x16x4_f64 loop: the fp64 matrix rate of the part, the floor of gd_eof_gram's arithmetic.
// Every wave keeps NACC independent accumulators busy from two operand registers; no memory traffic inside the loop.
// The figure is the rate of THIS loop at the clock the part held under it (the clock is not read), not a datasheet rate.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/mfma_f64_rate.hip -o tools/micro/mfma_f64_rate && tools/micro/mfma_f64_rate
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

typedef double f64x4_t __attribute__((ext_vector_type(4)));
constexpr int NACC = 8, ITERS = 65536, THREADS = 256;   // 2^19 MFMAs per wave: tens of ms a launch, so the clock settles
constexpr int WARMUP = 4, TIMED = 10;

__global__ __launch_bounds__(THREADS) void mfma_f64_loop(double* out, double seed) {
    f64x4_t acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j) acc[j] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    const double a = seed + threadIdx.x * 1e-3, b = seed - threadIdx.x * 1e-3;
#pragma nounroll
    for (int i = 0; i < ITERS; ++i) {
#pragma unroll
        for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NACC; ++j) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
    out[(size_t)blockIdx.x * THREADS + threadIdx.x] = s;
}

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    const int blocks = prop.multiProcessorCount * 2;   // 8 waves per CU, 2 per SIMD
    double* out;
    if (hipMalloc(&out, (size_t)blocks * THREADS * sizeof(double)) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    std::vector<float> ms;
    for (int r = 0; r < WARMUP + TIMED; ++r) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(mfma_f64_loop, dim3(blocks), dim3(THREADS), 0, 0, out, 1.0 + r);
        hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) return 1;
        float t;
        hipEventElapsedTime(&t, e0, e1);
        if (r >= WARMUP) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    const double flop = (double)blocks * (THREADS / 64) * ITERS * NACC * 2.0 * 16 * 16 * 4;
    const double med = 0.5 * (ms[ms.size() / 2 - 1] + ms[ms.size() / 2]);
    std::printf("mfma_f64_16x16x4 register loop: %d CUs, %d waves x %d MFMAs (%d accumulators), %d warm-up + %d timed launches, "
                "median %.3f ms (min %.3f, max %.3f) -> %.2f TFLOP/s, %.3e MFMA/s at the clock the part held (not read)\n",
                prop.multiProcessorCount, blocks * THREADS / 64, ITERS * NACC, NACC, WARMUP, TIMED, med, ms.front(), ms.back(),
                flop / med / 1e9, flop / 2048.0 / med * 1e3);
    std::printf("TFLOPS %.4f\n", flop / med / 1e9);
    hipFree(out);
    return 0;
}
