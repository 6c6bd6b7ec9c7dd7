// Stand-alone sanitizer run of gd_stl_decompose_host (csrc/stl.hip over csrc/stl_core.h): the short-series cases, whose
// windows are longer than the series (T = 24 and 25 at period 12), and a robust fit with outliers, with every buffer sized
// exactly so that an access one element outside is caught.  Host code only; nothing here touches a GPU.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/stl_host_check.cpp gan-danet_amd/csrc/stl.hip -o stl_host_check
//   ./stl_host_check
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/gandanet.h"

static char g_msg[512];
extern "C" void gd_set_error(const char* msg) { snprintf(g_msg, sizeof(g_msg), "%s", msg ? msg : ""); }

template <typename T>
static int run(long n, long m, int period, int seasonal, int trend, int low_pass, int ni, int no, bool outliers) {
    std::vector<T> x((size_t)(n * m)), tr(x.size()), se(x.size()), re(x.size()), rw(x.size());
    for (long t = 0; t < n; ++t)
        for (long c = 0; c < m; ++c)
            x[(size_t)(t * m + c)] = (T)(0.01 * t + std::sin(6.283185307179586 * t / period + c) + 0.3 * std::sin(12.9898 * (t * m + c + 1)));
    if (outliers)
        for (long t = 5; t < n; t += 57) x[(size_t)(t * m)] += (T)15;
    const int dtype = sizeof(T) == 8 ? 1 : 0;
    const int rc = gd_stl_decompose_host(x.data(), dtype, n, m, period, seasonal, trend, low_pass, 1, 1, 1, ni, no, tr.data(), se.data(),
                                         re.data(), rw.data());
    if (rc != 0) {
        printf("T = %ld: rc %d (%s)\n", n, rc, g_msg);
        return 1;
    }
    double worst = 0.0;
    for (size_t i = 0; i < x.size(); ++i) worst = std::fmax(worst, std::fabs((double)x[i] - (double)se[i] - (double)tr[i] - (double)re[i]));
    printf("T = %ld, M = %ld, period %d, (%d, %d) iterations, %s: max |x - seasonal - trend - resid| = %.3g\n", n, m, period, ni, no,
           dtype ? "fp64" : "fp32", worst);
    return std::isfinite(worst) && worst < 1e-4 ? 0 : 1;
}

int main() {
    int bad = 0;
    bad += run<double>(24, 3, 12, 13, 21, 13, 5, 0, false);
    bad += run<double>(25, 3, 12, 13, 21, 13, 5, 0, false);
    bad += run<float>(25, 2, 12, 13, 21, 13, 5, 0, false);
    bad += run<double>(30, 2, 12, 13, 35, 13, 5, 0, false);
    bad += run<double>(9, 2, 2, 7, 5, 3, 5, 0, false);
    bad += run<double>(181, 2, 12, 13, 21, 13, 2, 15, true);
    bad += run<double>(25, 2, 12, 13, 21, 13, 2, 3, true);
    // the weights are optional
    std::vector<double> x(48, 1.0), a(48), b(48), c(48);
    bad += gd_stl_decompose_host(x.data(), 1, 24, 2, 12, 13, 21, 13, 1, 1, 1, 1, 1, a.data(), b.data(), c.data(), nullptr) != 0;
    bad += gd_stl_decompose_host(x.data(), 1, 23, 2, 12, 13, 21, 13, 1, 1, 1, 1, 1, a.data(), b.data(), c.data(), nullptr) != -1;
    printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
