// Stand-alone sanitizer run of gd_hist_match_host (csrc/histmatch.hip over csrc/histmatch_core.h): every size pair (ns, nt)
// in 1 .. 12 x 1 .. 12 on quantised (k / 4 against k / 3, k in -3 .. 3) and continuous data at the weights 0, 0.35, 0.6 and 1,
// a few longer samples, and source NaNs of both signs, with every buffer sized exactly so that an access one element outside
// is caught.  What is checked besides the sanitizers: weight 0 returns the source, weight 1 returns values inside the range
// of the reference that rise with the source, NaNs stay at their positions.  (The bits are held to numpy by
// tests/test_cabi_histmatch.py.)  Host code only; nothing here touches a GPU.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/histmatch_host_check.cpp gan-danet_amd/csrc/histmatch.hip \
//         -o histmatch_host_check
//   ./histmatch_host_check
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/gandanet.h"

static char g_msg[512];
extern "C" void gd_set_error(const char* msg) { snprintf(g_msg, sizeof(g_msg), "%s", msg ? msg : ""); }

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
static float draw(bool quantised, float step) {
    if (quantised) return (float)((int)(next_u32() % 7) - 3) / step;
    return ((float)(next_u32() % 2000001) - 1000000.0f) * 3e-6f;
}

// one batch of B samples; nan_every > 0 puts a NaN at every nan_every-th source position, every second one negated
static int run(int B, long ns, long nt, bool quantised, double w, long nan_every) {
    std::vector<float> src((size_t)(B * ns)), ref((size_t)(B * nt));
    std::vector<double> out((size_t)(B * ns), -7.0);
    for (float& v : src) v = draw(quantised, 4.0f);
    for (float& v : ref) v = draw(quantised, 3.0f);
    long k = 0;
    if (nan_every > 0)
        for (size_t i = 0; i < src.size(); i += (size_t)nan_every) src[i] = (k++ & 1) ? -std::nanf("") : std::nanf("");
    const int rc = gd_hist_match_host(src.data(), ref.data(), B, ns, nt, w, out.data());
    if (rc != 0) {
        printf("ns = %ld, nt = %ld: rc %d (%s)\n", ns, nt, rc, g_msg);
        return 1;
    }
    int bad = 0;
    for (int b = 0; b < B; ++b) {
        const float* s = src.data() + b * ns;
        const float* r = ref.data() + b * nt;
        const double* o = out.data() + b * ns;
        const double lo = *std::min_element(r, r + nt), hi = *std::max_element(r, r + nt);
        for (long i = 0; i < ns; ++i) {
            if (s[i] != s[i]) {
                bad += o[i] == o[i];                                       // a NaN stays where it is
                continue;
            }
            bad += o[i] != o[i];
            if (w == 0.0) bad += o[i] != (double)s[i];
            if (w == 1.0) {
                bad += o[i] < lo || o[i] > hi;
                for (long j = 0; j < ns; ++j) bad += s[j] == s[j] && s[i] <= s[j] && o[i] > o[j];
            }
        }
    }
    if (bad) printf("ns = %ld, nt = %ld, %s, weight %g: %d violations\n", ns, nt, quantised ? "quantised" : "continuous", w, bad);
    return bad != 0;
}

int main() {
    const double weights[4] = {0.0, 0.35, 0.6, 1.0};
    int bad = 0, runs = 0;
    for (long ns = 1; ns <= 12; ++ns)
        for (long nt = 1; nt <= 12; ++nt)
            for (int q = 0; q < 2; ++q)
                for (double w : weights) {
                    bad += run(2, ns, nt, q == 1, w, 0);
                    ++runs;
                }
    for (double w : weights) {
        bad += run(3, 997, 991, false, w, 0);
        bad += run(2, 1000, 7, true, w, 0);
        bad += run(2, 400, 100, false, w, 20);                             // 5 % NaNs, both signs
        bad += run(2, 400, 100, true, w, 20);
        bad += run(1, 3, 5, false, w, 2);
        runs += 5;
    }
    // the refusals come before any access: these pointers are never read
    float one = 0.0f;
    double o = 0.0;
    bad += gd_hist_match_host(nullptr, &one, 1, 1, 1, 0.5, &o) != -1;
    bad += gd_hist_match_host(&one, nullptr, 1, 1, 1, 0.5, &o) != -1;
    bad += gd_hist_match_host(&one, &one, 1, 1, 1, 0.5, nullptr) != -1;
    bad += gd_hist_match_host(&one, &one, 0, 1, 1, 0.5, &o) != -1;
    bad += gd_hist_match_host(&one, &one, 1, 0, 1, 0.5, &o) != -1;
    bad += gd_hist_match_host(&one, &one, 1, 1, -1, 0.5, &o) != -1;
    bad += gd_hist_match_host(&one, &one, 1, 1L << 31, 1, 0.5, &o) != -1 || g_msg[0] == 0;
    bad += gd_hist_match_host(&one, &one, 1, 1, 1L << 31, 0.5, &o) != -1;
    printf("%d runs: %s\n", runs, bad ? "FAILED" : "OK");
    return bad != 0;
}
