// Error plumbing and version of the C ABI (include/gandanet.h).
#include "common.h"
#include "../../include/gandanet.h"

#include <string.h>

namespace {
thread_local char g_err[512] = {0};
}

extern "C" void gd_set_error(const char* msg) {
    strncpy(g_err, msg ? msg : "", sizeof(g_err) - 1);
    g_err[sizeof(g_err) - 1] = 0;
}

extern "C" int gd_last_error(char* buf, int n) {
    const int len = (int)strlen(g_err);
    if (buf && n > 0) {
        strncpy(buf, g_err, (size_t)n - 1);
        buf[n - 1] = 0;
    }
    return len;
}

extern "C" int gd_version(void) { return GD_VERSION; }

// struct sizes, so a binding can verify its mirror of the descriptors
extern "C" int gd_sizeof_conv_desc(void) { return (int)sizeof(gd_conv_desc); }
extern "C" int gd_sizeof_gemm_nt_desc(void) { return (int)sizeof(gd_gemm_nt_desc); }

// Deterministic mode: kernels that combine partial sums with fp32 atomics (split-K NT GEMM, 3x3
// weight gradient) run unsplit -- one adder per output element, bitwise reproducible, slower.  The PAM backward's dQ
// form is chosen by its caller (gd_pam_flash_bwd form 1).  Process-global.
namespace {
int g_deterministic = 0;
}
extern "C" void gd_set_deterministic(int on) { g_deterministic = on ? 1 : 0; }
extern "C" int gd_get_deterministic(void) { return g_deterministic; }

// How deterministic mode reduces over splits: 0 = unsplit (one adder per output element), 1 = ordered (every split writes
// its partial into a slab of the caller's workspace, det_reduce.hip adds the slabs in ascending order).  Only read while
// deterministic mode is on; the _ws entry points take the workspace.  Process-global.
namespace {
int g_det_reduce = 0;
}
extern "C" int gd_set_det_reduce(int mode) {
    GD_CHECK_ARG(mode == 0 || mode == 1, "gd_set_det_reduce: mode must be 0 (unsplit) or 1 (ordered)");
    g_det_reduce = mode;
    return 0;
}
extern "C" int gd_get_det_reduce(void) { return g_det_reduce; }

// How a split reduction combines its parts OUTSIDE deterministic mode: 0 = partial slabs in the library's own workspace
// (gd_split_ws) + the ordered sum of det_reduce.hip, the default; 1 = fp32 atomics onto the zeroed output, what the
// default used to be.  Discriminator1's stem gradient stays on atomics either way.  Process-global.
namespace {
int g_split_reduce = 0;
}
extern "C" int gd_set_split_reduce(int mode) {
    GD_CHECK_ARG(mode == 0 || mode == 1, "gd_set_split_reduce: mode must be 0 (ordered slabs) or 1 (atomics)");
    g_split_reduce = mode;
    return 0;
}
extern "C" int gd_get_split_reduce(void) { return g_split_reduce; }
