// Test driver (CPU only) for tests/test_enet_eval_host.py::test_a_host_only_build_refuses: linked with a --cuda-host-only
// build of pairs_api.hip alone -- neither srx_api.hip, nor the resample unit (resample_u8.hip), nor the eval-pair kernel
// (enet_eval.hip) is in the program.  The launcher and the coefficient routines are weak references there, and the
// srx_enet_eval_* entries that need them must refuse with a message, as the srx_enet_pairs_* ones do.  What pairs_api.hip
// takes from srx_api.hip -- the error text -- and the one HIP runtime call it names are defined here.  One line per call:
// the return code, then srx_last_error().
#include <stdarg.h>
#include <stdio.h>

#include <hip/hip_runtime.h>

#include "../include/srx.h"

static char g_err[512] = "";
namespace srx {
int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace srx
extern "C" {
const char* srx_last_error(void) { return g_err; }
const char* hipGetErrorString(hipError_t) { return "stubbed HIP runtime"; }
}

int main() {
    alignas(16) static int32_t block[1 + 39 * 4];
    alignas(16) static float out[3][4];
    static uint8_t arena[4];
    static srx_enet_eval_image table[1];
    int reach[4];
    printf("coeff_words %d\n", srx_enet_eval_coeff_words(16));
    printf("coeffs %d %s\n", srx_enet_eval_coeffs(16, block), srx_last_error());
    printf("footprint %d %s\n", srx_enet_eval_footprint(16, 0, reach), srx_last_error());
    printf("pairs %d %s\n", srx_enet_eval_pairs(arena, table, 1, block, out[0], out[1], out[2], nullptr), srx_last_error());
    printf("pairs_tables %d %s\n", srx_enet_pairs_tables(16, block), srx_last_error());
    return 0;
}
