// Test driver (CPU only) for tests/test_tsan_host.py::test_abi_host_code_is_thread_safe_under_tsan: linked with a
// ThreadSanitizer build of the HOST side of srx_api.hip.  The kernel launchers of the other translation units and the
// HIP runtime calls srx_api.hip makes are the stubs of host_stubs.h: this exercises the ABI's argument checking,
// planner, knob caches and error reporting from two threads.  The program never starts the HIP runtime, whose own
// threads are not instrumented, and runs the same on any machine.
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <thread>

#include "host_stubs.h"

namespace srx_stub {
// the launchers planned from a tile (grid, LDS bytes) take every shape; the ones that choose by size refuse; no errors
bool offer(const Call& c, hipError_t* err) {
    *err = hipSuccess;
    switch (c.id) {
        case k_conv_narrow: case k_wgrad_narrow: case k_conv_rows3x3: case k_conv_1x1: case k_conv_pack3: case k_conv_kwrows:
        case k_wgrad_kwcols: case k_wgrad_1x1: return false;
        default: return true;
    }
}
hipError_t call(const Call&) { return hipSuccess; }
int cu_count() { return 256; }   // (MI355X): read through the per-device cache, from both threads
}  // namespace srx_stub

static std::atomic<int> failures{0};

static void worker(int id) {
    alignas(16) static float buf[2][64];
    for (int it = 0; it < 20000; ++it) {
        srx_conv_desc d;
        memset(&d, 0, sizeof(d));
        d.N = 1 + (it % 7) + id; d.H = 17 + (it % 5); d.W = 41; d.Cin = 64; d.Cout = 64; d.KH = 3; d.KW = 3; d.stride = 1;
        const size_t a = srx_conv2d_workspace_bytes(&d, SRX_OP_BWD_FILTER);
        const size_t b = srx_conv2d_workspace_bytes(&d, SRX_OP_BWD_FILTER);
        if (a == 0 || a != b) failures++;
        if ((it & 15) == 0) srx_set_conv_path(it & 16 ? 1 : 0);
        // an argument error: the text is thread-local and names THIS thread's stride (1 and 2 are implemented)
        d.stride = 3 + id;
        if (srx_conv2d_fwd(&d, buf[id], buf[id], nullptr, nullptr, buf[id], nullptr, 0, nullptr) != SRX_ERR_UNSUPPORTED) failures++;
        char want[32];
        snprintf(want, sizeof(want), "stride %d:", 3 + id);
        if (!strstr(srx_last_error(), want)) failures++;
        // a planned (stubbed) launch
        d.stride = 1;
        if (srx_conv2d_fwd(&d, buf[id], buf[id], nullptr, nullptr, buf[id], nullptr, 0, nullptr) != SRX_OK) failures++;
    }
}

int main() {
    std::thread t0(worker, 0), t1(worker, 1);
    t0.join();
    t1.join();
    if (failures.load()) { printf("tsan driver: %d wrong results\n", failures.load()); return 1; }
    printf("tsan driver ok\n");
    return 0;
}
