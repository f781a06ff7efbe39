// Test driver (CPU only) for tests/test_lds_limit_host.py: the rule of csrc/lds_launch.h -- raise a kernel's dynamic-LDS
// ceiling once per kernel instance, device and thread -- checked without a launch.  The two HIP runtime calls that
// raise_lds_limit makes are defined here (they take precedence over libamdhip64's, which is never started), and the
// "kernels" are plain host functions, so the program runs the same on any machine.  Built a second time with
// ThreadSanitizer, it also shows that two threads share no state.
#include <stdio.h>
#include <mutex>
#include <thread>
#include <vector>

#include "../ml_super_resolution_amd/csrc/lds_launch.h"

namespace {
struct Record {
    int dev;
    const void* fn;
    int bytes;
};
std::mutex g_mu;
std::vector<Record> g_log;                      // every hipFuncSetAttribute call, of both threads
thread_local int t_dev = 0;                     // what this thread's hipGetDevice answers
thread_local hipError_t t_dev_status = hipSuccess;
thread_local int t_attr_failures = 0;           // this many hipFuncSetAttribute calls of this thread fail first

void kernel_a(int) {}
void kernel_b(int) {}                           // A's exact signature: one state per instance, not per type
void kernel_c(int) {}

size_t calls() {
    std::lock_guard<std::mutex> l(g_mu);
    return g_log.size();
}
Record last() {
    std::lock_guard<std::mutex> l(g_mu);
    return g_log.back();
}
int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipGetDevice(int* dev) {
    if (t_dev_status == hipSuccess) *dev = t_dev;
    return t_dev_status;
}
hipError_t hipFuncSetAttribute(const void* fn, hipFuncAttribute attr, int value) {
    if (attr != hipFuncAttributeMaxDynamicSharedMemorySize) return hipErrorInvalidValue;
    std::lock_guard<std::mutex> l(g_mu);
    g_log.push_back({t_dev, fn, value});
    if (t_attr_failures > 0) { --t_attr_failures; return hipErrorInvalidDeviceFunction; }
    return hipSuccess;
}
}

using srx::raise_lds_limit;

static void worker(int dev, int* errors) {
    t_dev = dev;
    for (int i = 0; i < 1000; ++i) *errors += raise_lds_limit<kernel_c>() != hipSuccess;
}

int main() {
    // kernel A twice on device 0: one call, of 160 KiB
    CHECK(raise_lds_limit<kernel_a>() == hipSuccess && raise_lds_limit<kernel_a>() == hipSuccess);
    CHECK(calls() == 1 && last().dev == 0 && last().fn == (const void*)kernel_a && last().bytes == 160 * 1024);
    CHECK(srx::kCuLdsBytes == 160 * 1024);
    // device 1 has a copy of the code object of its own: a second call; back on device 0, none
    t_dev = 1;
    CHECK(raise_lds_limit<kernel_a>() == hipSuccess && raise_lds_limit<kernel_a>() == hipSuccess);
    CHECK(calls() == 2 && last().dev == 1 && last().fn == (const void*)kernel_a && last().bytes == 160 * 1024);
    t_dev = 0;
    CHECK(raise_lds_limit<kernel_a>() == hipSuccess && calls() == 2);
    // kernel B, of A's signature, gets a call of its own
    CHECK(raise_lds_limit<kernel_b>() == hipSuccess);
    CHECK(calls() == 3 && last().dev == 0 && last().fn == (const void*)kernel_b && last().bytes == 160 * 1024);
    CHECK(raise_lds_limit<kernel_b>() == hipSuccess && calls() == 3);
    // a failing hipFuncSetAttribute is returned and not remembered: the next call tries again, and that one is kept
    t_dev = 2;
    t_attr_failures = 1;
    CHECK(raise_lds_limit<kernel_a>() == hipErrorInvalidDeviceFunction && calls() == 4);
    CHECK(raise_lds_limit<kernel_a>() == hipSuccess && calls() == 5 && last().dev == 2);
    CHECK(raise_lds_limit<kernel_a>() == hipSuccess && calls() == 5);
    // a failing hipGetDevice is returned, and nothing is set or remembered
    t_dev = 3;
    t_dev_status = hipErrorNoDevice;
    CHECK(raise_lds_limit<kernel_a>() == hipErrorNoDevice && calls() == 5);
    t_dev_status = hipSuccess;
    CHECK(raise_lds_limit<kernel_a>() == hipSuccess && calls() == 6 && last().dev == 3);
    // device index 64 (and a negative one) has no bit: set on each call, and devices 0..63 keep theirs
    t_dev = 63;
    CHECK(raise_lds_limit<kernel_a>() == hipSuccess && calls() == 7 && raise_lds_limit<kernel_a>() == hipSuccess && calls() == 7);
    t_dev = 64;
    CHECK(raise_lds_limit<kernel_a>() == hipSuccess && calls() == 8 && raise_lds_limit<kernel_a>() == hipSuccess && calls() == 9);
    CHECK(last().dev == 64 && last().bytes == 160 * 1024);
    t_dev = -1;
    CHECK(raise_lds_limit<kernel_a>() == hipSuccess && calls() == 10);
    for (int d : {0, 1, 2, 3, 63}) {
        t_dev = d;
        CHECK(raise_lds_limit<kernel_a>() == hipSuccess && calls() == 10);
    }
    t_dev = 4;                                  // (and a device never seen is still clear)
    CHECK(raise_lds_limit<kernel_a>() == hipSuccess && calls() == 11 && last().dev == 4);
    // two threads on one device: each raises once for itself, whatever the other did
    int e0 = 0, e1 = 0;
    std::thread th0(worker, 5, &e0), th1(worker, 5, &e1);
    th0.join();
    th1.join();
    CHECK(e0 + e1 == 0 && calls() == 13);
    CHECK(g_log[11].dev == 5 && g_log[11].fn == (const void*)kernel_c && g_log[12].dev == 5 && g_log[12].fn == (const void*)kernel_c);
    if (failures) { printf("lds limit driver: %d checks failed\n", failures); return 1; }
    printf("lds limit driver ok\n");
    return 0;
}
