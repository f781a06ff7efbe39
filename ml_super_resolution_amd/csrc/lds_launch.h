// lds_launch.h -- internal: the one place that launches a kernel with more than 64 KiB of dynamic LDS.
// Includes nothing of the project, so a unit that needs only the launch does not see the conv kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srx {

// The whole LDS of a CU: the ceiling every kernel is allowed to ask for.  It is only a ceiling; occupancy follows the
// `lds` of each launch.
constexpr int kCuLdsBytes = 160 * 1024;

// A launch that asks for more than 64 KiB of dynamic LDS needs the kernel's MaxDynamicSharedMemorySize attribute raised
// first, and the attribute belongs to ONE DEVICE's copy of the code object.  So "already raised" is one bit per device
// index, per kernel instance (the kernel is a template argument: two kernels of one signature do not share it).
// The state is thread_local: a new thread sets the attribute once more for itself, which is idempotent and needs no
// lock.  A failure is returned and nothing is remembered, so the next call tries again; a device index outside 0..63
// (the bound of cu_count() in srx_api.hip) is never remembered, and the attribute is set on each call.
template <auto Kernel>
inline hipError_t raise_lds_limit() {
    static thread_local uint64_t raised = 0;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = (dev >= 0 && dev < 64) ? (uint64_t)1 << dev : 0;
    if (bit && (raised & bit)) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kCuLdsBytes);
    if (e == hipSuccess) raised |= bit;
    return e;
}

// After a kernel's first launch on a device, a launch costs one hipGetDevice on top of the launch itself, so the launches
// of a captured step set no attribute.
template <auto Kernel, typename... Args>
inline hipError_t launch_with_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args&... args) {
    const hipError_t e = raise_lds_limit<Kernel>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
    return hipGetLastError();
}

}  // namespace srx
