// patch_pairs.h -- internal: what the host check (srx_api.hip: srx_vdsr_patch_table_check) and vdsr_patch_pairs_kernel
// (patch_pairs.hip) must agree on.  The check is the only thing between a table and the kernel's reads, so the two sizes the
// kernel derives from an entry's scaling factor -- the blur radius and the low-resolution side -- come from ONE function
// each, compiled for both sides: IEEE single / double operations with contraction off give the host and the device the same
// integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srx.h"

namespace srx {

constexpr int kPatchMinS = 2, kPatchMaxS = 128;
constexpr int kPatchMaxRadius = 63;            // gaussian_1d_kernel's limit (64 weights)
constexpr int kPatchMaxB = 0x7fffffff / 3;     // one workgroup per (entry, channel)

// sigma = 0.5 (s - 1), as vdsr/dataset.py: degrade_on_device passes it to srx_gaussian_blur (exact in fp32 for s >= 1)
__host__ __device__ inline float patch_sigma(float s) {
#pragma clang fp contract(off)
    return 0.5f * (s - 1.0f);
}
// launch_gaussian_blur's radius: int(4 sigma + 0.5).  Callers pass a finite s > 1.
__host__ __device__ inline int patch_radius(float s) {
#pragma clang fp contract(off)
    const float r = 4.0f * patch_sigma(s) + 0.5f;
    return r < 1.0e6f ? (int)r : 1000000;
}
// Python's int(S / s) on doubles (degrade_on_device, oracle.hd_to_sd).  Callers pass a finite s > 1, so 0 <= result <= S.
__host__ __device__ inline int patch_lr_size(int S, float s) { return (int)((double)S / (double)s); }

// dynamic LDS of one workgroup: 64 weights, then two S x S planes
inline size_t patch_pairs_lds_bytes(int S) { return 64 * sizeof(float) + 2 * (size_t)S * S * sizeof(float); }

struct PatchPairsArgs {
    const uint8_t* arena;
    const srx_patch_src* table;
    float* sd;
    float* hd;
    int S;
};

// A weak reference, like launch_conv_chain: a host-only build of srx_api.hip without the kernel units (the ThreadSanitizer
// test) links, and srx_vdsr_patch_pairs refuses.
__attribute__((weak)) hipError_t launch_vdsr_patch_pairs(const PatchPairsArgs& a, int B, hipStream_t s);

}  // namespace srx
