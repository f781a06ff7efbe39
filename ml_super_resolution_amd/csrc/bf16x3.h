// bf16x3.h -- internal: precision 1 (SRX_PRECISION_BF16X3) of 3x3 stride-1 SAME 64 -> 64 layers (conv_bf16x3.hip).
// Every fp32 operand of a product is split into a = hi + lo (hi = bf16_rne(a), lo = bf16_rne(a - hi)) and each product is
// hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with an fp32 accumulator; bias, activation, masks and sums stay fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace srx {

// Tiles of TH x TW output pixels of one image; `tiles` = N * nty * ntx, walked by `grid` persistent workgroups (two per CU).
struct Bf3Plan {
    int TH, TW, ntx, nty, tiles, grid;
    size_t lds;
};

// LDS bytes per staged pixel: forward / data gradient (64 hi + 64 lo bf16 + 16 pad: the 16 pixels of a ds_read_b128 hit
// disjoint banks) and filter gradient (+ 32 pad: the 8 slots a 32-lane half of a ds_read_b64_tr_b16 takes hit disjoint banks);
// every workgroup stays within 80 KiB (two per CU).  The tile planner is host code in srx_api.hip.
constexpr int kBf3ConvSlot = 272, kBf3WgradSlot = 288;
constexpr size_t kBf3Lds = 80 * 1024;

// The launchers are weak references: a host-only build of srx_api.hip without the kernel units (the ThreadSanitizer test)
// still links; srx_api.hip refuses precision 1 when they are absent.
// dgrad == false: y = act(x (*) w + bias), relu selects ReLU, bias nullable, mask unused.
// dgrad == true:  y = (dpre (*) flipped / transposed w) * (mask > 0) with x = dpre, mask = x_in (nullable: no mask).
__attribute__((weak)) hipError_t launch_conv3x3c64_bf16x3(bool dgrad, const float* x, const float* w, const float* bias, const float* mask, bool relu,
                                    float* y, int N, int H, int W, const Bf3Plan& p, hipStream_t s);
// One partial filter per workgroup: part[g * part_stride + (tap * 64 + ci) * 64 + co], dbias partial at + 9 * 64 * 64 + co.
__attribute__((weak)) hipError_t launch_wgrad3x3c64_bf16x3(const float* x, const float* dpre, float* part, int part_stride, int N, int H, int W,
                                     const Bf3Plan& p, hipStream_t s);

}  // namespace srx
