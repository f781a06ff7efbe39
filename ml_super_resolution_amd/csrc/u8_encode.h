// u8_encode.h -- the one statement of tf.saturate_cast(x * 127.5 + 127.5, uint8) that device code shares
// (feature_mosaic.hip, summary_panel.hip); srx_saturate_u8's arithmetic (elementwise.hip, saturate_u8_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srx {

// multiply and add rounded separately, clamp, truncate
__device__ __forceinline__ uint32_t encode_u8(float x) {
#pragma clang fp contract(off)
    float v = x * 127.5f;
    v = v + 127.5f;
    v = fminf(fmaxf(v, 0.f), 255.f);
    return (uint32_t)(uint8_t)v;
}

}  // namespace srx
