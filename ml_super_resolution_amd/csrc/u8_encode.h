// u8_encode.h -- the one statement of tf.saturate_cast(x * 127.5 + 127.5, uint8) that device code shares
// (feature_mosaic.hip, summary_panel.hip); srx_saturate_u8's arithmetic (elementwise.hip, saturate_u8_kernel) -- and the
// one statement of ESPCN's image encode (espcn_fused.hip, espcn_frames.hip).
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

// ESPCN's image encode (espcn/espcn/experiment_test.py:148-184: `* 0.5 + 0.5`, clip to [0, 1], `* 255.0 + 0.5`,
// astype(uint8)) in the roundings of the route that existed -- srx_affine(0.5, 0.5) (two), clamp_, numpy's fp32 multiply
// and add (two), truncation toward zero -- every step rounded on its own.  A NaN encodes to 0 (fmaxf drops it).
__device__ __forceinline__ uint32_t encode_unit_u8(float y) {
#pragma clang fp contract(off)
    float t = y * 0.5f;
    t = t + 0.5f;
    t = fminf(fmaxf(t, 0.f), 1.f);
    t = t * 255.f;
    t = t + 0.5f;
    return (uint32_t)(uint8_t)t;
}

// encode_unit_u8 for codes of 0..max (espcn_yuv_formats.hip: max 255, 1023 or 4095): the same five separately rounded steps
// with `255.f` replaced by (float)max.  At max 255 it gives encode_unit_u8's code for every float: t + 0.5f lies in
// [0.5, 255.5], so the cast through uint8_t there changes nothing.
__device__ __forceinline__ uint32_t encode_unit_bits(float y, uint32_t max) {
#pragma clang fp contract(off)
    float t = y * 0.5f;
    t = t + 0.5f;
    t = fminf(fmaxf(t, 0.f), 1.f);
    t = t * (float)max;
    t = t + 0.5f;
    return (uint32_t)t;
}

}  // namespace srx
