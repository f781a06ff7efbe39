// bicubic_tf.h -- internal: the tap positions and weights of tf.image.resize_bicubic as TensorFlow 1.x computes them, one
// text for every kernel that resizes this way: resize_bicubic_tf_kernel (enet_ops.hip, which documents the arithmetic),
// srcnn_patch_pairs_kernel (srcnn_pairs.hip) and srcnn_eval_pairs_kernel (srcnn_eval.hip), whose results must be the same
// bits.
#pragma once
#include <hip/hip_runtime.h>

namespace srx {

__device__ __forceinline__ void bicubic_tf_taps(int o, float scale, int limit, int (&idx)[4], float (&w)[4]) {
#pragma clang fp contract(off)
    const float A = -0.75f;
    const float in = (float)o * scale;
    const float fl = floorf(in);
    const int lower = (int)fl;
    const int offset = (int)lrintf((in - fl) * 1024.0f);
    const float x = (float)offset / 1024.0f, xr = (float)(1024 - offset) / 1024.0f;
    const float x1 = x + 1.0f, xr1 = xr + 1.0f;
    w[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    w[0] = ((A * x1 - 5.0f * A) * x1 + 8.0f * A) * x1 - 4.0f * A;
    w[2] = ((A + 2.0f) * xr - (A + 3.0f)) * xr * xr + 1.0f;
    w[3] = ((A * xr1 - 5.0f * A) * xr1 + 8.0f * A) * xr1 - 4.0f * A;
    for (int k = 0; k < 4; ++k) {
        int i = lower - 1 + k;
        idx[k] = i < 0 ? 0 : (i > limit - 1 ? limit - 1 : i);
    }
}

}  // namespace srx
