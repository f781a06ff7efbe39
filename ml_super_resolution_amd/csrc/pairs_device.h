// pairs_device.h -- internal, device only: the small pieces the four sampler kernels (patch_pairs.hip, espcn_pairs.hip,
// enet_pairs.hip, srcnn_pairs.hip) and the four whole-image pair kernels (espcn_eval.hip, vdsr_eval.hip, enet_eval.hip, srcnn_eval.hip) share.  Nothing
// here is seen by the host checks; what the host and the kernels must agree on is in patch_pairs.h.  Each helper is the expression its callers used to spell out, so that a change to one
// reaches every kernel that relies on it.
#pragma once
#include <hip/hip_runtime.h>

#include "patch_pairs.h"

namespace srx {

// n / d with one multiply.  Precondition: d >= 2 and n * d < 2^32 (n >= 0).  m = floor((2^32 - 1) / d) + 1 is
// ceil(2^32 / d): m d = 2^32 + e with 0 <= e < d, so n m / 2^32 = n / d + n e / (d 2^32), and the excess is below
// n / 2^32 < 1 / d: it cannot carry n / d past the next integer.  Each use site says why its n and d qualify.
struct SmallDiv {
    unsigned m;
    __device__ __forceinline__ explicit SmallDiv(unsigned d) : m(0xffffffffu / d + 1u) {}
    __device__ __forceinline__ int operator()(int n) const { return (int)__umulhi((unsigned)n, m); }
};

// byte -> [-1, 1] in fp32: u8_to_pm1_kernel's expression, a division and a subtraction, each rounded (contraction off)
__device__ __forceinline__ float byte_to_pm1(int b) {
#pragma clang fp contract(off)
    return (float)b / 127.5f - 1.0f;
}

// byte -> [-1, 1] as numpy forms it in float64 and then rounds to float32 (ESPCN's reference: image / 127.5 - 1)
__device__ __forceinline__ float byte_to_pm1_f64(int b) {
#pragma clang fp contract(off)
    return (float)((double)b / 127.5 - 1.0);
}

// The weight of tap t (0 <= t <= radius) of gaussian_1d_kernel's window: fp32 expf, normalised by the sum over
// -radius .. radius taken in that order.
__device__ __forceinline__ float gaussian_tap_weight(int t, int radius, float sigma) {
    float sum = 0.f;
    for (int i = -radius; i <= radius; ++i) sum += expf(-0.5f * (float)(i * i) / (sigma * sigma));
    return expf(-0.5f * (float)(t * t) / (sigma * sigma)) / sum;
}

// ESPCN's two tap loops, shared by espcn_patch_pairs_kernel (espcn_pairs.hip) and espcn_eval_pairs_kernel (espcn_eval.hip)
// so that a patch and the image it was cut from hold the same bits: taps -RAD .. RAD in order, one accumulator, every
// product and every sum rounded (contraction off).  Left to the compiler, the rounding depended on the loop around the
// call: it fused the products into FMAs where it had unrolled that loop by two and not in the loop's remainder, so one
// value came out in two ways according to its position in a patch.
// Along H, from bytes through tab: b is tap -RAD in a staged byte region whose rows are E3 bytes.
template <int RAD>
__device__ __forceinline__ float espcn_blur_h_taps(const uint8_t* b, int E3, const float* wts, const float* tab) {
#pragma clang fp contract(off)
    float acc = 0.f;
#pragma unroll
    for (int k = -RAD; k <= RAD; ++k) acc += wts[k < 0 ? -k : k] * tab[b[(k + RAD) * E3]];
    return acc;
}
// Along W, from the fp32 plane of the H pass: b is tap -RAD, columns are 3 floats apart.
template <int RAD>
__device__ __forceinline__ float espcn_blur_w_taps(const float* b, const float* wts) {
#pragma clang fp contract(off)
    float acc = 0.f;
#pragma unroll
    for (int k = -RAD; k <= RAD; ++k) acc += wts[k < 0 ? -k : k] * b[(k + RAD) * 3];
    return acc;
}

// One output byte of a Pillow resample pass, shared by enet_patch_pairs_kernel (enet_pairs.hip) and
// enet_eval_pairs_kernel (enet_eval.hip) so that a crop and the image it was cut from use one expression: taps src[0],
// src[stride], ... (the first `n` of K, n >= 1) against k[0 .. n).  Without a branch: k is zero past the count
// (srx_pil_resample_coeffs), so a tap past it re-reads tap n - 1 and adds nothing.
template <int K>
__device__ __forceinline__ int resample_byte(const uint8_t* src, int stride, const int* k, int n) {
    int ss = 1 << 21;
    const int last = n > 0 ? n - 1 : 0;
#pragma unroll
    for (int x = 0; x < K; ++x) ss += (int)src[(x < last ? x : last) * stride] * k[x];
    ss >>= 22;                       // (arithmetic shift: negative sums clip to 0 like Pillow's lookup table)
    return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

// One record of a tap table of bicubic_tf_taps (bicubic_tf.h) in LDS, 32 bytes: what srcnn_patch_pairs_kernel
// (srcnn_pairs.hip) and srcnn_eval_pairs_kernel (srcnn_eval.hip) keep per output index of a pass.
struct alignas(16) SrcnnTaps {
    int idx[4];
    float w[4];
};

// The record of tile `tile` in a whole-image table (srx_eval_image, srx_vdsr_eval_image, srx_enet_eval_image, srx_srcnn_eval_image) of n records on the device: the
// last one whose first_tile is <= tile.  first_tile is non-decreasing and table[0].first_tile == 0 <= tile (the table
// checks in pairs_api.hip), so the search ends on one record; every thread of a workgroup makes it on the same words.
template <class Rec>
__device__ __forceinline__ Rec eval_record_of_tile(const Rec* table, int n, unsigned tile) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_tile <= tile) lo = mid; else hi = mid - 1;
    }
    return table[lo];
}

// The tiles of a launch, from the table's last record: its first_tile and its own tiles of T pixels.  (ESPCN's tiles are
// of lr pixels, and espcn_eval.hip spells its own preamble: DESIGN.md 3.23.)
template <class Rec>
__device__ __forceinline__ unsigned eval_total_tiles(const Rec* table, int n, int T) {
    const Rec last = table[n - 1];
    return last.first_tile + (unsigned)eval_image_tiles(last.width, last.height, T);
}

// Where tile `tile` of a launch lies in its record `im`, an image of tiles_x tiles per row: the tile's row and column
struct EvalTileAt {
    int ty, tx;
};
template <class Rec>
__device__ __forceinline__ EvalTileAt eval_tile_at(const Rec& im, unsigned tile, int tiles_x) {
    const int local = (int)(tile - im.first_tile);
    EvalTileAt p;
    p.ty = local / tiles_x;
    p.tx = local - p.ty * tiles_x;
    return p;
}

// Stages n bytes of an image into dst (LDS): rows of `pitch` consecutive bytes from `base` on, image_row_bytes apart in
// the image and back to back in dst; t is the thread of 256.  Each call site says why pitch and n qualify for SmallDiv.
__device__ __forceinline__ void stage_image_rows(uint8_t* dst, const uint8_t* base, size_t image_row_bytes, int n, int pitch, int t) {
    const SmallDiv by_pitch(pitch);
#pragma unroll 8
    for (int o = t; o < n; o += 256) {
        const int row = by_pitch(o), rem = o - row * pitch;
        dst[o] = base[(size_t)row * image_row_bytes + rem];
    }
}

}  // namespace srx
