// image_scores.h -- internal: what the host side (srx_api.hip: srx_image_scores_plan, srx_image_scores_scratch_bytes,
// srx_image_scores) and the two kernels of image_scores.hip must agree on: the tile, the LDS layout, the scratch layout,
// the launch arguments and the launcher's weak declaration.  Every size comes from ONE function here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srx.h"

namespace srx {

// The "effective image" of a descriptor is [H, We, Ce] (include/srx.h).  A row of it is RL = We * Ce floats and the 11 taps
// of a window lie Ce floats apart, so a window position is a "flat column" x in [0, (We - 10) * Ce): it reads the flat
// columns x, x + Ce, ..., x + 10 Ce <= RL - 1.  One code path serves every C and the Y space (Ce = 1).
constexpr int kScoresTileH = 16;          // window rows of a tile (the vertical pass walks them in groups of 4)
constexpr int kScoresTileW = 128;         // flat window columns of a tile
constexpr int kScoresHaloH = kScoresTileH + 10;
constexpr int kScoresLdsLimit = 160 * 1024;
constexpr int kScoresMaxN = 65535;        // one grid row per image
constexpr long long kScoresMaxRow = 0x7fff0000LL;   // floats of an input row: flat columns are ints, a tile may overhang by < 2^16

// floats of one staged halo row: the tile's columns and the ten taps to their right
__host__ __device__ constexpr int scores_pitch(int Ce) { return kScoresTileW + 10 * Ce; }

// Dynamic LDS of one workgroup, float offsets (each a multiple of 4): 16 floats for the 11 window weights; the staged halo
// regions of ref (A) and of the candidate in turn (B), kScoresHaloH x scores_pitch each; three planes kScoresHaloH x
// kScoresTileW of horizontal moments (ref: mu, E[a^2]; a candidate: mu, E[b^2], E[ab]); 8 floats for the block sums.
struct ScoresLds {
    int g, A, B, H0, H1, H2, red, bytes;    // bytes = the whole allocation
};
__host__ __device__ constexpr ScoresLds scores_lds(int Ce) {
    const int raw = kScoresHaloH * scores_pitch(Ce), mom = kScoresHaloH * kScoresTileW;
    ScoresLds l = {};
    l.g = 0;
    l.A = 16;
    l.B = l.A + raw;
    l.H0 = l.B + raw;
    l.H1 = l.H0 + mom;
    l.H2 = l.H1 + mom;
    l.red = l.H2 + mom;
    l.bytes = (l.red + 8) * (int)sizeof(float);
    return l;
}
// the largest tap stride whose layout fits kScoresLdsLimit (SRX_SCORES_MAX_TAP_STRIDE of include/srx.h)
constexpr int kScoresMaxCe = SRX_SCORES_MAX_TAP_STRIDE;
static_assert(scores_lds(kScoresMaxCe).bytes <= kScoresLdsLimit && scores_lds(kScoresMaxCe + 1).bytes > kScoresLdsLimit,
              "SRX_SCORES_MAX_TAP_STRIDE is the largest tap stride whose layout fits the LDS");

// Scratch: one slot of two floats (sum of squared errors, sum of SSIM values) per (image, candidate, tile):
//   slot = ((n * n_cand + k) * tiles + tile) * 2,   tiles = tiles_y * tiles_x,   tile = ty * tiles_x + tx
__host__ __device__ inline size_t scores_scratch_floats(int N, int n_cand, int tiles) { return (size_t)N * n_cand * tiles * 2; }

struct ImageScoresArgs {
    const float* ref;
    const float* cand[SRX_SCORES_MAX_CAND];
    float* scratch;
    int H, row_in;            // rows of an image; floats of one input row (W * C)
    int RL, Ce;               // floats of one effective row; tap stride
    int n_cand, y_space, unit_clip;
    int tiles_y, tiles_x;
    float c1, c2;
};

// Two launches: the tile kernel (grid tiles x N) and the finish kernel (one workgroup per (candidate, image)).  A weak
// reference, as launch_vdsr_patch_pairs: a host-only build of srx_api.hip without the kernel units links, and
// srx_image_scores refuses.
__attribute__((weak)) hipError_t launch_image_scores(const ImageScoresArgs& a, int N, float max_val, float* out, hipStream_t s);

}  // namespace srx
