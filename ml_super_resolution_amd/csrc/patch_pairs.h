// patch_pairs.h -- internal: what the host side (pairs_api.hip: the srx_*_patch_table_check and srx_*_eval_table_check
// functions, the entry points and their launchers) and the eight pair kernels must agree on.  Each model has a section for
// its sampler -- VDSR (patch_pairs.hip), ESPCN (espcn_pairs.hip), EnhanceNet (enet_pairs.hip), SRCNN (srcnn_pairs.hip) -- and
// one for its whole-image builder (espcn_eval.hip, vdsr_eval.hip, enet_eval.hip, srcnn_eval.hip); what the four builders
// share stands once, in front of theirs.  Each section holds the limits both sides
// enforce, the sizes and LDS layout both derive, the launch arguments and the launcher's weak declaration.  A check is
// the only thing between a table and its kernel's reads, so every size a kernel derives from a table or a parameter comes
// from ONE function here, compiled for both sides: IEEE single / double operations with contraction off give the host and
// the device the same integers.  Helpers that only the kernels use are in pairs_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/srx.h"

namespace srx {

// ---- VDSR's (sd, hd) pairs: srx_vdsr_patch_table_check and vdsr_patch_pairs_kernel (patch_pairs.hip) ----
// S is the side of the crop (2..128); an entry's scaling factor s fixes the blur radius and the low-resolution side L.

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

// A weak reference, like launch_conv_chain: a host-only build of pairs_api.hip without the kernel units links, and
// srx_vdsr_patch_pairs refuses.
__attribute__((weak)) hipError_t launch_vdsr_patch_pairs(const PatchPairsArgs& a, int B, hipStream_t s);

// ---- ESPCN's (lr, label) pairs: srx_espcn_patch_table_check and espcn_patch_pairs_kernel (espcn_pairs.hip) ----
// r is the upscaling factor (2..4, the window EspcnModel serves), p the low-resolution patch side, P = p r <= 128.

constexpr int kEspcnMinR = 2, kEspcnMaxR = 4;
constexpr int kEspcnMaxP = 128;                // p * r

// int(4 * 0.5 (r - 1) + 0.5): 2 / 4 / 6 for r = 2 / 3 / 4 (exact in integers: 2 (r - 1))
__host__ __device__ inline int espcn_radius(int r) { return patch_radius((float)r); }
// side of the byte region a workgroup stages: the P x P patch with a halo of the radius all round
__host__ __device__ inline int espcn_region(int r, int p) { return p * r + 2 * espcn_radius(r); }
// columns the H pass produces per decimated row: from the first sampled column minus the radius to the last plus it
__host__ __device__ inline int espcn_span(int r, int p) { return r * (p - 1) + 1 + 2 * espcn_radius(r); }
// the region's bytes, rounded up to a float boundary
__host__ __device__ inline int espcn_region_bytes(int r, int p) { return (espcn_region(r, p) * espcn_region(r, p) * 3 + 3) & ~3; }
// dynamic LDS of one workgroup: 256 floats (byte -> [-1, 1]), 16 weights, the region's bytes, one p x span x 3 fp32 plane.
// At most 150.4 KiB (r = 2, p = 64) inside the limits above.
__host__ __device__ inline size_t espcn_pairs_lds_bytes(int r, int p) {
    return (256 + 16) * sizeof(float) + (size_t)espcn_region_bytes(r, p) + (size_t)p * espcn_span(r, p) * 3 * sizeof(float);
}

struct EspcnPairsArgs {
    const uint8_t* arena;
    const srx_patch_src* table;
    float* lr;
    float* label;
    int r, p;
};

// A weak reference, as launch_vdsr_patch_pairs.
__attribute__((weak)) hipError_t launch_espcn_patch_pairs(const EspcnPairsArgs& a, int B, hipStream_t s);

// ---- The whole-image builders (espcn_eval.hip, vdsr_eval.hip, enet_eval.hip, srcnn_eval.hip) ----
// A table's tiles are numbered across its records in 32 bits; every walk in pairs_api.hip refuses a running sum above this.
constexpr uint64_t kEvalMaxTiles = 0x7fffffffu;
// The launch's workgroups: the table, and with it the number of tiles, is on the device, so the grid has a fixed size and
// workgroup g handles tiles g, g + grid, ... -- each tile by one workgroup, alone.  Four workgroups for each of 256 CUs.
constexpr int kEvalGrid = 1024;

// tiles of T pixels along an axis of `side` pixels, and of a width x height image: at most 2^54 (ESPCN passes its lr sides)
__host__ __device__ inline int eval_tiles_along(int side, int T) { return (side + T - 1) / T; }
__host__ __device__ inline uint64_t eval_image_tiles(int width, int height, int T) {
    return (uint64_t)eval_tiles_along(width, T) * (uint64_t)eval_tiles_along(height, T);
}
// the pixels of tile `tile` (0 <= tile < eval_tiles_along(side, T)) along an axis: first and last, the last tile cut by the side
struct EvalTileSpan {
    int first, last;
};
__host__ __device__ inline EvalTileSpan eval_tile_span(int side, int T, int tile) {
    EvalTileSpan p;
    p.first = tile * T;
    p.last = p.first + T - 1 < side ? p.first + T - 1 : side - 1;
    return p;
}
// the floats of a width x height RGB image in an output, and where the next record starts in the outputs that pad: the next
// multiple of 4 floats (16 bytes)
__host__ __device__ inline uint64_t eval_image_floats(int width, int height) { return (uint64_t)width * (uint64_t)height * 3u; }
__host__ __device__ inline uint64_t eval_padded(uint64_t floats) { return (floats + 3u) & ~(uint64_t)3u; }
// the scale of a resize from `in` to `out` pixels along an axis, as resize_bilinear_kernel (VDSR) and srx_resize_bicubic_tf
// (SRCNN) form it
__host__ __device__ inline float eval_scale(int in, int out) {
#pragma clang fp contract(off)
    return (float)in / (float)out;
}

// ---- ESPCN's whole-image (lr, label) pairs: srx_espcn_eval_table_check and espcn_eval_pairs_kernel (espcn_eval.hip) ----
// A set's images, each trimmed to multiples of r, are cut into tiles of T x T lr pixels; a tile is staged like a patch of
// p = T at (x, y) = (T r tx, T r ty), so its region, span and LDS are the patch kernel's at p = T.

__host__ __device__ inline int espcn_eval_tile() { return SRX_ESPCN_EVAL_TILE; }
__host__ __device__ inline int espcn_eval_region(int r) { return espcn_region(r, espcn_eval_tile()); }
__host__ __device__ inline int espcn_eval_span(int r) { return espcn_span(r, espcn_eval_tile()); }
// 11696 / 20864 / 32432 bytes (11.4 / 20.4 / 31.7 KiB) at r = 2 / 3 / 4 and T = 16
__host__ __device__ inline size_t espcn_eval_lds_bytes(int r) { return espcn_pairs_lds_bytes(r, espcn_eval_tile()); }

struct EspcnEvalArgs {
    const uint8_t* arena;
    const srx_eval_image* table;
    float* lr;
    float* label;
    int n, r;
};

// A weak reference, as launch_vdsr_patch_pairs.
__attribute__((weak)) hipError_t launch_espcn_eval_pairs(const EspcnEvalArgs& a, hipStream_t s);

// ---- VDSR's whole-image (sd, hd) pairs: srx_vdsr_eval_table_check and vdsr_eval_pairs_kernel (vdsr_eval.hip) ----
// A record is one image at one scaling factor s; the image is cut into tiles of T x T hd pixels (T = SRX_VDSR_EVAL_TILE).
// Both resizes have non-integer ratios, so what a tile reaches in the low-resolution image, from there in the blurred image
// and from there in the source is derived per axis from the fp32 coordinate of resize_bilinear_kernel -- by the very
// function the kernel's pixel loops take their taps from (vdsr_eval_tap), contraction off, so that the host check, the
// footprint and every pixel see the same integers.

constexpr float kVdsrEvalMaxS = 8.0f;          // 1 < s <= 8: radius <= 14, 15 weights
constexpr int kVdsrEvalMaxRadius = 14;

__host__ __device__ inline bool vdsr_eval_factor_ok(float s) { return s > 1.0f && s <= kVdsrEvalMaxS; }    // false for a NaN

// The two taps and the weight of output pixel o of a bilinear resize from `in` pixels: the half-pixel coordinate clamped
// to [0, in - 1], every operation rounded.  i0 and i1 do not decrease with o (each operation is monotone), so the taps of
// a run of outputs lie between the first one's i0 and the last one's i1.
struct VdsrEvalTap {
    int i0, i1;
    float w;
};
__host__ __device__ inline VdsrEvalTap vdsr_eval_tap(int o, float scale, int in) {
#pragma clang fp contract(off)
    float f = ((float)o + 0.5f) * scale - 0.5f;
    f = fminf(fmaxf(f, 0.f), (float)(in - 1));
    VdsrEvalTap t;
    t.i0 = (int)f;
    t.i1 = t.i0 + 1 < in ? t.i0 + 1 : in - 1;
    t.w = f - (float)t.i0;
    return t;
}

// What tile `tile` (0 <= tile < eval_tiles_along(side, SRX_VDSR_EVAL_TILE)) of an axis of `side` hd pixels, L = patch_lr_size(side, s)
// low-resolution pixels and blur radius R reaches, all indices inclusive:
//   out_first .. out_last   its hd pixels
//   lo_first .. lo_last     the low-resolution pixels their up-resize taps name
//   bl_first .. bl_last     the blurred pixels the down-resize taps of those name
//   src_first .. src_last   the source pixels the blur of those reads: bl -/+ R, clamped to the image (borders replicate)
// n_lo and n_src count the two ranges.  The blur along H is kept only at n_samp sampled rows, laid out in one of two ways:
// `dense`, one slot per blurred index of bl_first .. bl_last (ratios below 2, where nearly every index is sampled), or in
// pairs, slots 2 k and 2 k + 1 for the two taps of low-resolution pixel lo_first + k -- whichever is fewer.
struct VdsrEvalAxis {
    int out_first, out_last, lo_first, lo_last, bl_first, bl_last, src_first, src_last, n_lo, n_samp, n_src, dense;
};
__host__ __device__ inline VdsrEvalAxis vdsr_eval_axis(int side, int L, int R, int tile) {
    VdsrEvalAxis a;
    const EvalTileSpan own = eval_tile_span(side, SRX_VDSR_EVAL_TILE, tile);
    a.out_first = own.first;
    a.out_last = own.last;
    const float up = eval_scale(L, side), down = eval_scale(side, L);
    a.lo_first = vdsr_eval_tap(a.out_first, up, L).i0;
    a.lo_last = vdsr_eval_tap(a.out_last, up, L).i1;
    a.bl_first = vdsr_eval_tap(a.lo_first, down, side).i0;
    a.bl_last = vdsr_eval_tap(a.lo_last, down, side).i1;
    a.src_first = a.bl_first - R > 0 ? a.bl_first - R : 0;
    a.src_last = a.bl_last + R < side - 1 ? a.bl_last + R : side - 1;
    a.n_lo = a.lo_last - a.lo_first + 1;
    a.n_src = a.src_last - a.src_first + 1;
    const int span = a.bl_last - a.bl_first + 1;
    a.dense = span <= 2 * a.n_lo;
    a.n_samp = a.dense ? span : 2 * a.n_lo;
    return a;
}
// the slot of blurred index b, tap j (0 / 1) of low-resolution pixel lo, and the blurred index of slot k
__host__ __device__ inline int vdsr_eval_slot(const VdsrEvalAxis& a, int lo, int j, int b) {
    return a.dense ? b - a.bl_first : 2 * (lo - a.lo_first) + j;
}
__host__ __device__ inline int vdsr_eval_slot_index(const VdsrEvalAxis& a, int k, float down, int side) {
    if (a.dense) return a.bl_first + k;
    const VdsrEvalTap t = vdsr_eval_tap(a.lo_first + (k >> 1), down, side);
    return (k & 1) ? t.i1 : t.i0;
}

// Dynamic LDS of one workgroup, byte offsets (each a multiple of 16): 256 floats (byte -> [0, 1]), 16 weights, then three
// regions a tile sizes from its own footprint (y: the rows' axis, x: the columns'): the source bytes
// [n_src_y][n_src_x][3] uint8, the blur along H at the sampled rows [n_samp_y][n_src_x][3] fp32, the tile's low-resolution
// pixels [n_lo_y][n_lo_x][3] fp32.  Every tile of a launch lives in kVdsrEvalLdsBytes; the table check refuses a record
// one of whose tiles would not (it takes each count's largest value over the record's tile rows and tile columns, which
// bounds every tile from above).
struct VdsrEvalLds {
    int src, hp, lo, bytes;                                 // bytes = what the tile needs
};
__host__ __device__ inline VdsrEvalLds vdsr_eval_lds(int n_src_y, int n_src_x, int n_samp_y, int n_lo_y, int n_lo_x) {
    VdsrEvalLds l;
    l.src = (256 + 16) * (int)sizeof(float);
    l.hp = l.src + ((n_src_y * n_src_x * 3 + 15) & ~15);
    l.lo = l.hp + ((n_samp_y * n_src_x * 3 * (int)sizeof(float) + 15) & ~15);
    l.bytes = l.lo + ((n_lo_y * n_lo_x * 3 * (int)sizeof(float) + 15) & ~15);
    return l;
}
// Swept at T = 32 over s = 1.001 .. 8 in steps of 0.001 and every side up to 1100 (and 2048, 3000, 4095, 4096), with each
// count's largest value over an axis's tiles: the largest layout is 33,600 bytes at s = 1.022 (36 source pixels, 36 sampled
// rows, 33 low-resolution pixels per axis: no halo yet, and a low-resolution tile almost as large as the tile); 29,504 at
// s = 1.25, 27,744 at s = 2, 24,432 at s = 3, 22,336 at s = 4, 28,032 at s = 8 (73 source pixels, radius 14).  Past 2^24
// pixels a side, where fp32 no longer holds every pixel centre, the ranges widen by a few indices: 36,624 bytes at
// s = 1.001.  40 KiB holds all of these and lets four workgroups share a CU's 160 KiB.
constexpr int kVdsrEvalLdsBytes = 40 * 1024;

struct VdsrEvalArgs {
    const uint8_t* arena;
    const srx_vdsr_eval_image* table;
    float* sd;
    float* hd;
    int n;
};

// A weak reference, as launch_vdsr_patch_pairs.
__attribute__((weak)) hipError_t launch_vdsr_eval_pairs(const VdsrEvalArgs& a, hipStream_t s);

// ---- EnhanceNet's (sd, bq, hd) batches: srx_enet_patch_table_check, srx_enet_pairs_tables and enet_patch_pairs_kernel
// (enet_pairs.hip) ----
// S is the side of the hd crop (a multiple of 4, 4..128), s = S / 4 the side of sd.  Both resizes have the fixed ratio 4, so
// Pillow's window sizes do not depend on S: ceil(1 * 4) * 2 + 1 = 9 taps for BILINEAR S -> s, ceil(2 * 1) * 2 + 1 = 5 for
// BICUBIC s -> S (srx_pil_resample_ksize; srx_enet_pairs_tables refuses to build a block if it says otherwise).

constexpr int kEnetMinS = 4, kEnetMaxS = 128;
constexpr int kEnetKDown = 9, kEnetKUp = 5;

__host__ __device__ inline bool enet_pairs_size_ok(int S) { return S >= kEnetMinS && S <= kEnetMaxS && (S & 3) == 0; }

// The coefficient block, int32 words: the S -> s BILINEAR table, then the s -> S BICUBIC one; each is its bounds
// [out][2] = (first input index, count) followed by its kk [out][ksize] (zero past the count) -- the arrays of
// srx_pil_resample_coeffs.  A square crop's horizontal and vertical pass share a table.
struct EnetPairsTables {
    int down_bounds, down_kk, up_bounds, up_kk, words;      // word offsets; words = the block's length
};
__host__ __device__ inline EnetPairsTables enet_pairs_tables(int S) {
    const int s = S / 4;
    EnetPairsTables t;
    t.down_bounds = 0;
    t.down_kk = t.down_bounds + 2 * s;
    t.up_bounds = t.down_kk + kEnetKDown * s;
    t.up_kk = t.up_bounds + 2 * S;
    t.words = t.up_kk + kEnetKUp * S;
    return t;
}

// Dynamic LDS of one workgroup, byte offsets (each a multiple of 4, S being one): 256 floats (byte -> [-1, 1]), the
// coefficient block, then four uint8 images: the flipped crop [S][S][3], the horizontal pass of the first resize
// [S][s][3], sd [s][s][3], the horizontal pass of the second resize [s][S][3].  80.9 KiB at S = 128.
struct EnetPairsLds {
    int tab, tables, crop, h1, sd, h3, bytes;               // bytes = the whole allocation
};
__host__ __device__ inline EnetPairsLds enet_pairs_lds(int S) {
    const int s = S / 4;
    EnetPairsLds l;
    l.tab = 0;
    l.tables = l.tab + 256 * (int)sizeof(float);
    l.crop = l.tables + enet_pairs_tables(S).words * (int)sizeof(int32_t);
    l.h1 = l.crop + S * S * 3;
    l.sd = l.h1 + S * s * 3;
    l.h3 = l.sd + s * s * 3;
    l.bytes = l.h3 + s * S * 3;
    return l;
}

struct EnetPairsArgs {
    const uint8_t* arena;
    const srx_patch_src* table;
    const int32_t* tables;      // the block of srx_enet_pairs_tables(S), on the device
    float* sd;
    float* bq;
    float* hd;
    int S;
};

// A weak reference, as launch_vdsr_patch_pairs.
__attribute__((weak)) hipError_t launch_enet_patch_pairs(const EnetPairsArgs& a, int B, hipStream_t s);

// ---- EnhanceNet's whole-image (sd, bq, hd) pairs: srx_enet_eval_table_check and enet_eval_pairs_kernel (enet_eval.hip) ----
// A record is one trimmed image (both sides multiples of 4, at least kEnetEvalMinSide); it is cut into tiles of T x T hd
// pixels (T = SRX_ENET_EVAL_TILE, a multiple of 4, so every sd pixel belongs to exactly one tile).  An axis of `side`
// pixels resamples with the block of enet_pairs_tables(side) -- the layout above, with no second one -- which sits in a
// coefficient arena behind kEnetEvalBlockHeader words, the first of which holds `side`: the table check compares it with
// the record's side, so a record cannot name a block that was built for another size.

constexpr int kEnetEvalMinSide = 12;           // the scores need 11 window positions, and a side is a multiple of 4
constexpr int kEnetEvalMaxSide = 1 << 20;      // keeps every word offset of a block (39 side / 4) far inside 32 bits
constexpr int kEnetEvalBlockHeader = 1;

__host__ __device__ inline bool enet_eval_side_ok(int side) {
    return side >= kEnetEvalMinSide && side <= kEnetEvalMaxSide && (side & 3) == 0;
}
__host__ __device__ inline int enet_eval_block_words(int side) { return kEnetEvalBlockHeader + enet_pairs_tables(side).words; }

// What tile `tile` (0 <= tile < eval_tiles_along(side, SRX_ENET_EVAL_TILE)) of an axis reaches, all indices inclusive, read from the bounds
// of `tables` (the block of enet_pairs_tables(side), past its header) -- the very words the pixel loops take their taps from:
//   out_first .. out_last   its hd pixels (and its bq pixels)
//   own_first .. own_last   the sd pixels it stores: out / 4
//   sd_first .. sd_last     the sd pixels the BICUBIC taps of out_first .. out_last name
//   hd_first .. hd_last     the hd pixels the BILINEAR taps of those name
// Pillow's first index and its end do not decrease along an axis (srx_enet_eval_table_check holds a block to that), so the
// taps of a run lie between the first one's first index and the last one's end.
struct EnetEvalAxis {
    int out_first, out_last, own_first, own_last, sd_first, sd_last, hd_first, hd_last, n_out, n_sd, n_hd;
};
__host__ __device__ inline EnetEvalAxis enet_eval_axis(const int32_t* tables, int side, int tile) {
    const EnetPairsTables t = enet_pairs_tables(side);
    const int32_t *up = tables + t.up_bounds, *down = tables + t.down_bounds;
    EnetEvalAxis a;
    const EvalTileSpan own = eval_tile_span(side, SRX_ENET_EVAL_TILE, tile);
    a.out_first = own.first;
    a.out_last = own.last;
    a.own_first = a.out_first >> 2;
    a.own_last = a.out_last >> 2;
    a.sd_first = up[2 * a.out_first];
    a.sd_last = up[2 * a.out_last] + up[2 * a.out_last + 1] - 1;
    a.hd_first = down[2 * a.sd_first];
    a.hd_last = down[2 * a.sd_last] + down[2 * a.sd_last + 1] - 1;
    a.n_out = a.out_last - a.out_first + 1;
    a.n_sd = a.sd_last - a.sd_first + 1;
    a.n_hd = a.hd_last - a.hd_first + 1;
    return a;
}

// The LDS budget, one function for the launcher, the table check and the kernel.  Dynamic LDS of one workgroup, byte
// offsets (each a multiple of 16): 256 floats (byte -> [-1, 1]); the coefficient slices of the tile's two axes (x: columns,
// y: rows), int32: the BILINEAR bounds [n_sd][2] and kk [n_sd][9] of its sd range, the BICUBIC bounds [n_out][2] and kk
// [n_out][5] of its own pixels; then four uint8 images a tile sizes from its own footprint: the staged hd bytes
// [n_hd_y][n_hd_x][3], the horizontal down pass [n_hd_y][n_sd_x][3], sd [n_sd_y][n_sd_x][3], the horizontal up pass
// [n_sd_y][n_out_x][3].  Every tile of a launch lives in kEnetEvalLdsBytes; the table check refuses a record one of whose
// tiles would not (it takes each count's largest value over the record's tile rows and tile columns).
// From Pillow's tables for every side 12 .. 768: a tile of 64 reaches at most 20 sd and 84 hd pixels per axis (37,616
// bytes), a tile of 32 at most 12 and 52 (15,440 bytes).  40 KiB holds both and lets four workgroups share a CU's 160 KiB.
struct EnetEvalLds {
    int coeff_x, coeff_y, src, h1, sd, h3, bytes;           // bytes = what the tile needs
};
__host__ __device__ inline int enet_eval_coeff_words(int n_sd, int n_out) { return (2 + kEnetKDown) * n_sd + (2 + kEnetKUp) * n_out; }
__host__ __device__ inline EnetEvalLds enet_eval_lds(int n_hd_y, int n_hd_x, int n_sd_y, int n_sd_x, int n_out_y, int n_out_x) {
    EnetEvalLds l;
    l.coeff_x = 256 * (int)sizeof(float);
    l.coeff_y = l.coeff_x + ((enet_eval_coeff_words(n_sd_x, n_out_x) * (int)sizeof(int32_t) + 15) & ~15);
    l.src = l.coeff_y + ((enet_eval_coeff_words(n_sd_y, n_out_y) * (int)sizeof(int32_t) + 15) & ~15);
    l.h1 = l.src + ((n_hd_y * n_hd_x * 3 + 15) & ~15);
    l.sd = l.h1 + ((n_hd_y * n_sd_x * 3 + 15) & ~15);
    l.h3 = l.sd + ((n_sd_y * n_sd_x * 3 + 15) & ~15);
    l.bytes = l.h3 + ((n_sd_y * n_out_x * 3 + 15) & ~15);
    return l;
}
constexpr int kEnetEvalLdsBytes = 40 * 1024;
// the largest footprint per axis that the check lets through: with these, no product above overflows and the kernel's
// one-multiply divisions hold (enet_eval.hip)
constexpr int kEnetEvalMaxReach = 128;

struct EnetEvalArgs {
    const uint8_t* arena;
    const srx_enet_eval_image* table;
    const int32_t* coeffs;      // the coefficient arena, on the device
    float* sd;
    float* bq;
    float* hd;
    int n;
};

// A weak reference, as launch_vdsr_patch_pairs.
__attribute__((weak)) hipError_t launch_enet_eval_pairs(const EnetEvalArgs& a, hipStream_t s);

// ---- SRCNN's (sd, hd) batches: srx_srcnn_patch_table_check and srcnn_patch_pairs_kernel (srcnn_pairs.hip) ----
// S is the side of the crop (2..256), f the integer factor (f >= 2, s = S / f >= 1 the side of lo, as SrcnnModel.degrade's
// h // f), border the margin the VALID network removes from the ground truth (0 <= 2 border < S).

constexpr int kSrcnnMinS = 2, kSrcnnMaxS = 256;
constexpr int kSrcnnLdsLimit = 160 * 1024;
constexpr int kSrcnnMaxB = 0x7fffffff / kSrcnnMaxS;     // one workgroup per (entry, band), at most S bands

__host__ __device__ inline bool srcnn_pairs_size_ok(int S, int f) { return S >= kSrcnnMinS && S <= kSrcnnMaxS && f >= 2 && S / f >= 1; }
__host__ __device__ inline bool srcnn_pairs_border_ok(int S, int border) { return border >= 0 && 2 * (int64_t)border < S; }

// floor(o * scale) as bicubic_tf_taps forms it (bicubic_tf.h: `lower`): the same IEEE single operations on both sides
__host__ __device__ inline int srcnn_pairs_lower(int o, float scale) {
#pragma clang fp contract(off)
    return (int)floorf((float)o * scale);
}

// A workgroup builds one band of an entry: output rows [k band, min(S, (k + 1) band)).  The band height: the output rows
// that reach kSrcnnFreshLoRows lo rows of their own (12 rows at S = 243, f = 3: 21 bands, 1344 workgroups at batch 64), the
// bands then evened out.  1 <= band <= S.  Measured at the reference's shape on one MI355X, bands of 3 / 6 / 9 / 12 / 15 / 18 /
// 27 / 31 rows: 67 / 52 / 58 / 53 / 58 / 67 / 78 / 60 us per batch; short bands put three or four workgroups on a CU, tall
// ones repeat fewer lo rows.
constexpr int kSrcnnFreshLoRows = 4;
__host__ __device__ inline int srcnn_pairs_band(int S, int f) {
    const int s = S / f;
    const int reach = (kSrcnnFreshLoRows * S + s - 1) / s;
    const int bands = (S + reach - 1) / reach;
    return (S + bands - 1) / bands;
}
__host__ __device__ inline int srcnn_pairs_bands(int S, int f) { return (S + srcnn_pairs_band(S, f) - 1) / srcnn_pairs_band(S, f); }

// The lo rows the output rows [R0, R1) reach through the four clamped taps of the s -> S pass: first and last
__host__ __device__ inline void srcnn_pairs_lo_rows(int s, float up_scale, int R0, int R1, int* first, int* last) {
    const int a = srcnn_pairs_lower(R0, up_scale) - 1, b = srcnn_pairs_lower(R1 - 1, up_scale) + 2;
    *first = a < 0 ? 0 : (a > s - 1 ? s - 1 : a);
    *last = b < 0 ? 0 : (b > s - 1 ? s - 1 : b);
}
// An upper bound of their number for any band of srcnn_pairs_band(S, f) rows: floor(a) - floor(b) <= floor(a - b) + 1,
// three more taps, and one row for the rounding of the fp32 products.  The launcher compares it with every band's count.
__host__ __device__ inline int srcnn_pairs_max_lo_rows(int S, int f) {
    const int s = S / f, n = (srcnn_pairs_band(S, f) - 1) * s / S + 6;
    return n < s ? n : s;
}

// Dynamic LDS of one workgroup, byte offsets (each a multiple of 16; n = srcnn_pairs_max_lo_rows): 256 floats (byte ->
// [-1, 1]); the tap tables of the down pass (s records) and of the up pass (S records), 32 bytes each: four indices, four
// weights, shared by rows and columns of the square crop; lo [n][s][3] fp32; then ONE region used twice: the bytes of the
// four crop rows each lo row reads [n][4][S][3] uint8, and, once lo is built, the horizontal pass of lo [n][S][3] fp32 --
// 12 n S bytes either way.  45.3 KiB at S = 243, f = 3 (n = 9); at most 53.5 KiB (S = 256, f = 2).
struct SrcnnPairsLds {
    int tab, down, up, lo, rows, bytes;                     // bytes = the whole allocation
};
__host__ __device__ inline SrcnnPairsLds srcnn_pairs_lds(int S, int f) {
    const int s = S / f, n = srcnn_pairs_max_lo_rows(S, f);
    SrcnnPairsLds l;
    l.tab = 0;
    l.down = l.tab + 256 * (int)sizeof(float);
    l.up = l.down + 32 * s;
    l.lo = l.up + 32 * S;
    l.rows = l.lo + ((n * s * 3 * (int)sizeof(float) + 15) & ~15);
    l.bytes = l.rows + 12 * n * S;
    return l;
}

struct SrcnnPairsArgs {
    const uint8_t* arena;
    const srx_patch_src* table;
    float* sd;
    float* hd;
    int S, f, border;
    float down_scale, up_scale;     // (float)S / (float)s and (float)s / (float)S, formed on the host as srx_resize_bicubic_tf does
};

// A weak reference, as launch_vdsr_patch_pairs.
__attribute__((weak)) hipError_t launch_srcnn_patch_pairs(const SrcnnPairsArgs& a, int B, hipStream_t s);

// ---- SRCNN's whole-image (sd, bq, hd) pairs: srx_srcnn_eval_table_check and srcnn_eval_pairs_kernel (srcnn_eval.hip) ----
// A record is one image of height x width pixels; f (2..8) and border are the table's.  An axis of `side` pixels has
// L = side / f low-resolution pixels (SrcnnModel.degrade's h // f) and two scales of its own: (float)side / (float)L down,
// (float)L / (float)side up -- srx_resize_bicubic_tf's expressions, so a record with height != width has four.  The image
// is cut into tiles of T x T pixels of sd (T = SRX_SRCNN_EVAL_TILE); what a tile reaches is derived per axis from
// srcnn_pairs_lower, the floor bicubic_tf_taps forms, so that the host check, the footprint and every pixel see the same
// integers.

constexpr int kSrcnnEvalMinF = 2, kSrcnnEvalMaxF = 8;
// Keeps every fp32 position below 2^31, so that its conversion to int is defined.  Past 2^24 pixels a side fp32 no longer
// holds every index and a tile's ranges widen; the table check then decides per record (srcnn_eval_lds).
constexpr int kSrcnnEvalMaxSide = 1 << 30;

__host__ __device__ inline bool srcnn_eval_factor_ok(int f) { return f >= kSrcnnEvalMinF && f <= kSrcnnEvalMaxF; }
// a side has a low-resolution pixel and something left inside the margin (border >= 0; no overflow: 2 border in 64 bits)
__host__ __device__ inline bool srcnn_eval_side_ok(int side, int f, int border) { return side / f >= 1 && 2 * (int64_t)border < side; }
// a record's floats in bq (and in hd): the image without its margin.  Callers pass sides above 2 border.
__host__ __device__ inline uint64_t srcnn_eval_crop_floats(int width, int height, int border) {
    return (uint64_t)(width - 2 * border) * (uint64_t)(height - 2 * border) * 3u;
}

// What tile `tile` (0 <= tile < eval_tiles_along(side, SRX_SRCNN_EVAL_TILE)) of an axis of `side` pixels and L = side / f
// low-resolution pixels reaches, all indices inclusive:
//   out_first .. out_last   its pixels of sd
//   lo_first .. lo_last     the low-resolution pixels the four clamped taps of the L -> side pass name for them:
//                           clamp(lower(out_first, up) - 1) .. clamp(lower(out_last, up) + 2)
//   src_first .. src_last   the source pixels the four clamped taps of the side -> L pass name for those:
//                           clamp(lower(lo_first, down) - 1) .. clamp(lower(lo_last, down) + 2)
// bicubic_tf_taps names clamp(lower - 1 + k), k = 0..3, and floor((float)o * scale) does not decrease with o (each
// operation is monotone), so the two ends bracket every tap of the run.
struct SrcnnEvalAxis {
    int out_first, out_last, lo_first, lo_last, src_first, src_last, n_out, n_lo, n_src;
};
__host__ __device__ inline int srcnn_eval_clamp(int i, int limit) { return i < 0 ? 0 : (i > limit - 1 ? limit - 1 : i); }
__host__ __device__ inline SrcnnEvalAxis srcnn_eval_axis(int side, int f, int tile) {
    const int L = side / f;
    const float up = eval_scale(L, side), down = eval_scale(side, L);
    const EvalTileSpan own = eval_tile_span(side, SRX_SRCNN_EVAL_TILE, tile);
    SrcnnEvalAxis a;
    a.out_first = own.first;
    a.out_last = own.last;
    a.lo_first = srcnn_eval_clamp(srcnn_pairs_lower(a.out_first, up) - 1, L);
    a.lo_last = srcnn_eval_clamp(srcnn_pairs_lower(a.out_last, up) + 2, L);
    a.src_first = srcnn_eval_clamp(srcnn_pairs_lower(a.lo_first, down) - 1, side);
    a.src_last = srcnn_eval_clamp(srcnn_pairs_lower(a.lo_last, down) + 2, side);
    a.n_out = a.out_last - a.out_first + 1;
    a.n_lo = a.lo_last - a.lo_first + 1;
    a.n_src = a.src_last - a.src_first + 1;
    return a;
}

// Dynamic LDS of one workgroup, byte offsets (each a multiple of 16; y: the rows' axis, x: the columns'): 256 floats (byte
// -> [-1, 1]); the four tap tables of the tile's ranges, 32 bytes a record (four indices, four weights): the up pass's rows
// [n_out_y] and columns [n_out_x], the down pass's rows [n_lo_y] and columns [n_lo_x]; the source bytes
// [n_src_y][n_src_x][3] uint8; the down pass along the rows of the source [n_src_y][n_lo_x][3] fp32; the tile's
// low-resolution pixels [n_lo_y][n_lo_x][3] fp32; the up pass along their rows [n_lo_y][n_out_x][3] fp32.  Every tile of a
// launch lives in kSrcnnEvalLdsBytes; the table check refuses a record one of whose tiles would not (it takes each count's
// largest value over the record's tile rows and tile columns, which bounds every tile from above).
struct SrcnnEvalLds {
    int up_y, up_x, down_y, down_x, src, hdn, lo, hup, bytes;      // bytes = what the tile needs
};
__host__ __device__ inline SrcnnEvalLds srcnn_eval_lds(int n_src_y, int n_src_x, int n_lo_y, int n_lo_x, int n_out_y, int n_out_x) {
    SrcnnEvalLds l;
    l.up_y = 256 * (int)sizeof(float);
    l.up_x = l.up_y + 32 * n_out_y;
    l.down_y = l.up_x + 32 * n_out_x;
    l.down_x = l.down_y + 32 * n_lo_y;
    l.src = l.down_x + 32 * n_lo_x;
    l.hdn = l.src + ((n_src_y * n_src_x * 3 + 15) & ~15);
    l.lo = l.hdn + ((n_src_y * n_lo_x * 3 * (int)sizeof(float) + 15) & ~15);
    l.hup = l.lo + ((n_lo_y * n_lo_x * 3 * (int)sizeof(float) + 15) & ~15);
    l.bytes = l.hup + ((n_lo_y * n_out_x * 3 * (int)sizeof(float) + 15) & ~15);
    return l;
}
// Swept on the host over f = 2 .. 8 and every side 2 .. 1100 (and 2048, 3000, 4095, 4096, 10000, 65536, 1000003, 2^24 - 1,
// 2^24), with each count's largest value over an axis's tiles, both axes at their largest at once.  At T = 32 the largest
// layout is 32,704 bytes at f = 2 (43 source and 20 low-resolution pixels per axis); 27,600 at f = 3 (47 and 15), 24,880 at
// f = 4 (50 and 12), 25,808 / 26,288 / 26,816 / 26,352 at f = 5 / 6 / 7 / 8 (65 source pixels and 8 low-resolution ones at
// f = 8).  40 KiB holds all of these and lets four workgroups share a CU's 160 KiB.  Past 2^24 pixels a
// side the ranges widen: 37,424 bytes at 2^28 and f = 3, 47,024 at 2^29, which the check refuses.  At T = 16 the largest
// is 15,376 bytes (f = 7); at T = 64 it is 99,904 (f = 2: 75 and 36), one workgroup per CU, which is what a build with
// that tile gets.
constexpr int kSrcnnEvalLdsBytes = SRX_SRCNN_EVAL_TILE <= 32 ? 40 * 1024 : 100 * 1024;
// the largest footprint per axis that the check lets through: with it no product above overflows and the kernel's
// one-multiply divisions hold (srcnn_eval.hip)
constexpr int kSrcnnEvalMaxReach = 128;

struct SrcnnEvalArgs {
    const uint8_t* arena;
    const srx_srcnn_eval_image* table;
    float* sd;
    float* bq;
    float* hd;
    int n, f, border;
};

// A weak reference, as launch_vdsr_patch_pairs.
__attribute__((weak)) hipError_t launch_srcnn_eval_pairs(const SrcnnEvalArgs& a, hipStream_t s);

}  // namespace srx
