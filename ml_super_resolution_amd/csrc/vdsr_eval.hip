// vdsr_eval.hip -- VDSR's evaluation pairs of a whole image set built on the device, one launch per set.
//
// The reference prepares an evaluation pair per image on the host (vdsr/vdsr/experiment_evaluate.py:14-33): the image as
// floats in [0, 1], hd_image_to_sd_image (vdsr/vdsr/dataset.py:13-38: gaussian blur sigma = 0.5 (s - 1), bilinear resize to
// (int(H / s), int(W / s)) and back) on the WHOLE image, both mapped to [-1, 1].  Here the decoded images sit in one uint8
// arena and a table of srx_vdsr_eval_image records names an image, a scaling factor, where the record's outputs start and
// how many tiles the records before it have.  A record is cut into tiles of T x T hd pixels (T = SRX_VDSR_EVAL_TILE).
//
// This is not vdsr_patch_pairs_kernel (patch_pairs.hip) with a larger S: that kernel holds a whole S x S plane in LDS and
// its borders are the crop's own.  A tile's borders are the image's, and neither resize has an integer ratio, so what a
// tile reaches is derived per axis by vdsr_eval_axis (patch_pairs.h) from the taps of its first and last pixel -- through
// vdsr_eval_tap, the function every pixel loop below takes its taps from, so a pixel cannot name a slot the footprint
// left out.  The per-value arithmetic is that of gaussian_1d_kernel, resize_bilinear_kernel (elementwise.hip) and
// vdsr_patch_pairs_kernel: gaussian_tap_weight, taps -R .. R in order, the same four-term bilinear expression; every
// product and sum is rounded on its own (contraction off), so a value does not depend on how its loop was unrolled.
//
// The grid is kEvalGrid workgroups of 256 threads that stride over the tiles (patch_pairs.h) -- each tile, all three
// channels, by one workgroup alone.  LDS (kVdsrEvalLdsBytes = 40 KiB, vdsr_eval_lds): tab, 256 floats byte -> [0, 1] (a
// division, as u8_to_float_kernel), written once per workgroup; wts, 16 floats; then three regions sized by the tile's
// footprint (y: rows, x: columns).  Per tile, a barrier between the steps and one before the next tile's step 1:
//   0. the tile's record (eval_record_of_tile, pairs_device.h); its s, radius and low-resolution sizes; the two axes'
//      footprints; wts[0 .. R]
//   1. src [n_src_y][n_src_x][3] uint8 = the source rows src_first_y .. src_last_y, columns src_first_x .. src_last_x:
//      blurred index -/+ R clamped to the image, so no read is clamped here and the taps below clamp into this range
//   2. hp [n_samp_y][n_src_x][3] = blur along H of tab[src] at the sampled rows only (slot k is blurred row
//      vdsr_eval_slot_index(k)), at every staged column
//   3. lo [n_lo_y][n_lo_x][3] = the tile's low-resolution pixels: each takes its two rows' slots and its two columns from
//      its down-resize taps, blurs hp along W at those two columns only, and combines the four values
//   4. sd = (lo up-resized) * 2 - 1 and hd = tab[byte] * 2 - 1 (the byte read from the arena again: a tile's own pixels need
//      not all lie inside src), stored: the 3 T floats of a tile row to consecutive lanes
// Every slot a step reads was written by the step before it: step 2 reads src rows clamp(b + i) - src_first_y for
// bl_first_y <= b <= bl_last_y, which step 1 wrote whole; step 3 reads the slots of its own taps, all below n_samp_y, at
// columns clamp(x + i) - src_first_x; step 4 reads lo at taps between lo_first and lo_last.  So the result does not depend
// on what the LDS held (SRX_POISON_LDS).  No atomics, no communication between workgroups, plain vector stores.
//
// The table is trusted: srx_vdsr_eval_table_check (pairs_api.hip) keeps every image inside the arena, s inside (1, 8] (radius
// <= 14), both low-resolution sides >= 1, out_offset and first_tile the running sums (so no two records' outputs overlap
// and the search finds one record per tile), the total inside sd / hd, and the layout of every tile inside
// kVdsrEvalLdsBytes.  Every global read is at a (row, column) inside such an image.
#include "lds_launch.h"
#include "pairs_device.h"
#include "patch_pairs.h"

namespace srx {

// The blur's taps -R .. R in order, one accumulator, every product and sum rounded.  Along H from the staged bytes: b is
// the blurred row, rows are `pitch` bytes, `first` / `last` the image's clamp and `org` the first staged row.
__device__ __forceinline__ float vdsr_eval_blur_h(const uint8_t* col, int pitch, int b, int R, int last, int org, const float* wts,
                                                  const float* tab) {
#pragma clang fp contract(off)
    float acc = 0.f;
    for (int i = -R; i <= R; ++i) {
        int r = b + i;
        r = r < 0 ? 0 : (r > last ? last : r);
        acc += wts[i < 0 ? -i : i] * tab[col[(r - org) * pitch]];
    }
    return acc;
}
// Along W from the fp32 plane of the H pass: columns are 3 floats apart.
__device__ __forceinline__ float vdsr_eval_blur_w(const float* row, int b, int R, int last, int org, const float* wts) {
#pragma clang fp contract(off)
    float acc = 0.f;
    for (int i = -R; i <= R; ++i) {
        int x = b + i;
        x = x < 0 ? 0 : (x > last ? last : x);
        acc += wts[i < 0 ? -i : i] * row[(x - org) * 3];
    }
    return acc;
}
// resize_bilinear_kernel's expression
__device__ __forceinline__ float vdsr_eval_bilinear(float v00, float v01, float v10, float v11, float wy, float wx) {
#pragma clang fp contract(off)
    return (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
}
__device__ __forceinline__ float vdsr_eval_to_pm1(float v) {
#pragma clang fp contract(off)
    return v * 2.0f - 1.0f;
}

__global__ __launch_bounds__(256) void vdsr_eval_pairs_kernel(const VdsrEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_vdsr_eval[];
    float* tab = reinterpret_cast<float*>(lds_vdsr_eval);
    float* wts = tab + 256;
    const int t = threadIdx.x;

    tab[t] = (float)t / 255.0f;

    const unsigned total = eval_total_tiles(a.table, a.n, SRX_VDSR_EVAL_TILE);
    for (unsigned tile = blockIdx.x; tile < total; tile += gridDim.x) {
        // 0. the record
        const srx_vdsr_eval_image im = eval_record_of_tile(a.table, a.n, tile);
        const float s = im.scaling_factor;
        const int H = im.height, W = im.width, R = patch_radius(s);
        const int Lh = patch_lr_size(H, s), Lw = patch_lr_size(W, s);
        const EvalTileAt here = eval_tile_at(im, tile, eval_tiles_along(W, SRX_VDSR_EVAL_TILE));
        const VdsrEvalAxis ay = vdsr_eval_axis(H, Lh, R, here.ty), ax = vdsr_eval_axis(W, Lw, R, here.tx);
        const VdsrEvalLds l = vdsr_eval_lds(ay.n_src, ax.n_src, ay.n_samp, ay.n_lo, ax.n_lo);
        uint8_t* src = lds_vdsr_eval + l.src;
        float* hp = reinterpret_cast<float*>(lds_vdsr_eval + l.hp);
        float* lo = reinterpret_cast<float*>(lds_vdsr_eval + l.lo);
        const float down_y = eval_scale(H, Lh), down_x = eval_scale(W, Lw);
        const float up_y = eval_scale(Lh, H), up_x = eval_scale(Lw, W);
        const uint8_t* img = a.arena + im.offset;
        const int pitch = ax.n_src * 3;                      // of src in bytes, of hp in floats

        if (t <= R) wts[t] = gaussian_tap_weight(t, R, patch_sigma(s));
        // 1. the source bytes: a run of `pitch` consecutive bytes per row.  Not stage_image_rows (pairs_device.h), whose
        //    eight loads in flight cost this kernel 43 registers (66 -> 109) for a loop that is not its long one
        {
            const int n = ay.n_src * pitch;
            const uint8_t* base = img + ((size_t)ay.src_first * W + ax.src_first) * 3;
            for (int o = t; o < n; o += 256) {
                const int row = o / pitch, rem = o - row * pitch;
                src[o] = base[(size_t)row * W * 3 + rem];
            }
        }
        __syncthreads();
        // 2. blur along H at the sampled rows
        {
            const int n = ay.n_samp * pitch;
            for (int o = t; o < n; o += 256) {
                const int k = o / pitch, rem = o - k * pitch;
                const int b = vdsr_eval_slot_index(ay, k, down_y, H);
                hp[o] = vdsr_eval_blur_h(src + rem, pitch, b, R, H - 1, ay.src_first, wts, tab);
            }
        }
        __syncthreads();
        // 3. the tile's low-resolution pixels: blur along W at the two sampled columns of each, then H x W -> Lh x Lw
        {
            const int run = ax.n_lo * 3, n = ay.n_lo * run;
            for (int o = t; o < n; o += 256) {
                const int i = o / run, q = o - i * run, j = q / 3, c = q - j * 3;
                const VdsrEvalTap py = vdsr_eval_tap(ay.lo_first + i, down_y, H), px = vdsr_eval_tap(ax.lo_first + j, down_x, W);
                const float* r0 = hp + vdsr_eval_slot(ay, ay.lo_first + i, 0, py.i0) * pitch + c;
                const float* r1 = hp + vdsr_eval_slot(ay, ay.lo_first + i, 1, py.i1) * pitch + c;
                const float v00 = vdsr_eval_blur_w(r0, px.i0, R, W - 1, ax.src_first, wts);
                const float v01 = vdsr_eval_blur_w(r0, px.i1, R, W - 1, ax.src_first, wts);
                const float v10 = vdsr_eval_blur_w(r1, px.i0, R, W - 1, ax.src_first, wts);
                const float v11 = vdsr_eval_blur_w(r1, px.i1, R, W - 1, ax.src_first, wts);
                lo[o] = vdsr_eval_bilinear(v00, v01, v10, v11, py.w, px.w);
            }
        }
        __syncthreads();
        // 4. Lh x Lw -> H x W, mapped to [-1, 1] and stored with hd
        {
            const int th = ay.out_last - ay.out_first + 1, run = (ax.out_last - ax.out_first + 1) * 3, n = th * run;
            const int lo_pitch = ax.n_lo * 3;
            const size_t at = ((size_t)ay.out_first * W + ax.out_first) * 3;
            float* sd = a.sd + im.out_offset + at;
            float* hd = a.hd + im.out_offset + at;
            const uint8_t* px0 = img + at;
            for (int o = t; o < n; o += 256) {
                const int i = o / run, q = o - i * run, j = q / 3, c = q - j * 3;
                const VdsrEvalTap py = vdsr_eval_tap(ay.out_first + i, up_y, Lh), px = vdsr_eval_tap(ax.out_first + j, up_x, Lw);
                const float* r0 = lo + (py.i0 - ay.lo_first) * lo_pitch + c;
                const float* r1 = lo + (py.i1 - ay.lo_first) * lo_pitch + c;
                const int x0 = (px.i0 - ax.lo_first) * 3, x1 = (px.i1 - ax.lo_first) * 3;
                const float v = vdsr_eval_bilinear(r0[x0], r0[x1], r1[x0], r1[x1], py.w, px.w);
                const size_t g = (size_t)i * W * 3 + q;
                sd[g] = vdsr_eval_to_pm1(v);
                hd[g] = vdsr_eval_to_pm1(tab[px0[g]]);
            }
        }
        __syncthreads();    // the next tile's step 0 overwrites wts, its step 1 src
    }
}

hipError_t launch_vdsr_eval_pairs(const VdsrEvalArgs& a, hipStream_t s) {
    return launch_with_lds<vdsr_eval_pairs_kernel>(dim3(kEvalGrid), dim3(256), kVdsrEvalLdsBytes, s, a);
}

}  // namespace srx
