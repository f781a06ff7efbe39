// srcnn_eval.hip -- SRCNN's evaluation pairs of a whole image set built on the device, one launch per set.
//
// The reference scores nothing; its in-graph degradation (srcnn/srcnn.py:89-93: tf.image.resize_bicubic down by the factor
// and back up) and the margin its VALID network removes (:132-139) are what a held-out image is scored against here,
// applied to the WHOLE image.  The decoded images sit in one uint8 arena and a table of srx_srcnn_eval_image records names
// an image, where its outputs start and how many tiles the records before it have; f and border are the launch's.  A
// record is cut into tiles of T x T pixels of sd (T = SRX_SRCNN_EVAL_TILE).  The arithmetic is that of the route it
// replaces (u8_to_pm1_kernel's expression, then two srx_resize_bicubic_tf launches), bit for bit:
//   hd_full = (float)byte / 127.5f - 1.0f                                  two roundings, contraction off
//   lo      = the 16-tap loop of resize_bicubic_tf_kernel on hd_full       (H x W -> h x w = H / f x W / f)
//   sd      = the same resize of lo                                        (h x w -> H x W)
// each with the scale (float)in / (float)out of its own axis and direction, as srx_resize_bicubic_tf forms it, and the tap
// positions and weights of bicubic_tf_taps (bicubic_tf.h), the text resize_bicubic_tf_kernel compiles.  Both resizes are
// evaluated separably: the kernel's inner sum
//     v = 0.f; for k in 0..3: v += wx[k] * row[ix[k]]
// depends on (input row, output column, channel) alone -- the argument srcnn_pairs.hip makes for its up pass -- so it is
// computed ONCE per input row into LDS (`hdn`, `hup`), and the outer sum acc = 0.f; for r in 0..3: acc += wy[r] * v[iy[r]]
// adds the same four floats in the same order (srcnn_eval_sum4, contraction off).
//
// This is not srcnn_patch_pairs_kernel (srcnn_pairs.hip) with a larger S: that kernel holds whole rows of a square crop of
// at most 256 pixels in LDS, one tap table serves rows and columns, and every border is the crop's own.  An image's two
// sides differ, so it has two down scales and two up scales and four tap tables; its sides are arbitrary; a tile's borders
// are the image's.  What a tile reaches is derived per axis by srcnn_eval_axis (patch_pairs.h) from srcnn_pairs_lower, the
// floor bicubic_tf_taps forms; the pixel loops take their indices from bicubic_tf_taps and subtract the footprint's first
// index, so a tap outside the footprint would show up as a wrong value, not as a stray read: every index bicubic_tf_taps
// returns is clamped to its input and lies between the footprint's two ends.  The decimation shortcut of srcnn_pairs.hip
// (side == (side / f) f) is not taken: every side runs the sixteen taps.
//
// The grid is kEvalGrid workgroups of 256 threads that stride over the tiles (patch_pairs.h) -- each tile, all three
// channels, by one workgroup alone.  LDS (kSrcnnEvalLdsBytes = 40 KiB, srcnn_eval_lds): tab, 256 floats byte -> [-1, 1],
// written once per workgroup; then regions a tile sizes from its own footprint (y: rows, x: columns).  Per tile, a barrier
// between the steps and one before the next tile's step 1:
//   0. the tile's record (eval_record_of_tile, pairs_device.h), its four scales and its two axes' footprints
//   1. the four tap tables: uy [n_out_y] and ux [n_out_x] of the up pass, dy [n_lo_y] and dx [n_lo_x] of the down pass;
//      src [n_src_y][n_src_x][3] uint8 = rows src_first_y .. src_last_y, columns src_first_x .. src_last_x of the image:
//      consecutive lanes read consecutive bytes of an image row
//   2. hd = tab[byte] at the tile's own pixels inside the margin, read from the arena (a tile's own pixels need not all lie
//      inside src) and stored; hdn [n_src_y][n_lo_x][3] = the inner sum of the down pass along every staged row
//   3. lo [n_lo_y][n_lo_x][3] = the outer sum of the down pass
//   4. hup [n_lo_y][n_out_x][3] = the inner sum of the up pass along every row of lo
//   5. sd = the outer sum of the up pass, stored straight from registers; the same value to bq where the pixel lies
//      inside the margin
// Every slot a step reads was written in full by an earlier step of the same tile: step 2 reads src at the taps of dx,
// columns between src_first_x and src_last_x, in every staged row; step 3 reads hdn at the taps of dy, rows between
// src_first_y and src_last_y; step 4 reads lo at the taps of ux, step 5 hup at the taps of uy, both inside lo_first ..
// lo_last.  So the result does not depend on what the LDS held (SRX_POISON_LDS).  No atomics, no communication between
// workgroups, plain vector stores; consecutive lanes store consecutive floats of a row (steps 3 to 5 read LDS the same
// way, one bank per lane); only a record's own floats are written, never the padding between records.
//
// The table is trusted: srx_srcnn_eval_table_check (pairs_api.hip) keeps f inside 2..8, border >= 0, every image inside the
// arena with side / f >= 1 and side > 2 border, the offsets and first_tile the running sums (so no two records' outputs
// overlap and the search finds one record per tile), the totals inside sd, bq and hd, and the layout of every tile inside
// kSrcnnEvalLdsBytes with at most kSrcnnEvalMaxReach indices per range.  Every global read is at a (row, column) inside
// such an image.
#include "bicubic_tf.h"
#include "lds_launch.h"
#include "pairs_device.h"
#include "patch_pairs.h"

namespace srx {

static_assert(sizeof(SrcnnTaps) == 32, "srcnn_eval_lds counts 32 bytes per record");
static_assert(sizeof(srx_srcnn_eval_image) == 40, "srx_srcnn_eval_image is 40 bytes (include/srx.h)");

// One sum of resize_bicubic_tf_kernel, inner or outer: four products added to 0.f in tap order, each product and each sum
// rounded on its own.
__device__ __forceinline__ float srcnn_eval_sum4(const float (&w)[4], float v0, float v1, float v2, float v3) {
#pragma clang fp contract(off)
    float acc = 0.f;
    acc += w[0] * v0;
    acc += w[1] * v1;
    acc += w[2] * v2;
    acc += w[3] * v3;
    return acc;
}

__global__ __launch_bounds__(256) void srcnn_eval_pairs_kernel(const SrcnnEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_srcnn_eval[];
    float* tab = reinterpret_cast<float*>(lds_srcnn_eval);
    const int t = threadIdx.x;
    const int f = a.f, b = a.border;

    tab[t] = byte_to_pm1(t);

    const unsigned total = eval_total_tiles(a.table, a.n, SRX_SRCNN_EVAL_TILE);
    for (unsigned tile = blockIdx.x; tile < total; tile += gridDim.x) {
        // 0. the record and what the tile reaches
        const srx_srcnn_eval_image im = eval_record_of_tile(a.table, a.n, tile);
        const int H = im.height, W = im.width, Lh = H / f, Lw = W / f;
        const EvalTileAt here = eval_tile_at(im, tile, eval_tiles_along(W, SRX_SRCNN_EVAL_TILE));
        const SrcnnEvalAxis ay = srcnn_eval_axis(H, f, here.ty), ax = srcnn_eval_axis(W, f, here.tx);
        const SrcnnEvalLds l = srcnn_eval_lds(ay.n_src, ax.n_src, ay.n_lo, ax.n_lo, ay.n_out, ax.n_out);
        SrcnnTaps* uy = reinterpret_cast<SrcnnTaps*>(lds_srcnn_eval + l.up_y);        // the four tables lie back to back
        const SrcnnTaps* ux = reinterpret_cast<const SrcnnTaps*>(lds_srcnn_eval + l.up_x);
        const SrcnnTaps* dy = reinterpret_cast<const SrcnnTaps*>(lds_srcnn_eval + l.down_y);
        const SrcnnTaps* dx = reinterpret_cast<const SrcnnTaps*>(lds_srcnn_eval + l.down_x);
        uint8_t* src = lds_srcnn_eval + l.src;
        float* hdn = reinterpret_cast<float*>(lds_srcnn_eval + l.hdn);
        float* lo = reinterpret_cast<float*>(lds_srcnn_eval + l.lo);
        float* hup = reinterpret_cast<float*>(lds_srcnn_eval + l.hup);
        const float down_y = eval_scale(H, Lh), down_x = eval_scale(W, Lw);
        const float up_y = eval_scale(Lh, H), up_x = eval_scale(Lw, W);
        const uint8_t* img = a.arena + im.offset;
        const int pitch = ax.n_src * 3, p1 = ax.n_lo * 3, p3 = ax.n_out * 3;      // of src; of hdn and lo; of hup and a tile row
        // d >= 3 and, every count being at most kSrcnnEvalMaxReach = 128 (the table check), n < 128 * 384 and n d < 2^25
        const SmallDiv by_p1(p1), by_p3(p3);

        // 1a. the tap tables, in the order of the layout: uy, ux, dy, dx
        {
            const int n0 = ay.n_out, n1 = n0 + ax.n_out, n2 = n1 + ay.n_lo, n3 = n2 + ax.n_lo;
            for (int o = t; o < n3; o += 256) {
                int index, limit;
                float scale;
                if (o < n0) { index = ay.out_first + o; scale = up_y; limit = Lh; }
                else if (o < n1) { index = ax.out_first + (o - n0); scale = up_x; limit = Lw; }
                else if (o < n2) { index = ay.lo_first + (o - n1); scale = down_y; limit = H; }
                else { index = ax.lo_first + (o - n2); scale = down_x; limit = W; }
                bicubic_tf_taps(index, scale, limit, uy[o].idx, uy[o].w);
            }
        }
        // 1b. the source bytes: a run of `pitch` consecutive bytes per row
        stage_image_rows(src, img + ((size_t)ay.src_first * W + ax.src_first) * 3, (size_t)W * 3, ay.n_src * pitch, pitch, t);      // d = pitch, n: as above
        __syncthreads();
        // 2a. hd: the tile's own pixels inside the margin, rows r0 .. r1 and columns c0 .. c1 of the image
        {
            const int r0 = ay.out_first > b ? ay.out_first : b, r1 = ay.out_last < H - 1 - b ? ay.out_last : H - 1 - b;
            const int c0 = ax.out_first > b ? ax.out_first : b, c1 = ax.out_last < W - 1 - b ? ax.out_last : W - 1 - b;
            if (r1 >= r0 && c1 >= c0) {
                const int run = (c1 - c0 + 1) * 3, n = (r1 - r0 + 1) * run;       // run >= 3, n <= T * 3 T
                const SmallDiv by_run(run);
                const uint8_t* own = img + ((size_t)r0 * W + c0) * 3;
                float* hd = a.hd + im.crop_offset + ((size_t)(r0 - b) * (W - 2 * b) + (c0 - b)) * 3;
#pragma unroll 4
                for (int o = t; o < n; o += 256) {
                    const int i = by_run(o), q = o - i * run;
                    hd[(size_t)i * (W - 2 * b) * 3 + q] = tab[own[(size_t)i * W * 3 + q]];
                }
            }
        }
        // 2b. hdn[r][j][c]: the inner sum of the H x W -> Lh x Lw resize along staged row r
        {
            const int n = ay.n_src * p1;
            for (int o = t; o < n; o += 256) {
                const int r = by_p1(o), rem = o - r * p1, j = rem / 3, c = rem - j * 3;
                const SrcnnTaps tx_ = dx[j];
                const uint8_t* row = src + r * pitch + c;
                const int x0 = ax.src_first;
                hdn[o] = srcnn_eval_sum4(tx_.w, tab[row[(tx_.idx[0] - x0) * 3]], tab[row[(tx_.idx[1] - x0) * 3]],
                                         tab[row[(tx_.idx[2] - x0) * 3]], tab[row[(tx_.idx[3] - x0) * 3]]);
            }
        }
        __syncthreads();
        // 3. lo[i][j][c]: the outer sum
        {
            const int n = ay.n_lo * p1;
            for (int o = t; o < n; o += 256) {
                const int i = by_p1(o), rem = o - i * p1;
                const SrcnnTaps ty_ = dy[i];
                const float* col = hdn + rem;
                const int y0 = ay.src_first;
                lo[o] = srcnn_eval_sum4(ty_.w, col[(ty_.idx[0] - y0) * p1], col[(ty_.idx[1] - y0) * p1], col[(ty_.idx[2] - y0) * p1],
                                        col[(ty_.idx[3] - y0) * p1]);
            }
        }
        __syncthreads();
        // 4. hup[i][J][c]: the inner sum of the Lh x Lw -> H x W resize along row i of lo
        {
            const int n = ay.n_lo * p3;
            for (int o = t; o < n; o += 256) {
                const int i = by_p3(o), rem = o - i * p3, J = rem / 3, c = rem - J * 3;
                const SrcnnTaps tx_ = ux[J];
                const float* row = lo + i * p1 + c;
                const int x0 = ax.lo_first;
                hup[o] = srcnn_eval_sum4(tx_.w, row[(tx_.idx[0] - x0) * 3], row[(tx_.idx[1] - x0) * 3], row[(tx_.idx[2] - x0) * 3],
                                         row[(tx_.idx[3] - x0) * 3]);
            }
        }
        __syncthreads();
        // 5. sd[I][J][c]: the outer sum, stored; and to bq where (I, J) lies inside the margin
        {
            const int n = ay.n_out * p3, Wc = W - 2 * b;
            float* sd = a.sd + im.out_offset + ((size_t)ay.out_first * W + ax.out_first) * 3;
            float* bq = a.bq + im.crop_offset;
#pragma unroll 4
            for (int o = t; o < n; o += 256) {
                const int i = by_p3(o), rem = o - i * p3, j = rem / 3;
                const SrcnnTaps ty_ = uy[i];
                const float* col = hup + rem;
                const int y0 = ay.lo_first;
                const float v = srcnn_eval_sum4(ty_.w, col[(ty_.idx[0] - y0) * p3], col[(ty_.idx[1] - y0) * p3], col[(ty_.idx[2] - y0) * p3],
                                                col[(ty_.idx[3] - y0) * p3]);
                sd[(size_t)i * W * 3 + rem] = v;
                const int I = ay.out_first + i, J = ax.out_first + j;
                if (I >= b && I < H - b && J >= b && J < W - b) bq[((size_t)(I - b) * Wc + (J - b)) * 3 + (rem - j * 3)] = v;
            }
        }
        __syncthreads();    // the next tile's step 1 overwrites the tables and src
    }
}

hipError_t launch_srcnn_eval_pairs(const SrcnnEvalArgs& a, hipStream_t s) {
    return launch_with_lds<srcnn_eval_pairs_kernel>(dim3(kEvalGrid), dim3(256), kSrcnnEvalLdsBytes, s, a);
}

}  // namespace srx
