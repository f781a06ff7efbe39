// enet_eval.hip -- EnhanceNet's evaluation pairs of a whole image set built on the device, one launch per set.
//
// The reference has no evaluation; its training degradation (enet/enet/datasets.py:95-127) is what a held-out image is
// scored against here, applied to the WHOLE image trimmed to multiples of 4: sd = imresize(hd, 25) (Pillow BILINEAR,
// antialiased), bq = imresize(sd, 400, 'bicubic') (Pillow BICUBIC, a = -0.5), all three as float32 / 127.5 - 1.  The decoded
// images sit in one uint8 arena and a table of srx_enet_eval_image records names an image, where its outputs start, how
// many tiles the records before it have, and the coefficient blocks of its two sides.  A record is cut into tiles of
// T x T hd pixels (T = SRX_ENET_EVAL_TILE, a multiple of 4: every sd pixel belongs to one tile).
//
// This is not enet_patch_pairs_kernel (enet_pairs.hip) with a larger S: that kernel holds a whole S x S crop in LDS, one
// square block of coefficients serves both axes, and every border is the crop's own.  Here an image has a block per side,
// the rows of a block near the image's edge differ from the interior's, and a tile's halo runs back through four passes
// and is cut by the image's edge.  What a tile reaches is read per axis by enet_eval_axis (patch_pairs.h) from the bounds
// of the blocks -- the words every pixel loop below takes its taps from, so a pixel cannot name a slot the footprint left
// out.  The arithmetic is resample_u8.hip's and enet_patch_pairs_kernel's, byte for byte (resample_byte, pairs_device.h):
// each resize is Pillow's two passes in Pillow's order, horizontal then vertical, each pass
//     out = clip8((2^21 + sum_k kk[k] * in[first + k]) >> 22)          (arithmetic shift)
// with a uint8 intermediate.  Everything before the final table lookup is integer.
//
// The grid is kEvalGrid workgroups of 256 threads that stride over the tiles (patch_pairs.h) -- each tile, all three
// channels, by one workgroup alone.  LDS (kEnetEvalLdsBytes = 40 KiB, enet_eval_lds): tab, 256 floats byte -> [-1, 1]
// (u8_to_pm1_kernel's two roundings), written once per workgroup; then regions a tile sizes from its own footprint
// (y: rows, x: columns).  Per tile, a barrier between the steps and one before the next tile's step 1:
//   0. the tile's record (eval_record_of_tile, pairs_device.h) and its two axes' footprints
//   1. cx, cy: the coefficient slices of the two axes -- the BILINEAR bounds and kk of sd_first .. sd_last, the BICUBIC
//      bounds and kk of out_first .. out_last; src [n_hd_y][n_hd_x][3] uint8 = rows hd_first_y .. hd_last_y, columns
//      hd_first_x .. hd_last_x of the image: consecutive lanes read consecutive bytes of an image row
//   2. hd = tab[src] at the tile's own pixels, stored; h1 [n_hd_y][n_sd_x][3] = src resampled along its rows
//   3. sdb [n_sd_y][n_sd_x][3] = h1 resampled along its columns; sd = tab[sdb] stored at the pixels the tile owns
//   4. h3 [n_sd_y][n_out_x][3] = sdb resampled along its rows
//   5. bq = tab[h3 resampled along its columns], stored straight from registers
// Every slot a step reads was written in full by the step before it: a pass reads the taps first .. first + count - 1 of
// an output, and the footprints are the union of those over the outputs of the next pass.  So the result does not depend
// on what the LDS held (SRX_POISON_LDS).  A tap loop has no branch (kk is zero past its count).  No atomics, no
// communication between workgroups, plain vector stores; consecutive lanes store consecutive floats of a row; only a
// record's own floats are written, never the padding between records.
//
// The table and the coefficient arena are trusted: srx_enet_eval_table_check (pairs_api.hip) keeps every image inside the
// arena, every side a multiple of 4 of at least 12, the offsets and first_tile the running sums (so no two records'
// outputs overlap and the search finds one record per tile), each block inside the arena of coefficients, built for its
// record's side and Pillow's in shape (counts in 1 .. ksize, taps inside the input, first indices and ends that do not
// decrease), and every tile's footprint inside the image, around the tile's own pixels and inside kEnetEvalLdsBytes.
#include "lds_launch.h"
#include "pairs_device.h"
#include "patch_pairs.h"

namespace srx {

namespace {

// The coefficient slices of one axis of a tile, in LDS: pointers into the region stage_coeffs fills
struct AxisCoeffs {
    int *down_bounds, *down_kk, *up_bounds, *up_kk;
    int words;
};
__device__ __forceinline__ AxisCoeffs axis_coeffs(int* region, const EnetEvalAxis& a) {
    AxisCoeffs c;
    c.down_bounds = region;
    c.down_kk = c.down_bounds + 2 * a.n_sd;
    c.up_bounds = c.down_kk + kEnetKDown * a.n_sd;
    c.up_kk = c.up_bounds + 2 * a.n_out;
    c.words = enet_eval_coeff_words(a.n_sd, a.n_out);
    return c;
}
// The four runs of consecutive words of `tables` (an axis's block past its header) that make up the slices, in order
__device__ __forceinline__ void stage_coeffs(const AxisCoeffs& c, const int32_t* tables, int side, const EnetEvalAxis& a, int t) {
    const EnetPairsTables T = enet_pairs_tables(side);
    const int n0 = 2 * a.n_sd, n1 = n0 + kEnetKDown * a.n_sd, n2 = n1 + 2 * a.n_out;
    for (int o = t; o < c.words; o += 256) {
        const int32_t* from = o < n0   ? tables + T.down_bounds + 2 * a.sd_first + o
                              : o < n1 ? tables + T.down_kk + kEnetKDown * a.sd_first + (o - n0)
                              : o < n2 ? tables + T.up_bounds + 2 * a.out_first + (o - n1)
                                       : tables + T.up_kk + kEnetKUp * a.out_first + (o - n2);
        c.down_bounds[o] = *from;
    }
}

}  // namespace

__global__ __launch_bounds__(256) void enet_eval_pairs_kernel(const EnetEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_enet_eval[];
    float* tab = reinterpret_cast<float*>(lds_enet_eval);
    const int t = threadIdx.x;

    tab[t] = byte_to_pm1(t);

    const unsigned total = eval_total_tiles(a.table, a.n, SRX_ENET_EVAL_TILE);
    for (unsigned tile = blockIdx.x; tile < total; tile += gridDim.x) {
        // 0. the record and what the tile reaches
        const srx_enet_eval_image im = eval_record_of_tile(a.table, a.n, tile);
        const int H = im.height, W = im.width, w = W >> 2;
        const int32_t* tables_x = a.coeffs + im.width_coeffs + kEnetEvalBlockHeader;
        const int32_t* tables_y = a.coeffs + im.height_coeffs + kEnetEvalBlockHeader;
        const EvalTileAt here = eval_tile_at(im, tile, eval_tiles_along(W, SRX_ENET_EVAL_TILE));
        const EnetEvalAxis ay = enet_eval_axis(tables_y, H, here.ty), ax = enet_eval_axis(tables_x, W, here.tx);
        const EnetEvalLds l = enet_eval_lds(ay.n_hd, ax.n_hd, ay.n_sd, ax.n_sd, ay.n_out, ax.n_out);
        const AxisCoeffs cx = axis_coeffs(reinterpret_cast<int*>(lds_enet_eval + l.coeff_x), ax);
        const AxisCoeffs cy = axis_coeffs(reinterpret_cast<int*>(lds_enet_eval + l.coeff_y), ay);
        uint8_t* src = lds_enet_eval + l.src;
        uint8_t* h1 = lds_enet_eval + l.h1;
        uint8_t* sdb = lds_enet_eval + l.sd;
        uint8_t* h3 = lds_enet_eval + l.h3;
        const uint8_t* img = a.arena + im.offset;
        const int pitch = ax.n_hd * 3, p1 = ax.n_sd * 3, p3 = ax.n_out * 3;      // of src; of h1 and sdb; of h3 and a tile row
        // d >= 3 and, every count being at most kEnetEvalMaxReach = 128 (the table check), n < 128 * 384 and n d < 2^25
        const SmallDiv by_p1(p1), by_p3(p3);

        // 1. the coefficient slices and the source bytes: a run of `pitch` consecutive bytes per row
        stage_coeffs(cx, tables_x, W, ax, t);
        stage_coeffs(cy, tables_y, H, ay, t);
        stage_image_rows(src, img + ((size_t)ay.hd_first * W + ax.hd_first) * 3, (size_t)W * 3, ay.n_hd * pitch, pitch, t);      // d = pitch, n: as above
        __syncthreads();
        // 2a. hd: the tile's own pixels from the staged bytes
        {
            const int n = ay.n_out * p3;
            const uint8_t* own = src + (ay.out_first - ay.hd_first) * pitch + (ax.out_first - ax.hd_first) * 3;
            float* hd = a.hd + im.out_offset + ((size_t)ay.out_first * W + ax.out_first) * 3;
#pragma unroll 4
            for (int o = t; o < n; o += 256) {
                const int i = by_p3(o), q = o - i * p3;
                hd[(size_t)i * W * 3 + q] = tab[own[i * pitch + q]];
            }
        }
        // 2b. h1[r][j][c] = the BILINEAR pass along row r of src
        {
            const int n = ay.n_hd * p1;
            for (int o = t; o < n; o += 256) {
                const int r = by_p1(o), rem = o - r * p1, j = rem / 3, c = rem - j * 3;
                const int first = cx.down_bounds[2 * j] - ax.hd_first, cnt = cx.down_bounds[2 * j + 1];
                h1[o] = (uint8_t)resample_byte<kEnetKDown>(src + r * pitch + first * 3 + c, 3, cx.down_kk + j * kEnetKDown, cnt);
            }
        }
        __syncthreads();
        // 3. sdb[i][j][c] = the BILINEAR pass along column (j, c) of h1; the pixels this tile owns are stored
        {
            const int n = ay.n_sd * p1;
            float* sd = a.sd + im.sd_offset;
            for (int o = t; o < n; o += 256) {
                const int i = by_p1(o), rem = o - i * p1, j = rem / 3;
                const int first = cy.down_bounds[2 * i] - ay.hd_first, cnt = cy.down_bounds[2 * i + 1];
                const int v = resample_byte<kEnetKDown>(h1 + first * p1 + rem, p1, cy.down_kk + i * kEnetKDown, cnt);
                sdb[o] = (uint8_t)v;
                const int gi = ay.sd_first + i, gj = ax.sd_first + j;
                if (gi >= ay.own_first && gi <= ay.own_last && gj >= ax.own_first && gj <= ax.own_last)
                    sd[((size_t)gi * w + ax.sd_first) * 3 + rem] = tab[v];
            }
        }
        __syncthreads();
        // 4. h3[i][J][c] = the BICUBIC pass along row i of sdb
        {
            const int n = ay.n_sd * p3;
            for (int o = t; o < n; o += 256) {
                const int i = by_p3(o), rem = o - i * p3, J = rem / 3, c = rem - J * 3;
                const int first = cx.up_bounds[2 * J] - ax.sd_first, cnt = cx.up_bounds[2 * J + 1];
                h3[o] = (uint8_t)resample_byte<kEnetKUp>(sdb + i * p1 + first * 3 + c, 3, cx.up_kk + J * kEnetKUp, cnt);
            }
        }
        __syncthreads();
        // 5. bq[I][J][c] = the BICUBIC pass along column (J, c) of h3
        {
            const int n = ay.n_out * p3;
            float* bq = a.bq + im.out_offset + ((size_t)ay.out_first * W + ax.out_first) * 3;
#pragma unroll 4
            for (int o = t; o < n; o += 256) {
                const int I = by_p3(o), rem = o - I * p3;
                const int first = cy.up_bounds[2 * I] - ay.sd_first, cnt = cy.up_bounds[2 * I + 1];
                bq[(size_t)I * W * 3 + rem] = tab[resample_byte<kEnetKUp>(h3 + first * p3 + rem, p3, cy.up_kk + I * kEnetKUp, cnt)];
            }
        }
        __syncthreads();    // the next tile's step 1 overwrites the slices and src
    }
}

hipError_t launch_enet_eval_pairs(const EnetEvalArgs& a, hipStream_t s) {
    return launch_with_lds<enet_eval_pairs_kernel>(dim3(kEvalGrid), dim3(256), kEnetEvalLdsBytes, s, a);
}

}  // namespace srx
