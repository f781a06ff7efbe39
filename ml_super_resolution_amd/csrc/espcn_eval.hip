// espcn_eval.hip -- ESPCN's evaluation pairs of a whole image set built on the device, one launch per set.
//
// The reference prepares an evaluation pair per image on the host (espcn/espcn/experiment_test.py:60-98): the image is
// trimmed to multiples of r (:68-71), mapped to [-1, 1] (:73), blurred with sigma = 0.5 (r - 1), borders replicated at the
// TRIMMED edge (:75-85), decimated at offset r / 2 (:87) and the label is the trimmed image in sub-pixel layout (:91-96).
// Here the trimmed images sit in one uint8 arena and a table of srx_eval_image records says where each lies, where its
// outputs start and how many tiles the images before it have.  An image is cut into tiles of T x T lr pixels
// (T = SRX_ESPCN_EVAL_TILE); a tile is what espcn_patch_pairs_kernel (espcn_pairs.hip) calls a patch of p = T at
// (x, y) = (T r tx, T r ty) with no flip, except that it may hang over the image's right and lower edge: its reads are
// clamped to the image like all others, and only i < h', j < w' is computed and stored.  The LDS layout, the steps and the
// two tap loops (pairs_device.h) are that kernel's, so a patch and the image it was cut from hold the same bits.
//
// The grid is kEvalGrid workgroups of 256 threads that stride over the tiles (patch_pairs.h) -- each tile by one workgroup,
// alone.  Per workgroup, once: tab and wts.  Per tile (a barrier between the steps, and one before the next tile's step 1
// overwrites reg):
//   0. the tile's image (eval_record_of_tile, pairs_device.h); ty, tx from the image's tiles per row
//   1. reg = the bytes of image rows T r ty - R .. T r (ty + 1) - 1 + R and the columns likewise, indices clamped
//   2. pl = blur along H of tab[reg] at the sampled rows i < ph; label = tab[reg] in label layout, stored: the qw 3 r^2
//      floats of a tile row to consecutive lanes
//   3. lr = blur along W of pl at the sampled columns j < qw, stored: the 3 qw floats of a tile row to consecutive lanes
// ph = min(T, h' - T ty), qw = min(T, w' - T tx).  Every slot a step reads was written by the step before it (step 2 reads
// region rows off + r i - R .. off + r i + R for i < ph and all span columns; step 1 writes the whole region), so the
// result does not depend on what the LDS held (SRX_POISON_LDS).  No atomics, no communication between workgroups, plain
// vector stores.
//
// The table is trusted: srx_espcn_eval_table_check (pairs_api.hip) keeps every image inside the arena, its sizes multiples
// of r, lr_offset and first_tile the running sums (so no two images' outputs overlap and the search finds one image per
// tile) and the total inside lr / label.  Every global read is at a clamped (row, column) of such an image.
#include "lds_launch.h"
#include "pairs_device.h"
#include "patch_pairs.h"

namespace srx {

template <int R_>
__global__ __launch_bounds__(256) void espcn_eval_pairs_kernel(const EspcnEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds_espcn_eval[];
    constexpr int r = R_, RAD = 2 * (R_ - 1), CH = 3 * R_ * R_, T = SRX_ESPCN_EVAL_TILE;   // RAD == espcn_radius(r) (the launcher)
    constexpr int P = T * r, E = P + 2 * RAD, E3 = E * 3;
    constexpr int span = r * (T - 1) + 1 + 2 * RAD, S3 = span * 3, off = r / 2;
    float* tab = lds_espcn_eval;
    float* wts = lds_espcn_eval + 256;
    uint8_t* reg = reinterpret_cast<uint8_t*>(lds_espcn_eval + 272);
    float* pl = reinterpret_cast<float*>(reg + espcn_region_bytes(r, T));
    const int t = threadIdx.x;

    tab[t] = byte_to_pm1_f64(t);
    if (t <= RAD) wts[t] = gaussian_tap_weight(t, RAD, patch_sigma((float)r));

    const srx_eval_image last = a.table[a.n - 1];
    const unsigned total = last.first_tile + (unsigned)eval_image_tiles(last.width / r, last.height / r, T);
    for (unsigned tile = blockIdx.x; tile < total; tile += gridDim.x) {
        // 0. the image
        const srx_eval_image im = eval_record_of_tile(a.table, a.n, tile);
        const int hp = im.height / r, wp = im.width / r, tiles_x = eval_tiles_along(wp, T);
        const int local = (int)(tile - im.first_tile), ty = local / tiles_x, tx = local - ty * tiles_x;
        const int i0 = ty * T, j0 = tx * T;
        const int ph = hp - i0 < T ? hp - i0 : T, qw = wp - j0 < T ? wp - j0 : T;
        // 1. the region
        {
            const uint8_t* img = a.arena + im.offset;
            constexpr int n = E * E3;
            const int y0 = i0 * r - RAD, x0 = j0 * r - RAD, hm = im.height - 1, wm = im.width - 1;
#pragma unroll 8
            for (int o = t; o < n; o += 256) {
                const int row = o / E3, rem = o - row * E3, col = rem / 3, c = rem - col * 3;
                int yy = y0 + row, xx = x0 + col;
                yy = yy < 0 ? 0 : (yy > hm ? hm : yy);
                xx = xx < 0 ? 0 : (xx > wm ? wm : xx);
                reg[o] = img[((size_t)yy * im.width + xx) * 3 + c];
            }
        }
        __syncthreads();
        // 2a. blur along H at the sampled rows: pl[i][s][c], image row T r ty + off + r i = region row RAD + off + r i,
        //     region column off + s
        {
            const int n = ph * S3;
            for (int o = t; o < n; o += 256) {
                const int i = o / S3, sc = o - i * S3;
                pl[o] = espcn_blur_h_taps<RAD>(reg + (off + r * i) * E3 + off * 3 + sc, E3, wts, tab);
            }
        }
        // 2b. the label: out[i0 + i][j0 + j][(dy r + dx) 3 + c] = image[(i0 + i) r + dy][(j0 + j) r + dx][c]
        {
            const int run = qw * CH, n = ph * run;
            float* label = a.label + (size_t)im.lr_offset * (r * r) + ((size_t)i0 * wp + j0) * CH;
            for (int o = t; o < n; o += 256) {
                const int i = o / run, q0 = o - i * run, j = q0 / CH, q = q0 - j * CH;
                const int d = q / 3, c = q - d * 3, dy = d / r, dx = d - dy * r;
                label[(size_t)i * wp * CH + q0] = tab[reg[(RAD + i * r + dy) * E3 + (RAD + j * r + dx) * 3 + c]];
            }
        }
        __syncthreads();
        // 3. blur along W at the sampled columns: column T r tx + off + r j is span index RAD + r j
        {
            const int run = qw * 3, n = ph * run;
            float* lr = a.lr + (size_t)im.lr_offset + ((size_t)i0 * wp + j0) * 3;
            for (int o = t; o < n; o += 256) {
                const int i = o / run, q0 = o - i * run, j = q0 / 3, c = q0 - j * 3;
                lr[(size_t)i * wp * 3 + q0] = espcn_blur_w_taps<RAD>(pl + i * S3 + (r * j) * 3 + c, wts);
            }
        }
        __syncthreads();    // the next tile's step 1 overwrites reg, its step 2 pl
    }
}

hipError_t launch_espcn_eval_pairs(const EspcnEvalArgs& a, hipStream_t s) {
    const size_t lds = espcn_eval_lds_bytes(a.r);
    // the kernel's constants are these functions' values
    if (espcn_radius(a.r) != 2 * (a.r - 1) || espcn_eval_tile() != SRX_ESPCN_EVAL_TILE ||
        espcn_eval_region(a.r) != espcn_eval_tile() * a.r + 4 * (a.r - 1) ||
        espcn_eval_span(a.r) != a.r * (espcn_eval_tile() - 1) + 1 + 4 * (a.r - 1) || lds > 64 * 1024)
        return hipErrorInvalidValue;
    switch (a.r) {
        case 2: return launch_with_lds<espcn_eval_pairs_kernel<2>>(dim3(kEvalGrid), dim3(256), lds, s, a);
        case 3: return launch_with_lds<espcn_eval_pairs_kernel<3>>(dim3(kEvalGrid), dim3(256), lds, s, a);
        case 4: return launch_with_lds<espcn_eval_pairs_kernel<4>>(dim3(kEvalGrid), dim3(256), lds, s, a);
    }
    return hipErrorInvalidValue;
}

}  // namespace srx
