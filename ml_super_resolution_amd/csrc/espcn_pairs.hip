// espcn_pairs.hip -- ESPCN's training pairs sampled on the device from a resident image set, one launch per batch.
//
// The reference prepares every (lr patch, sub-pixel label) pair ahead of training (espcn/espcn/dataset.py:81-158): the WHOLE
// image is mapped to [-1, 1] (:94) and blurred with sigma = 0.5 (r - 1), borders replicated at the image's edge (:97-101);
// the image is tiled into P x P patches, P = p r (:110-113), each in its four flips (:121-122); the lr patch is the blurred
// image decimated at offset r / 2 (:116-118) and the label is the HR patch in sub-pixel layout (:140-156).  Here the decoded
// images sit in one uint8 arena on the device and a batch is B records {image, patch corner, flips} (srx_patch_src).  A
// blurred value depends on the image within the radius R only, so the blur is evaluated just where it is sampled, with its
// source indices clamped to the IMAGE: the same numbers as blurring the whole image, per entry, from the entry's record alone.
//
// One workgroup (256 threads) per entry, all three channels; everything between the uint8 reads and the fp32 stores is in LDS:
//   tab   256 floats        tab[b] = (float)((double)b / 127.5 - 1.0): thread t writes entry t -- the reference's float64
//                           arithmetic, so the label is bit-exact, with no fp64 in the loops
//   wts   16 floats         the gaussian weights (threads 0 .. R write 0 .. R; nothing else is read), R <= 6
//   reg   E x E x 3 bytes   E = P + 2R: image rows y - R .. y + P - 1 + R, columns x - R .. x + P - 1 + R, indices clamped
//                           to the image as they are read
//   pl    p x span x 3 fp32 the p sampled rows blurred along H, over the span = r (p - 1) + 1 + 2R columns the W pass reads
// Steps (a barrier between them):
//   1. tab, wts, reg are written in full
//   2. pl = blur along H of tab[reg] at the p sampled rows; label = tab[reg] of the flipped patch in label layout, stored:
//      consecutive floats of the entry's p p 3 r^2 to consecutive lanes
//   3. lr = blur along W of pl at the p sampled columns, flipped, stored: consecutive floats of the entry's p p 3
// gaussian_1d_kernel's arithmetic: fp32 expf weights normalised by their sum in the same order, taps -R .. R in order, H
// first; the two tap loops are pairs_device.h's (espcn_blur_h_taps, espcn_blur_w_taps: every product and sum rounded), shared
// with espcn_eval.hip, whose whole-image pairs hold these patches bit for bit.  Every slot a step reads was written by the step before it, so the result does not depend on what the LDS held
// (SRX_POISON_LDS).  No atomics, no communication between workgroups, plain vector stores.
//
// The table is trusted: srx_espcn_patch_table_check (pairs_api.hip) keeps x, y, x + P, y + P inside the image and the image
// inside the arena; every global read is at a clamped (row, column) of that image.  patch_pairs.h holds the sizes both
// sides derive (radius, region, span, LDS bytes).
#include "lds_launch.h"
#include "pairs_device.h"
#include "patch_pairs.h"

namespace srx {

template <int R_>
__global__ __launch_bounds__(256) void espcn_patch_pairs_kernel(const EspcnPairsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds_espcn[];
    constexpr int r = R_, RAD = 2 * (R_ - 1), CH = 3 * R_ * R_;   // RAD == espcn_radius(r) (checked in the launcher)
    const int p = a.p, P = p * r, E = P + 2 * RAD, E3 = E * 3;
    const int span = r * (p - 1) + 1 + 2 * RAD, S3 = span * 3, off = r / 2;
    float* tab = lds_espcn;
    float* wts = lds_espcn + 256;
    uint8_t* reg = reinterpret_cast<uint8_t*>(lds_espcn + 272);
    float* pl = reinterpret_cast<float*>(reg + espcn_region_bytes(r, p));
    const int t = threadIdx.x;
    const unsigned e = blockIdx.x;
    const srx_patch_src src = a.table[e];
    const bool fw = src.flip & 1, fh = src.flip & 2;

    // 1. the byte table, the weights, the region
    tab[t] = byte_to_pm1_f64(t);
    if (t <= RAD) wts[t] = gaussian_tap_weight(t, RAD, patch_sigma((float)r));
    {
        const uint8_t* img = a.arena + src.offset;
        const int n = E * E3;
        const int y0 = src.y - RAD, x0 = src.x - RAD, hm = src.height - 1, wm = src.width - 1;
#pragma unroll 8
        for (int o = t; o < n; o += 256) {
            const int row = o / E3, rem = o - row * E3, col = rem / 3, c = rem - col * 3;
            int yy = y0 + row, xx = x0 + col;
            yy = yy < 0 ? 0 : (yy > hm ? hm : yy);
            xx = xx < 0 ? 0 : (xx > wm ? wm : xx);
            reg[o] = img[((size_t)yy * src.width + xx) * 3 + c];
        }
    }
    __syncthreads();
    // 2a. blur along H at the sampled rows: pl[i][s][c], image row y + off + r i = region row RAD + off + r i, image column
    //     x + off - RAD + s = region column off + s
    {
        const int n = p * S3;
        for (int o = t; o < n; o += 256) {
            const int i = o / S3, sc = o - i * S3;
            const uint8_t* b = reg + (off + r * i) * E3 + off * 3 + sc;     // tap -RAD
            pl[o] = espcn_blur_h_taps<RAD>(b, E3, wts, tab);
        }
    }
    // 2b. the label: out[i][j][(dy r + dx) 3 + c] = patch[i r + dy][j r + dx][c] of the flipped patch
    {
        const int n = p * p * CH;
        float* label = a.label + (size_t)e * n;
        for (int o = t; o < n; o += 256) {
            const int pix = o / CH, q = o - pix * CH, i = pix / p, j = pix - i * p;
            const int d = q / 3, c = q - d * 3, dy = d / r, dx = d - dy * r;
            int ya = i * r + dy, xa = j * r + dx;
            ya = fh ? P - 1 - ya : ya;
            xa = fw ? P - 1 - xa : xa;
            label[o] = tab[reg[(RAD + ya) * E3 + (RAD + xa) * 3 + c]];
        }
    }
    __syncthreads();
    // 3. blur along W at the sampled columns: column x + off + r j' is span index RAD + r j'
    {
        const int n = p * p * 3;
        float* lr = a.lr + (size_t)e * n;
        for (int o = t; o < n; o += 256) {
            const int pix = o / 3, c = o - pix * 3, i = pix / p, j = pix - i * p;
            const int is = fh ? p - 1 - i : i, js = fw ? p - 1 - j : j;
            const float* b = pl + is * S3 + (r * js) * 3 + c;                // tap -RAD
            lr[o] = espcn_blur_w_taps<RAD>(b, wts);
        }
    }
}

hipError_t launch_espcn_patch_pairs(const EspcnPairsArgs& a, int B, hipStream_t s) {
    const size_t lds = espcn_pairs_lds_bytes(a.r, a.p);
    if (espcn_radius(a.r) != 2 * (a.r - 1) || lds > 160 * 1024) return hipErrorInvalidValue;
    switch (a.r) {
        case 2: return launch_with_lds<espcn_patch_pairs_kernel<2>>(dim3(B), dim3(256), lds, s, a);
        case 3: return launch_with_lds<espcn_patch_pairs_kernel<3>>(dim3(B), dim3(256), lds, s, a);
        case 4: return launch_with_lds<espcn_patch_pairs_kernel<4>>(dim3(B), dim3(256), lds, s, a);
    }
    return hipErrorInvalidValue;
}

}  // namespace srx
