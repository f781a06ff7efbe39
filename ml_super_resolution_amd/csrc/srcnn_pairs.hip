// srcnn_pairs.hip -- SRCNN's training batches sampled on the device from a resident image set, one launch per batch.
//
// The reference builds every batch in its graph (srcnn/srcnn.py:46-93, :132-136): a random S x S crop of a decoded JPEG,
// a random left-right flip, / 127.5 - 1; lo = tf.image.resize_bicubic down to S / f, sd = resize_bicubic back up to S; the
// ground truth loses `border` pixels all round, as the VALID network's output does.  Here the decoded images sit in one
// uint8 arena on the device and a batch is B records {image, crop corner, flip} (srx_patch_src).  The arithmetic is that
// of the route it replaces (u8_to_pm1_kernel's expression, then two srx_resize_bicubic_tf launches), bit for bit:
//   hd_full = (float)byte / 127.5f - 1.0f                                  two roundings, contraction off
//   lo      = the 16-tap loop of resize_bicubic_tf_kernel on hd_full       (S -> s = S / f, scale (float)S / (float)s)
//   sd      = the same resize of lo (s -> S), evaluated separably: the kernel's inner sum
//                 v = 0.f; for k in 0..3: v += wx[k] * row[ix[k]]
//             depends on (input row, output column, channel) alone, so it is computed ONCE per lo row into LDS (`hup`), and
//             the outer sum acc = 0.f; for r in 0..3: acc += wy[r] * v[iy[r]] adds the same four floats in the same order.
//   The tap positions and weights are bicubic_tf_taps (bicubic_tf.h), the text resize_bicubic_tf_kernel compiles.
//
// One workgroup (256 threads) per (entry, band): blockIdx.x the entry, blockIdx.y the band of output rows [R0, R1)
// (patch_pairs.h: srcnn_pairs_band; 21 bands of 12 rows at S = 243, f = 3, so a batch of 64 is 1344 workgroups).  A band
// needs the lo rows l0 .. l1 its four clamped y taps reach (srcnn_pairs_lo_rows; n = l1 - l0 + 1, 7 at the default) and,
// for each, the four crop rows ITS y taps reach -- one, when S = s f (below).  LDS (patch_pairs.h: srcnn_pairs_lds):
//   tab     256 floats         tab[b] = (float)b / 127.5f - 1.0f; thread t writes entry t
//   down    s records          the taps of S -> s for output index j (a row or a column: the crop is square): idx[4], w[4]
//   up      S records          the taps of s -> S
//   lo      n x s x 3 fp32     the lo rows l0 .. l1
//   rows    n x 4 x S x 3 B    crop row down[l0 + i].idx[r] for lo row i, tap r, columns reversed if flip;
//           n x S x 3 fp32     later, in the same bytes (12 n S either way), hup: the horizontal pass of the lo rows
// Steps (a barrier between them):
//   1. tab, down and up are written in full
//   2. rows is filled: consecutive lanes read consecutive bytes of an image row; the band's rows of hd that lie inside the
//      border are read the same way and stored as tab[byte]
//   3. lo[i][j][c] from rows through tab: the 16-tap loop, or the one pixel it returns when S = s f
//   4. hup[i][J][c] from lo (over the bytes of rows, which step 3 has finished reading)
//   5. sd[I][J][c] = sum over r of up[I].w[r] * hup[up[I].idx[r] - l0][J][c], stored straight from registers
// Every store gives consecutive floats of the entry's contiguous run (a band's rows of sd, and of hd, are one run each) to
// consecutive lanes; step 5 reads LDS the same way, one bank per lane.  Every slot a step reads was written in full by an
// earlier step of the same workgroup, so the result does not depend on what the LDS held (SRX_POISON_LDS).  Each band is
// computed from its entry's record alone.  No atomics, no communication between workgroups, plain vector stores.
//
// The table is trusted: srx_srcnn_patch_table_check (pairs_api.hip) keeps x, y, x + S, y + S inside the image and the image
// inside the arena; bicubic_tf_taps clamps every index to its input, and srcnn_pairs_lo_rows brackets the up pass's row
// taps because floor(o * scale) does not decrease with o.
#include "bicubic_tf.h"
#include "lds_launch.h"
#include "pairs_device.h"
#include "patch_pairs.h"

namespace srx {

static_assert(sizeof(SrcnnTaps) == 32, "srcnn_pairs_lds counts 32 bytes per record");

__global__ __launch_bounds__(256) void srcnn_patch_pairs_kernel(const SrcnnPairsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_srcnn[];
    const int S = a.S, s = S / a.f, S3 = S * 3, s3 = s * 3;
    const SrcnnPairsLds L = srcnn_pairs_lds(S, a.f);
    float* tab = reinterpret_cast<float*>(lds_srcnn + L.tab);
    SrcnnTaps* down = reinterpret_cast<SrcnnTaps*>(lds_srcnn + L.down);
    SrcnnTaps* up = reinterpret_cast<SrcnnTaps*>(lds_srcnn + L.up);
    float* lo = reinterpret_cast<float*>(lds_srcnn + L.lo);
    uint8_t* rows = lds_srcnn + L.rows;
    float* hup = reinterpret_cast<float*>(lds_srcnn + L.rows);
    const int t = threadIdx.x;
    const unsigned e = blockIdx.x;
    const int band = srcnn_pairs_band(S, a.f);
    const int R0 = (int)blockIdx.y * band, R1 = R0 + band < S ? R0 + band : S;
    int l0, l1;
    srcnn_pairs_lo_rows(s, a.up_scale, R0, R1, &l0, &l1);
    const int n = l1 - l0 + 1;
    const srx_patch_src src = a.table[e];
    const uint8_t* img = a.arena + src.offset + ((size_t)src.y * src.width + src.x) * 3;     // the crop's pixel (0, 0)
    const size_t pitch = (size_t)src.width * 3;
    const bool flip = src.flip != 0;
    const SmallDiv by_S3(S3), by_s3(s3);     // 3 <= d <= 768, n < 256 * 768: n d < 2^28
    // S = s f: the down scale is the integer f, every position j * f is exact, every offset 0 and every weight of the S -> s
    // pass exactly (0, 1, 0, 0) (bicubic_tf_taps at x = 0, xr = 1: each expression is exact in fp32).  The 16-tap loop then
    // returns the tap-(1, 1) pixel itself: 0.f + 0 * p = 0.f, 0.f + 1 * q = q, q + 0 * p = q for finite p, q, and a pixel
    // b / 127.5 - 1 is finite and never -0.  So only that pixel is staged and read.
    const bool unit = s * a.f == S;

    // 1. the byte table and both tap tables
    tab[t] = byte_to_pm1(t);
    for (int j = t; j < s; j += 256) bicubic_tf_taps(j, a.down_scale, S, down[j].idx, down[j].w);
    for (int j = t; j < S; j += 256) bicubic_tf_taps(j, a.up_scale, s, up[j].idx, up[j].w);
    __syncthreads();
    // 2a. the crop rows the lo rows read, flipped: all four y taps of each, or tap 1 alone when the down pass is a decimation
    {
        const int total = n * (unit ? 1 : 4) * S3;
#pragma unroll 8
        for (int o = t; o < total; o += 256) {
            const int q = by_S3(o), rem = o - q * S3, col = rem / 3, c = rem - col * 3;
            const int yy = unit ? down[l0 + q].idx[1] : down[l0 + (q >> 2)].idx[q & 3], xx = flip ? S - 1 - col : col;
            rows[o] = img[(size_t)yy * pitch + (size_t)(xx * 3 + c)];
        }
    }
    // 2b. hd: the band's rows inside the border, one contiguous run of the entry's [T][T][3]
    {
        const int T = S - 2 * a.border, T3 = T * 3;
        const int h0 = (R0 > a.border ? R0 : a.border) - a.border, h1 = (R1 < S - a.border ? R1 : S - a.border) - a.border;
        if (h1 > h0) {
            const SmallDiv by_T3(T3);      // h1 > h0 gives T >= 1: 3 <= d <= 768, n < 256 * 768
            float* hd = a.hd + (size_t)e * T * T3 + (size_t)h0 * T3;
            const int total = (h1 - h0) * T3;
#pragma unroll 8
            for (int o = t; o < total; o += 256) {
                const int r = by_T3(o), rem = o - r * T3, col = rem / 3 + a.border, c = rem - (rem / 3) * 3;
                const int yy = h0 + r + a.border, xx = flip ? S - 1 - col : col;
                hd[o] = tab[img[(size_t)yy * pitch + (size_t)(xx * 3 + c)]];
            }
        }
    }
    __syncthreads();
    // 3. lo[i][j][c]: resize_bicubic_tf_kernel's loop on the staged rows; its value when the weights are (0, 1, 0, 0)
    if (unit) {
        const int total = n * s3;
        for (int o = t; o < total; o += 256) {
            const int i = by_s3(o), rem = o - i * s3, j = rem / 3, c = rem - j * 3;
            lo[o] = tab[rows[i * S3 + down[j].idx[1] * 3 + c]];
        }
    } else {
        const int total = n * s3;
        for (int o = t; o < total; o += 256) {
#pragma clang fp contract(off)
            const int i = by_s3(o), rem = o - i * s3, j = rem / 3, c = rem - j * 3;
            const SrcnnTaps ty = down[l0 + i], tx = down[j];
            float acc = 0.f;
            for (int r = 0; r < 4; ++r) {
                const uint8_t* row = rows + (i * 4 + r) * S3 + c;
                float v = 0.f;
                for (int k = 0; k < 4; ++k) v += tx.w[k] * tab[row[tx.idx[k] * 3]];
                acc += ty.w[r] * v;
            }
            lo[o] = acc;
        }
    }
    __syncthreads();
    // 4. hup[i][J][c]: the inner sum of the s -> S resize, once per lo row
    {
        const int total = n * S3;
#pragma unroll 4
        for (int o = t; o < total; o += 256) {
#pragma clang fp contract(off)
            const int i = by_S3(o), rem = o - i * S3, J = rem / 3, c = rem - J * 3;
            const SrcnnTaps tx = up[J];
            const float* row = lo + i * s3 + c;
            float v = 0.f;
            for (int k = 0; k < 4; ++k) v += tx.w[k] * row[tx.idx[k] * 3];
            hup[o] = v;
        }
    }
    __syncthreads();
    // 5. sd[I][J][c]: the outer sum
    {
        const int total = (R1 - R0) * S3;
        float* sd = a.sd + (size_t)e * S * S3 + (size_t)R0 * S3;
#pragma unroll 4
        for (int o = t; o < total; o += 256) {
#pragma clang fp contract(off)
            const int I = by_S3(o), rem = o - I * S3;
            const SrcnnTaps ty = up[R0 + I];
            float acc = 0.f;
            for (int r = 0; r < 4; ++r) acc += ty.w[r] * hup[(ty.idx[r] - l0) * S3 + rem];
            sd[o] = acc;
        }
    }
}

hipError_t launch_srcnn_patch_pairs(const SrcnnPairsArgs& a, int B, hipStream_t s) {
    if (!srcnn_pairs_size_ok(a.S, a.f) || !srcnn_pairs_border_ok(a.S, a.border) || B < 1 || B > kSrcnnMaxB) return hipErrorInvalidValue;
    const SrcnnPairsLds L = srcnn_pairs_lds(a.S, a.f);
    if (L.bytes > kSrcnnLdsLimit) return hipErrorInvalidValue;
    // the allocation holds srcnn_pairs_max_lo_rows rows: no band may reach more
    const int band = srcnn_pairs_band(a.S, a.f), bands = srcnn_pairs_bands(a.S, a.f), sl = a.S / a.f;
    for (int k = 0; k < bands; ++k) {
        int l0, l1;
        srcnn_pairs_lo_rows(sl, a.up_scale, k * band, (k + 1) * band < a.S ? (k + 1) * band : a.S, &l0, &l1);
        if (l1 - l0 + 1 > srcnn_pairs_max_lo_rows(a.S, a.f)) return hipErrorInvalidValue;
    }
    return launch_with_lds<srcnn_patch_pairs_kernel>(dim3(B, bands), dim3(256), (size_t)L.bytes, s, a);
}

}  // namespace srx
