// enet_pairs.hip -- EnhanceNet's training batches sampled on the device from a resident image set, one launch per batch.
//
// The reference builds every (sd, bq, hd) triple inside the training loop (enet/enet/datasets.py:104-125): a 128 x 128 crop
// of a decoded image at a random corner (:107-110), sd = scipy.misc.imresize(hd, 25) (:112: Pillow BILINEAR, antialiased,
// on the uint8 crop), bq = imresize(sd, 400, 'bicubic') (:113: Pillow BICUBIC, a = -0.5), all three as float32 / 127.5 - 1
// (:115-117).  Here the decoded images sit in one uint8 arena on the device and a batch is B records {image, crop corner,
// flips} (srx_patch_src).  The arithmetic is resample_u8.hip's, byte for byte: each resize is Pillow's two passes in
// Pillow's order, horizontal then vertical, each pass
//     out = clip8((2^21 + sum_k kk[k] * in[xmin + k]) >> 22)          (arithmetic shift)
// with a uint8 intermediate image and the integer coefficients of srx_pil_resample_coeffs.  The order and the uint8
// intermediate are what make the bytes Pillow's, so the four passes stay four passes.
//
// One workgroup (256 threads) per entry, all three channels; everything between the uint8 reads and the fp32 stores is in
// LDS (patch_pairs.h: enet_pairs_lds; S the crop's side, s = S / 4):
//   tab     256 floats       tab[b] = (float)b / 127.5f - 1.0f, contraction off: u8_to_pm1_kernel's two roundings; thread t
//                            writes entry t
//   tables  the block of srx_enet_pairs_tables(S): bounds and kk of S -> s BILINEAR (9 taps), then of s -> S BICUBIC (5)
//   crop    S x S x 3 bytes  the crop with its flips applied: rows reversed if flip & 2, columns if flip & 1
//   h1      S x s x 3 bytes  crop resampled along its rows (the first resize's horizontal pass)
//   sd      s x s x 3 bytes  h1 resampled along its columns
//   h3      s x S x 3 bytes  sd resampled along its rows (the second resize's horizontal pass)
// Steps (a barrier between them):
//   1. tab, tables and crop are written in full; consecutive lanes read consecutive bytes of an image row
//   2. hd = tab[crop], stored; h1 from crop
//   3. sd bytes from h1; sd = tab[sd], stored
//   4. h3 from sd
//   5. bq = tab[h3 resampled along its columns], stored straight from registers
// Every store gives consecutive floats of the entry's contiguous run to consecutive lanes.  Every slot a step reads was
// written in full by the step before it, so the result does not depend on what the LDS held (SRX_POISON_LDS).  Each entry
// is computed from its own record alone.  No atomics, no communication between workgroups, plain vector stores.
// In the vertical passes (3, 5) consecutive lanes read consecutive BYTES of a row: four lanes share a dword (a broadcast)
// and the 32 lanes of a group touch 8 consecutive banks; in the horizontal passes (2, 4) consecutive outputs step through
// the row by about 12 bytes / 3 output bytes (down) or 3 bytes / 12 output bytes (up), one bank per dword again.
//
// The table and the coefficient block are trusted: srx_enet_patch_table_check (pairs_api.hip) keeps x, y, x + S, y + S
// inside the image and the image inside the arena; srx_enet_pairs_tables writes bounds with first + count <= the input
// side, so every LDS read of a pass is inside the image the pass reads.
#include "lds_launch.h"
#include "pairs_device.h"
#include "patch_pairs.h"

namespace srx {

// (one output byte of a pass: resample_byte, pairs_device.h)

__global__ __launch_bounds__(256) void enet_patch_pairs_kernel(const EnetPairsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_enet[];
    const int S = a.S, s = S >> 2, S3 = S * 3, s3 = s * 3;
    const EnetPairsLds L = enet_pairs_lds(S);
    const EnetPairsTables T = enet_pairs_tables(S);
    float* tab = reinterpret_cast<float*>(lds_enet + L.tab);
    int* tables = reinterpret_cast<int*>(lds_enet + L.tables);
    uint8_t* crop = lds_enet + L.crop;
    uint8_t* h1 = lds_enet + L.h1;
    uint8_t* sdb = lds_enet + L.sd;
    uint8_t* h3 = lds_enet + L.h3;
    const int *dbnd = tables + T.down_bounds, *dkk = tables + T.down_kk, *ubnd = tables + T.up_bounds, *ukk = tables + T.up_kk;
    const int t = threadIdx.x;
    const unsigned e = blockIdx.x;
    const srx_patch_src src = a.table[e];
    const SmallDiv by_S3(S3), by_s3(s3);     // d = 3 S or 3 s >= 3, n < 3 S^2 <= 49152: n d < 2^25

    // 1. the byte table, the coefficient block, the flipped crop
    tab[t] = byte_to_pm1(t);
    for (int o = t; o < T.words; o += 256) tables[o] = a.tables[o];
    {
        const bool fw = src.flip & 1, fh = src.flip & 2;
        const uint8_t* img = a.arena + src.offset;
        const size_t pitch = (size_t)src.width * 3;
        const int n = S * S3;
#pragma unroll 16
        for (int o = t; o < n; o += 256) {
            const int row = by_S3(o), rem = o - row * S3, col = rem / 3, c = rem - col * 3;
            const int yy = src.y + (fh ? S - 1 - row : row), xx = src.x + (fw ? S - 1 - col : col);
            crop[o] = img[(size_t)yy * pitch + (size_t)(xx * 3 + c)];
        }
    }
    __syncthreads();
    // 2a. hd: the staged bytes as they lie
    {
        const int n = S * S3;
        float* hd = a.hd + (size_t)e * n;
#pragma unroll 8
        for (int o = t; o < n; o += 256) hd[o] = tab[crop[o]];
    }
    // 2b. h1[r][j][c] = the S -> s pass along row r of crop
    {
        const int n = S * s3;
        for (int o = t; o < n; o += 256) {
            const int r = by_s3(o), rem = o - r * s3, j = rem / 3, c = rem - j * 3;
            const int first = dbnd[2 * j], cnt = dbnd[2 * j + 1];
            h1[o] = (uint8_t)resample_byte<kEnetKDown>(crop + r * S3 + first * 3 + c, 3, dkk + j * kEnetKDown, cnt);
        }
    }
    __syncthreads();
    // 3. sd[i][j][c] = the S -> s pass along column (j, c) of h1
    {
        const int n = s * s3;
        float* sd = a.sd + (size_t)e * n;
        for (int o = t; o < n; o += 256) {
            const int i = by_s3(o), rem = o - i * s3;
            const int first = dbnd[2 * i], cnt = dbnd[2 * i + 1];
            const int v = resample_byte<kEnetKDown>(h1 + first * s3 + rem, s3, dkk + i * kEnetKDown, cnt);
            sdb[o] = (uint8_t)v;
            sd[o] = tab[v];
        }
    }
    __syncthreads();
    // 4. h3[i][J][c] = the s -> S pass along row i of sd
    {
        const int n = s * S3;
        for (int o = t; o < n; o += 256) {
            const int i = by_S3(o), rem = o - i * S3, J = rem / 3, c = rem - J * 3;
            const int first = ubnd[2 * J], cnt = ubnd[2 * J + 1];
            h3[o] = (uint8_t)resample_byte<kEnetKUp>(sdb + i * s3 + first * 3 + c, 3, ukk + J * kEnetKUp, cnt);
        }
    }
    __syncthreads();
    // 5. bq[I][J][c] = the s -> S pass along column (J, c) of h3
    {
        const int n = S * S3;
        float* bq = a.bq + (size_t)e * n;
#pragma unroll 4
        for (int o = t; o < n; o += 256) {
            const int I = by_S3(o), rem = o - I * S3;
            const int first = ubnd[2 * I], cnt = ubnd[2 * I + 1];
            bq[o] = tab[resample_byte<kEnetKUp>(h3 + first * S3 + rem, S3, ukk + I * kEnetKUp, cnt)];
        }
    }
}

hipError_t launch_enet_patch_pairs(const EnetPairsArgs& a, int B, hipStream_t s) {
    if (!enet_pairs_size_ok(a.S)) return hipErrorInvalidValue;
    return launch_with_lds<enet_patch_pairs_kernel>(dim3(B), dim3(256), (size_t)enet_pairs_lds(a.S).bytes, s, a);
}

}  // namespace srx
