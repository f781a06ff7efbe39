// patch_pairs.hip -- VDSR's training pairs sampled on the device from a resident image set, one launch per batch.
//
// The reference builds every (sd, hd) pair on the host (vdsr/vdsr/dataset.py:41-128): random crop, random flip, then
// hd_image_to_sd_image (:13-38) on the crop -- gaussian blur sigma = 0.5 (s - 1), bilinear resize to int(S / s) and back.
// vdsr/dataset.py: image_batches mirrors it with a host loop per patch, one host-to-device copy and about 17 small launches
// per batch.  Here the decoded images sit in one uint8 arena on the device and a batch is a table of B entries
// {image, crop corner, flip, scaling factor} (srx_patch_src); the degradation is applied to the crop, so its borders are the
// patch's own and every entry is independent of the others.
//
// One workgroup (256 threads) per (entry, channel); everything between the uint8 read and the two fp32 stores lives in LDS:
//   wts   64 floats      the gaussian weights of this entry's factor (threads 0 .. radius write 0 .. radius; nothing else is read)
//   P, Q  S x S floats   two planes, used in turn:
//     1. P  = crop / 255 (a division, as u8_to_float_kernel), mirrored along the width if flip; hd = P * 2 - 1 is stored
//     2. Q  = blur of P along H, P = blur of Q along W          gaussian_1d_kernel's arithmetic, indices clamped to the patch
//     3. Q[L x L] = P resized to L = int(S / s)                 resize_bilinear_kernel's arithmetic
//     4. sd = (Q[L x L] resized to S x S) * 2 - 1               stored, never staged
// Every slot a step reads was written by the step before it in full (S x S, or the L x L corner of Q that step 3 wrote), so
// the result does not depend on what the LDS held before (SRX_POISON_LDS).  LDS: 256 + 8 S^2 bytes -- 13.4 KiB at S = 41,
// 128.25 KiB at S = 128 (above 64 KiB: launch_with_lds of lds_launch.h raises the kernel's ceiling once per device).  No atomics, no communication between workgroups.
//
// The table is trusted: srx_vdsr_patch_table_check (pairs_api.hip) is what keeps the reads inside the arena, the radius inside
// wts and L >= 1; patch_pairs.h holds the functions both sides derive the radius and L from.
#include "lds_launch.h"
#include "pairs_device.h"
#include "patch_pairs.h"

namespace srx {

__global__ __launch_bounds__(256) void vdsr_patch_pairs_kernel(const PatchPairsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds_patch[];
    const int S = a.S, SS = S * S;
    float* wts = lds_patch;
    float* P = lds_patch + 64;
    float* Q = P + SS;
    const int t = threadIdx.x;
    const unsigned e = blockIdx.x / 3u, c = blockIdx.x % 3u;
    const srx_patch_src src = a.table[e];
    const float s = src.scaling_factor;
    const float sigma = patch_sigma(s);
    const int radius = patch_radius(s);
    const int L = patch_lr_size(S, s);

    if (t <= radius && t < 64) wts[t] = gaussian_tap_weight(t, radius, sigma);
    // 1. the crop: channel c of rows y .. y+S-1, columns x .. x+S-1 of the image; rows are width * 3 bytes
    const uint8_t* img = a.arena + src.offset + ((size_t)src.y * src.width + src.x) * 3 + c;
    float* hd = a.hd + (size_t)e * SS * 3 + c;
    float* sd = a.sd + (size_t)e * SS * 3 + c;
    for (int o = t; o < SS; o += 256) {
        const int h = o / S, w = o - h * S;
        const int ws = src.flip ? S - 1 - w : w;
        const float v = (float)img[((size_t)h * src.width + ws) * 3] / 255.0f;
        P[o] = v;
        hd[(size_t)o * 3] = v * 2.0f - 1.0f;
    }
    __syncthreads();
    // 2. blur along H, then along W; borders replicate
    for (int o = t; o < SS; o += 256) {
        const int h = o / S, w = o - h * S;
        float acc = 0.f;
        for (int i = -radius; i <= radius; ++i) {
            int hh = h + i;
            hh = hh < 0 ? 0 : (hh >= S ? S - 1 : hh);
            acc += wts[i < 0 ? -i : i] * P[hh * S + w];
        }
        Q[o] = acc;
    }
    __syncthreads();
    for (int o = t; o < SS; o += 256) {
        const int h = o / S, w = o - h * S;
        float acc = 0.f;
        for (int i = -radius; i <= radius; ++i) {
            int ww = w + i;
            ww = ww < 0 ? 0 : (ww >= S ? S - 1 : ww);
            acc += wts[i < 0 ? -i : i] * Q[h * S + ww];
        }
        P[o] = acc;
    }
    __syncthreads();
    // 3. S x S -> L x L
    {
        const float sc = (float)S / (float)L;
        for (int o = t; o < L * L; o += 256) {
            const int oh = o / L, ow = o - oh * L;
            float fy = ((float)oh + 0.5f) * sc - 0.5f, fx = ((float)ow + 0.5f) * sc - 0.5f;
            fy = fminf(fmaxf(fy, 0.f), (float)(S - 1));
            fx = fminf(fmaxf(fx, 0.f), (float)(S - 1));
            const int y0 = (int)fy, x0 = (int)fx;
            const int y1 = y0 + 1 < S ? y0 + 1 : S - 1, x1 = x0 + 1 < S ? x0 + 1 : S - 1;
            const float wy = fy - (float)y0, wx = fx - (float)x0;
            const float v00 = P[y0 * S + x0], v01 = P[y0 * S + x1], v10 = P[y1 * S + x0], v11 = P[y1 * S + x1];
            Q[o] = (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
        }
    }
    __syncthreads();
    // 4. L x L -> S x S, mapped to [-1, 1] and stored
    {
        const float sc = (float)L / (float)S;
        for (int o = t; o < SS; o += 256) {
            const int oh = o / S, ow = o - oh * S;
            float fy = ((float)oh + 0.5f) * sc - 0.5f, fx = ((float)ow + 0.5f) * sc - 0.5f;
            fy = fminf(fmaxf(fy, 0.f), (float)(L - 1));
            fx = fminf(fmaxf(fx, 0.f), (float)(L - 1));
            const int y0 = (int)fy, x0 = (int)fx;
            const int y1 = y0 + 1 < L ? y0 + 1 : L - 1, x1 = x0 + 1 < L ? x0 + 1 : L - 1;
            const float wy = fy - (float)y0, wx = fx - (float)x0;
            const float v00 = Q[y0 * L + x0], v01 = Q[y0 * L + x1], v10 = Q[y1 * L + x0], v11 = Q[y1 * L + x1];
            const float v = (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
            sd[(size_t)o * 3] = v * 2.0f - 1.0f;
        }
    }
}

hipError_t launch_vdsr_patch_pairs(const PatchPairsArgs& a, int B, hipStream_t s) {
    return launch_with_lds<vdsr_patch_pairs_kernel>(dim3(3 * B), dim3(256), patch_pairs_lds_bytes(a.S), s, a);
}

}  // namespace srx
