// conv_bf16x3.hip -- precision 1 (SRX_PRECISION_BF16X3) of 3x3 stride-1 SAME 64 -> 64 layers, VDSR's body.
//
// Every fp32 operand of a product is split into hi = bf16_rne(a), lo = bf16_rne(a - hi) (the subtraction is exact; a plain
// cast, so a NaN stays a NaN) when it is staged, and each product is hi*hi + hi*lo + lo*hi: three v_mfma_f32_16x16x32_bf16
// into one fp32 accumulator, 3/16 of the MFMA time of the exact path's v_mfma_f32_16x16x4_f32.  Bias, activation, the
// ReLU-gradient mask and the bias gradient are fp32 as on the exact path.
//
// Forward / data gradient (conv3x3c64_bf16x3_kernel): one tile of TH x TW output pixels of one image at a time, its input
// with a one-pixel zero halo staged in LDS as [slot][64 hi | 64 lo | pad] bf16 (272 B: the 16 pixels of a ds_read_b128 hit
// disjoint banks).  Wave w owns output channels 16w .. 16w+15; its filter slice (9 taps x 2 K-steps of 32 channels, hi and
// lo: 144 VGPRs) stays in registers for the whole launch.  An MFMA's B operand is 8 consecutive channels of one pixel
// (ds_read_b128), its 16 columns 16 consecutive output pixels of the tile.  Every output pixel sums the same 54 MFMAs in
// the same order wherever it falls in a tile (outside the image the halo holds zeros): image n of a batch gets the bits it
// gets alone.  Two workgroups per CU (<= 80 KiB of LDS each), so one's staging runs under the other's MFMAs.
//
// Filter gradient (wgrad3x3c64_bf16x3_kernel): K = output pixels.  Both operands need 8 consecutive PIXELS of one channel
// per lane: ds_read_b64_tr_b16 reads them from the same [slot][channel] image (4 slots x 16 channels per 16-lane group,
// every slot addressed by its own lane, so the 3x3 window shift is a per-lane address offset).  Wave w owns input
// channels 16w .. 16w+15 and all 64 output channels of the 9 taps (144 accumulator VGPRs) over all tiles of the
// workgroup; one fp32 partial filter per workgroup, summed by the fixed-order reduction of the exact path.
#include "bf16x3.h"
#include "lds_launch.h"

namespace srx {

namespace {

constexpr int kConvSlot = kBf3ConvSlot;

}  // namespace

struct Bf3ConvArgs {
    const float* x;      // staged tensor [N,H,W,64]: the layer input (forward) or dpre (data gradient)
    const float* w;      // HWIO [3,3,64,64] of the forward layer
    const float* bias;   // forward, nullable
    const float* mask;   // data gradient: x_in, nullable
    float* y;
    int N, H, W, TH, TW, ntx, nty, tiles, relu;
};

struct Bf3WgradArgs {
    const float* x;
    const float* dpre;
    float* part;
    int part_stride, N, H, W, TH, TW, ntx, nty, tiles;
};

template <bool DGRAD>
__global__ __launch_bounds__(256, 2) void conv3x3c64_bf16x3_kernel(Bf3ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, r16 = lane & 15;
    // A[row = output channel 16 wave + r16][k = input channel 32 kc + 8 g + j]
    bf16x8_t whi[9][2], wlo[9][2];
    {
        const int oc = 16 * wave + r16;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int kc = 0; kc < 2; ++kc)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ic = 32 * kc + 8 * g + j;
                    // data gradient: the flipped tap, input / output channels exchanged
                    const float v = DGRAD ? a.w[((8 - t) * 64 + oc) * 64 + ic] : a.w[(t * 64 + ic) * 64 + oc];
                    __bf16 h, l;
                    split_bf16(v, h, l);
                    whi[t][kc][j] = h;
                    wlo[t][kc][j] = l;
                }
    }
    const int RS = a.TW + 2, nslots = (a.TH + 2) * RS, npx = a.TH * a.TW, nsub = (npx + 15) / 16;
    const int c4 = threadIdx.x & 15;
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int tx = tile % a.ntx, rest = tile / a.ntx, ty = rest % a.nty, n = rest / a.nty;
        const int r0 = ty * a.TH, c0 = tx * a.TW;
        const float* xn = a.x + (size_t)n * a.H * a.W * 64;
        __syncthreads();   // the previous tile's reads are done
        for (int s0 = threadIdx.x >> 4; s0 < nslots; s0 += 64) {
            f32x4_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int s = s0 + 16 * u, sr = s / RS, sc = s - sr * RS;
                const int ih = r0 - 1 + sr, iw = c0 - 1 + sc;
                v[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                if (s < nslots && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W)
                    v[u] = *(const f32x4_t*)(xn + ((size_t)ih * a.W + iw) * 64 + 4 * c4);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int s = s0 + 16 * u;
                if (s < nslots) store_split4(lds + (size_t)s * kConvSlot, 8 * c4, v[u]);
            }
        }
        __syncthreads();
        for (int sub = 0; sub < nsub; ++sub) {
            int p = sub * 16 + r16;
            const bool live = p < npx;
            if (!live) p = npx - 1;          // (a real slot; the column is not stored)
            const int pr = p / a.TW, pc = p - pr * a.TW;
            const char* base = lds + (pr * RS + pc) * kConvSlot + 16 * g;
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int off = ((t / 3) * RS + (t % 3)) * kConvSlot;
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    const bf16x8_t bhi = *(const bf16x8_t*)(base + off + 64 * kc);
                    const bf16x8_t blo = *(const bf16x8_t*)(base + off + 128 + 64 * kc);
                    acc = mfma3(whi[t][kc], wlo[t][kc], bhi, blo, acc);
                }
            }
            const int oh = r0 + pr, ow = c0 + pc;
            if (live && oh < a.H && ow < a.W) {
                const int co = 16 * wave + 4 * g;
                const size_t idx = (((size_t)n * a.H + oh) * a.W + ow) * 64 + co;
                f32x4_t out = acc;
                if (DGRAD) {
                    if (a.mask) {
                        const f32x4_t m = *(const f32x4_t*)(a.mask + idx);
#pragma unroll
                        for (int j = 0; j < 4; ++j) out[j] = m[j] > 0.0f ? out[j] : 0.0f;
                    }
                } else {
                    if (a.bias) out += *(const f32x4_t*)(a.bias + co);
                    if (a.relu) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) out[j] = fmaxf(out[j], 0.0f);
                    }
                }
                *(f32x4_t*)(a.y + idx) = out;
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void wgrad3x3c64_bf16x3_kernel(Bf3WgradArgs a) {
    wgrad3x3c64_bf16x3_body(a.x, a.dpre, a.part + (size_t)blockIdx.x * a.part_stride, a.N, a.H, a.W, a.TH, a.TW, a.ntx, a.nty,
                            a.tiles, blockIdx.x, gridDim.x);
}

hipError_t launch_conv3x3c64_bf16x3(bool dgrad, const float* x, const float* w, const float* bias, const float* mask, bool relu,
                                    float* y, int N, int H, int W, const Bf3Plan& p, hipStream_t s) {
    Bf3ConvArgs a{x, w, bias, mask, y, N, H, W, p.TH, p.TW, p.ntx, p.nty, p.tiles, relu ? 1 : 0};
    if (dgrad) return launch_with_lds<conv3x3c64_bf16x3_kernel<true>>(dim3(p.grid), dim3(256), p.lds, s, a);
    return launch_with_lds<conv3x3c64_bf16x3_kernel<false>>(dim3(p.grid), dim3(256), p.lds, s, a);
}

hipError_t launch_wgrad3x3c64_bf16x3(const float* x, const float* dpre, float* part, int part_stride, int N, int H, int W,
                                     const Bf3Plan& p, hipStream_t s) {
    Bf3WgradArgs a{x, dpre, part, part_stride, N, H, W, p.TH, p.TW, p.ntx, p.nty, p.tiles};
    return launch_with_lds<wgrad3x3c64_bf16x3_kernel>(dim3(p.grid), dim3(256), p.lds, s, a);
}

}  // namespace srx
