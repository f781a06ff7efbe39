// bf16x3.h -- internal: precision 1 (SRX_PRECISION_BF16X3) of 3x3 stride-1 SAME 64 -> 64 layers (conv_bf16x3.hip) and of
// channel-blocked layers wider than 64 channels (conv_wide_bf16x3.hip).
// Every fp32 operand of a product is split into a = hi + lo (hi = bf16_rne(a), lo = bf16_rne(a - hi)) and each product is
// hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with an fp32 accumulator; bias, activation, masks and sums stay fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace srx {

// Tiles of TH x TW output pixels of one image; `tiles` = N * nty * ntx, walked by `grid` persistent workgroups (two per CU).
struct Bf3Plan {
    int TH, TW, ntx, nty, tiles, grid;
    size_t lds;
};

// LDS bytes per staged pixel: forward / data gradient (64 hi + 64 lo bf16 + 16 pad: the 16 pixels of a ds_read_b128 hit
// disjoint banks) and filter gradient (+ 32 pad: the 8 slots a 32-lane half of a ds_read_b64_tr_b16 takes hit disjoint banks);
// every workgroup stays within 80 KiB (two per CU).  The tile planner is host code in srx_api.hip.
constexpr int kBf3ConvSlot = 272, kBf3WgradSlot = 288;
constexpr size_t kBf3Lds = 80 * 1024;

// ---- device helpers shared by conv_bf16x3.hip and conv_wide_bf16x3.hip
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;

__device__ __forceinline__ void split_bf16(float v, __bf16& hi, __bf16& lo) {
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);
}

// four consecutive channels of one pixel -> 8 bytes of hi and 8 bytes of lo at byte offset `off` of the slot
__device__ __forceinline__ void store_split4(char* slot, int off, f32x4_t v) {
    bf16x4_t h, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        __bf16 a, b;
        split_bf16(v[j], a, b);
        h[j] = a;
        l[j] = b;
    }
    *(bf16x4_t*)(slot + off) = h;
    *(bf16x4_t*)(slot + 128 + off) = l;
}

__device__ __forceinline__ f32x4_t mfma3(bf16x8_t ahi, bf16x8_t alo, bf16x8_t bhi, bf16x8_t blo, f32x4_t acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, bhi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, blo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, bhi, acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ bf16x8_t read_tr8(const char* lds, unsigned off0, unsigned off1) {
    const s16x4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(lds + off0));
    const s16x4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(lds + off1));
    const s16x8_t c = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8_t, c);
}

// The filter gradient of one 64 -> 64 problem (conv_bf16x3.hip: the layer; conv_wide_bf16x3.hip: every block pair of a
// wider layer): workgroup `wg` of `nwg` walks tiles wg, wg + nwg, ..; its fp32 partial filter goes to P (see
// launch_wgrad3x3c64_bf16x3 for the layout).
__device__ __forceinline__ void wgrad3x3c64_bf16x3_body(const float* x, const float* dpre, float* P, int N,
                                                        int H, int W, int TH, int TW, int ntx, int nty, int tiles, int wg, int nwg) {
    extern __shared__ __attribute__((aligned(16))) char bf3_lds[];
    char* const lds = bf3_lds;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, r16 = lane & 15;
    const int q = (lane >> 2) & 3, p4 = lane & 3;   // a transposed read: lane 4q + p of a group addresses slot q, channels 4p .. 4p+3
    const int ci0 = 16 * wave;
    const int RS = TW + 2, nx = (TH + 2) * RS, npx = TH * TW, nslots = nx + 1 + npx;
    const int zero = nx;                            // an all-zero slot: the operand of K positions past the tile or the image
    const int c4 = threadIdx.x & 15;
    f32x4_t acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[t][cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    f32x4_t bsum = {0.f, 0.f, 0.f, 0.f};            // this thread's share of the bias gradient, channels 4 c4 .. 4 c4 + 3
    for (int tile = wg; tile < tiles; tile += nwg) {
        const int tx = tile % ntx, rest = tile / ntx, ty = rest % nty, n = rest / nty;
        const int r0 = ty * TH, c0 = tx * TW;
        const size_t img = (size_t)n * H * W * 64;
        __syncthreads();
        // slots [0, nx): x with its zero halo; nx: zeros; nx + 1 + k: dpre of output pixel k of the tile
        for (int s0 = threadIdx.x >> 4; s0 < nslots; s0 += 64) {
            f32x4_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int s = s0 + 16 * u;
                v[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                if (s < nx) {
                    const int sr = s / RS, sc = s - sr * RS, ih = r0 - 1 + sr, iw = c0 - 1 + sc;
                    if (ih >= 0 && ih < H && iw >= 0 && iw < W)
                        v[u] = *(const f32x4_t*)(x + img + ((size_t)ih * W + iw) * 64 + 4 * c4);
                } else if (s > nx && s < nslots) {
                    const int k = s - nx - 1, kr = k / TW, kc = k - kr * TW, oh = r0 + kr, ow = c0 + kc;
                    if (oh < H && ow < W) v[u] = *(const f32x4_t*)(dpre + img + ((size_t)oh * W + ow) * 64 + 4 * c4);
                    bsum += v[u];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int s = s0 + 16 * u;
                if (s < nslots) store_split4(lds + (size_t)s * kBf3WgradSlot, 8 * c4, v[u]);
            }
        }
        __syncthreads();
        for (int k0 = 0; k0 < npx; k0 += 32) {
            unsigned xa[2], da[2], rstep[2], cstep[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = k0 + 8 * g + 4 * h + q, kr = k / TW, kc = k - kr * TW;
                const bool ok = k < npx && r0 + kr < H && c0 + kc < W;
                xa[h] = (ok ? (kr * RS + kc) : zero) * kBf3WgradSlot + 2 * (ci0 + 4 * p4);
                da[h] = (ok ? (nx + 1 + k) : zero) * kBf3WgradSlot + 2 * (4 * p4);
                rstep[h] = ok ? RS * kBf3WgradSlot : 0;
                cstep[h] = ok ? kBf3WgradSlot : 0;
            }
            // B[k = pixel][col = output channel 16 cb + r16]
            bf16x8_t bhi[4], blo[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                bhi[cb] = read_tr8(lds, da[0] + 32 * cb, da[1] + 32 * cb);
                blo[cb] = read_tr8(lds, da[0] + 128 + 32 * cb, da[1] + 128 + 32 * cb);
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                // A[row = input channel ci0 + r16][k = pixel], the window shifted by the tap
                const unsigned o0 = xa[0] + (t / 3) * rstep[0] + (t % 3) * cstep[0];
                const unsigned o1 = xa[1] + (t / 3) * rstep[1] + (t % 3) * cstep[1];
                const bf16x8_t ahi = read_tr8(lds, o0, o1);
                const bf16x8_t alo = read_tr8(lds, o0 + 128, o1 + 128);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) acc[t][cb] = mfma3(ahi, alo, bhi[cb], blo[cb], acc[t][cb]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) P[(t * 64 + ci0 + 4 * g + j) * 64 + 16 * cb + r16] = acc[t][cb][j];
    // bias gradient: the 16 threads of each channel group in a fixed order
    __syncthreads();
    f32x4_t* red = (f32x4_t*)lds;
    red[threadIdx.x] = bsum;
    __syncthreads();
    if (threadIdx.x < 16) {
        f32x4_t s = red[threadIdx.x];
        for (int r = 1; r < 16; ++r) s += red[16 * r + threadIdx.x];
        *(f32x4_t*)(P + 9 * 64 * 64 + 4 * threadIdx.x) = s;
    }
}

// The launchers are weak references: a host-only build of srx_api.hip without the kernel units (the ThreadSanitizer test)
// still links; srx_api.hip refuses precision 1 when they are absent.
// dgrad == false: y = act(x (*) w + bias), relu selects ReLU, bias nullable, mask unused.
// dgrad == true:  y = (dpre (*) flipped / transposed w) * (mask > 0) with x = dpre, mask = x_in (nullable: no mask).
__attribute__((weak)) hipError_t launch_conv3x3c64_bf16x3(bool dgrad, const float* x, const float* w, const float* bias, const float* mask, bool relu,
                                    float* y, int N, int H, int W, const Bf3Plan& p, hipStream_t s);
// One partial filter per workgroup: part[g * part_stride + (tap * 64 + ci) * 64 + co], dbias partial at + 9 * 64 * 64 + co.
__attribute__((weak)) hipError_t launch_wgrad3x3c64_bf16x3(const float* x, const float* dpre, float* part, int part_stride, int N, int H, int W,
                                     const Bf3Plan& p, hipStream_t s);

// Channel-blocked layers (conv_wide_bf16x3.hip), the arguments of srx_conv3x3_blocked_ex / _bwd_filter_ex at precision 1.
struct Bf3WideArgs {
    const float* x;      // staged tensor, SB blocks of [N,H,W,64]
    const float* w;      // blocked filters [CIB][COB][9][64][64] of the FORWARD layer
    const float* bias;   // [PB*64] or null
    const float* mask;   // produced-shaped or null
    float* y;            // produced tensor, PB blocks of [N,H,W,64]
    int N, H, W, SB, PB;
    int TH, TW, tiles_y, tiles_x, units_total;
    int act, mask_act;
};
// Tiles of the blocked forward / data gradient: <= 128 pixels, (TH + 2) x (TW + 2) <= kBf3WideSlots, two LDS buffers.
constexpr int kBf3WideSlots = 288;
constexpr size_t kBf3WideLds = (size_t)2 * kBf3WideSlots * kBf3ConvSlot;
__attribute__((weak)) hipError_t launch_conv_wide_bf16x3(bool transpose, const Bf3WideArgs& a, int grid, hipStream_t s);
// All (ib, ob) pairs of a blocked filter gradient: x [cib][N,H,W,64], dpre [cob][N,H,W,64]; pair ib * cob + ob writes its
// p.grid partials at part + (pair * p.grid + g) * part_stride (the layout of launch_wgrad3x3c64_bf16x3).
__attribute__((weak)) hipError_t launch_wgrad3x3c64_bf16x3_pairs(const float* x, const float* dpre, float* part, int part_stride,
                                                               int cib, int cob, int N, int H, int W, const Bf3Plan& p, hipStream_t s);

}  // namespace srx
