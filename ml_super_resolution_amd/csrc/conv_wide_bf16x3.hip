// conv_wide_bf16x3.hip -- precision 1 (SRX_PRECISION_BF16X3) of the channel-blocked 3x3 SAME stride-1 layers wider than
// 64 channels (srx_conv3x3_blocked_ex, srx_conv3x3_blocked_bwd_filter_ex): VGG-19's blocks 2-5 and the discriminator's
// 128..512-channel layers.  The split and the products are those of conv_bf16x3.hip (bf16x3.h): hi = bf16_rne(a),
// lo = bf16_rne(a - hi), each product hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 into an fp32 accumulator.
//
// Forward / data gradient (conv_wide_bf16x3_kernel): the walk of conv_wide_pipe_kernel.  A work unit is (a tile of
// <= 128 pixels of one image, one produced block); its 8 sub-tiles of 16 pixels x 16 channels per wave stay in
// registers while the unit walks the staged blocks, one STEP per staged block (steps numbered flat, unit * SB + block,
// one persistent workgroup per CU).  A step's tile is in LDS as [slot][64 hi | 64 lo | pad] (272 B); its filter slice
// (the wave's 16 output channels x 9 taps x 64 input channels, hi and lo: 144 registers) in registers.  Under a step's
// MFMAs: the next step's tile is loaded in the first half of the sub-tiles and split into the other LDS buffer, the next
// filter slice is loaded (fp32) in the second half and split behind the last sub-tile.  One barrier per step.
// Every output element sums 54 MFMAs per staged block in block order, wherever its pixel lies (halo slots hold
// zeros): deterministic, and image n of a batch gets the bits it gets alone.  Bias, activation and mask: fp32 epilogue.
//
// Filter gradient (wgrad3x3c64_bf16x3_pairs_kernel): the body of wgrad3x3c64_bf16x3_kernel with the block pair in
// blockIdx.y (the trick of wgrad_lin_pairs_kernel): one fp32 partial per (pair, workgroup), summed by the fixed-order
// pair reduction of the exact path.
#include "bf16x3.h"
#include "launchers.h"

namespace srx {
namespace {

constexpr int kSlot = kBf3ConvSlot;
constexpr int kPasses = kBf3WideSlots / 16;   // staging passes of 16 slots (16 threads x 4 channels per slot)
constexpr int kSub = 8;                       // sub-tiles of 16 pixels per unit

struct Step {                                 // wave-uniform
    int n, h0, ox, pb, sb;
};

// Tap t of the wave's filter slice as fp32: raw[kc][j] = A[row = output channel oc][k = input channel 32 kc + 8 g + j];
// the data gradient reads the tap flipped and the channels exchanged.
template <bool WT>
__device__ __forceinline__ void load_tap(float (&raw)[2][8], const float* w, int t, int oc, int g) {
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
        const int ic = 32 * kc + 8 * g;
        if constexpr (WT) {
            const f32x4_t a = *(const f32x4_t*)(w + ((8 - t) * 64 + oc) * 64 + ic);
            const f32x4_t b = *(const f32x4_t*)(w + ((8 - t) * 64 + oc) * 64 + ic + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { raw[kc][j] = a[j]; raw[kc][4 + j] = b[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) raw[kc][j] = w[(t * 64 + ic + j) * 64 + oc];
        }
    }
}

__device__ __forceinline__ void split_tap(const float (&raw)[2][8], bf16x8_t (&whi)[2], bf16x8_t (&wlo)[2]) {
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 h, l;
            split_bf16(raw[kc][j], h, l);
            whi[kc][j] = h;
            wlo[kc][j] = l;
        }
}

template <bool WT, bool MASK>
__global__ __launch_bounds__(256, 1) void conv_wide_bf16x3_kernel(const Bf3WideArgs a) {
    extern __shared__ __attribute__((aligned(16))) char bf3_lds[];
    char* const lds = bf3_lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r16 = lane & 15;
    const int oc = 16 * wave + r16, c4 = tid & 15, sp = tid >> 4;
    const size_t blk = (size_t)a.N * a.H * a.W * 64, img = (size_t)a.H * a.W * 64;
    const int RS = a.TW + 2, nslots = (a.TH + 2) * RS, npx = a.TH * a.TW, nsub = (npx + 15) / 16;
    const long G_ = gridDim.x;
    const int s_begin = (int)(((long)blockIdx.x * a.units_total) / G_) * a.SB;
    const int s_end = (int)(((long)(blockIdx.x + 1) * a.units_total) / G_) * a.SB;
    if (s_begin >= s_end) return;

    auto decode = [&](int s, Step& d) {
        const int u = s / a.SB;
        d.sb = s - u * a.SB;
        d.pb = u % a.PB;
        int tile = u / a.PB;
        const int tx = tile % a.tiles_x;
        tile /= a.tiles_x;
        d.n = tile / a.tiles_y;
        d.h0 = (tile % a.tiles_y) * a.TH;
        d.ox = tx * a.TW;
    };
    auto slice = [&](const Step& d) {
        return a.w + (size_t)(WT ? (d.pb * a.SB + d.sb) : (d.sb * a.PB + d.pb)) * (9 * 64 * 64);
    };
    // staging pass j of a step's tile: slots outside the image (the halo) or past the tile read as zero
    auto issue = [&](const Step& d, int j) {
        const int s = sp + 16 * j, sr = s / RS, sc = s - sr * RS;
        const int ih = d.h0 - 1 + sr, iw = d.ox - 1 + sc;
        f32x4_t v = {0.f, 0.f, 0.f, 0.f};
        if (s < nslots && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W)
            v = *(const f32x4_t*)(a.x + d.sb * blk + d.n * img + ((size_t)ih * a.W + iw) * 64 + 4 * c4);
        return v;
    };
    auto commit = [&](char* buf, int j, f32x4_t v) {
        const int s = sp + 16 * j;
        if (s < nslots) store_split4(buf + (size_t)s * kSlot, 8 * c4, v);
    };
    // lane's pixel of sub-tile m -> LDS byte offset of its (tap 0, 0) slot, channels 8 g ..; pixels past the tile
    // compute on pixel 0 and are not stored
    int laddr[kSub];
#pragma unroll
    for (int m = 0; m < kSub; ++m) {
        int p = 16 * m + r16;
        if (p >= npx) p = 0;
        const int pr = p / a.TW, pc = p - pr * a.TW;
        laddr[m] = (pr * RS + pc) * kSlot + 16 * g;
    }

    Step d;
    decode(s_begin, d);
    bf16x8_t whi[9][2], wlo[9][2];
    {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            float raw[2][8];
            load_tap<WT>(raw, slice(d), t, oc, g);
            split_tap(raw, whi[t], wlo[t]);
        }
#pragma unroll
        for (int j = 0; j < kPasses; ++j) commit(lds, j, issue(d, j));
    }
    __syncthreads();
    int cur = 0;
    f32x4_t acc[kSub];
    for (int s = s_begin; s < s_end; ++s) {
        const bool has_next = s + 1 < s_end;
        Step dn = d;
        if (has_next) decode(s + 1, dn);
        const char* buf = lds + (size_t)cur * (kBf3WideSlots * kSlot);
        char* nbuf = lds + (size_t)(cur ^ 1) * (kBf3WideSlots * kSlot);
        if (d.sb == 0) {
#pragma unroll
            for (int m = 0; m < kSub; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        // (the last step "prefetches" its own operands again: no conditional loads, the results are never read)
        // the next tile: loads out before the sub-tiles but the last, split into the other buffer behind them
        f32x4_t stg[kPasses];
#pragma unroll
        for (int j = 0; j < kPasses; ++j) stg[j] = issue(dn, j);
        auto subtile = [&](f32x4_t& acc_m, int m, bool reload) {
            const char* base = buf + laddr[m];
            const float* wn = slice(dn);
            float raw[9][2][8];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int off = ((t / 3) * RS + (t % 3)) * kSlot;
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    const bf16x8_t bhi = *(const bf16x8_t*)(base + off + 64 * kc);
                    const bf16x8_t blo = *(const bf16x8_t*)(base + off + 128 + 64 * kc);
                    acc_m = mfma3(whi[t][kc], wlo[t][kc], bhi, blo, acc_m);
                }
                if (reload) {
                    // tap t of the next filter slice goes out once its MFMAs have issued; it is split into the
                    // registers of tap t three taps later (the loads have 18 MFMAs to land)
                    load_tap<WT>(raw[t], wn, t, oc, g);
                    if (t >= 3) split_tap(raw[t - 3], whi[t - 3], wlo[t - 3]);
                }
            }
            if (reload) {
#pragma unroll
                for (int t = 6; t < 9; ++t) split_tap(raw[t], whi[t], wlo[t]);
            }
        };
        // sub-tiles but the last
#pragma unroll
        for (int m = 0; m < kSub - 1; ++m)
            if (m < nsub - 1) subtile(acc[m], m, false);
#pragma unroll
        for (int j = 0; j < kPasses; ++j) commit(nbuf, j, stg[j]);
        // the last sub-tile carries the next filter slice
        {
            const int ml = nsub - 1;
            f32x4_t al = acc[0];
#pragma unroll
            for (int m = 1; m < kSub; ++m)
                if (m == ml) al = acc[m];
            subtile(al, ml, true);
#pragma unroll
            for (int m = 0; m < kSub; ++m)
                if (m == ml) acc[m] = al;
        }
        if (d.sb == a.SB - 1) {
            // epilogue in fp32: bias, activation, mask
            const int co = 16 * wave + 4 * g;
            f32x4_t bias4 = {0.f, 0.f, 0.f, 0.f};
            if (a.bias) bias4 = *(const f32x4_t*)(a.bias + d.pb * 64 + co);
            const float slope = act_slope(a.act), mslope = act_slope(a.mask_act);
            const size_t unit_base = d.pb * blk + d.n * img + co;
#pragma unroll
            for (int m = 0; m < kSub; ++m) {
                const int p = 16 * m + r16, pr = p / a.TW, pc = p - pr * a.TW;
                const int oh = d.h0 + pr, ow = d.ox + pc;
                if (m < nsub && p < npx && oh < a.H && ow < a.W) {
                    const size_t o = unit_base + ((size_t)oh * a.W + ow) * 64;
                    f32x4_t v = act_apply4(acc[m] + bias4, a.act, slope);
                    if constexpr (MASK) v = act_grad4(v, *(const f32x4_t*)(a.mask + o), a.mask_act, mslope);
                    *(f32x4_t*)(a.y + o) = v;
                }
            }
        }
        __syncthreads();                 // the next tile is complete; nobody reads this one any more
        cur ^= 1;
        d = dn;
    }
}

struct Bf3PairsArgs {
    const float* x;
    const float* dpre;
    float* part;
    int part_stride, cob, N, H, W, TH, TW, ntx, nty, tiles;
};

__global__ __launch_bounds__(256, 2) void wgrad3x3c64_bf16x3_pairs_kernel(Bf3PairsArgs a) {
    const int pair = blockIdx.y, ib = pair / a.cob, ob = pair - ib * a.cob;
    const size_t blk = (size_t)a.N * a.H * a.W * 64;
    wgrad3x3c64_bf16x3_body(a.x + ib * blk, a.dpre + ob * blk, a.part + ((size_t)pair * gridDim.x + blockIdx.x) * a.part_stride,
                            a.N, a.H, a.W, a.TH, a.TW, a.ntx, a.nty, a.tiles, blockIdx.x, gridDim.x);
}

}  // namespace

hipError_t launch_conv_wide_bf16x3(bool transpose, const Bf3WideArgs& a, int grid, hipStream_t s) {
    const bool mask = a.mask != nullptr;
    if (transpose) {
        if (mask) return launch_with_lds<conv_wide_bf16x3_kernel<true, true>>(dim3(grid), dim3(256), kBf3WideLds, s, a);
        return launch_with_lds<conv_wide_bf16x3_kernel<true, false>>(dim3(grid), dim3(256), kBf3WideLds, s, a);
    }
    if (mask) return launch_with_lds<conv_wide_bf16x3_kernel<false, true>>(dim3(grid), dim3(256), kBf3WideLds, s, a);
    return launch_with_lds<conv_wide_bf16x3_kernel<false, false>>(dim3(grid), dim3(256), kBf3WideLds, s, a);
}

hipError_t launch_wgrad3x3c64_bf16x3_pairs(const float* x, const float* dpre, float* part, int part_stride, int cib, int cob, int N,
                                           int H, int W, const Bf3Plan& p, hipStream_t s) {
    Bf3PairsArgs a{x, dpre, part, part_stride, cob, N, H, W, p.TH, p.TW, p.ntx, p.nty, p.tiles};
    return launch_with_lds<wgrad3x3c64_bf16x3_pairs_kernel>(dim3(p.grid, cib * cob), dim3(256), p.lds, s, a);
}

}  // namespace srx
