// feature_mosaic.hip -- the reference's feature-map figure encoder on the GPU, byte for byte.
//
// vdsr/vdsr/experiment_feature_map_visualize.py:80-110 splits a [1,H,W,64] activation into its 64 maps, concatenates
// rows of 8 along the width and the 8 rows along the height, and encodes the [8H,8W] mosaic as
// saturate_cast(x * 127.5 + 127.5, uint8): channel k at tile row k / 8, tile column k % 8.  Pinned by the reference's own
// output: assets/vdsr-fig2-conv.1.png and conv.19.png (P8), every pixel.
//
// A channel-last -> planar transpose with a 4:1 narrowing; memory-bound (reads 256 B, writes 64 B per pixel).
//
// One workgroup (256 threads) owns kTW = 128 pixels of one image row.
//   load    thread (cg = t % 16, q = t / 16) reads one float4 (channels 4cg .. 4cg+3) of pixels 4q' .. 4q'+3 for
//           q' = q and q + 16: 8 loads in flight per thread; 16 lanes cover a pixel's 256 B, so every request is two whole
//           128-byte lines.
//   encode  the four pixels of one channel pack into one dword: the tile is written with ds_write_b32, not with bytes.
//   tile    LDS [64 channels][128 bytes], no padding; the 16-byte slot s of row c sits at slot s ^ ((c / 4) % 8).
//           Rows are 32 dwords apart (no bank change), so within a half-wave (16 cg x 2 adjacent q') the swizzle alone
//           spreads the 16 channel groups over the 8 slots: 2 addresses per bank, which ds_write_b32 absorbs.  A padded
//           row cannot do this and keep the 16-byte alignment ds_read_b128 needs: 128 + 16 bytes leaves rows 4cg on two banks.
//   store   after one barrier thread (s = t % 8, c = t / 8 and c + 32) reads slot s of row c (ds_read_b128: each of its
//           16-lane groups holds rows of both parities and both slot halves, no conflict) and stores it; 8 lanes write
//           a channel's whole 128-byte run.
// The destination of channel k starts at (k % 8) * W + x0 in an output row of 8W bytes, so its alignment depends on W,
// on the segment and on `out` itself: each store looks at its own address.  16-byte aligned and wholly inside the run: one
// 16-byte store; 4-byte aligned: four dwords; else bytes.  A store never extends past the run: the next byte belongs to
// the neighbouring map or the next row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srx.h"
#include "u8_encode.h"

namespace srx {
int set_error(int code, const char* fmt, ...);

namespace {
constexpr int kTW = SRX_FEATURE_MOSAIC_TW;
static_assert(kTW == 128, "the lane maps below are written for 128-pixel segments");

__global__ __launch_bounds__(256) void feature_mosaic_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int H,
                                                                int W, int segs) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[64 * kTW];
    const int t = threadIdx.x;
    const int seg = (int)(blockIdx.x % (unsigned)segs);
    const size_t row = blockIdx.x / (unsigned)segs;          // n * H + y
    const int y = (int)(row % (unsigned)H);
    const size_t n = row / (unsigned)H;
    const int x0 = seg * kTW;
    const int tw = W - x0 < kTW ? W - x0 : kTW;              // pixels of this segment (>= 1)

    const int cg = t & 15, q = t >> 4;
    const float* src = x + ((row * W + x0) * 64 + 4 * cg);
    float4 v[2][4];
#pragma unroll
    for (int P = 0; P < 2; ++P)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = 64 * P + 4 * q + i;
            v[P][i] = p < tw ? *reinterpret_cast<const float4*>(src + (size_t)p * 64) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
    for (int P = 0; P < 2; ++P) {
        const int qq = 16 * P + q;                           // dword column of the row: pixels 4qq .. 4qq+3
        const int phys = (((qq >> 2) ^ (cg & 7)) << 4) | ((qq & 3) << 2);
        const float f[4][4] = {{v[P][0].x, v[P][1].x, v[P][2].x, v[P][3].x},
                               {v[P][0].y, v[P][1].y, v[P][2].y, v[P][3].y},
                               {v[P][0].z, v[P][1].z, v[P][2].z, v[P][3].z},
                               {v[P][0].w, v[P][1].w, v[P][2].w, v[P][3].w}};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t d = encode_u8(f[j][0]) | (encode_u8(f[j][1]) << 8) | (encode_u8(f[j][2]) << 16) | (encode_u8(f[j][3]) << 24);
            *reinterpret_cast<uint32_t*>(tile + (4 * cg + j) * kTW + phys) = d;
        }
    }
    __syncthreads();

    const int s = t & 7;
    const int valid = tw - 16 * s;                           // bytes of this slot that lie inside the run
    if (valid <= 0) return;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = (t >> 3) + 32 * k;
        const uint4 d = *reinterpret_cast<const uint4*>(tile + c * kTW + ((s ^ ((c >> 2) & 7)) << 4));
        uint8_t* dst = out + (((n * 8 + (c >> 3)) * H + y) * 8 * (size_t)W + (size_t)(c & 7) * W + x0 + 16 * s);
        const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
        if (valid >= 16 && (a & 15) == 0) {
            *reinterpret_cast<uint4*>(dst) = d;
        } else if (valid >= 16 && (a & 3) == 0) {
            uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
            d4[0] = d.x; d4[1] = d.y; d4[2] = d.z; d4[3] = d.w;
        } else {
            const uint32_t w[4] = {d.x, d.y, d.z, d.w};
            const int nb = valid < 16 ? valid : 16;
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (b < nb) dst[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
        }
    }
}

}  // namespace
}  // namespace srx

using namespace srx;

extern "C" int srx_feature_mosaic_u8(const float* x, uint8_t* out, int N, int H, int W, srx_stream_t stream) {
    if (!x || !out) return set_error(SRX_ERR_BAD_ARG, "feature_mosaic_u8: null pointer");
    if (N <= 0 || H <= 0 || W <= 0) return set_error(SRX_ERR_BAD_ARG, "feature_mosaic_u8: bad dims N %d H %d W %d", N, H, W);
    const size_t pixels = (size_t)N * H * W;
    const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
    if (xa < oa + pixels * 64 && oa < xa + pixels * 256) return set_error(SRX_ERR_BAD_ARG, "feature_mosaic_u8: out overlaps x");
    if (xa & 15) return set_error(SRX_ERR_ALIGN, "feature_mosaic_u8: x is not 16-byte aligned");
    const int segs = (W + kTW - 1) / kTW;
    const size_t blocks = (size_t)N * H * segs;
    if (blocks > 0x7fffffffu) return set_error(SRX_ERR_BAD_ARG, "feature_mosaic_u8: N*H*ceil(W/%d) = %zu exceeds the grid limit", kTW, blocks);
    hipLaunchKernelGGL(feature_mosaic_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, out, H, W, segs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(SRX_ERR_LAUNCH, "feature_mosaic_u8 launch failed: %s", hipGetErrorString(e));
    return SRX_OK;
}
