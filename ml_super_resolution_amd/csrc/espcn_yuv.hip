// espcn_yuv.hip -- planar YUV 4:2:0 frames (the YUV4MPEG2 frame payload) on either side of ESPCN's float network: the colour
// conversion next to the byte decode and encode of espcn_frames.hip, so that a frame travels as 1.5 bytes per pixel.
//
// A frame of H x W is one byte string: Y [H,W], U [CH,CW], V [CH,CW], CH = (H + 1) / 2, CW = (W + 1) / 2; N frames lie back to
// back, so a frame of odd size starts at an odd address.  All arithmetic is int32 with 14 fractional bits, h = 1 << 13, `>>`
// the arithmetic shift, clip8 the clamp to [0, 255]; the coefficients are floor(v * 16384 + 0.5) of the real values in
// double (srx_yuv420_coeffs, the one place that computes them).
//
//   srx_yuv420_lut_float  LR-sized.  Pixel (y, x) takes the chroma sample (y >> 1, x >> 1): replication, no siting filter.
//                         c = Y - yoff, d = U - 128, e = V - 128;  R = clip8((cy c + crv e + h) >> 14),
//                         G = clip8((cy c - cgu d - cgv e + h) >> 14),  B = clip8((cy c + cbu d + h) >> 14);  out = lut[byte],
//                         the table in LDS as in u8_lut_float_kernel.  One thread per pixel: 1 + 2 cached bytes read, 12 written.
//   srx_unit_yuv420       HR-sized, the hot one: 12 bytes read and 1.5 written per pixel.  Each float goes through
//                         encode_unit_u8 to a byte;  Y = clip8(yoff + ((kry R + kgy G + kby B + h) >> 14));  chroma sample
//                         (j, i) from the sums over the pixels (min(2 j + a, H - 1), min(2 i + b, W - 1)):
//                         U = clip8(128 + ((kru SR + kgu SG + kbu SB + (1 << 15)) >> 16)), V likewise -- one rounding for the
//                         average and the matrix.  A thread owns whole 2 x 2 chroma blocks: every float is read once and the
//                         sums stay in registers.  W % 8 == 0, x 16-byte and yuv 4-byte aligned: 4 x 2 pixels per thread,
//                         16-byte nontemporal loads with consecutive lanes on consecutive addresses, handed to the owning
//                         thread through LDS (a lane that read its own 48 bytes of a row would make every load touch six
//                         times the cache lines), 4-byte stores of luma and, a lane pair trading chroma, of U and V.
//                         Any other W or alignment: 8 x 2 pixels per thread, 4-byte loads clamped at the edges, byte stores.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>

#include "../../include/srx.h"
#include "u8_encode.h"

namespace srx {
int set_error(int code, const char* fmt, ...);

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFrac = 14, kHalf = 1 << 13;
constexpr int kUnitW = 8;           // pixels of a row a thread of the general encode owns (two rows of them)
constexpr int kVecW = 4, kVecPieces = 3 * kVecW / 4;       // the 16-byte path: 4 x 2 pixels, three 16-byte pieces of each row
// grids are capped and the kernels stride: 4 M pixels (decode), 1 M units = 8 M / 16 M pixels (encode: 16-byte / general) per sweep
constexpr uint32_t kMaxBlocksDecode = 16384, kMaxBlocksEncode = 4096;

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void yuv420_lut_float_kernel(const uint8_t* __restrict__ yuv, const float* __restrict__ lut,
                                                               float* __restrict__ out, uint32_t H, uint32_t W, uint32_t pixels,
                                                               srx_yuv420_coeffs_t c) {
    __shared__ float table[256];
    table[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const uint32_t CH = (H + 1) / 2, CW = (W + 1) / 2, plane = H * W, frame = plane + 2 * CH * CW;
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < pixels; p += gridDim.x * 256) {
        const uint32_t n = p / plane, q = p - n * plane, y = q / W, x = q - y * W;
        const uint8_t* f = yuv + (size_t)n * frame;
        const uint32_t ci = plane + (y >> 1) * CW + (x >> 1);
        const int cc = c.cy * ((int)f[q] - c.yoff) + kHalf, d = (int)f[ci] - 128, e = (int)f[ci + CH * CW] - 128;
        float* o = out + (size_t)p * 3;
        o[0] = table[clip8((cc + c.crv * e) >> kFrac)];
        o[1] = table[clip8((cc - c.cgu * d - c.cgv * e) >> kFrac)];
        o[2] = table[clip8((cc + c.cbu * d) >> kFrac)];
    }
}

// One unit of the encode: PW pixels of each row of a row pair in f[a][3 i + ch], PW / 2 whole chroma blocks.  Gives the luma
// bytes of each row packed four to a word and the PW / 2 bytes of U and of V packed from bit 0.
template <int PW>
__device__ __forceinline__ void encode_unit(const float (&f)[2][3 * PW], const srx_yuv420_coeffs_t& c, uint32_t (&luma)[2][PW / 4],
                                            uint32_t& cu, uint32_t& cv) {
    cu = cv = 0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int g = 0; g < PW / 4; ++g) luma[a][g] = 0;
#pragma unroll
    for (int k = 0; k < PW / 2; ++k) {
        int sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int i = 2 * k + b;
                const int R = (int)encode_unit_u8(f[a][3 * i]), G = (int)encode_unit_u8(f[a][3 * i + 1]), B = (int)encode_unit_u8(f[a][3 * i + 2]);
                sr += R; sg += G; sb += B;
                const uint32_t yv = (uint32_t)clip8(c.yoff + ((c.kry * R + c.kgy * G + c.kby * B + kHalf) >> kFrac));
                luma[a][i / 4] |= yv << (8 * (i % 4));
            }
        cu |= (uint32_t)clip8(128 + ((c.kru * sr + c.kgu * sg + c.kbu * sb + (1 << 15)) >> 16)) << (8 * k);
        cv |= (uint32_t)clip8(128 + ((c.krv * sr + c.kgv * sg + c.kbv * sb + (1 << 15)) >> 16)) << (8 * k);
    }
}

// The 16-byte path: W % 8 == 0, x 16-byte aligned, yuv 4-byte aligned (then every row of x, every luma row and every chroma row
// of every frame is aligned as well: 12 W, W and W / 2 are multiples of 16, 8 and 4).  A unit is 4 x 2 pixels, 48 bytes of
// each row; units are numbered along a row pair, then over the row pairs and frames, so the units of a row pair are contiguous
// in x.  A workgroup takes 256 consecutive units at a time: thread t loads the 16-byte pieces t, t + 256, t + 512 of the
// tile's 768 per row -- consecutive lanes, consecutive addresses -- into LDS, then reads back the three pieces of its own
// unit (48-byte stride: the 16 lanes of a 16-byte LDS read fall on 16 different slots).  A lane pair trades its chroma
// bytes, so that the even lane stores four bytes of U and the odd lane four of V.  UW = W / 4 units per row pair, even.
__global__ __launch_bounds__(256) void unit_yuv420_vec_kernel(const float* __restrict__ x, uint8_t* __restrict__ yuv, uint32_t H, uint32_t W,
                                                              uint32_t UW, uint32_t units, srx_yuv420_coeffs_t c) {
    __shared__ f32x4 tile[2][kVecPieces * 256];
    const uint32_t CH = (H + 1) / 2, CW = W / 2, plane = H * W, frame = plane + 2 * CH * CW;
    for (uint32_t base = blockIdx.x * 256; base < units; base += gridDim.x * 256) {
#pragma unroll
        for (int k = 0; k < kVecPieces; ++k) {
            const uint32_t q = k * 256 + threadIdx.x, u = base + q / kVecPieces, part = q % kVecPieces;
            if (u < units) {
                const uint32_t t = u / UW, ux = u - t * UW, n = t / CH, j = t - n * CH;
                const float* row = x + ((size_t)(n * H + 2 * j) * W + ux * kVecW) * 3;
                tile[0][q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row) + part);
                tile[1][q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row + (2 * j + 1 < H ? (size_t)W * 3 : 0)) + part);
            }
        }
        __syncthreads();
        const uint32_t u = base + threadIdx.x;
        float f[2][3 * kVecW];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int k = 0; k < kVecPieces; ++k) {
                const f32x4 v = tile[a][kVecPieces * threadIdx.x + k];
                f[a][4 * k] = v[0]; f[a][4 * k + 1] = v[1]; f[a][4 * k + 2] = v[2]; f[a][4 * k + 3] = v[3];
            }
        __syncthreads();                // (the next round's loads overwrite the tile)
        uint32_t luma[2][1], cu, cv;
        encode_unit<kVecW>(f, c, luma, cu, cv);
        // units 2 m and 2 m + 1 lie in one row pair (UW is even) and in one wave; both exist or neither (units is even)
        const uint32_t mine = (threadIdx.x & 1) ? cv : cu, theirs = (threadIdx.x & 1) ? cu : cv;
        const uint32_t got = (uint32_t)__shfl_xor((int)theirs, 1);
        if (u < units) {
            const uint32_t t = u / UW, ux = u - t * UW, n = t / CH, j = t - n * CH;
            uint8_t* fr = yuv + (size_t)n * frame;
            uint8_t* yo = fr + 2 * j * W + ux * kVecW;
            *reinterpret_cast<uint32_t*>(yo) = luma[0][0];
            if (2 * j + 1 < H) *reinterpret_cast<uint32_t*>(yo + W) = luma[1][0];
            // even lane: U of units u, u + 1; odd lane: V of units u - 1, u -- four chroma samples from column (ux & ~1) * 2 on
            uint8_t* co = fr + plane + ((threadIdx.x & 1) ? CH * CW : 0) + j * CW + (ux & ~1u) * (kVecW / 2);
            *reinterpret_cast<uint32_t*>(co) = (threadIdx.x & 1) ? (got | mine << 16) : (mine | got << 16);
        }
    }
}

// Any W, any float offset of x and byte offset of yuv: a thread owns 8 x 2 pixels, reads them float by float with the edge
// replicated, and stores bytes.  UW = ceil(W / 8) units per row pair.
__global__ __launch_bounds__(256) void unit_yuv420_kernel(const float* __restrict__ x, uint8_t* __restrict__ yuv, uint32_t H, uint32_t W,
                                                          uint32_t UW, uint32_t units, srx_yuv420_coeffs_t c) {
    const uint32_t CH = (H + 1) / 2, CW = (W + 1) / 2, plane = H * W, frame = plane + 2 * CH * CW;
    for (uint32_t u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
        const uint32_t t = u / UW, ux = u - t * UW, n = t / CH, j = t - n * CH;
        const uint32_t x0 = ux * kUnitW, y0 = 2 * j, rows = y0 + 1 < H ? 2 : 1;
        float f[2][3 * kUnitW];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float* row = x + ((size_t)(n * H + y0 + (a < (int)rows ? a : 0)) * W + x0) * 3;
#pragma unroll
            for (int i = 0; i < kUnitW; ++i) {
                const uint32_t px = min((uint32_t)i, W - 1 - x0);      // the edge replicated
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) f[a][3 * i + ch] = row[3 * px + ch];
            }
        }
        uint32_t luma[2][kUnitW / 4], cu, cv;
        encode_unit<kUnitW>(f, c, luma, cu, cv);
        uint8_t* fr = yuv + (size_t)n * frame;
        uint8_t* yo = fr + y0 * W + x0;
        uint8_t* uo = fr + plane + j * CW + x0 / 2;
        uint8_t* vo = uo + CH * CW;
#pragma unroll
        for (int i = 0; i < kUnitW; ++i)
            if (x0 + i < W) {
                yo[i] = (uint8_t)(luma[0][i / 4] >> (8 * (i % 4)));
                if (rows == 2) yo[W + i] = (uint8_t)(luma[1][i / 4] >> (8 * (i % 4)));
            }
#pragma unroll
        for (int k = 0; k < kUnitW / 2; ++k)
            if (x0 / 2 + k < CW) {
                uo[k] = (uint8_t)(cu >> (8 * k));
                vo[k] = (uint8_t)(cv >> (8 * k));
            }
    }
}

// 0 and the element count N H W 3 in *elems, or the refusal
int check_frames(const char* what, int N, int H, int W, const srx_yuv420_coeffs_t* c, long* elems) {
    if (!c) return set_error(SRX_ERR_BAD_ARG, "null pointer");
    if (N <= 0 || H <= 0 || W <= 0) return set_error(SRX_ERR_BAD_ARG, "non-positive dimension");
    const long rows = (long)N * H;
    if (rows >= (1L << 31) || rows * W * 3L >= (1L << 31)) return set_error(SRX_ERR_UNSUPPORTED, "%s: frames beyond 32-bit offsets", what);
    *elems = rows * W * 3L;
    return SRX_OK;
}

int fixed(double v) { return (int)__builtin_floor(v * 16384.0 + 0.5); }

}  // namespace
}  // namespace srx

using namespace srx;

namespace srx {
// The one statement of the coefficient formulas, for samples of `depth` bits: limited range puts luma on 219 and chroma on 224
// steps of 2^(depth - 8) codes above 16 << (depth - 8); depth 8 gives srx_yuv420_coeffs' integers (219 * 1 / 255 is 219 / 255).
int yuv_coeffs_fill(const char* what, int matrix, int full_range, int depth, srx_yuv420_coeffs_t* c) {
    if (!c) return set_error(SRX_ERR_BAD_ARG, "null pointer");
    double kr, kb;
    if (matrix == SRX_YUV_BT601) { kr = 0.299; kb = 0.114; }
    else if (matrix == SRX_YUV_BT709) { kr = 0.2126; kb = 0.0722; }
    else return set_error(SRX_ERR_BAD_ARG, "%s: matrix %d (0: bt601, 1: bt709)", what, matrix);
    const double kg = 1.0 - kr - kb;
    const double step = (double)(1 << (depth - 8)), top = (double)((1 << depth) - 1);
    const double ys = full_range ? 1.0 : 219.0 * step / top, cs = full_range ? 1.0 : 224.0 * step / top;
    c->yoff = full_range ? 0 : 16 << (depth - 8);
    c->cy = fixed(1.0 / ys);
    c->crv = fixed(2.0 * (1.0 - kr) / cs);
    c->cgu = fixed(2.0 * (1.0 - kb) * kb / kg / cs);
    c->cgv = fixed(2.0 * (1.0 - kr) * kr / kg / cs);
    c->cbu = fixed(2.0 * (1.0 - kb) / cs);
    c->kry = fixed(kr * ys);
    c->kgy = fixed(kg * ys);
    c->kby = fixed(kb * ys);
    c->kru = fixed(-kr / (2.0 * (1.0 - kb)) * cs);
    c->kgu = fixed(-kg / (2.0 * (1.0 - kb)) * cs);
    c->kbu = fixed(0.5 * cs);
    c->krv = fixed(0.5 * cs);
    c->kgv = fixed(-kg / (2.0 * (1.0 - kr)) * cs);
    c->kbv = fixed(-kb / (2.0 * (1.0 - kr)) * cs);
    c->reserved = 0;
    return SRX_OK;
}
}  // namespace srx

extern "C" int srx_yuv420_coeffs(int matrix, int full_range, srx_yuv420_coeffs_t* c) {
    return yuv_coeffs_fill("yuv420_coeffs", matrix, full_range, 8, c);
}

extern "C" int srx_yuv_coeffs(int matrix, int full_range, int depth, srx_yuv420_coeffs_t* c) {
    if (depth != 8 && depth != 10 && depth != 12) return set_error(SRX_ERR_BAD_ARG, "yuv_coeffs: depth %d (8, 10 or 12)", depth);
    return yuv_coeffs_fill("yuv_coeffs", matrix, full_range, depth, c);
}

extern "C" int srx_yuv420_lut_float(const uint8_t* yuv, int N, int H, int W, const srx_yuv420_coeffs_t* c, const float* lut, float* out,
                                    srx_stream_t stream) {
    if (!yuv || !lut || !out) return set_error(SRX_ERR_BAD_ARG, "null pointer");
    long elems;
    const int rc = check_frames("yuv420_lut_float", N, H, W, c, &elems);
    if (rc != SRX_OK) return rc;
    if ((uintptr_t)out & 3u) return set_error(SRX_ERR_ALIGN, "yuv420_lut_float: out must be 4-byte aligned");
    const uint32_t pixels = (uint32_t)(elems / 3), blocks = (pixels + 255) / 256;
    hipLaunchKernelGGL(yuv420_lut_float_kernel, dim3(blocks < kMaxBlocksDecode ? blocks : kMaxBlocksDecode), dim3(256), 0, (hipStream_t)stream, yuv, lut, out,
                       (uint32_t)H, (uint32_t)W, pixels, *c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(SRX_ERR_LAUNCH, "yuv420_lut_float launch failed: %s", hipGetErrorString(e));
    return SRX_OK;
}

extern "C" int srx_unit_yuv420(const float* x, int N, int H, int W, const srx_yuv420_coeffs_t* c, uint8_t* yuv, srx_stream_t stream) {
    if (!x || !yuv) return set_error(SRX_ERR_BAD_ARG, "null pointer");
    long elems;
    const int rc = check_frames("unit_yuv420", N, H, W, c, &elems);
    if (rc != SRX_OK) return rc;
    if ((uintptr_t)x & 3u) return set_error(SRX_ERR_ALIGN, "unit_yuv420: x must be 4-byte aligned");
    const bool vec = W % 8 == 0 && ((uintptr_t)x & 15u) == 0 && ((uintptr_t)yuv & 3u) == 0;
    const uint32_t UW = vec ? (uint32_t)W / kVecW : ((uint32_t)W + kUnitW - 1) / kUnitW;
    const uint32_t units = (uint32_t)N * (((uint32_t)H + 1) / 2) * UW, blocks = (units + 255) / 256;
    const dim3 grid(blocks < kMaxBlocksEncode ? blocks : kMaxBlocksEncode);
    if (vec)
        hipLaunchKernelGGL(unit_yuv420_vec_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, yuv, (uint32_t)H, (uint32_t)W, UW, units, *c);
    else
        hipLaunchKernelGGL(unit_yuv420_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, yuv, (uint32_t)H, (uint32_t)W, UW, units, *c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(SRX_ERR_LAUNCH, "unit_yuv420 launch failed: %s", hipGetErrorString(e));
    return SRX_OK;
}
