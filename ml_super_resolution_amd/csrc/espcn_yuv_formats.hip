// espcn_yuv_formats.hip -- planar YUV frames of 8, 10 or 12 bits, sampled 4:4:4, 4:2:2 or 4:2:0, on either side of ESPCN's float
// network: espcn_yuv.hip's arithmetic with the offsets scaled by the depth, the chroma rounding shifted by the block size and the
// float table widened.  8-bit 4:2:0 itself stays with espcn_yuv.hip: the entry points here hand (8, 1, 1) over to its launchers.
//
// A format is (depth, sub_x, sub_y); max = (1 << depth) - 1, mid = 1 << (depth - 1).  A sample is one byte at depth 8 and two
// bytes, little-endian, above; a sample above max in a 16-bit container is read as max.  A frame of H x W is Y [H,W], U [CH,CW],
// V [CH,CW], CH = (H + sub_y) >> sub_y, CW = (W + sub_x) >> sub_x; N frames lie back to back.  All arithmetic is int32 with 14
// fractional bits; the coefficients are srx_yuv_coeffs' at the depth; clip the clamp to [0, max].
//
//   srx_yuv_lut_float  LR-sized, one thread per pixel.  Pixel (y, x) takes the chroma sample (y >> sub_y, x >> sub_x);
//                      c = Y - yoff, d = U - mid, e = V - mid;  R = clip((cy c + crv e + h) >> 14), G and B as at 4:2:0;
//                      out = lut[code], the caller's 2^depth floats in LDS (16 KB at depth 12).
//   srx_unit_yuv       HR-sized.  Each float goes through encode_unit_bits(y, max);  Y = clip(yoff + ((kry R + kgy G + kby B + h)
//                      >> 14));  chroma sample (j, i) from the sums over the (1 << sub_y) x (1 << sub_x) pixels
//                      (min((j << sub_y) + a, H - 1), min((i << sub_x) + b, W - 1)):  U = clip(mid + ((kru SR + kgu SG + kbu SB +
//                      (1 << (13 + sub_x + sub_y))) >> (14 + sub_x + sub_y))), V likewise -- one rounding for the average and the
//                      matrix.  A thread owns whole chroma blocks: every float is read once and the sums stay in registers.
//                      The two paths are unit_yuv420's: 4 pixels of 1 << sub_y rows per thread from lane-contiguous 16-byte
//                      nontemporal loads handed over through LDS, stores of 4 bytes and more; or 8 pixels of as many rows from
//                      4-byte loads clamped at the edges, with sample-sized stores.
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
constexpr int kUnitW = 8;           // pixels of a row a thread of the general encode owns (1 << sub_y rows of them)
constexpr int kVecW = 4, kVecPieces = 3 * kVecW / 4;       // the 16-byte path: 4 pixels of a row, three 16-byte pieces
// grids are capped and the kernels stride, as in espcn_yuv.hip: 4 M pixels (decode), 1 M units (encode) per sweep
constexpr uint32_t kMaxBlocksDecode = 16384, kMaxBlocksEncode = 4096;

template <int BPS> struct sample_of { typedef uint8_t type; };
template <> struct sample_of<2> { typedef uint16_t type; };

__device__ __forceinline__ int clip_to(int v, int top) { return min(max(v, 0), top); }

template <int SX, int SY, int BPS>
__global__ __launch_bounds__(256) void yuv_lut_float_kernel(const void* __restrict__ yuv_, const float* __restrict__ lut, float* __restrict__ out,
                                                            uint32_t H, uint32_t W, uint32_t pixels, int depth, srx_yuv420_coeffs_t c) {
    typedef typename sample_of<BPS>::type T;
    __shared__ float table[BPS == 1 ? 256 : 4096];
    const int top = (1 << depth) - 1, mid = 1 << (depth - 1);
    for (int i = threadIdx.x; i <= top; i += 256) table[i] = lut[i];
    __syncthreads();
    const T* yuv = static_cast<const T*>(yuv_);
    const uint32_t CH = (H + SY) >> SY, CW = (W + SX) >> SX, plane = H * W, frame = plane + 2 * CH * CW;       // in samples
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < pixels; p += gridDim.x * 256) {
        const uint32_t n = p / plane, q = p - n * plane, y = q / W, x = q - y * W;
        const T* f = yuv + (size_t)n * frame;
        const uint32_t ci = plane + (y >> SY) * CW + (x >> SX);
        // a sample above max is read as max: no accumulator leaves the range the coefficients were checked for
        const int Y = min((int)f[q], top), U = min((int)f[ci], top), V = min((int)f[ci + CH * CW], top);
        const int cc = c.cy * (Y - c.yoff) + kHalf, d = U - mid, e = V - mid;
        float* o = out + (size_t)p * 3;
        o[0] = table[clip_to((cc + c.crv * e) >> kFrac, top)];
        o[1] = table[clip_to((cc - c.cgu * d - c.cgv * e) >> kFrac, top)];
        o[2] = table[clip_to((cc + c.cbu * d) >> kFrac, top)];
    }
}

// One unit of the encode: PW pixels of each of the 1 << SY rows in f[a][3 i + ch], PW >> SX whole chroma blocks.  Gives the luma
// codes of each row and the codes of U and of V, one per element.
template <int PW, int SX, int SY>
__device__ __forceinline__ void encode_unit(const float (&f)[1 << SY][3 * PW], const srx_yuv420_coeffs_t& c, int depth,
                                            uint32_t (&luma)[1 << SY][PW], uint32_t (&cu)[PW >> SX], uint32_t (&cv)[PW >> SX]) {
    const int top = (1 << depth) - 1, mid = 1 << (depth - 1);
    constexpr int kShift = kFrac + SX + SY, kRound = 1 << (kShift - 1);
#pragma unroll
    for (int k = 0; k < (PW >> SX); ++k) {
        int sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int a = 0; a < (1 << SY); ++a)
#pragma unroll
            for (int b = 0; b < (1 << SX); ++b) {
                const int i = (k << SX) + b;
                const int R = (int)encode_unit_bits(f[a][3 * i], (uint32_t)top), G = (int)encode_unit_bits(f[a][3 * i + 1], (uint32_t)top),
                          B = (int)encode_unit_bits(f[a][3 * i + 2], (uint32_t)top);
                sr += R; sg += G; sb += B;
                luma[a][i] = (uint32_t)clip_to(c.yoff + ((c.kry * R + c.kgy * G + c.kby * B + kHalf) >> kFrac), top);
            }
        cu[k] = (uint32_t)clip_to(mid + ((c.kru * sr + c.kgu * sg + c.kbu * sb + kRound) >> kShift), top);
        cv[k] = (uint32_t)clip_to(mid + ((c.krv * sr + c.kgv * sg + c.kbv * sb + kRound) >> kShift), top);
    }
}

// Four codes of BPS bytes each, stored as one or two 4-byte words at a 4-byte aligned address.
template <int BPS>
__device__ __forceinline__ void store4(uint8_t* at, const uint32_t* v) {
    uint32_t* w = reinterpret_cast<uint32_t*>(at);
    if constexpr (BPS == 1) {
        w[0] = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
    } else {
        w[0] = v[0] | v[1] << 16;
        w[1] = v[2] | v[3] << 16;
    }
}

// The 16-byte path: W % 8 == 0, x 16-byte aligned, yuv 4-byte aligned.  Then every row of x, every luma row and every chroma row
// of every frame is aligned as well, in all nine formats: a row of x is 12 W bytes, a multiple of 16; a luma row is W bps
// bytes, a multiple of 8; a chroma row is CW bps bytes with CW = W or W / 2, a multiple of 4; so the planes H W bps and
// CH CW bps and with them the frames are multiples of 4 bytes.  A unit is 4 pixels of each of the 1 << SY rows of a chroma
// row, 48 bytes a row; units are numbered along a chroma row, then over the chroma rows and frames.  A workgroup takes 256
// consecutive units at a time: thread t loads the 16-byte pieces t, t + 256, t + 512 of the tile's 768 per row -- consecutive
// lanes, consecutive addresses -- into LDS, then reads back the three pieces of its own unit (48-byte stride: the 16 lanes of
// a 16-byte LDS read fall on 16 different slots).  12 KB of LDS a row: 24 KB with SY = 1, as unit_yuv420_vec_kernel, six
// workgroups to a CU.  A unit's luma is 4 or 8 bytes a row, its U and V 4 or 8 bytes each -- except at 8 bits with SX = 1,
// where they are two bytes each and a lane pair trades them, so that the even lane stores four bytes of U and the odd lane
// four of V.  UW = W / 4 units per chroma row, even.
template <int SX, int SY, int BPS>
__global__ __launch_bounds__(256) void unit_yuv_vec_kernel(const float* __restrict__ x, uint8_t* __restrict__ yuv, uint32_t H, uint32_t W,
                                                           uint32_t UW, uint32_t units, int depth, srx_yuv420_coeffs_t c) {
    constexpr int ROWS = 1 << SY, NC = kVecW >> SX;
    __shared__ f32x4 tile[ROWS][kVecPieces * 256];
    const uint32_t CH = (H + SY) >> SY, CW = W >> SX, plane = H * W, frame = plane + 2 * CH * CW;             // in samples
    for (uint32_t base = blockIdx.x * 256; base < units; base += gridDim.x * 256) {
#pragma unroll
        for (int k = 0; k < kVecPieces; ++k) {
            const uint32_t q = k * 256 + threadIdx.x, u = base + q / kVecPieces, part = q % kVecPieces;
            if (u < units) {
                const uint32_t t = u / UW, ux = u - t * UW, n = t / CH, j = t - n * CH;
                const float* row = x + ((size_t)(n * H + (j << SY)) * W + ux * kVecW) * 3;
#pragma unroll
                for (int a = 0; a < ROWS; ++a)          // (a row past the last is the last: SY = 1 and an odd H)
                    tile[a][q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row + ((j << SY) + a < H ? (size_t)a * W * 3 : 0)) + part);
            }
        }
        __syncthreads();
        const uint32_t u = base + threadIdx.x;
        float f[ROWS][3 * kVecW];
#pragma unroll
        for (int a = 0; a < ROWS; ++a)
#pragma unroll
            for (int k = 0; k < kVecPieces; ++k) {
                const f32x4 v = tile[a][kVecPieces * threadIdx.x + k];
                f[a][4 * k] = v[0]; f[a][4 * k + 1] = v[1]; f[a][4 * k + 2] = v[2]; f[a][4 * k + 3] = v[3];
            }
        __syncthreads();                // (the next round's loads overwrite the tile)
        uint32_t luma[ROWS][kVecW], cu[NC], cv[NC];
        encode_unit<kVecW, SX, SY>(f, c, depth, luma, cu, cv);
        uint32_t traded = 0;
        if constexpr (NC * BPS == 2) {
            // units 2 m and 2 m + 1 lie in one chroma row (UW is even) and in one wave; both exist or neither (units is even)
            const uint32_t pu = cu[0] | cu[1] << 8, pv = cv[0] | cv[1] << 8;
            const uint32_t mine = (threadIdx.x & 1) ? pv : pu, theirs = (threadIdx.x & 1) ? pu : pv;
            const uint32_t got = (uint32_t)__shfl_xor((int)theirs, 1);
            traded = (threadIdx.x & 1) ? (got | mine << 16) : (mine | got << 16);
        }
        if (u < units) {
            const uint32_t t = u / UW, ux = u - t * UW, n = t / CH, j = t - n * CH;
            uint8_t* fr = yuv + (size_t)n * frame * BPS;
#pragma unroll
            for (int a = 0; a < ROWS; ++a)
                if ((j << SY) + a < H) store4<BPS>(fr + ((size_t)((j << SY) + a) * W + ux * kVecW) * BPS, luma[a]);
            if constexpr (NC * BPS == 2) {
                // even lane: U of units u, u + 1; odd lane: V of units u - 1, u -- four chroma bytes from column (ux & ~1) * 2 on
                uint8_t* co = fr + plane + ((threadIdx.x & 1) ? CH * CW : 0) + j * CW + (ux & ~1u) * NC;
                *reinterpret_cast<uint32_t*>(co) = traded;
            } else {
                uint8_t* uo = fr + ((size_t)plane + j * CW + ux * NC) * BPS;
                uint8_t* vo = uo + (size_t)CH * CW * BPS;
                if constexpr (NC == 4) {
                    store4<BPS>(uo, cu);
                    store4<BPS>(vo, cv);
                } else {                                // two 16-bit codes
                    *reinterpret_cast<uint32_t*>(uo) = cu[0] | cu[1] << 16;
                    *reinterpret_cast<uint32_t*>(vo) = cv[0] | cv[1] << 16;
                }
            }
        }
    }
}

// Any W, any float offset of x and any sample offset of yuv: a thread owns 8 pixels of each of the 1 << SY rows of a chroma row,
// reads them float by float with the edge replicated, and stores sample by sample.  UW = ceil(W / 8) units per chroma row.
template <int SX, int SY, int BPS>
__global__ __launch_bounds__(256) void unit_yuv_kernel(const float* __restrict__ x, void* __restrict__ yuv_, uint32_t H, uint32_t W, uint32_t UW,
                                                       uint32_t units, int depth, srx_yuv420_coeffs_t c) {
    typedef typename sample_of<BPS>::type T;
    constexpr int ROWS = 1 << SY, NC = kUnitW >> SX;
    T* yuv = static_cast<T*>(yuv_);
    const uint32_t CH = (H + SY) >> SY, CW = (W + SX) >> SX, plane = H * W, frame = plane + 2 * CH * CW;     // in samples
    for (uint32_t u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
        const uint32_t t = u / UW, ux = u - t * UW, n = t / CH, j = t - n * CH;
        const uint32_t x0 = ux * kUnitW, y0 = j << SY, rows = y0 + ROWS <= H ? ROWS : 1;
        float f[ROWS][3 * kUnitW];
#pragma unroll
        for (int a = 0; a < ROWS; ++a) {
            const float* row = x + ((size_t)(n * H + y0 + (a < (int)rows ? a : 0)) * W + x0) * 3;
#pragma unroll
            for (int i = 0; i < kUnitW; ++i) {
                const uint32_t px = min((uint32_t)i, W - 1 - x0);      // the edge replicated
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) f[a][3 * i + ch] = row[3 * px + ch];
            }
        }
        uint32_t luma[ROWS][kUnitW], cu[NC], cv[NC];
        encode_unit<kUnitW, SX, SY>(f, c, depth, luma, cu, cv);
        T* fr = yuv + (size_t)n * frame;
        T* yo = fr + (size_t)y0 * W + x0;
        T* uo = fr + plane + j * CW + (x0 >> SX);
        T* vo = uo + CH * CW;
#pragma unroll
        for (int i = 0; i < kUnitW; ++i)
            if (x0 + i < W) {
#pragma unroll
                for (int a = 0; a < ROWS; ++a)
                    if (a < (int)rows) yo[(size_t)a * W + i] = (T)luma[a][i];
            }
#pragma unroll
        for (int k = 0; k < NC; ++k)
            if ((x0 >> SX) + k < CW) {
                uo[k] = (T)cu[k];
                vo[k] = (T)cv[k];
            }
    }
}

// 0, or the refusal of a format
int check_format(const char* what, const srx_yuv_format_t* f) {
    if (f->depth != 8 && f->depth != 10 && f->depth != 12) return set_error(SRX_ERR_BAD_ARG, "%s: depth %d (8, 10 or 12)", what, f->depth);
    if (!((f->sub_x == 0 && f->sub_y == 0) || (f->sub_x == 1 && f->sub_y == 0) || (f->sub_x == 1 && f->sub_y == 1)))
        return set_error(SRX_ERR_BAD_ARG, "%s: subsampling (%d, %d) (4:4:4 is (0, 0), 4:2:2 (1, 0), 4:2:0 (1, 1))", what, f->sub_x, f->sub_y);
    if (f->reserved != 0) return set_error(SRX_ERR_BAD_ARG, "%s: the format's reserved field must be 0, got %d", what, f->reserved);
    return SRX_OK;
}

// 0 and the element count N H W 3 in *elems, or the refusal; the product is formed stepwise
int check_frames(const char* what, int N, int H, int W, const srx_yuv_format_t* f, const srx_yuv420_coeffs_t* c, long* elems) {
    if (!f || !c) return set_error(SRX_ERR_BAD_ARG, "null pointer");
    if (N <= 0 || H <= 0 || W <= 0) return set_error(SRX_ERR_BAD_ARG, "non-positive dimension");
    const int rc = check_format(what, f);
    if (rc != SRX_OK) return rc;
    const long rows = (long)N * H;
    if (rows >= (1L << 31) || rows * W * 3L >= (1L << 31)) return set_error(SRX_ERR_UNSUPPORTED, "%s: frames beyond 32-bit offsets", what);
    *elems = rows * W * 3L;
    return SRX_OK;
}

}  // namespace
}  // namespace srx

using namespace srx;

// every format but 8-bit 4:2:0, which espcn_yuv.hip's kernels serve: one instance of each kernel per (sub_x, sub_y, bytes per sample)
#define SRX_YUV_DISPATCH(f, LAUNCH)                                                          \
    do {                                                                                     \
        const int bps_ = (f)->depth > 8 ? 2 : 1;                                             \
        if ((f)->sub_x == 0 && bps_ == 1) { LAUNCH(0, 0, 1); }                               \
        else if ((f)->sub_x == 0) { LAUNCH(0, 0, 2); }                                       \
        else if ((f)->sub_y == 0 && bps_ == 1) { LAUNCH(1, 0, 1); }                          \
        else if ((f)->sub_y == 0) { LAUNCH(1, 0, 2); }                                       \
        else { LAUNCH(1, 1, 2); }                                                            \
    } while (0)

extern "C" size_t srx_yuv_frame_bytes(const srx_yuv_format_t* f, int H, int W) {
    if (!f) { set_error(SRX_ERR_BAD_ARG, "null pointer"); return 0; }
    if (H <= 0 || W <= 0) { set_error(SRX_ERR_BAD_ARG, "non-positive dimension"); return 0; }
    if (check_format("yuv_frame_bytes", f) != SRX_OK) return 0;
    const unsigned __int128 ch = ((unsigned long)H + f->sub_y) >> f->sub_y, cw = ((unsigned long)W + f->sub_x) >> f->sub_x;
    const unsigned __int128 bytes = ((unsigned __int128)H * W + 2 * ch * cw) * (f->depth > 8 ? 2 : 1);
    if (bytes > (unsigned __int128)SIZE_MAX) { set_error(SRX_ERR_UNSUPPORTED, "yuv_frame_bytes: a frame of %d x %d does not fit a size_t", H, W); return 0; }
    return (size_t)bytes;
}

extern "C" int srx_yuv_lut_float(const void* yuv, int N, int H, int W, const srx_yuv_format_t* f, const srx_yuv420_coeffs_t* c,
                                 const float* lut, float* out, srx_stream_t stream) {
    if (!yuv || !lut || !out) return set_error(SRX_ERR_BAD_ARG, "null pointer");
    long elems;
    const int rc = check_frames("yuv_lut_float", N, H, W, f, c, &elems);
    if (rc != SRX_OK) return rc;
    if ((uintptr_t)out & 3u) return set_error(SRX_ERR_ALIGN, "yuv_lut_float: out must be 4-byte aligned");
    if (f->depth > 8 && ((uintptr_t)yuv & 1u)) return set_error(SRX_ERR_ALIGN, "yuv_lut_float: yuv must be 2-byte aligned at depth %d", f->depth);
    if (f->depth == 8 && f->sub_x == 1 && f->sub_y == 1) return srx_yuv420_lut_float((const uint8_t*)yuv, N, H, W, c, lut, out, stream);
    const uint32_t pixels = (uint32_t)(elems / 3), blocks = (pixels + 255) / 256;
    const dim3 grid(blocks < kMaxBlocksDecode ? blocks : kMaxBlocksDecode);
#define LAUNCH(SX, SY, BPS)                                                                                                                 \
    hipLaunchKernelGGL((yuv_lut_float_kernel<SX, SY, BPS>), grid, dim3(256), 0, (hipStream_t)stream, yuv, lut, out, (uint32_t)H, (uint32_t)W, \
                       pixels, (int)f->depth, *c)
    SRX_YUV_DISPATCH(f, LAUNCH);
#undef LAUNCH
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(SRX_ERR_LAUNCH, "yuv_lut_float launch failed: %s", hipGetErrorString(e));
    return SRX_OK;
}

extern "C" int srx_unit_yuv(const float* x, int N, int H, int W, const srx_yuv_format_t* f, const srx_yuv420_coeffs_t* c, void* yuv,
                            srx_stream_t stream) {
    if (!x || !yuv) return set_error(SRX_ERR_BAD_ARG, "null pointer");
    long elems;
    const int rc = check_frames("unit_yuv", N, H, W, f, c, &elems);
    if (rc != SRX_OK) return rc;
    if ((uintptr_t)x & 3u) return set_error(SRX_ERR_ALIGN, "unit_yuv: x must be 4-byte aligned");
    if (f->depth > 8 && ((uintptr_t)yuv & 1u)) return set_error(SRX_ERR_ALIGN, "unit_yuv: yuv must be 2-byte aligned at depth %d", f->depth);
    if (f->depth == 8 && f->sub_x == 1 && f->sub_y == 1) return srx_unit_yuv420(x, N, H, W, c, (uint8_t*)yuv, stream);
    const bool vec = W % 8 == 0 && ((uintptr_t)x & 15u) == 0 && ((uintptr_t)yuv & 3u) == 0;
    const uint32_t UW = vec ? (uint32_t)W / kVecW : ((uint32_t)W + kUnitW - 1) / kUnitW;
    const uint32_t units = (uint32_t)N * (((uint32_t)H + f->sub_y) >> f->sub_y) * UW, blocks = (units + 255) / 256;
    const dim3 grid(blocks < kMaxBlocksEncode ? blocks : kMaxBlocksEncode);
#define LAUNCH_VEC(SX, SY, BPS)                                                                                                                      \
    hipLaunchKernelGGL((unit_yuv_vec_kernel<SX, SY, BPS>), grid, dim3(256), 0, (hipStream_t)stream, x, (uint8_t*)yuv, (uint32_t)H, (uint32_t)W, UW, \
                       units, (int)f->depth, *c)
#define LAUNCH_ANY(SX, SY, BPS)                                                                                                           \
    hipLaunchKernelGGL((unit_yuv_kernel<SX, SY, BPS>), grid, dim3(256), 0, (hipStream_t)stream, x, yuv, (uint32_t)H, (uint32_t)W, UW, units, \
                       (int)f->depth, *c)
    if (vec)
        SRX_YUV_DISPATCH(f, LAUNCH_VEC);
    else
        SRX_YUV_DISPATCH(f, LAUNCH_ANY);
#undef LAUNCH_VEC
#undef LAUNCH_ANY
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(SRX_ERR_LAUNCH, "unit_yuv launch failed: %s", hipGetErrorString(e));
    return SRX_OK;
}
