// summary_panel.hip -- the image panel of the reference's TensorBoard summaries, encoded on the GPU in one launch.
//
// All four trainers build the same picture: K float NHWC tensors of equal N and H side by side along the width, the batch
// stacked along the height, encoded to bytes (vdsr/vdsr/experiment_train.py:65-77, enet/enet/experiment_train.py:64-74,
// srcnn/srcnn.py:169-192, espcn/espcn/experiment_train.py:44-60).  ESPCN's sources are in its label layout [N,p,p,3r^2]:
// channel (dy*r + dx)*3 + ch of pixel (n, y, x) lands at panel row (n*p + y)*r + dy, column (W_before + x)*r + dx.
//
// Memory-bound: 12 bytes read and 3 written per panel pixel.  The panel is one flat, dense byte range whose rows
// (3 * r * sum(W) bytes: odd for 41-pixel patches) are not dword aligned, so the work is cut along the flat range and not
// along rows: a thread owns ALIGNED output dwords.  A workgroup (256 threads) owns 1024 consecutive dwords; thread t
// takes dwords t, t + 256, t + 512, t + 768 of them, so a wave's store instruction writes 256 contiguous bytes.  Per dword
// two divisions find panel row / column and image / row.  A dword that lies inside one source row (r = 1) is four
// consecutive floats: each of the four load instructions of a wave reads every fourth float of a contiguous 1 KiB run (the
// four together read all of it: every line is fetched once and served to the other three instructions from the L1).  A
// dword that crosses a source or row boundary, r > 1 and the ranged mode locate each byte on its own.  All 16 loads of a thread are
// issued before the first byte is encoded.  Only the first and the last dword of the whole panel can lie partly outside
// [out, out + size): those are written byte by byte, and no byte outside the range is read for or written.
//
// Ranged encoding (SRCNN hands tf.summary.image a FLOAT panel and TensorFlow 1.x rescales it): a first pass
// (srx_summary_panel_range) reduces min and max over the finite values -- a fixed grid, one partial pair per workgroup,
// then one workgroup folds them; min and max are exact in any order, so the result is deterministic -- and leaves
// {scale, offset} in device memory for the panel launch: no host round trip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/srx.h"
#include "u8_encode.h"

namespace srx {
int set_error(int code, const char* fmt, ...);

namespace {
constexpr int kMaxSrc = SRX_SUMMARY_PANEL_MAX_SRC;
constexpr int kDwordsPerThread = 4;
constexpr int kThreads = 256;
constexpr int kRangeBlocks = SRX_SUMMARY_RANGE_BLOCKS;

struct PanelArgs {
    const float* x[kMaxSrc];
    long long row_pitch[kMaxSrc];      // floats between rows of one image
    long long image_pitch[kMaxSrc];    // floats between images
    uint32_t cbeg[kMaxSrc + 1];        // first byte column of source s in a panel row: 3 * r * (W_0 + .. + W_{s-1})
    int n_src;
    int HR;                            // panel rows per image: H * r
    uint32_t row_bytes;                // 3 * r * sum(W)
    unsigned long long total;          // bytes of the panel
    unsigned mis;                      // out & 3: panel byte i sits at aligned byte i + mis
};

// the source a byte column belongs to (constant indices and selects: a lane-dependent index into the kernel arguments
// would send them through scratch; the loop ends at n_src, a uniform branch)
struct Source {
    const float* x;
    long long row_pitch, image_pitch;
    uint32_t cbeg, cend;
};
__device__ __forceinline__ Source source_of(const PanelArgs& a, uint32_t col) {
    Source s = {a.x[0], a.row_pitch[0], a.image_pitch[0], 0u, a.cbeg[1]};
#pragma unroll
    for (int k = 1; k < kMaxSrc; ++k) {
        if (k >= a.n_src) break;
        if (col >= a.cbeg[k]) s = {a.x[k], a.row_pitch[k], a.image_pitch[k], a.cbeg[k], a.cbeg[k + 1]};
    }
    return s;
}

// the float behind byte column `col` of panel row q of image n.  Ranged mode also reports the pixel: 0 wholly finite, else
// TensorFlow's bad colour (255, 0, 0) decides the byte -- 1 for the red channel, 2 for the other two
template <int R, bool RANGED>
__device__ __forceinline__ float fetch(const PanelArgs& a, uint32_t n, uint32_t q, uint32_t col, uint32_t* bad) {
    const Source s = source_of(a, col);
    const uint32_t lc = col - s.cbeg;
    const uint32_t y = q / R, dy = q - y * R;
    const uint32_t px = lc / 3u, ch = lc - 3u * px;
    const uint32_t x = px / R, dx = px - x * R;
    const float* p = s.x + ((long long)n * s.image_pitch + (long long)y * s.row_pitch + (long long)x * (3 * R * R) + (dy * R + dx) * 3);
    if (RANGED) *bad = (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) ? 0u : (ch == 0 ? 1u : 2u);
    return p[ch];
}

template <int R, bool RANGED, typename idx_t>
__global__ __launch_bounds__(kThreads) void summary_panel_kernel(PanelArgs a, const float* __restrict__ range, uint8_t* __restrict__ out) {
    const unsigned long long d0 = (unsigned long long)blockIdx.x * (kThreads * kDwordsPerThread) + threadIdx.x;
    float v[kDwordsPerThread][4];
    uint32_t bad[kDwordsPerThread][4];
#pragma unroll
    for (int j = 0; j < kDwordsPerThread; ++j) {
        // aligned byte 4d is panel byte 4d - mis: the panel's first dword may begin before it, its last may end after it
        const long long i0 = (long long)((d0 + (unsigned long long)j * kThreads) * 4) - a.mis;
        const long long is = i0 < 0 ? 0 : i0;                              // the dword's first byte inside the panel
        // two divisions per dword: panel row and column, then image and row within the image
        const uint32_t row = (uint32_t)((idx_t)is / (idx_t)a.row_bytes);
        const uint32_t col = (uint32_t)((idx_t)is - (idx_t)row * (idx_t)a.row_bytes);
        const uint32_t n = row / (uint32_t)a.HR, q = row - n * (uint32_t)a.HR;
#pragma unroll
        for (int b = 0; b < 4; ++b) { v[j][b] = 0.f; bad[j][b] = 0u; }
        const Source s = source_of(a, col);
        if (R == 1 && !RANGED && i0 >= 0 && (unsigned long long)(i0 + 4) <= a.total && col + 3 < s.cend) {
            // the common case: the dword lies inside one source row, its bytes are four consecutive floats
            const float* p = s.x + ((long long)n * s.image_pitch + (long long)q * s.row_pitch + (col - s.cbeg));
#pragma unroll
            for (int b = 0; b < 4; ++b) v[j][b] = p[b];
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long long i = i0 + b;
                if (i >= 0 && (unsigned long long)i < a.total) {
                    uint32_t nn = n, qq = q, c = col + (uint32_t)(i - is);
                    if (c >= a.row_bytes) {                                // (a row has >= 3 bytes and c < row_bytes + 3: once)
                        c -= a.row_bytes;
                        if (++qq == (uint32_t)a.HR) { qq = 0; ++nn; }
                    }
                    v[j][b] = fetch<R, RANGED>(a, nn, qq, c, &bad[j][b]);
                }
            }
        }
    }
    float scale = 0.f, offset = 0.f;
    if (RANGED) { scale = range[0]; offset = range[1]; }
#pragma unroll
    for (int j = 0; j < kDwordsPerThread; ++j) {
        const long long i0 = (long long)((d0 + (unsigned long long)j * kThreads) * 4) - a.mis;
        uint32_t byte[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (RANGED) {
#pragma clang fp contract(off)
                float w = v[j][b] * scale;
                w = w + offset;
                byte[b] = bad[j][b] ? (bad[j][b] == 1u ? 255u : 0u) : (uint32_t)(uint8_t)w;
            } else {
                byte[b] = encode_u8(v[j][b]);
            }
        }
        if (i0 >= 0 && (unsigned long long)(i0 + 4) <= a.total) {
            *reinterpret_cast<uint32_t*>(out + i0) = byte[0] | (byte[1] << 8) | (byte[2] << 16) | (byte[3] << 24);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (i0 + b >= 0 && (unsigned long long)(i0 + b) < a.total) out[i0 + b] = (uint8_t)byte[b];
        }
    }
}

// one partial {min, max} pair per workgroup over the finite values; a workgroup walks (source, image row) pairs
__global__ __launch_bounds__(kThreads) void summary_range_partials_kernel(PanelArgs a, int N, int H, int r, float* __restrict__ partials) {
    float lo = INFINITY, hi = -INFINITY;
    const unsigned long long rows = (unsigned long long)N * H;
    for (int s = 0; s < a.n_src; ++s) {
        const uint32_t len = (a.cbeg[s + 1] - a.cbeg[s]) * (uint32_t)r;      // W_s * 3r^2 floats in a source row
        for (unsigned long long q = blockIdx.x; q < rows; q += gridDim.x) {
            const unsigned long long n = q / (unsigned)H, y = q - n * (unsigned)H;
            const float* p = a.x[s] + ((long long)n * a.image_pitch[s] + (long long)y * a.row_pitch[s]);
            for (uint32_t k = threadIdx.x; k < len; k += kThreads) {
                const float f = p[k];
                if (isfinite(f)) { lo = fminf(lo, f); hi = fmaxf(hi, f); }
            }
        }
    }
    __shared__ float slo[kThreads], shi[kThreads];
    slo[threadIdx.x] = lo; shi[threadIdx.x] = hi;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            slo[threadIdx.x] = fminf(slo[threadIdx.x], slo[threadIdx.x + w]);
            shi[threadIdx.x] = fmaxf(shi[threadIdx.x], shi[threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = slo[0]; partials[2 * blockIdx.x + 1] = shi[0]; }
}

// folds the partials and applies TensorFlow 1.x's rule for float images (tf.summary.image on a float tensor)
__global__ __launch_bounds__(kRangeBlocks) void summary_range_finish_kernel(float* __restrict__ range) {
    __shared__ float slo[kRangeBlocks], shi[kRangeBlocks];
    const float* partials = range + 2;
    slo[threadIdx.x] = partials[2 * threadIdx.x]; shi[threadIdx.x] = partials[2 * threadIdx.x + 1];
    __syncthreads();
    for (int w = kRangeBlocks / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            slo[threadIdx.x] = fminf(slo[threadIdx.x], slo[threadIdx.x + w]);
            shi[threadIdx.x] = fmaxf(shi[threadIdx.x], shi[threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float lo = slo[0], hi = shi[0];
        float scale, offset;
        if (lo < 0.f) {
            const float m = fmaxf(fabsf(lo), fabsf(hi));
            scale = m < 1e-6f ? 0.f : 127.f / m;
            offset = 128.f;
        } else {
            scale = hi < 1e-6f ? 0.f : 255.f / hi;
            offset = 0.f;
        }
        range[0] = scale; range[1] = offset;
    }
}

// argument checks shared by the entry points; fills `a`.  out / out_bytes: the range no source may overlap (out_bytes 0:
// the panel's own size)
int fill_args(const char* who, const srx_panel_src* srcs, int n_src, int N, int H, int r, const void* out, size_t out_bytes, PanelArgs* a) {
    if (!srcs) return set_error(SRX_ERR_BAD_ARG, "%s: null pointer", who);
    if (n_src < 1 || n_src > kMaxSrc) return set_error(SRX_ERR_BAD_ARG, "%s: n_src %d outside 1..%d", who, n_src, kMaxSrc);
    if (r < 1 || r > 4) return set_error(SRX_ERR_BAD_ARG, "%s: r %d outside 1..4", who, r);
    if (N <= 0 || H <= 0) return set_error(SRX_ERR_BAD_ARG, "%s: bad dims N %d H %d", who, N, H);
    if ((long long)N * H * r > 0x7fffffffLL) return set_error(SRX_ERR_BAD_ARG, "%s: N*H*r = %lld panel rows exceed 2^31", who, (long long)N * H * r);
    const long long C = 3LL * r * r;
    long long sumW = 0;
    for (int s = 0; s < kMaxSrc; ++s) { a->x[s] = nullptr; a->row_pitch[s] = a->image_pitch[s] = 0; }
    for (int s = 0; s < n_src; ++s) {
        if (!srcs[s].x) return set_error(SRX_ERR_BAD_ARG, "%s: null pointer (source %d)", who, s);
        if ((uintptr_t)srcs[s].x & 3) return set_error(SRX_ERR_ALIGN, "%s: source %d is not 4-byte aligned", who, s);
        if (srcs[s].W <= 0) return set_error(SRX_ERR_BAD_ARG, "%s: bad dims: source %d has W %d", who, s, srcs[s].W);
        const long long rowlen = srcs[s].W * C;
        const long long rp = srcs[s].row_pitch ? srcs[s].row_pitch : rowlen;
        const long long ip = srcs[s].image_pitch ? srcs[s].image_pitch : rp * H;
        if (rp < rowlen || ip < (H - 1) * rp + rowlen)
            return set_error(SRX_ERR_BAD_ARG, "%s: source %d: row pitch %lld / image pitch %lld shorter than a row of %lld floats / an image", who, s, rp, ip, rowlen);
        a->x[s] = srcs[s].x; a->row_pitch[s] = rp; a->image_pitch[s] = ip;
        a->cbeg[s] = (uint32_t)(3 * r * sumW);
        sumW += srcs[s].W;
        if (sumW * C > 0x7fffffffLL) return set_error(SRX_ERR_BAD_ARG, "%s: a panel row of %lld floats exceeds 2^31", who, sumW * C);
    }
    for (int s = n_src; s <= kMaxSrc; ++s) a->cbeg[s] = (uint32_t)(3 * r * sumW);
    a->n_src = n_src;
    a->HR = H * r;
    a->row_bytes = (uint32_t)(3 * r * sumW);
    a->total = (unsigned long long)N * H * r * a->row_bytes;
    a->mis = 0;
    if (out) {
        const uintptr_t oa = (uintptr_t)out;
        const size_t ob = out_bytes ? out_bytes : (size_t)a->total;
        for (int s = 0; s < n_src; ++s) {
            const uintptr_t xa = (uintptr_t)srcs[s].x;
            const size_t extent = (size_t)((N - 1) * a->image_pitch[s] + (H - 1) * a->row_pitch[s] + srcs[s].W * C) * sizeof(float);
            if (xa < oa + ob && oa < xa + extent) return set_error(SRX_ERR_BAD_ARG, "%s: out overlaps source %d", who, s);
        }
    }
    return SRX_OK;
}

template <int R, bool RANGED>
void launch_panel(const PanelArgs& a, const float* range, uint8_t* out, unsigned blocks, hipStream_t stream) {
    if (a.total + 8 < 0xffffffffull)
        hipLaunchKernelGGL((summary_panel_kernel<R, RANGED, uint32_t>), dim3(blocks), dim3(kThreads), 0, stream, a, range, out);
    else
        hipLaunchKernelGGL((summary_panel_kernel<R, RANGED, unsigned long long>), dim3(blocks), dim3(kThreads), 0, stream, a, range, out);
}

template <int R>
void launch_panel_r(const PanelArgs& a, const float* range, uint8_t* out, unsigned blocks, hipStream_t stream) {
    if (range) launch_panel<R, true>(a, range, out, blocks, stream);
    else launch_panel<R, false>(a, range, out, blocks, stream);
}

}  // namespace
}  // namespace srx

using namespace srx;

extern "C" size_t srx_summary_panel_bytes(const srx_panel_src* srcs, int n_src, int N, int H, int r) {
    PanelArgs a;
    if (fill_args("summary_panel_bytes", srcs, n_src, N, H, r, nullptr, 0, &a) != SRX_OK) return 0;
    return (size_t)a.total;
}

extern "C" size_t srx_summary_panel_range_bytes(void) { return (size_t)(2 + 2 * kRangeBlocks) * sizeof(float); }

extern "C" int srx_summary_panel_u8(const srx_panel_src* srcs, int n_src, int N, int H, int r, const float* range_dev, uint8_t* out,
                                    srx_stream_t stream) {
    if (!srcs || !out) return set_error(SRX_ERR_BAD_ARG, "summary_panel_u8: null pointer");
    PanelArgs a;
    const int rc = fill_args("summary_panel_u8", srcs, n_src, N, H, r, out, 0, &a);
    if (rc != SRX_OK) return rc;
    if (range_dev && ((uintptr_t)range_dev & 3)) return set_error(SRX_ERR_ALIGN, "summary_panel_u8: range_dev is not 4-byte aligned");
    a.mis = (unsigned)((uintptr_t)out & 3);
    const unsigned long long dwords = (a.total + a.mis + 3) / 4;
    const unsigned long long blocks = (dwords + kThreads * kDwordsPerThread - 1) / (kThreads * kDwordsPerThread);
    if (blocks > 0x7fffffffull) return set_error(SRX_ERR_BAD_ARG, "summary_panel_u8: %llu workgroups exceed the grid limit", blocks);
    hipStream_t st = (hipStream_t)stream;
    switch (r) {
        case 1: launch_panel_r<1>(a, range_dev, out, (unsigned)blocks, st); break;
        case 2: launch_panel_r<2>(a, range_dev, out, (unsigned)blocks, st); break;
        case 3: launch_panel_r<3>(a, range_dev, out, (unsigned)blocks, st); break;
        default: launch_panel_r<4>(a, range_dev, out, (unsigned)blocks, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(SRX_ERR_LAUNCH, "summary_panel_u8 launch failed: %s", hipGetErrorString(e));
    return SRX_OK;
}

extern "C" int srx_summary_panel_range(const srx_panel_src* srcs, int n_src, int N, int H, int r, float* range_dev, srx_stream_t stream) {
    if (!srcs || !range_dev) return set_error(SRX_ERR_BAD_ARG, "summary_panel_range: null pointer");
    PanelArgs a;
    const int rc = fill_args("summary_panel_range", srcs, n_src, N, H, r, range_dev, srx_summary_panel_range_bytes(), &a);
    if (rc != SRX_OK) return rc;
    if ((uintptr_t)range_dev & 3) return set_error(SRX_ERR_ALIGN, "summary_panel_range: range_dev is not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(summary_range_partials_kernel, dim3(kRangeBlocks), dim3(kThreads), 0, st, a, N, H, r, range_dev + 2);
    hipLaunchKernelGGL(summary_range_finish_kernel, dim3(1), dim3(kRangeBlocks), 0, st, range_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(SRX_ERR_LAUNCH, "summary_panel_range launch failed: %s", hipGetErrorString(e));
    return SRX_OK;
}
