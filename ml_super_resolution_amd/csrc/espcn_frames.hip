// espcn_frames.hip -- the two streaming passes of ESPCN's bytes-in, bytes-out inference for frames above the one-launch
// window (espcn/espcn/experiment_test.py:148-184): decode the LR bytes through the caller's table before the three
// convolution launches, encode the HR floats to bytes after them.  Below the window srx_espcn_forward_u8 does both inside
// its one launch (espcn_fused.hip).
//
//   srx_u8_lut_float  out[i] = lut[in[i]].  The table is the caller's, so the floats are whatever the host route feeds:
//                     `(bytes / 127.5 - 1.0).astype(float32)` is float64 arithmetic and one cast, which the fp32
//                     `(float)b / 127.5f - 1.0f` of u8_to_pm1_kernel is not guaranteed to reproduce.  LR-sized: n bytes read,
//                     4 n written; the table sits in LDS (one load per entry per workgroup).
//   srx_unit_u8       out[i] = encode_unit_u8(x[i]) (u8_encode.h).  HR-sized: 4 n bytes read, n written -- bound by the
//                     read.  Interior: 16-byte nontemporal loads, four of them in flight per thread, one packed 4-byte store
//                     each; the up to three elements before the first 16-byte boundary of x and after the last whole group
//                     are stored byte by byte, and so is everything when no element index aligns x to 16 and out to 4 at
//                     once.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>

#include "../../include/srx.h"
#include "u8_encode.h"

namespace srx {
int set_error(int code, const char* fmt, ...);

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void u8_lut_float_kernel(const uint8_t* __restrict__ in, const float* __restrict__ lut,
                                                           float* __restrict__ out, size_t n) {
    __shared__ float table[256];
    table[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = table[in[i]];
}

constexpr int kInFlight = 4;        // 16-byte loads a thread issues before its first store

// x + head is 16-byte aligned and out + head 4-byte aligned; groups = (n - head) / 4 whole groups of four elements follow.
__global__ __launch_bounds__(256) void unit_u8_vec_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, size_t n,
                                                          int head, size_t groups) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x + head);
    uint32_t* o4 = reinterpret_cast<uint32_t*>(out + head);
    const size_t per = (size_t)kInFlight * 256;
    for (size_t base = (size_t)blockIdx.x * per; base < groups; base += (size_t)gridDim.x * per) {
        f32x4 v[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const size_t g = base + (size_t)k * 256 + threadIdx.x;
            if (g < groups) v[k] = __builtin_nontemporal_load(x4 + g);
        }
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const size_t g = base + (size_t)k * 256 + threadIdx.x;
            if (g < groups)
                o4[g] = encode_unit_u8(v[k][0]) | encode_unit_u8(v[k][1]) << 8 | encode_unit_u8(v[k][2]) << 16 | encode_unit_u8(v[k][3]) << 24;
        }
    }
    if (blockIdx.x == 0) {          // head: elements 0 .. head - 1; tail: the < 4 elements behind the last whole group
        const size_t tail0 = (size_t)head + 4 * groups;
        if ((int)threadIdx.x < head) out[threadIdx.x] = (uint8_t)encode_unit_u8(x[threadIdx.x]);
        else if (threadIdx.x >= 64 && tail0 + (threadIdx.x - 64) < n) out[tail0 + (threadIdx.x - 64)] = (uint8_t)encode_unit_u8(x[tail0 + (threadIdx.x - 64)]);
    }
}

__global__ __launch_bounds__(256) void unit_u8_scalar_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (uint8_t)encode_unit_u8(x[i]);
}

}  // namespace
}  // namespace srx

using namespace srx;

extern "C" int srx_u8_lut_float(const uint8_t* in, const float* lut, float* out, size_t n, srx_stream_t stream) {
    if (!in || !lut || !out) return set_error(SRX_ERR_BAD_ARG, "null pointer");
    if ((uintptr_t)out & 3u) return set_error(SRX_ERR_ALIGN, "u8_lut_float: out must be 4-byte aligned");
    if (n == 0) return SRX_OK;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(u8_lut_float_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, in, lut, out, n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(SRX_ERR_LAUNCH, "u8_lut_float launch failed: %s", hipGetErrorString(e));
    return SRX_OK;
}

extern "C" int srx_unit_u8(const float* x, uint8_t* out, size_t n, srx_stream_t stream) {
    if (!x || !out) return set_error(SRX_ERR_BAD_ARG, "null pointer");
    if ((uintptr_t)x & 3u) return set_error(SRX_ERR_ALIGN, "unit_u8: x must be 4-byte aligned");
    if (n == 0) return SRX_OK;
    // the first element index that aligns x to 16 bytes; the vector path needs it to align out to 4 bytes as well
    const int head = (int)(((16u - ((uintptr_t)x & 15u)) & 15u) >> 2);
    if ((((uintptr_t)out + head) & 3u) == 0 && n >= (size_t)head + 4) {
        const size_t groups = (n - head) / 4, per = (size_t)kInFlight * 256;
        const size_t blocks = (groups + per - 1) / per;
        hipLaunchKernelGGL(unit_u8_vec_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, x, out, n,
                           head, groups);
    } else {
        const size_t blocks = (n + 255) / 256;
        hipLaunchKernelGGL(unit_u8_scalar_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, x, out, n);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(SRX_ERR_LAUNCH, "unit_u8 launch failed: %s", hipGetErrorString(e));
    return SRX_OK;
}
