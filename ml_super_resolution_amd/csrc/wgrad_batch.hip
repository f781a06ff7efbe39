// Conv2DBackpropFilter of several 3x3 64 -> 64 layers of one shape (41-pixel rows: VDSR's body) in ONE launch, layer-major
// (wgrad_rows_batch_kernel), and ONE reduction of all the layers' partial filters.  See DESIGN.md, 3.12.
#include "launchers.h"
namespace srx {

// blockIdx.y = layer; its partials are slots layer * wpl .. layer * wpl + wpl - 1 of `part`.  Every thread owns four
// consecutive outputs and adds the wpl partials in index order g = 0, 1, ... (loads eight at a time, additions in order):
//   j <  wn : dw[layer][j]       = sum_g part[layer * wpl + g][j] (+ wd * w[layer][j])
//   j >= wn : dbias[layer][j-wn] = sum_g part[layer * wpl + g][j]
__global__ __launch_bounds__(256) void wgrad_batch_reduce_kernel(const float* __restrict__ part, const int wpl, const int stride,
                                                                 const int wn, const int n, const WgradBatchOut o, const float wd) {
    const int layer = blockIdx.y;
    const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (j >= n) return;
    const float* p = part + (size_t)layer * wpl * stride + j;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    int g = 0;
    for (; g + 8 <= wpl; g += 8) {
        f32x4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f32x4*>(p + (size_t)(g + i) * stride);
#pragma unroll
        for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; g < wpl; ++g) s += *reinterpret_cast<const f32x4*>(p + (size_t)g * stride);
    float* __restrict__ dw = o.dw[layer];
    float* __restrict__ dbias = o.dbias[layer];
    const float* __restrict__ w = o.w[layer];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int jj = j + e;
        if (jj < wn)
            dw[jj] = s[e] + (w ? wd * w[jj] : 0.f);
        else if (jj < n && dbias)
            dbias[jj - wn] = s[e];
    }
}

hipError_t launch_wgrad_rows_batch(const WgradArgs& a, const WgradBatchPtrs& c, int wpl, int layers, size_t lds, hipStream_t s) {
    return launch_with_lds<wgrad_rows_batch_kernel<3, 3, 64, 4, 41>>(dim3((unsigned)(wpl * layers)), dim3(256), lds, s, a, c, wpl);
}

hipError_t launch_wgrad_batch_reduce(const float* part, int wpl, int layers, int stride, int wn, int cout, const WgradBatchOut& o,
                                     float wd, hipStream_t s) {
    const int n = wn + cout;   // stride is a multiple of 4 >= n, so the float4 loads stay in the row
    hipLaunchKernelGGL(wgrad_batch_reduce_kernel, dim3((unsigned)((n + 1023) / 1024), (unsigned)layers), dim3(256), 0, s, part, wpl,
                       stride, wn, n, o, wd);
    return hipGetLastError();
}
}  // namespace srx
