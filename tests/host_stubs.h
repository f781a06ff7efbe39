// Stubs (CPU only) for the drivers that link a --cuda-host-only build of srx_api.hip: tsan_abi_driver.cpp and
// route_trace_driver.cpp.  Every kernel launcher of the other translation units and the five HIP runtime calls
// srx_api.hip makes are defined here (the latter take precedence over libamdhip64's, which is never started), so the
// programs run the same on any machine.  What a stub DOES when called is the including driver's: it defines
//     bool       srx_stub::offer(const Call&, hipError_t* err)  the launchers that answer "is this shape mine?"
//     hipError_t srx_stub::call(const Call&)                    the launchers that only report a launch status
//     int        srx_stub::cu_count()                           hipDeviceAttributeMultiprocessorCount
// Define SRX_STUB_WEAK_LAUNCHERS before including to get the weak launchers (chains, batched filter gradients, bf16x3)
// as well; without them srx_api.hip refuses those entry points.  Neither driver calls a pair builder's entry point, so
// neither links pairs_api.hip, whose host-only build has a driver of its own (enet_eval_host_driver.cpp) and needs no stub.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../include/srx.h"
#include "../ml_super_resolution_amd/csrc/elementwise.h"
#include "../ml_super_resolution_amd/csrc/launchers.h"
#include "../ml_super_resolution_amd/csrc/bf16x3.h"

namespace srx_stub {

#define SRX_STUB_IDS(X)                                                                                                  \
    X(conv_narrow) X(conv_kwrows) X(conv_pack3) X(conv_1x1) X(pipe_strip) X(pipe_k3c64) X(pipe_other) X(conv_rows3x3)    \
    X(conv_k3c64) X(conv_k3c32) X(conv_c4) X(conv_misc) X(conv_generic)                                                  \
    X(wgrad_1x1) X(wgrad_kwcols) X(wgrad_rows_full) X(wgrad_pipe) X(wgrad_narrow) X(wgrad_rows_strip) X(wgrad_lin_pack3) \
    X(wgrad_lin_strip) X(wgrad_lin) X(wgrad) X(wgrad_generic) X(wgrad_lin_pairs)                                         \
    X(conv_chain) X(wgrad_rows_batch) X(wgrad_batch_reduce) X(conv3x3c64_bf16x3) X(wgrad3x3c64_bf16x3)                   \
    X(wgrad3x3c64_bf16x3_pairs) X(reduce_partials) X(reduce_partials_pairs) X(elementwise)
enum Id {
#define X(n) k_##n,
    SRX_STUB_IDS(X)
#undef X
    kIds
};
constexpr int kOffered = k_wgrad_lin_pairs + 1;   // the ids below it go through offer(), the rest through call()
inline const char* name(int id) {
    static const char* const names[] = {
#define X(n) "launch_" #n,
        SRX_STUB_IDS(X)
#undef X
    };
    return names[id];
}

// One call of a launcher: whichever of the argument structs it was given, and its extra arguments (-1: has none).
struct Call {
    Id id;
    const srx::ConvKey* key = nullptr;
    const srx::ConvArgs* conv = nullptr;
    const srx::WgradArgs* wgrad = nullptr;
    const srx::WgradPairs* pairs_args = nullptr;
    const srx::ChainPtrs* chain = nullptr;
    const srx::WgradBatchPtrs* batch = nullptr;
    const srx::WgradBatchOut* batch_out = nullptr;
    const srx::Bf3Plan* bf3 = nullptr;
    long grid = -1, lds = -1, min_pixels = -1, max_partials = -1;
    int wt = -1, aux = -1, fixed = -1, wpl = -1, layers = -1, G = -1, pairs = -1, strips = -1, stride = -1, wn = -1, cout = -1, cob = -1;
    int* n_partials = nullptr;      // launch_wgrad_1x1 / launch_wgrad_kwcols: the stub's own partial count goes here
    const void* ptr[8] = {};        // the launchers with bare pointer arguments (bf16x3, reductions), in argument order
    int n_ptr = 0;
    float wd = 0.f;
    int dims[4] = {-1, -1, -1, -1}; // N, H, W (bf16x3 launchers), relu
};

bool offer(const Call& c, hipError_t* err);
hipError_t call(const Call& c);
int cu_count();

}  // namespace srx_stub

namespace srx {
using srx_stub::Call;
#define STUB_CONV(n)                                                                                           \
    bool launch_##n(const ConvKey& k, const ConvArgs& a, int grid, size_t lds, hipStream_t, hipError_t* err) {  \
        Call c; c.id = srx_stub::k_##n; c.key = &k; c.conv = &a; c.grid = grid; c.lds = (long)lds;             \
        return srx_stub::offer(c, err);                                                                        \
    }
STUB_CONV(conv_k3c64) STUB_CONV(conv_k3c32) STUB_CONV(conv_c4) STUB_CONV(conv_misc)
STUB_CONV(pipe_k3c64) STUB_CONV(pipe_other) STUB_CONV(pipe_strip) STUB_CONV(conv_generic)
#define STUB_CONV_MINPX(n)                                                                                     \
    bool launch_##n(const ConvKey& k, const ConvArgs& a, long min_pixels, hipStream_t, hipError_t* err) {      \
        Call c; c.id = srx_stub::k_##n; c.key = &k; c.conv = &a; c.min_pixels = min_pixels;                    \
        return srx_stub::offer(c, err);                                                                        \
    }
STUB_CONV_MINPX(conv_rows3x3) STUB_CONV_MINPX(conv_1x1) STUB_CONV_MINPX(conv_pack3) STUB_CONV_MINPX(conv_kwrows)
bool launch_conv_narrow(const ConvKey& k, const ConvArgs& a, hipStream_t, hipError_t* err) {
    Call c; c.id = srx_stub::k_conv_narrow; c.key = &k; c.conv = &a;
    return srx_stub::offer(c, err);
}
#define STUB_WGRAD(n)                                                                                          \
    bool launch_##n(const ConvKey& k, const WgradArgs& a, int grid, size_t lds, hipStream_t, hipError_t* err) { \
        Call c; c.id = srx_stub::k_##n; c.key = &k; c.wgrad = &a; c.grid = grid; c.lds = (long)lds;            \
        return srx_stub::offer(c, err);                                                                        \
    }
STUB_WGRAD(wgrad) STUB_WGRAD(wgrad_lin) STUB_WGRAD(wgrad_lin_strip) STUB_WGRAD(wgrad_lin_pack3) STUB_WGRAD(wgrad_generic)
STUB_WGRAD(wgrad_pipe) STUB_WGRAD(wgrad_rows_full) STUB_WGRAD(wgrad_rows_strip)
bool launch_wgrad_narrow(const ConvKey& k, const WgradArgs& a, int grid, hipStream_t, hipError_t* err) {
    Call c; c.id = srx_stub::k_wgrad_narrow; c.key = &k; c.wgrad = &a; c.grid = grid;
    return srx_stub::offer(c, err);
}
bool launch_wgrad_kwcols(const ConvKey& k, const WgradArgs& a, int max_partials, long min_pixels, int* n, hipStream_t, hipError_t* err) {
    Call c; c.id = srx_stub::k_wgrad_kwcols; c.key = &k; c.wgrad = &a; c.max_partials = max_partials; c.min_pixels = min_pixels; c.n_partials = n;
    return srx_stub::offer(c, err);
}
bool launch_wgrad_1x1(const ConvKey& k, const WgradArgs& a, int max_partials, int* n, hipStream_t, hipError_t* err) {
    Call c; c.id = srx_stub::k_wgrad_1x1; c.key = &k; c.wgrad = &a; c.max_partials = max_partials; c.n_partials = n;
    return srx_stub::offer(c, err);
}
bool launch_wgrad_lin_pairs(const ConvKey& k, const WgradPairs& q, int grid, int pairs, bool strips, size_t lds, hipStream_t, hipError_t* err) {
    Call c; c.id = srx_stub::k_wgrad_lin_pairs; c.key = &k; c.pairs_args = &q; c.wgrad = &q.a; c.G = grid; c.pairs = pairs; c.strips = strips; c.lds = (long)lds;
    return srx_stub::offer(c, err);
}
hipError_t launch_reduce_partials(const float* part, int G, int stride, int wn, int cout, float* dw, float* dbias, const float* w, float wd, hipStream_t) {
    Call c; c.id = srx_stub::k_reduce_partials; c.G = G; c.stride = stride; c.wn = wn; c.cout = cout; c.wd = wd;
    c.ptr[0] = part; c.ptr[1] = dw; c.ptr[2] = dbias; c.ptr[3] = w; c.n_ptr = 4;
    return srx_stub::call(c);
}
hipError_t launch_reduce_partials_pairs(const float* part, int G, int stride, int wn, int cout, float* dw, float* dbias, int pairs, int cob, hipStream_t) {
    Call c; c.id = srx_stub::k_reduce_partials_pairs; c.G = G; c.stride = stride; c.wn = wn; c.cout = cout; c.pairs = pairs; c.cob = cob;
    c.ptr[0] = part; c.ptr[1] = dw; c.ptr[2] = dbias; c.n_ptr = 3;
    return srx_stub::call(c);
}
#ifdef SRX_STUB_WEAK_LAUNCHERS
hipError_t launch_conv_chain(bool wt, bool aux, bool fixed, const ConvArgs& a, const ChainPtrs& p, int grid, size_t lds, hipStream_t) {
    Call c; c.id = srx_stub::k_conv_chain; c.conv = &a; c.chain = &p; c.wt = wt; c.aux = aux; c.fixed = fixed; c.grid = grid; c.lds = (long)lds;
    return srx_stub::call(c);
}
hipError_t launch_wgrad_rows_batch(const WgradArgs& a, const WgradBatchPtrs& p, int wpl, int layers, size_t lds, hipStream_t) {
    Call c; c.id = srx_stub::k_wgrad_rows_batch; c.wgrad = &a; c.batch = &p; c.wpl = wpl; c.layers = layers; c.lds = (long)lds;
    return srx_stub::call(c);
}
hipError_t launch_wgrad_batch_reduce(const float* part, int wpl, int layers, int stride, int wn, int cout, const WgradBatchOut& o, float wd, hipStream_t) {
    Call c; c.id = srx_stub::k_wgrad_batch_reduce; c.batch_out = &o; c.wpl = wpl; c.layers = layers; c.stride = stride; c.wn = wn; c.cout = cout; c.wd = wd;
    c.ptr[0] = part; c.n_ptr = 1;
    return srx_stub::call(c);
}
hipError_t launch_conv3x3c64_bf16x3(bool dgrad, const float* x, const float* w, const float* bias, const float* mask, bool relu, float* y,
                                    int N, int H, int W, const Bf3Plan& p, hipStream_t) {
    Call c; c.id = srx_stub::k_conv3x3c64_bf16x3; c.bf3 = &p; c.wt = dgrad; c.dims[0] = N; c.dims[1] = H; c.dims[2] = W; c.dims[3] = relu;
    c.ptr[0] = x; c.ptr[1] = w; c.ptr[2] = bias; c.ptr[3] = mask; c.ptr[4] = y; c.n_ptr = 5;
    return srx_stub::call(c);
}
hipError_t launch_wgrad3x3c64_bf16x3(const float* x, const float* dpre, float* part, int part_stride, int N, int H, int W, const Bf3Plan& p, hipStream_t) {
    Call c; c.id = srx_stub::k_wgrad3x3c64_bf16x3; c.bf3 = &p; c.stride = part_stride; c.dims[0] = N; c.dims[1] = H; c.dims[2] = W;
    c.ptr[0] = x; c.ptr[1] = dpre; c.ptr[2] = part; c.n_ptr = 3;
    return srx_stub::call(c);
}
hipError_t launch_wgrad3x3c64_bf16x3_pairs(const float* x, const float* dpre, float* part, int part_stride, int cib, int cob, int N, int H, int W,
                                           const Bf3Plan& p, hipStream_t) {
    Call c; c.id = srx_stub::k_wgrad3x3c64_bf16x3_pairs; c.bf3 = &p; c.stride = part_stride; c.pairs = cib; c.cob = cob; c.dims[0] = N; c.dims[1] = H; c.dims[2] = W;
    c.ptr[0] = x; c.ptr[1] = dpre; c.ptr[2] = part; c.n_ptr = 3;
    return srx_stub::call(c);
}
#endif

// the element-wise launchers: no route depends on them
inline hipError_t stub_elementwise() { Call c; c.id = srx_stub::k_elementwise; return srx_stub::call(c); }
hipError_t launch_subpixel(const float*, float*, int, int, int, int, int, bool, int, hipStream_t) { return stub_elementwise(); }
hipError_t launch_stream_copy(const float*, float*, size_t, hipStream_t) { return stub_elementwise(); }
hipError_t launch_mse(const float*, const float*, size_t, float, float*, int, float*, float*, hipStream_t) { return stub_elementwise(); }
hipError_t launch_l2(const float*, const float*, size_t, float, float*, int, float*, hipStream_t) { return stub_elementwise(); }
hipError_t launch_adam(float*, const float*, float*, float*, size_t, float, float, float, float, float, hipStream_t) { return stub_elementwise(); }
hipError_t launch_adam_dev(float*, const float*, float*, float*, size_t, void*, float, float, float, float, hipStream_t) { return stub_elementwise(); }
hipError_t launch_momentum(float*, const float*, float*, size_t, float, float, float, float, hipStream_t) { return stub_elementwise(); }
hipError_t launch_rownorm_loss(const float*, const float*, size_t, size_t, float*, float*, float*, hipStream_t) { return stub_elementwise(); }
size_t ssim_scratch_bytes(int N) { return (size_t)N * 64; }
hipError_t launch_ssim(const float*, const float*, float*, int, int, int, int, float, float*, hipStream_t) { return stub_elementwise(); }
hipError_t launch_u8_to_float(const uint8_t*, float*, size_t, hipStream_t) { return stub_elementwise(); }
hipError_t launch_gaussian_blur(const float*, float*, float*, int, int, int, int, float, hipStream_t) { return stub_elementwise(); }
hipError_t launch_resize_bilinear(const float*, float*, int, int, int, int, int, int, hipStream_t) { return stub_elementwise(); }
hipError_t launch_act_bwd(const float*, const float*, float*, size_t, int, hipStream_t) { return stub_elementwise(); }
hipError_t launch_affine(const float*, float*, size_t, float, float, hipStream_t) { return stub_elementwise(); }
hipError_t launch_saturate_u8(const float*, uint8_t*, size_t, hipStream_t) { return stub_elementwise(); }
hipError_t launch_psnr(const float*, const float*, float*, int, size_t, float, hipStream_t) { return stub_elementwise(); }
hipError_t launch_upsample_nearest(const float*, float*, int, int, int, int, int, hipStream_t) { return stub_elementwise(); }
hipError_t launch_upsample_nearest_bwd(const float*, float*, int, int, int, int, int, hipStream_t) { return stub_elementwise(); }
hipError_t launch_add_relu_grad(const float*, const float*, const float*, float*, size_t, hipStream_t) { return stub_elementwise(); }
hipError_t launch_poison_lds(hipStream_t) { return stub_elementwise(); }
}  // namespace srx

// the HIP runtime calls of srx_api.hip: the CU count is read through its per-device cache
extern "C" {
hipError_t hipGetDevice(int* dev) { *dev = 0; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t attr, int) {
    *v = attr == hipDeviceAttributeMultiprocessorCount ? srx_stub::cu_count() : 0;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stubbed HIP runtime"; }
hipError_t hipMemsetD32Async(hipDeviceptr_t, int, size_t, hipStream_t) { return hipSuccess; }
}
