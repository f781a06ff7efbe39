// launchers.h -- internal: typed launch entry points for the kernel instances, one per
// translation unit so the instances compile in parallel.
#pragma once
#include "conv_kernels.hip.h"
#include "lds_launch.h"

namespace srx {

struct ConvKey {
    int kh, kw, cinp, nch;
    bool wt;
};

// Each returns true if the key belongs to that unit (then *err holds the launch status).
bool launch_conv_k3c64(const ConvKey& k, const ConvArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_conv_k3c32(const ConvKey& k, const ConvArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_conv_c4(const ConvKey& k, const ConvArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_conv_misc(const ConvKey& k, const ConvArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_pipe_k3c64(const ConvKey& k, const ConvArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_pipe_other(const ConvKey& k, const ConvArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_wgrad_narrow(const ConvKey& k, const WgradArgs& a, int grid, hipStream_t s, hipError_t* err);
bool launch_conv_narrow(const ConvKey& k, const ConvArgs& a, hipStream_t s, hipError_t* err);
bool launch_conv_1x1(const ConvKey& k, const ConvArgs& a, long min_pixels, hipStream_t s, hipError_t* err);
bool launch_conv_rows3x3(const ConvKey& k, const ConvArgs& a, long min_pixels, hipStream_t s, hipError_t* err);
bool launch_conv_pack3(const ConvKey& k, const ConvArgs& a, long min_pixels, hipStream_t s, hipError_t* err);
bool launch_conv_kwrows(const ConvKey& k, const ConvArgs& a, long min_pixels, hipStream_t s, hipError_t* err);
bool launch_pipe_strip(const ConvKey& k, const ConvArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_conv_generic(const ConvKey& k, const ConvArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_wgrad(const ConvKey& k, const WgradArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_wgrad_generic(const ConvKey& k, const WgradArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_wgrad_lin(const ConvKey& k, const WgradArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_wgrad_lin_pack3(const ConvKey& k, const WgradArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_wgrad_lin_strip(const ConvKey& k, const WgradArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_wgrad_pipe(const ConvKey& k, const WgradArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_wgrad_kwcols(const ConvKey& k, const WgradArgs& a, int max_partials, long min_pixels, int* n_partials, hipStream_t s, hipError_t* err);
bool launch_wgrad_1x1(const ConvKey& k, const WgradArgs& a, int max_partials, int* n_partials, hipStream_t s, hipError_t* err);
bool launch_wgrad_rows_full(const ConvKey& k, const WgradArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_wgrad_rows_strip(const ConvKey& k, const WgradArgs& a, int grid, size_t lds, hipStream_t s, hipError_t* err);
bool launch_wgrad_lin_pairs(const ConvKey& k, const WgradPairs& q, int grid, int pairs, bool strips, size_t lds, hipStream_t s, hipError_t* err);

// Chained 3x3 64 -> 64 body layers (conv_chain.hip): forward (wt = false, no aux operand) or data gradient (wt = true,
// aux = ReLU-gradient masks present), c.L <= kChainMax layers of one shape in one launch.  A weak reference, like the bf16x3
// launchers: a host-only build of srx_api.hip without the kernel units (the ThreadSanitizer test) links, and refuses chains.
// fixed = true: the instance with the tile geometry compiled in (Geo41), if the plan in `a` equals its constants field by
// field; any other plan, or fixed = false, runs the instance that reads the shape from `a`.
__attribute__((weak)) hipError_t launch_conv_chain(bool wt, bool aux, bool fixed, const ConvArgs& a, const ChainPtrs& c, int grid, size_t lds, hipStream_t s);

// The filter gradients of `layers` 3x3 64 -> 64 layers of 41-pixel rows in one launch, wpl workgroups per layer, and the one
// reduction of their wpl * layers partials (wgrad_batch.hip).  Weak references, like launch_conv_chain: a host-only build
// links without them, and srx_conv2d_bwd_filter_batch refuses.
__attribute__((weak)) hipError_t launch_wgrad_rows_batch(const WgradArgs& a, const WgradBatchPtrs& c, int wpl, int layers, size_t lds, hipStream_t s);
__attribute__((weak)) hipError_t launch_wgrad_batch_reduce(const float* part, int wpl, int layers, int stride, int wn, int cout,
                                                           const WgradBatchOut& o, float wd, hipStream_t s);

hipError_t launch_reduce_partials(const float* part, int G, int stride, int wn, int cout, float* dw, float* dbias,
                                  const float* w, float wd, hipStream_t s);
// `pairs` problems at once: partials [pair][G][stride] -> dw [pair][wn], dbias [cob][cout] (taken from the pairs ib == 0)
hipError_t launch_reduce_partials_pairs(const float* part, int G, int stride, int wn, int cout, float* dw, float* dbias,
                                        int pairs, int cob, hipStream_t s);

// Every kernel instance of the case macros below: 256 threads, one argument struct `a`, the caller's grid, lds and s.
#define SRX_LAUNCH(...) launch_with_lds<__VA_ARGS__>(dim3(grid), dim3(256), lds, s, a)

#define SRX_CONV_CASE(KH, KW, CINP, NCH, WT, MINW)                                                        \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH && k.wt == WT) {                       \
        if (a.skip || a.mask)                                                                             \
            *err = SRX_LAUNCH(conv_mfma_kernel<KH, KW, CINP, NCH, WT, MINW, true>);                       \
        else                                                                                              \
            *err = SRX_LAUNCH(conv_mfma_kernel<KH, KW, CINP, NCH, WT, MINW, false>);                      \
        return true;                                                                                      \
    }
// Pipelined one-wave-per-SIMD kernel (>= 16 input channels): one workgroup per CU, two LDS buffers.
// (forward launches carry at most a residual operand, dgrad launches at most a ReluGrad mask)
#define SRX_PIPE_CASE_FWD(KH, KW, CINP, NCH)                                                              \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH && !k.wt) {                            \
        if (a.skip)                                                                                       \
            *err = SRX_LAUNCH(conv_pipe_kernel<KH, KW, CINP, NCH, false, 2>);                             \
        else                                                                                              \
            *err = SRX_LAUNCH(conv_pipe_kernel<KH, KW, CINP, NCH, false, 0>);                             \
        return true;                                                                                      \
    }
#define SRX_PIPE_CASE_DGRAD(KH, KW, CINP, NCH)                                                            \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH && k.wt) {                             \
        if (a.mask)                                                                                       \
            *err = SRX_LAUNCH(conv_pipe_kernel<KH, KW, CINP, NCH, true, 1>);                              \
        else                                                                                              \
            *err = SRX_LAUNCH(conv_pipe_kernel<KH, KW, CINP, NCH, true, 0>);                              \
        return true;                                                                                      \
    }
#define SRX_PIPE_STRIP_CASE(KH, KW, CINP, NCH)                                                            \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH && !k.wt) {                            \
        if (a.skip)                                                                                       \
            *err = SRX_LAUNCH(conv_pipe_strip_kernel<KH, KW, CINP, NCH, false, 2>);                       \
        else                                                                                              \
            *err = SRX_LAUNCH(conv_pipe_strip_kernel<KH, KW, CINP, NCH, false, 0>);                       \
        return true;                                                                                      \
    }                                                                                                     \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH && k.wt) {                             \
        if (a.mask)                                                                                       \
            *err = SRX_LAUNCH(conv_pipe_strip_kernel<KH, KW, CINP, NCH, true, 1>);                        \
        else                                                                                              \
            *err = SRX_LAUNCH(conv_pipe_strip_kernel<KH, KW, CINP, NCH, true, 0>);                        \
        return true;                                                                                      \
    }
// forward only, 32 output channels (two chunks), no aux operand: none / ReLU, or tanh (ESPCN's f2 on whole images)
#define SRX_PIPE_STRIP_CASE_FWD2(KH, KW, CINP, NCH)                                                       \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH && !k.wt && !a.skip && !a.mask) {      \
        if (a.act == ACT_TANH)                                                                            \
            *err = SRX_LAUNCH(conv_pipe_strip_kernel<KH, KW, CINP, NCH, false, 3>);                       \
        else                                                                                              \
            *err = SRX_LAUNCH(conv_pipe_strip_kernel<KH, KW, CINP, NCH, false, 0>);                       \
        return true;                                                                                      \
    }
#define SRX_PIPE_STRIP_CASE_D2S(KH, KW, CINP, NCH)                                                        \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH && !k.wt && !a.skip && !a.mask && a.d2s_r) { \
        *err = SRX_LAUNCH(conv_pipe_strip_kernel<KH, KW, CINP, NCH, false, 4>);                           \
        return true;                                                                                      \
    }
#define SRX_WGRAD_LIN_CASE(KH, KW, CINP, NCH, MINW)                                                       \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH) {                                     \
        *err = SRX_LAUNCH(wgrad_lin_kernel<KH, KW, CINP, NCH, MINW>);                                     \
        return true;                                                                                      \
    }
#define SRX_WGRAD_LIN_STRIP_CASE(KH, KW, CINP, NCH, MINW)                                                 \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH) {                                     \
        *err = SRX_LAUNCH(wgrad_lin_strip_kernel<KH, KW, CINP, NCH, MINW>);                               \
        return true;                                                                                      \
    }
#define SRX_WGRAD_PIPE_CASE(KH, KW, CINP, NCH)                                                            \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH) {                                     \
        *err = SRX_LAUNCH(wgrad_pipe_kernel<KH, KW, CINP, NCH>);                                          \
        return true;                                                                                      \
    }
#define SRX_WGRAD_CASE(KH, KW, CINP, NCH, MINW)                                                           \
    if (k.kh == KH && k.kw == KW && k.cinp == CINP && k.nch == NCH) {                                     \
        *err = SRX_LAUNCH(wgrad_mfma_kernel<KH, KW, CINP, NCH, MINW>);                                    \
        return true;                                                                                      \
    }

}  // namespace srx
