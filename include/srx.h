/*
 * srx.h -- C ABI of libsrx.so, the MI355X (gfx950) super-resolution conv engine.
 *
 * The reference (imironhead/ml_super_resolution) has no FFI / plugin boundary: its
 * hot path is reached through TensorFlow-1.8's Python op API.  Each entry point below
 * names the reference call site(s) whose TF op it replaces (paths relative to
 * /root/reference).  INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer owned by the caller (e.g. a PyTorch-ROCm
 *     tensor's data_ptr()); fp32; activations NHWC, filters HWIO [KH,KW,Cin,Cout];
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); the
 *     library never synchronises the device and allocates nothing per call;
 *   - returns SRX_OK (0) or a negative srx_status; srx_last_error() gives the text
 *     (thread-local); bad shapes / alignment are errors, never undefined behaviour;
 *   - calls may come from several host threads at once and may target any device (the calling thread's current
 *     one); per-device launch state is kept per calling thread;
 *   - base pointers of activations / filters must be 16-byte aligned.
 */
#ifndef SRX_H_
#define SRX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* srx_stream_t; /* hipStream_t */

typedef enum {
    SRX_OK = 0,
    SRX_ERR_BAD_ARG = -1,     /* null pointer, non-positive dim, unknown enum */
    SRX_ERR_UNSUPPORTED = -2, /* shape outside the compiled kernel set (e.g. stride 3, a stride-2 data gradient) */
    SRX_ERR_WORKSPACE = -3,   /* workspace missing or too small */
    SRX_ERR_LAUNCH = -4,      /* HIP runtime reported an error at launch */
    SRX_ERR_ALIGN = -5        /* pointer not 16-byte aligned */
} srx_status;

typedef enum { SRX_PAD_SAME = 0, SRX_PAD_VALID = 1 } srx_pad_mode;

typedef enum {
    SRX_ACT_NONE = 0,
    SRX_ACT_RELU = 1,   /* vdsr/vdsr/model_vdsr.py:68, srcnn/srcnn.py:106,117 */
    SRX_ACT_TANH = 2,   /* espcn/espcn/model_espcn.py:36,46,120,126; srcnn/srcnn.py:128 */
    SRX_ACT_LRELU = 3,  /* leaky_relu(0.2): enet/enet/model_enet.py:130-146 */
    SRX_ACT_SIGMOID = 4 /* enet/enet/model_enet.py:160 */
} srx_act;

typedef enum { SRX_OP_FWD = 0, SRX_OP_BWD_DATA = 1, SRX_OP_BWD_FILTER = 2 } srx_conv_op;

/* srx_conv_desc.precision -- how the convolution's PRODUCTS are computed.
 *   SRX_PRECISION_FP32 (0, the default)  exact fp32: v_mfma_f32_16x16x4_f32.
 *   SRX_PRECISION_BF16X3 (1)             split bf16 ("bf16x3", what torch.set_float32_matmul_precision("high") may
 *       mean): each fp32 operand a of a product is split inside the kernel into hi = bf16_rne(a), lo = bf16_rne(a - hi)
 *       (the subtraction is exact in fp32), and each product is hi*hi + hi*lo + lo*hi, accumulated in fp32 by
 *       v_mfma_f32_16x16x32_bf16 -- about 2^-16 relative error per product at 3/16 of the fp32 MFMA time.  The split
 *       applies to both operands of the products: forward x and w, data gradient dpre and w, filter gradient x and dpre.
 *       Everything else stays exact fp32 as at precision 0: bias, activation, the ReLU-gradient mask, the bias gradient
 *       (a plain fp32 sum of dpre), the reduction of the partial filters and the weight-decay term.  Tensors in and out
 *       stay fp32; no bf16 copy is kept anywhere.  The split is a plain cast: a NaN stays a NaN, and non-finite inputs
 *       give non-finite outputs.  Worst case per output element: |y - exact| <= 2^-13 (|x| (*) |w| + |b|).
 *       Forward and data gradient sum every output element in one fixed order wherever its pixel lies: image n of a
 *       batch gets the same bits as the image run alone.  Deterministic like precision 0.
 *       Supported set (srx_conv2d_precision_supported): 3x3, stride 1, SAME, Cin = Cout = 64, post_add_relu 0,
 *       subpixel_r 0 / 1, act NONE / RELU; forward without a skip operand, data gradient with in_act NONE / RELU (not
 *       srx_conv2d_bwd_data_acc), the filter gradient and its _partials / _reduce halves.  Any N, H, W.  Other layers at
 *       precision 1 return SRX_ERR_UNSUPPORTED.  srx_set_conv_path / srx_set_wgrad_path do not apply to it: one kernel
 *       family (conv_bf16x3.hip).  Layers wider than 64 channels run at it through srx_conv3x3_blocked_ex and
 *       srx_conv3x3_blocked_bwd_filter_ex (below), with the same split, bound and determinism.
 * Any other value is SRX_ERR_BAD_ARG. */
typedef enum { SRX_PRECISION_FP32 = 0, SRX_PRECISION_BF16X3 = 1 } srx_precision;

/* One convolution layer.  N,H,W,Cin describe the layer INPUT x; the output is [N,OH,OW,Cout] with OH,OW from
 * pad_mode and stride, TensorFlow's geometry: SAME -> OH = ceil(H / stride), pad_total = max((OH-1) stride + KH - H, 0),
 * pad_before = pad_total / 2 (the odd pixel goes AFTER); VALID -> OH = (H - KH) / stride + 1. */
typedef struct {
    int32_t N, H, W, Cin, Cout, KH, KW;
    int32_t stride;        /* 1, or 2: tf.layers.conv2d(strides=2, padding='same') of ENet's discriminator
                            * (enet/enet/model_enet.py:136-146; 0 before / 1 after on an even-sized image).  Stride 2 is
                            * implemented by srx_conv2d_fwd and srx_conv2d_bwd_filter (+ _partials / _reduce / the
                            * workspace query; there dpre is the gradient at the half-resolution output), at a quarter of
                            * the stride-1 layer's MFMA work.  srx_conv2d_bwd_data(_acc) refuses it: the data gradient of
                            * a stride-2 layer is the stride-1 data gradient of the zero-stuffed upstream gradient
                            * (srx_subsample2_bwd below), and srx_conv3x3_blocked (> 64 channels) is stride 1: the
                            * stride-1 layer sampled at the odd positions (srx_subsample2). */
    int32_t pad_mode;      /* srx_pad_mode */
    int32_t act;           /* srx_act fused after bias */
    int32_t post_add_relu; /* activation applied AFTER the skip add: 0 none, SRX_ACT_RELU (1) relu(conv + skip) as in
                            * enet/enet/model_enet.py:8-31, SRX_ACT_LRELU (3) leaky ReLU -- the closing launch of a
                            * layer whose input channels are accumulated over several launches (see
                            * srx_conv2d_bwd_data_acc) */
    int32_t precision;     /* srx_precision: 0 exact fp32 (default), 1 bf16x3 (see above) */
    int32_t subpixel_r;    /* srx_conv2d_fwd only.  0 / 1: y is [N,OH,OW,Cout].  r > 1: the epilogue stores through the
                            * sub-pixel (depth-to-space) index map, y is [N,OH*r,OW*r,Cout/(r*r)]:
                            *   y[n, h*r+dy, w*r+dx, c] = conv[n, h, w, (dy*r+dx)*C + c]
                            * bit-identical to srx_conv2d_fwd followed by srx_depth_to_space, without the intermediate
                            * tensor (ESPCN's f3 layer + espcn/espcn/experiment_test.py:171-177 in one launch).
                            * Ignored (must be 0 or 1) by the backward entry points. */
} srx_conv_desc;

const char* srx_version(void);
const char* srx_last_error(void);

/* Selects the forward / dgrad kernel family for layers with >= 16 input channels:
 *   1 (default)  3x3 body layers (16..64 exact-fit input channels, none / ReLU / ReluGrad / residual
 *                epilogues; full-width tiles, or column strips for 64 -> 64 layers of images too wide
 *                for them) run on one workgroup per CU with a double-buffered LDS tile, everything but
 *                the MFMAs done by scalar and memory instructions; all other shapes use the kernels of
 *                path 0;
 *   0            two persistent workgroups per CU, one LDS tile each (conv_mfma_kernel), for every shape.
 * Same results bit for bit on both paths, with ONE exception: path 1 runs SRCNN's 5x5 32 -> 3 layer (from
 * SRX_KWROWS_MIN_PIXELS = 4096 output pixels) on conv_kwrows_kernel, which adds the kw partial sums of an output in
 * another order: equal to path 0 to rounding (<= 2e-6 of the output scale).  (Path 1's kernels for the RGB-input 9x9 / 5x5
 * layers, conv_pack3.hip, keep the order of the products and are bit-identical to path 0 for FINITE inputs: a zero-weighted
 * slot past each filter row lets an Inf / NaN one column right of an output's window reach it as a NaN.)
 * A tuning / A-B switch (also: environment SRX_PIPE).  Returns the old value. */
int srx_set_conv_path(int pipelined);

/* Selects the filter-gradient (Conv2DBackpropFilter) kernel family:
 *   2 (default)  3x3 64 -> 64 layers on one workgroup per CU with a double-buffered LDS tile (full-width tiles:
 *                wgrad_pipe_kernel; images too wide for them: 32-column strips, wgrad_rows_strip_kernel); other
 *                shapes as path 1;
 *   1            the linear-walk kernels with two workgroups per CU (wgrad_lin_kernel / wgrad_lin_strip_kernel)
 *                wherever they apply; other shapes as path 0;
 *   0            the per-lane cursor kernel (wgrad_mfma_kernel) for every shape;
 *   < 0          back to the environment's default (SRX_WGRAD_LIN / SRX_WGRAD_PIPE / SRX_WGRAD_PIPE_STRIP).
 * The paths differ in how a layer's pixels are dealt out to workgroups, i.e. in the order of the fp32 additions:
 * results agree to rounding.  A tuning / A-B switch.  Returns the old value. */
int srx_set_wgrad_path(int path);

/* Chained body layers: ONE launch runs `layers` (1..32) consecutive layers of the same shape and pass instead of one launch
 * per layer.  d describes one layer (as for srx_conv2d_fwd / srx_conv2d_bwd_data); layer l reads x[l], w[l] (HWIO of the
 * forward layer) and writes y[l].
 *   op SRX_OP_FWD:       y[l] = act(bias[l] + x[l] (*) w[l]); aux must be NULL (no skip operand), bias NULL or per layer
 *                        (entries nullable); in_act is ignored.
 *   op SRX_OP_BWD_DATA:  x[l] = dpre, y[l] = dx_out as in srx_conv2d_bwd_data; in_act SRX_ACT_RELU with aux[l] = x_in (the
 *                        ReLU-gradient mask), or SRX_ACT_NONE with aux NULL; bias is ignored.
 * Layers run in order, each after the whole previous one, so any layer may read what an earlier one wrote.  Eligible
 * (srx_conv_chain_supported): precision 0, 3x3 64 -> 64, stride 1, SAME, act none / ReLU, conv path 1, images on the
 * full-width pipelined route (not column strips), and N a multiple of the pipelined grid (the compute-unit count): each
 * workgroup then owns whole images, and no workgroup ever waits for another.  Anything else returns SRX_ERR_UNSUPPORTED
 * with the reason; the caller launches the layers one by one.  Same results bit for bit as one srx_conv2d_fwd /
 * srx_conv2d_bwd_data per layer. */
int srx_conv_chain(const srx_conv_desc* d, int op, int in_act, int layers, const float* const* x, const float* const* w,
                   const float* const* bias, const float* const* aux, float* const* y, srx_stream_t stream);

/* 1 when srx_conv_chain takes this layer / op / in_act, else 0 with the reason in srx_last_error().  Host-only. */
int srx_conv_chain_supported(const srx_conv_desc* d, int op, int in_act);

/* 1 (default): srx_conv_chain runs eligible chains; 0: it refuses them all (SRX_ERR_UNSUPPORTED), so callers launch per
 * layer; < 0: back to the environment's default (SRX_CHAIN).  A tuning / A-B switch.  Returns the old value. */
int srx_set_chain(int on);

/* 1 (default): a chain whose plan is that of VDSR's 41 x 41 patches (41-pixel rows, 5-row tiles) runs the kernel instance
 * with that tile geometry compiled in; 0: every chain runs the instance that reads the shape from its arguments; < 0: back
 * to the environment's default (SRX_CHAIN_FIXED).  Both instances issue the same MFMAs in the same order: the same bits.
 * A tuning / A-B switch.  Returns the old value. */
int srx_set_chain_fixed(int on);

/* 1 when `op` (srx_conv_op) runs at d->precision for this descriptor, else 0 with the reason in srx_last_error().  Always 1
 * for a valid descriptor at precision 0.  Depends on the filter, channels, stride, padding and epilogue, never on N, H, W.
 * Host-only (no device call). */
int srx_conv2d_precision_supported(const srx_conv_desc* d, int op);

/* Bytes of caller-owned workspace an op uses.  BWD_FILTER: required (per-workgroup partials).
 * FWD / BWD_DATA: 256 bytes reserved; the ws / ws_bytes arguments of srx_conv2d_fwd, srx_conv2d_bwd_data and
 * srx_conv2d_bwd_data_acc may be NULL / 0 and are not used. */
size_t srx_conv2d_workspace_bytes(const srx_conv_desc* d, int op);

/* y = act(bias + x (*) w) [+ skip] [relu]
 * Replaces tf.layers.conv2d / tf.contrib.layers.convolution2d / tf.nn.conv2d +
 * tf.nn.bias_add + tf.nn.{relu,tanh} and the residual add:
 *   vdsr/vdsr/model_vdsr.py:62-76 (conv+bias+relu), :85-104 (conv+bias, sd + res)
 *   espcn/espcn/model_espcn.py:30-62, :117-134
 *   srcnn/srcnn.py:100-130
 *   enet/enet/model_enet.py:13-29, :63-113
 * bias, skip nullable.  skip has the output's shape. */
int srx_conv2d_fwd(const srx_conv_desc* d, const float* x, const float* w, const float* bias,
                   const float* skip, float* y, void* ws, size_t ws_bytes, srx_stream_t stream);

/* Conv2DBackpropInput with the UPSTREAM activation gradient fused:
 *   dx[n,h,w,ci] = sum_{kh,kw,co} dpre[n,h+pt-kh,w+pl-kw,co] * w[kh,kw,ci,co]
 *   dx_out = dx * act'(x_in)      (x_in = this layer's input = the previous layer's
 *                                  post-activation output; ReluGrad masks on x_in > 0)
 * dpre is the gradient w.r.t. this layer's PRE-activation output.  x_in nullable
 * (then in_act is ignored and plain dx is written).
 * Replaces the Conv2DBackpropInput + ReluGrad/TanhGrad pairs TF autodiff emits for
 * optimizer.minimize: vdsr/vdsr/model_vdsr.py:146-148,174;
 * espcn/espcn/model_espcn.py:87-89; srcnn/srcnn.py:155-157. */
int srx_conv2d_bwd_data(const srx_conv_desc* d, const float* dpre, const float* w,
                        const float* x_in, int in_act, float* dx_out, void* ws, size_t ws_bytes,
                        srx_stream_t stream);

/* The same without the activation mask but with an ACCUMULATE operand: dx_out = dx + dx_acc (dx_out may alias
 * dx_acc).  Layers wider than the kernels' 64 channels (ENet's discriminator, VGG-19: enet/enet/model_enet.py:
 * 118-162, enet/enet/model_vgg.py:65-99) keep their tensors as blocks of 64 channels; the data gradient of an
 * input block is the sum over the output blocks of one launch each:
 *   dx[ib] = sum_ob bwd_data(dpre[ob], w[ib][ob]);   then srx_act_bwd applies the activation mask once.
 * The forward counterpart needs no extra entry point: y[ob] = act(sum_ib conv(x[ib], w[ib][ob]) + bias) is
 * srx_conv2d_fwd with skip = the running sum, act = NONE and, in the last launch, post_add_relu = the layer's
 * activation.  The filter gradients of the block pairs are independent srx_conv2d_bwd_filter calls. */
int srx_conv2d_bwd_data_acc(const srx_conv_desc* d, const float* dpre, const float* w, const float* dx_acc,
                            float* dx_out, void* ws, size_t ws_bytes, srx_stream_t stream);

/* Conv2DBackpropFilter + BiasAddGrad (+ the L2 regulariser's gradient):
 *   dw[kh,kw,ci,co] = sum_{n,oh,ow} x[n,oh+kh-pt,ow+kw-pl,ci] * dpre[n,oh,ow,co]
 *                     + wd_scale * w[kh,kw,ci,co]          (if w_for_decay != NULL)
 *   dbias[co]       = sum_{n,oh,ow} dpre[n,oh,ow,co]       (if dbias != NULL)
 * Deterministic: fixed work partition, partials reduced in a fixed order.
 * Same reference call sites as srx_conv2d_bwd_data; the regulariser is
 * tf.contrib.layers.l2_regularizer(1e-4): vdsr/vdsr/model_vdsr.py:34,70,93,125. */
int srx_conv2d_bwd_filter(const srx_conv_desc* d, const float* x, const float* dpre, float* dw,
                          float* dbias, const float* w_for_decay, float wd_scale, void* ws,
                          size_t ws_bytes, srx_stream_t stream);

/* The same in two calls, for callers that want the (HBM-bound) reduction of the per-workgroup partials to run
 * on another stream than the (MFMA-bound) gradient kernel -- e.g. under the next layer's dgrad:
 *   srx_conv2d_bwd_filter_partials   fills `ws` with *n_partials partial filters;
 *   srx_conv2d_bwd_filter_reduce     sums them in a fixed order into dw / dbias (+ the regulariser term).
 * The caller orders the two (event / stream wait) and keeps `ws` untouched in between.
 * srx_conv2d_bwd_filter(...) == partials + reduce on one stream, bit for bit. */
int srx_conv2d_bwd_filter_partials(const srx_conv_desc* d, const float* x, const float* dpre, void* ws,
                                   size_t ws_bytes, int* n_partials, srx_stream_t stream);
int srx_conv2d_bwd_filter_reduce(const srx_conv_desc* d, const void* ws, int n_partials, float* dw,
                                 float* dbias, const float* w_for_decay, float wd_scale,
                                 srx_stream_t stream);

/* The filter gradients of n_layers (2..32) layers of ONE shape in one launch plus one reduction, instead of a launch and a
 * reduction per layer: layer l reads x[l], dpre[l] and writes dw[l], dbias[l] (dbias, w_for_decay: NULL, or per layer with
 * nullable entries) exactly as srx_conv2d_bwd_filter would.  The work is cut layer-major: wgs_per_layer = min(grid / n_layers,
 * N * OH) workgroups share a layer's N * OH rows evenly, each accumulates its rows -- of several images -- into ONE
 * partial filter, and the reduction adds a layer's partials in index order.  Deterministic; the additions are grouped
 * otherwise than in srx_conv2d_bwd_filter, so the results agree with it to rounding (and exactly where every sum is exact).
 * Eligible exactly where the per-layer call runs wgrad_rows_full_kernel: precision 0, 3x3 64 -> 64, stride 1, SAME, W = 41,
 * filter-gradient path 2, and every pointer 16-byte aligned.  Anything else returns SRX_ERR_UNSUPPORTED with the reason and
 * writes nothing; the caller launches per layer.  Does not depend on srx_set_conv_path or srx_set_chain.
 * Workspace: srx_conv2d_bwd_filter_batch_workspace_bytes (n_layers * wgs_per_layer partial filters; 0 when not eligible). */
int srx_conv2d_bwd_filter_batch(const srx_conv_desc* d, int n_layers, const float* const* x, const float* const* dpre,
                                float* const* dw, float* const* dbias, const float* const* w_for_decay, float wd_scale,
                                void* ws, size_t ws_bytes, srx_stream_t stream);
size_t srx_conv2d_bwd_filter_batch_workspace_bytes(const srx_conv_desc* d, int n_layers);
/* The split srx_conv2d_bwd_filter_batch uses: workgroups per layer and the grid they were fitted into (0 and 0 when the
 * batch is not eligible; the status says why).  Host-only. */
int srx_conv2d_bwd_filter_batch_plan(const srx_conv_desc* d, int n_layers, int* wgs_per_layer, int* grid);
/* 1 (default): srx_conv2d_bwd_filter_batch runs eligible batches; 0: it refuses them all (SRX_ERR_UNSUPPORTED), so callers
 * launch per layer; < 0: back to the environment's default (SRX_WGRAD_BATCH).  A tuning / A-B switch.  Returns the old value. */
int srx_set_wgrad_batch(int on);

/* dpre = dy * act'(y)  (ReluGrad / TanhGrad on the post-activation tensor). */
int srx_act_bwd(const float* dy, const float* y, float* dpre, size_t numel, int act,
                srx_stream_t stream);

/* Sub-pixel (depth-to-space) index map, bit-exact permutation:
 *   out[n, h*r+dy, w*r+dx, c] = in[n, h, w, (dy*r+dx)*C + c]
 * in [N,H,W,C*r*r] -> out [N,H*r,W*r,C].  Replaces the host NumPy split/reshape/
 * concatenate of espcn/espcn/experiment_test.py:171-177 and the TF split/reshape/concat
 * of espcn/espcn/experiment_train.py:47-56. */
int srx_depth_to_space(const float* in, float* out, int N, int H, int W, int C, int r,
                       srx_stream_t stream);

/* Measurement aid, not an operator of the path: a plain streaming copy (nontemporal 16-byte loads and stores, the
 * launch shape of the sub-pixel kernels).  bench.py times it on the sub-pixel map's own buffers: what a kernel that
 * only moves these bytes reaches at this transfer size is the ceiling the map is compared with
 * (`subpixel.copy_ceiling_gbps`).  in / out 16-byte aligned, bytes a multiple of 16.  No reference counterpart. */
int srx_stream_copy(const void* in, void* out, size_t bytes, srx_stream_t stream);

/* ESPCN inference in ONE launch (espcn/espcn/model_espcn.py:117-134 + espcn/espcn/experiment_test.py:171-177):
 *   t1 = tanh(conv5x5(x; 3->64) + b1), t2 = tanh(conv3x3(t1; 64->32) + b2), y = conv3x3(t2; 32->3 r^2) + b3 (all SAME),
 *   hr[n, h r + dy, w r + dx, c] = y[n, h, w, (dy r + dx) 3 + c]
 * x [N,H,W,3], filters HWIO ([5,5,3,64], [3,3,64,32], [3,3,32,3 r^2]), hr [N,H r,W r,3], r in 2..4.  A workgroup chains
 * the three layers through LDS on a tile of <= 16x16 LR pixels (halo recomputed per tile): meant for latency-bound sizes
 * such as BASELINE configs[1] (batch 32 of 17x17 patches) and images of up to ~130 k pixels; beyond, the per-layer launches
 * do less work.
 * Bit-identical to the three srx_conv2d_fwd launches (the last with subpixel_r). */
int srx_espcn_forward(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                      const float* w3, const float* b3, float* hr, int N, int H, int W, int r,
                      srx_stream_t stream);
/* The same launch as the FORWARD PASS OF A TRAIN STEP (espcn/espcn/model_espcn.py:117-134 under the trainer of
 * model_espcn.py:137-160): besides chaining the layers through LDS it writes what backward needs -- t1 [N,H,W,64] and
 * t2 [N,H,W,32] (post-tanh; every pixel by the one tile that owns it) -- and y [N,H,W,3 r^2] in sub-pixel space (the loss of
 * the reference is taken there), instead of the shuffled HR image.  Bit-identical to three srx_conv2d_fwd launches.
 * t1 / t2 16-byte aligned. */
int srx_espcn_forward_keep(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                           const float* w3, const float* b3, float* t1, float* t2, float* y, int N, int H, int W, int r,
                           srx_stream_t stream);

/* ESPCN inference from bytes to bytes (espcn/espcn/experiment_test.py:148-184: `lr_image / 127.5 - 1.0`, the network, the
 * sub-pixel shuffle, `* 0.5 + 0.5`, clip to [0, 1], `* 255.0 + 0.5`, astype(uint8)).
 *   decode  x = lut[byte]; lut is the caller's 256 floats in device memory.  The host route's map is float64 arithmetic and
 *           one cast, `(np.arange(256, dtype=np.uint8) / 127.5 - 1.0).astype(np.float32)`, which fp32 arithmetic on the
 *           device (srx_u8_to_pm1) is not guaranteed to reproduce: a table of those floats is that route by construction.
 *   encode  t = y * 0.5f; t = t + 0.5f; t = min(max(t, 0), 1); t = t * 255.f; t = t + 0.5f; (uint8_t)t -- every step
 *           rounded on its own, truncation toward zero: srx_affine(0.5, 0.5), clamp_ and numpy's fp32 `* 255.0 + 0.5` and
 *           astype, in that order.  A NaN encodes to 0 (the host route's astype of a NaN is undefined).
 *
 * srx_espcn_forward_u8 (espcn/espcn/experiment_test.py:148-184): srx_espcn_forward's ONE launch with both maps inside --
 *   lr [N,H,W,3] bytes read through lut while the halo is staged, hr [N,H r,W r,3] = encode of the f3 accumulators, stored
 *   through the same sub-pixel offsets.  The MFMA sequence is srx_espcn_forward's: hr is the encode of its bits.
 *   Refuses: null lr, lut, hr, filter or bias; non-positive N, H, W; r outside 2..4; b1 / b2 not 16-byte aligned;
 *   N H W 3 r^2 >= 2^31.  lr and hr need no alignment.
 * srx_u8_lut_float (experiment_test.py:148-184, the decode alone): out[i] = lut[in[i]].  Refuses null in, lut, out and an
 *   out that is not 4-byte aligned.  n == 0 is a no-op.
 * srx_unit_u8 (experiment_test.py:148-184, the encode alone): out[i] = encode(x[i]), 16-byte loads and packed 4-byte stores
 *   where x and out allow it, byte stores elsewhere; any byte offset of out and any float offset of x.  Refuses null x, out and
 *   an x that is not 4-byte aligned.  n == 0 is a no-op.
 * Frames above the one-launch window run srx_u8_lut_float, three srx_conv2d_fwd (the last with subpixel_r), srx_unit_u8. */
int srx_espcn_forward_u8(const uint8_t* lr, const float* lut, const float* w1, const float* b1, const float* w2,
                         const float* b2, const float* w3, const float* b3, uint8_t* hr, int N, int H, int W, int r,
                         srx_stream_t stream);
int srx_u8_lut_float(const uint8_t* in, const float* lut, float* out, size_t n, srx_stream_t stream);
int srx_unit_u8(const float* x, uint8_t* out, size_t n, srx_stream_t stream);

/* Planar YUV 4:2:0 frames on either side of ESPCN's float network (no reference counterpart: the reference reads image
 * files).  A frame of H x W is one byte string, the YUV4MPEG2 frame payload: Y [H,W], U [CH,CW], V [CH,CW] with
 * CH = (H + 1) / 2, CW = (W + 1) / 2 -- H W + 2 CH CW bytes; N frames lie back to back, so a frame may start at any address.
 * Integer arithmetic, 14 fractional bits, h = 1 << 13, `>>` the arithmetic shift, clip8 the clamp to [0, 255].
 *
 * srx_yuv420_coeffs: host only, no GPU call.  The integers for a matrix (SRX_YUV_BT601: Kr 0.299, Kb 0.114; SRX_YUV_BT709:
 *   Kr 0.2126, Kb 0.0722) and a range (limited: yoff 16, luma scale 219/255, chroma scale 224/255; full: 0, 1, 1), each
 *   floor(v * 16384 + 0.5) of the real value in double.  bt601 limited: cy 19077, crv 26149, cgu 6419, cgv 13320, cbu 33050;
 *   kry 4207, kgy 8260, kby 1604; kru -2428, kgu -4768, kbu 7196, krv 7196, kgv -6026, kbv -1170.  Every accumulator below stays
 *   under 2^24 in magnitude.  Refuses a null c and an unknown matrix.
 * srx_yuv420_lut_float: yuv [N frames] -> out [N,H,W,3] floats.  Pixel (y, x) takes the chroma sample (y >> 1, x >> 1)
 *   (replication, no siting filter); c = Y - yoff, d = U - 128, e = V - 128;
 *   R = clip8((cy c + crv e + h) >> 14), G = clip8((cy c - cgu d - cgv e + h) >> 14), B = clip8((cy c + cbu d + h) >> 14);
 *   out = lut[byte], lut as for srx_u8_lut_float.
 * srx_unit_yuv420: x [N,H,W,3] floats -> yuv [N frames].  R, G, B = encode(x) as srx_unit_u8;
 *   Y = clip8(yoff + ((kry R + kgy G + kby B + h) >> 14)); chroma sample (j, i) from SR, SG, SB, the sums over the pixels
 *   (min(2 j + a, H - 1), min(2 i + b, W - 1)), a, b in {0, 1}: U = clip8(128 + ((kru SR + kgu SG + kbu SB + (1 << 15)) >> 16)),
 *   V likewise -- one rounding for the average and the matrix.  16-byte loads and 4-byte stores when W % 8 == 0, x is
 *   16-byte and yuv 4-byte aligned; 4-byte loads and byte stores for any other W, float offset of x and byte offset of yuv.
 * Both refuse: a null pointer; non-positive N, H, W; an out / x that is not 4-byte aligned; N H W 3 >= 2^31.  The coefficients
 * travel by value as kernel arguments. */
enum { SRX_YUV_BT601 = 0, SRX_YUV_BT709 = 1 };
typedef struct srx_yuv420_coeffs_t {
    int32_t yoff;
    int32_t cy, crv, cgu, cgv, cbu;                 /* decode */
    int32_t kry, kgy, kby;                          /* encode, luma */
    int32_t kru, kgu, kbu, krv, kgv, kbv;           /* encode, chroma */
    int32_t reserved;
} srx_yuv420_coeffs_t;
int srx_yuv420_coeffs(int matrix, int full_range, srx_yuv420_coeffs_t* c);
int srx_yuv420_lut_float(const uint8_t* yuv, int N, int H, int W, const srx_yuv420_coeffs_t* c, const float* lut, float* out,
                         srx_stream_t stream);
int srx_unit_yuv420(const float* x, int N, int H, int W, const srx_yuv420_coeffs_t* c, uint8_t* yuv, srx_stream_t stream);

/* Planar YUV frames of other samplings and depths, the same arithmetic with the offsets scaled by the depth.  A pixel format is
 * (depth, sub_x, sub_y): depth 8, 10 or 12; (sub_x, sub_y) = (0, 0) for 4:4:4, (1, 0) for 4:2:2, (1, 1) for 4:2:0; reserved 0.
 * max = (1 << depth) - 1, mid = 1 << (depth - 1).  A sample is one byte at depth 8 and two bytes, little-endian, above (Y4M's
 * p10 / p12); a sample above max in a 16-bit container is read as max.  A frame of H x W is Y [H,W], U [CH,CW], V [CH,CW] with
 * CH = (H + sub_y) >> sub_y, CW = (W + sub_x) >> sub_x: one byte string of bps (H W + 2 CH CW) bytes, N frames back to back.
 *
 * srx_yuv_frame_bytes: host only.  That byte count; 0 with the reason in srx_last_error() for a null or refused format, a
 *   non-positive size or a count that does not fit a size_t.
 * srx_yuv_coeffs: host only.  srx_yuv420_coeffs' formulas (one piece of code) with the range scales made depth-aware: limited
 *   range yoff = 16 << (depth - 8), luma scale 219 2^(depth-8) / max, chroma scale 224 2^(depth-8) / max; full range 0, 1, 1.
 *   Depth 8 gives srx_yuv420_coeffs' integers.  bt709 limited at depth 10: yoff 64, cy 19133, crv 29459, cgu 3504, cgv 8757,
 *   cbu 34711; kry 2983, kgy 10034, kby 1013; kru -1644, kgu -5531, kbu 7175, krv 7175, kgv -6517, kbv -658.  Every accumulator
 *   below stays under 2^28 in magnitude.  Refuses a null c, an unknown matrix and a depth other than 8, 10, 12.
 * srx_yuv_lut_float: yuv [N frames] -> out [N,H,W,3] floats.  Pixel (y, x) takes the chroma sample (y >> sub_y, x >> sub_x);
 *   c = Y - yoff, d = U - mid, e = V - mid; R = clip((cy c + crv e + h) >> 14, 0, max), G and B as srx_yuv420_lut_float's;
 *   out = lut[code], lut the caller's 2^depth floats in device memory.
 * srx_unit_yuv: x [N,H,W,3] floats -> yuv [N frames].  R, G, B = encode_unit_bits(x, max): srx_unit_u8's five roundings with
 *   255 replaced by max; Y = clip(yoff + ((kry R + kgy G + kby B + h) >> 14)); chroma sample (j, i) from SR, SG, SB, the sums
 *   over the (1 << sub_y) x (1 << sub_x) pixels (min((j << sub_y) + a, H - 1), min((i << sub_x) + b, W - 1)):
 *   U = clip(mid + ((kru SR + kgu SG + kbu SB + (1 << (13 + sub_x + sub_y))) >> (14 + sub_x + sub_y))), V likewise.  16-byte
 *   loads and stores of 4 bytes and more when W % 8 == 0, x is 16-byte and yuv 4-byte aligned; 4-byte loads and sample-sized
 *   stores for any other W, float offset of x and sample offset of yuv.
 * The two refuse before any launch: a null pointer; non-positive N, H, W; a depth outside {8, 10, 12}; (sub_x, sub_y) outside
 * the three pairs; reserved != 0; an out / x that is not 4-byte aligned; a yuv that is not 2-byte aligned at depth > 8;
 * N H W 3 >= 2^31.  Called with (8, 1, 1) they hand over to srx_yuv420_lut_float / srx_unit_yuv420: one kernel per job. */
typedef struct srx_yuv_format_t { int32_t depth, sub_x, sub_y, reserved; } srx_yuv_format_t;
size_t srx_yuv_frame_bytes(const srx_yuv_format_t* f, int H, int W);
int srx_yuv_coeffs(int matrix, int full_range, int depth, srx_yuv420_coeffs_t* c);
int srx_yuv_lut_float(const void* yuv, int N, int H, int W, const srx_yuv_format_t* f, const srx_yuv420_coeffs_t* c,
                      const float* lut, float* out, srx_stream_t stream);
int srx_unit_yuv(const float* x, int N, int H, int W, const srx_yuv_format_t* f, const srx_yuv420_coeffs_t* c,
                 void* yuv, srx_stream_t stream);

/* SRCNN inference in ONE launch (srcnn/srcnn.py:100-130, tf.contrib.layers.convolution2d x 3, padding 'VALID'):
 *   t1 = relu(conv9x9(x; 3->64) + b1), t2 = relu(conv1x1(t1; 64->32) + b2), y = tanh(conv5x5(t2; 32->3) + b3)
 * x [N,H,W,3] (H, W >= 13), filters HWIO ([9,9,3,64], [1,1,64,32], [5,5,32,3]), y [N,H-12,W-12,3].  A workgroup chains the
 * three layers through LDS for a tile of <= 15x15 output pixels; bit-identical to three srx_conv2d_fwd launches.  For
 * latency-bound problems (BASELINE configs[0]: one 243x243 image = 256 tiles, one per CU); halo pixels of the hidden
 * layers are recomputed per tile (x1.6), so large batches stay on the per-layer launches.  b1 / b2 16-byte aligned. */
int srx_srcnn_forward(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                      const float* w3, const float* b3, float* y, int N, int H, int W, srx_stream_t stream);

/* Inverse map (HR image -> sub-pixel label layout): in [N,H*r,W*r,C] -> out [N,H,W,C*r*r].
 * Replaces espcn/espcn/dataset.py:140-156 and espcn/espcn/experiment_test.py:91-96. */
int srx_space_to_depth(const float* in, float* out, int N, int H, int W, int C, int r,
                       srx_stream_t stream);

/* tf.losses.mean_squared_error(reduction=MEAN) forward + gradient:
 *   *loss_out (+)= sum((pred-target)^2) * inv_numel     (device scalar; accumulate != 0 adds)
 *   dpred      = 2 * (pred-target) * inv_numel          (dpred nullable)
 * vdsr/vdsr/model_vdsr.py:120-123, espcn/espcn/model_espcn.py:76-77.
 * scratch: >= srx_reduce_scratch_bytes() bytes of device memory. */
int srx_mse_fwd_bwd(const float* pred, const float* target, size_t numel, float inv_numel,
                    float* loss_out, int accumulate, float* dpred, void* scratch,
                    srx_stream_t stream);

/* *loss_out (+)= scale * sum(mask * w^2)/2  -- sum over kernels of
 * tf.contrib.layers.l2_regularizer(scale)(w), vdsr/vdsr/model_vdsr.py:34,125.
 * mask (nullable) has w's shape: 1 for regularised elements (kernels), 0 otherwise (biases), so
 * one launch covers a model's whole flat parameter buffer. */
int srx_l2_loss(const float* w, const float* mask, size_t numel, float scale, float* loss_out,
                int accumulate, void* scratch, srx_stream_t stream);

size_t srx_reduce_scratch_bytes(void);

/* TF-1.x AdamOptimizer._apply_dense over a flat parameter buffer ("epsilon hat"):
 *   lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m=b1*m+(1-b1)*g; v=b2*v+(1-b2)*g*g;
 *   w -= lr_t*m/(sqrt(v)+eps);  g is multiplied by grad_scale first (1/world for DP sums).
 * t = 1-based step.  vdsr/vdsr/model_vdsr.py:145-148; espcn/espcn/model_espcn.py:87-89;
 * srcnn/srcnn.py:155-157 (b1 .5, b2 .9). */
int srx_adam_tf_step(float* w, const float* g, float* m, float* v, size_t numel, float lr,
                     float beta1, float beta2, float eps, int64_t t, float grad_scale,
                     srx_stream_t stream);

/* The same update with the step count and the learning rate in DEVICE memory, so that a whole train step captured as a
 * HIP graph replays without a per-step kernel argument (ESPCN / SRCNN steps are a dozen launches of ~10 us:
 * espcn/makefile:30-36 trains 1.6 M of them).  `state` is 32 bytes of 16-byte-aligned device memory owned by the caller:
 *   { int64 t;      steps applied so far (0 before the first); the kernel uses t + 1 and advances it
 *     float lr;     the fed learning rate (the caller rewrites it when its schedule changes it)
 *     float lr_t;   out: the bias-corrected rate the last step used
 *     uint32 done, pad;   zero-initialised scratch }
 * lr_t = lr*sqrt(1-b2^(t+1))/(1-b1^(t+1)) is evaluated on the device in double precision, the expression of
 * srx_adam_tf_step.  Steps on one state block must be ordered on one stream. */
int srx_adam_tf_step_dev(float* w, const float* g, float* m, float* v, size_t numel, void* state,
                         float beta1, float beta2, float eps, float grad_scale, srx_stream_t stream);

/* tf.train.MomentumOptimizer(lr, mom) on gradients clipped element-wise to +-cap:
 *   g=clip(g*grad_scale,-cap,cap); acc=mom*acc+g; w-=lr*acc.
 * vdsr/vdsr/model_vdsr.py:158-184 (cap = 0.01/lr). */
int srx_momentum_clip_step(float* w, const float* g, float* acc, size_t numel, float lr,
                           float momentum, float cap, float grad_scale, srx_stream_t stream);

/* SRCNN's loss (srcnn/srcnn.py:142-144): rows = reshape(pred - target, [-1, row_len]);
 *   *loss_out = mean_rows( ||row||_2 )        dpred = d / (||row||_2 * rows)   (dpred nullable)
 * (the reference reshapes to [-1, bb*bb], so a row mixes channels: 3 rows per RGB image).
 * row_norms: caller-owned device scratch of `rows` floats. */
int srx_rownorm_loss_fwd_bwd(const float* pred, const float* target, size_t rows, size_t row_len,
                             float* loss_out, float* dpred, float* row_norms, srx_stream_t stream);

/* tf.image.psnr(a,b,max_val) per image: out[n] = 20log10(max) - 10log10(mean((a-b)^2)).
 * vdsr/vdsr/experiment_train.py:80-82, vdsr/vdsr/experiment_evaluate.py:57-60. */
int srx_psnr(const float* a, const float* b, float* out, int N, size_t per_image, float max_val,
             srx_stream_t stream);

/* tf.image.ssim(a, b, max_val) per image (TF-1.8 defaults: 11x11 gaussian window sigma 1.5, k1 .01,
 * k2 .03, VALID windows, mean over positions then channels):
 *   out[n] = mean_c mean_{oh,ow} [ (2 mu_a mu_b + c1)/(mu_a^2 + mu_b^2 + c1) *
 *                                  (2 cov_ab + c2)/(var_a + var_b + c2) ],  c_i = (k_i max_val)^2
 * a, b: [N,H,W,C] with H, W >= 11.  scratch: >= srx_ssim_scratch_bytes(N) bytes.
 * vdsr/vdsr/experiment_evaluate.py:57-60, vdsr/vdsr/experiment_resolve.py, espcn/espcn/experiment_test.py:55. */
int srx_ssim(const float* a, const float* b, float* out, int N, int H, int W, int C, float max_val,
             void* scratch, srx_stream_t stream);
size_t srx_ssim_scratch_bytes(int N);

/* PSNR and SSIM of up to four candidates against one reference image in two launches, whatever N and n_cand: what the
 * evaluation scripts ask per image -- (hd, sd) and (hd, sr), tf.image.psnr and tf.image.ssim each
 * (vdsr/vdsr/experiment_evaluate.py:57-60), and ESPCN's scores of the sub-pixel arrangement
 * (espcn/espcn/experiment_test.py:32-55).  ref and every cand[k]: [N,H,W,C] fp32, dense.
 *   unit_clip 1: every value is first mapped x -> min(max(x * 0.5 + 0.5, 0), 1)        (experiment_test.py:32-36)
 *   space SRX_SCORES_RGB: the effective image is [H, We = W, Ce = C];
 *   space SRX_SCORES_Y (C % 3 == 0): the row of W*C floats is read as [We = W*C/3, 3] and Y = 0.299 R + 0.587 G + 0.114 B
 *     is kept, Ce = 1 -- the reference's reshape [h,w,3r^2] -> [h,w*r^2,3] reinterprets contiguous memory
 *     (experiment_test.py:39-52), so no data moves.
 *   out[k][n][0] = srx_psnr's formula over the H*We*Ce effective values (+inf for identical images),
 *   out[k][n][1] = srx_ssim's formula on the effective image (11x11 window, sigma 1.5, VALID, c_i = (k_i max_val)^2, mean
 *     over positions then channels).
 * out: [n_cand][N][2] floats.  cand: a HOST array of n_cand device pointers.  scratch: >= srx_image_scores_scratch_bytes(d)
 * bytes, 4-byte aligned; its contents before the call never matter, and the result is deterministic (no atomics: a tile's
 * workgroup writes its partial sums to its own slot, a finish launch adds an image's slots in a fixed order in double).
 * A workgroup owns a tile of tile_h x tile_w window positions (tile_w counted in floats of the effective row, i.e. window
 * columns x channels); the 11x11 window is computed separably through LDS and ref's moments are shared by the
 * candidates.  Refused before any launch, with the reason in srx_last_error(): a null d / ref / cand / out / scratch or
 * cand[k]; N outside 1..65535 (one grid row per image); C < 1; n_cand outside 1..SRX_SCORES_MAX_CAND; space outside
 * {0, 1}; Y with C % 3 != 0; unit_clip outside {0, 1}; H < 11 or We < 11; max_val NaN, infinite or <= 0; Ce above
 * SRX_SCORES_MAX_TAP_STRIDE (the halo of 10 Ce columns must fit the LDS); H or W*C above 0x7fff0000, or more than 2^31 - 1
 * tiles per image (sizes that overflow the kernel's 32-bit indices). */
#define SRX_SCORES_MAX_CAND 4
#define SRX_SCORES_RGB 0      /* score the channels as they are */
#define SRX_SCORES_Y   1      /* C % 3 == 0: read [H,W,C] as [H, W*C/3, 3], keep Y = 0.299 R + 0.587 G + 0.114 B */
#define SRX_SCORES_MAX_TAP_STRIDE 46
typedef struct srx_scores_desc {
    int32_t N, H, W, C;
    int32_t n_cand;           /* 1..SRX_SCORES_MAX_CAND */
    int32_t space;            /* SRX_SCORES_RGB / SRX_SCORES_Y */
    int32_t unit_clip;        /* 1: x -> min(max(x*0.5 + 0.5, 0), 1) first (espcn/espcn/experiment_test.py:32-36) */
    float   max_val;
} srx_scores_desc;
/* Host only.  Scratch bytes of srx_image_scores: N * n_cand * tiles_y * tiles_x * 2 floats (per image, candidate and tile:
 * the sum of squared errors and the sum of SSIM values).  0 with the reason in srx_last_error() when d is refused. */
size_t srx_image_scores_scratch_bytes(const srx_scores_desc* d);
/* Host only.  The tile (window rows, window columns x channels) and the tile counts of one image: tiles_y * tile_h covers
 * the H - 10 window rows, tiles_x * tile_w the (We - 10) * Ce window floats of a row.  The one place the launcher and the
 * scratch size take them from. */
int srx_image_scores_plan(const srx_scores_desc* d, int* tile_h, int* tile_w, int* tiles_y, int* tiles_x);
/* Host only.  The dynamic LDS of one workgroup of srx_image_scores in bytes, at most 160 KiB; 0 with the reason in
 * srx_last_error() when d is refused. */
size_t srx_image_scores_lds_bytes(const srx_scores_desc* d);
int srx_image_scores(const srx_scores_desc* d, const float* ref, const float* const* cand, float* out, void* scratch,
                     srx_stream_t stream);

/* Geometric self-ensemble (the "+" variants of the super-resolution literature): run the model on the eight flips and
 * transposes of the input, undo each on the result, average.  No reference counterpart: the reference has no such
 * option.  Transform k in 0..7 of an image x[H,W,C] is
 *   T_k(x) = flipH^(k&1)( flipV^((k>>1)&1)( transpose^((k>>2)&1)(x) ) )
 * transpose swaps rows and columns and keeps a pixel's C floats in order, flipV reverses rows, flipH reverses columns:
 * in numpy swapaxes(0,1) if bit 2, then [::-1] if bit 1, then [:, ::-1] if bit 0.
 *
 * srx_dihedral_expand: x [N,H,W,C] -> a [4N,H,W,C] with a[k*N+n] = T_k(x[n]) for k = 0..3, and b [4N,W,H,C] with
 *   b[(k-4)*N+n] = T_k(x[n]) for k = 4..7.  Transform-major: each group is an ordinary batch.  ONE launch: a workgroup
 *   reads its 32 x 32 pixel tile of x once and writes it to all eight images; the four transposed images go through a
 *   padded LDS tile, so every store is a contiguous run.  Plain copies: the same bits.
 * srx_dihedral_merge: H and W are those of out [N,H,W,C]; a [4N,H,W,C], b [4N,W,H,C] as above.
 *   out[n] = (((((((U_0 + U_1) + U_2) + U_3) + U_4) + U_5) + U_6) + U_7) * 0.125f,  U_k = T_k^-1(group[k])
 *   fp32 adds in exactly this order: deterministic, and restated bit for bit by sequential float32 adds.  ONE launch.
 * Both refuse before any launch, with the reason in srx_last_error(): a null pointer; N, H or W < 1; C outside
 * 1..SRX_DIHEDRAL_MAX_C; an output pointer equal to an input pointer (or a == b in expand); a pointer that is not
 * 4-byte aligned (SRX_ERR_ALIGN -- these two calls do NOT need 16-byte bases: a pixel of C = 3 has 12 bytes, and every
 * access is one float); more than 2^31 - 1 tiles of 32 x 32 pixels over the N images (the grid; element offsets
 * themselves are 64-bit in the kernels, so no smaller size is refused).  Any H and W, also below the tile and H != W. */
#define SRX_DIHEDRAL_MAX_C 8
int srx_dihedral_expand(const float* x, float* a, float* b, int N, int H, int W, int C, srx_stream_t stream);
int srx_dihedral_merge(const float* a, const float* b, float* out, int N, int H, int W, int C, srx_stream_t stream);

/* tf.saturate_cast(x*127.5+127.5, uint8): clamp to [0,255], truncate.
 * vdsr/vdsr/experiment_resolve.py:65-69, espcn/espcn/experiment_train.py:58. */
int srx_saturate_u8(const float* x, uint8_t* out, size_t numel, srx_stream_t stream);

/* The feature-map figure: the 64 maps of a layer as one 8 x 8 mosaic of bytes, channel k at tile row k / 8, tile
 * column k % 8, encoded as srx_saturate_u8 encodes (two roundings, clamp to [0,255], truncation):
 *   out[n, (k / 8) * H + y, (k % 8) * W + x] = saturate_cast<uint8>(x[n, y, x, k] * 127.5 + 127.5)
 * x [N,H,W,64] fp32 (16-byte aligned), out [N,8H,8W] uint8 at ANY byte alignment (a misaligned out only takes narrower
 * stores); out must not overlap x.  64 maps in rows of 8 and nothing else, as the reference's encoder is written:
 * split into 64, rows of 8 concatenated along the width, the rows along the height, saturate_cast
 * (vdsr/vdsr/experiment_feature_map_visualize.py:80-110).  One launch; a workgroup moves SRX_FEATURE_MOSAIC_TW pixels
 * of one image row. */
#define SRX_FEATURE_MOSAIC_TW 128
int srx_feature_mosaic_u8(const float* x, uint8_t* out, int N, int H, int W, srx_stream_t stream);

/* The image panel of the reference's TensorBoard summaries: n_src float tensors [N, H, W_i, 3*r*r] side by side along the
 * width, the batch stacked along the height, encoded to bytes in ONE launch that reads every source once:
 *   out [N*H*r, (W_0 + .. + W_{n_src-1})*r, 3] uint8, dense, at ANY byte alignment; it must not overlap a source.
 * r = 1: plain NHWC RGB sources (vdsr/vdsr/experiment_train.py:65-77, enet/enet/experiment_train.py:64-74,
 * srcnn/srcnn.py:169-192).  r = 2..4: ESPCN's label layout -- channel (dy*r + dx)*3 + ch of source pixel (n, y, x) lands
 * at out[(n*H + y)*r + dy, (W_before + x)*r + dx, ch] (espcn/espcn/experiment_train.py:47-56).
 * A source is a view: `row_pitch` floats between its rows and `image_pitch` between its images (0: dense), so a crop of
 * a larger tensor needs no copy; the W*3*r*r floats of a row are contiguous.
 * range_dev NULL: tf.saturate_cast(x*127.5 + 127.5, uint8), srx_saturate_u8's arithmetic.
 * range_dev set: TensorFlow 1.x's rescale of a FLOAT image (tf.summary.image): byte = (uint8)(x*scale + offset) with the
 *   {scale, offset} srx_summary_panel_range left there; a pixel with a non-finite channel becomes (255, 0, 0).
 * srx_summary_panel_range: min / max over the finite values of all sources (deterministic, no host round trip), then
 *   min < 0: m = max(|min|, |max|), scale = m < 1e-6 ? 0 : 127/m, offset = 128;  else scale = max < 1e-6 ? 0 : 255/max,
 *   offset = 0.  range_dev: srx_summary_panel_range_bytes() bytes of device memory, {scale, offset} first.
 * srx_summary_panel_bytes: the size of `out` (0 and srx_last_error() for arguments the panel refuses). */
#define SRX_SUMMARY_PANEL_MAX_SRC 8
#define SRX_SUMMARY_RANGE_BLOCKS 256
typedef struct srx_panel_src {
    const float* x;
    int32_t W;
    int32_t reserved;        /* 0 */
    int64_t row_pitch;       /* floats; 0: W*3*r*r */
    int64_t image_pitch;     /* floats; 0: H*row_pitch */
} srx_panel_src;
size_t srx_summary_panel_bytes(const srx_panel_src* srcs, int n_src, int N, int H, int r);
size_t srx_summary_panel_range_bytes(void);
int srx_summary_panel_u8(const srx_panel_src* srcs, int n_src, int N, int H, int r, const float* range_dev, uint8_t* out,
                         srx_stream_t stream);
int srx_summary_panel_range(const srx_panel_src* srcs, int n_src, int N, int H, int r, float* range_dev,
                            srx_stream_t stream);

/* out = a*x + b (elementwise); used for the [0,255] <-> [-1,1] maps at the model edge
 * (espcn/espcn/experiment_test.py:160,179). */
int srx_affine(const float* x, float* out, size_t numel, float a, float b, srx_stream_t stream);

/* ---- "next" row N1: on-device low-resolution synthesis (vdsr/vdsr/dataset.py:13-38,95-115) ---- */

/* skimage.util.img_as_float32 of uint8 data: out = in / 255. */
int srx_u8_to_unit_float(const uint8_t* in, float* out, size_t numel, srx_stream_t stream);

/* skimage.filters.gaussian(image, sigma, mode='nearest') on [N,H,W,C] (channels are not blurred):
 * separable 1-D kernels of radius int(4*sigma + 0.5), weights exp(-x^2/(2 sigma^2)) normalised, borders
 * replicated (scipy.ndimage.gaussian_filter, truncate 4.0).  tmp: N*H*W*C floats.  sigma <= 0 copies. */
int srx_gaussian_blur(const float* in, float* out, float* tmp, int N, int H, int W, int C, float sigma,
                      srx_stream_t stream);

/* skimage.transform.resize(image, [OH, OW], mode='edge', anti_aliasing=False) with order 1: bilinear
 * sampling at in = (out + 0.5) * (H / OH) - 0.5, coordinates clamped to the image.  [N,H,W,C] -> [N,OH,OW,C]. */
int srx_resize_bilinear(const float* in, float* out, int N, int H, int W, int C, int OH, int OW,
                        srx_stream_t stream);

/* ---- VDSR's training pairs sampled on the device from a resident image set (vdsr/vdsr/dataset.py:41-128) ---- */

/* One patch of a batch: which image of the arena, where the crop starts, whether it is mirrored, and the scaling factor
 * it is degraded with -- the random draws of vdsr/vdsr/dataset.py:59-63 (image), :96-97 (crop corner), :102 (flip), :109 (factor). */
typedef struct srx_patch_src {   /* 32 bytes */
    uint64_t offset;             /* byte offset of the image's pixel (0,0) in the arena; rows are width*3 bytes */
    int32_t width, height;       /* of that image */
    int32_t x, y;                /* top-left of the crop */
    int32_t flip;                /* 0 / 1: mirror along the width */
    float scaling_factor;        /* > 1 */
} srx_patch_src;

/* Pure host code, no GPU call: 0 if every entry of table_host[0..B) is safe to hand to srx_vdsr_patch_pairs with an arena
 * of arena_bytes bytes, else SRX_ERR_BAD_ARG with the entry and the reason in srx_last_error().  Refused: a null table,
 * B < 1, S outside 2..128, a crop that leaves its image (x < 0, y < 0, x + S > width, y + S > height), an image that
 * leaves the arena (offset + width*height*3 > arena_bytes), flip outside {0, 1}, a factor that is NaN, infinite or <= 1,
 * int(S / factor) < 1, and a blur radius int(4 * 0.5 (factor - 1) + 0.5) above 63 (srx_gaussian_blur's limit).  It stands
 * where the reference's size test and numpy slicing stand (vdsr/vdsr/dataset.py:90-99); the kernel trusts the table. */
int srx_vdsr_patch_table_check(const srx_patch_src* table_host, int B, int S, size_t arena_bytes);

/* One launch for a whole batch of (sd, hd) pairs, replacing vdsr/vdsr/dataset.py:99-123 per patch: the S x S x 3 uint8
 * crop at (x, y) of its image (:99), mirrored along the width first if flip (:102-103), hd01 = crop / 255
 * (img_as_float32, :106), sd01 = hd_image_to_sd_image(hd01, factor) (:111, :13-38) with the arithmetic of srx_gaussian_blur
 * and srx_resize_bilinear on the patch alone (borders are the patch's own), both mapped to [-1, 1] (:114-115) and stacked
 * (:122-123): sd, hd [B,S,S,3] fp32 in table order.  arena: the packed uint8 images; table_dev: a DEVICE copy of a table that passed srx_vdsr_patch_table_check for
 * this arena, B and S (the kernel does not check it again).  One workgroup per (entry, channel), intermediates in LDS
 * (256 + 8 S^2 bytes).  Null pointers, B < 1 and S outside 2..128 are refused before any launch. */
int srx_vdsr_patch_pairs(const uint8_t* arena, const srx_patch_src* table_dev, int B, int S,
                         float* sd, float* hd, srx_stream_t stream);

/* ---- ESPCN's training pairs sampled on the device from a resident image set (espcn/espcn/dataset.py:81-158) ----
 * r: the upscaling factor (2..4); p: the low-resolution patch side; P = p r <= 128 the high-resolution side.  A table is
 * srx_patch_src records read this way: offset / width / height name the image, (x, y) is the patch's top-left corner on
 * the grid of espcn/espcn/dataset.py:110-113; flip is a 2-bit field -- bit 0 mirrors along the width (v = -1), bit 1 along
 * the height (u = -1), the [::u, ::v] of :121-122; scaling_factor holds (float)r, so a table says what it was built for. */

/* Pure host code, no GPU call: 0 if every entry of table_host[0..n) is safe to hand to srx_espcn_patch_pairs with an arena
 * of arena_bytes bytes, else SRX_ERR_BAD_ARG with the entry and the reason in srx_last_error().  Refused: a null table,
 * n < 1, r outside 2..4, p < 1 or p r > 128, a patch that leaves its image (x < 0, y < 0, x + P > width, y + P > height),
 * an image that leaves the arena (offset + 3 width height > arena_bytes, formed without overflow), flip outside 0..3,
 * scaling_factor != r.  It stands where the reference's ranges and numpy slicing stand (espcn/espcn/dataset.py:110-118);
 * the kernel trusts the table. */
int srx_espcn_patch_table_check(const srx_patch_src* table_host, int n, int r, int p, size_t arena_bytes);

/* One launch for a whole batch of (lr, label) pairs, replacing espcn/espcn/dataset.py:94-156 per patch:
 *   hr = u8 / 127.5 - 1 in float64, written as float32 (:94);
 *   bl = gaussian blur of the WHOLE image, sigma = 0.5 (r - 1), radius int(4 sigma + 0.5), borders replicated at the
 *        image's edge (:97-101), with srx_gaussian_blur's arithmetic, evaluated only where it is sampled;
 *   lr[i, j, c] = bl[y + r/2 + r i', x + r/2 + r j', c], i' = p-1-i if flip & 2, j' = p-1-j if flip & 1 (:116-118, :122);
 *   label[i, j, (dy r + dx) 3 + c] = hr_f[i r + dy, j r + dx, c], hr_f the P x P patch at (x, y) with its rows reversed
 *        if flip & 2 and its columns if flip & 1 (:114, :121, :140-156); bit for bit the float64 value cast to float32.
 * lr [B,p,p,3] and label [B,p,p,3 r^2] fp32 in table order.  arena: the packed uint8 images; table_dev: B consecutive
 * DEVICE records of a table that passed srx_espcn_patch_table_check for this arena, r and p (the kernel does not check
 * them again).  One workgroup per entry, intermediates in LDS (1088 + 3 (P + 2R)^2 + 12 p (r (p-1) + 1 + 2R) bytes).
 * Null pointers, B < 1, r outside 2..4, p < 1 and p r > 128 are refused before any launch. */
int srx_espcn_patch_pairs(const uint8_t* arena, const srx_patch_src* table_dev, int B, int r, int p,
                          float* lr, float* label, srx_stream_t stream);

/* ---- ESPCN's evaluation pairs of a whole image set built on the device (espcn/espcn/experiment_test.py:60-98) ----
 * The decoded images of a set lie in one uint8 arena, each already trimmed to multiples of r (:68-71: the reference trims
 * first and blurs then, so the blur's replicated border is the trimmed edge).  One launch writes, for image k with
 * h' = height / r and w' = width / r, at lr + lr_offset and label + lr_offset r^2:
 *   lr    [h', w', 3]      lr[i, j, c] = bl[r/2 + r i, r/2 + r j, c], bl the gaussian blur of the trimmed image mapped to
 *                          [-1, 1]: sigma = 0.5 (r - 1), radius int(4 sigma + 0.5), borders replicated (:73-85), with the
 *                          arithmetic of srx_gaussian_blur and srx_espcn_patch_pairs, evaluated only where it is sampled;
 *   label [h', w', 3 r^2]  label[i, j, (dy r + dx) 3 + c] = (float)((double)u8[i r + dy, j r + dx, c] / 127.5 - 1.0) (:91-96).
 * A patch of srx_espcn_patch_pairs with flip 0 at (x, y) of an image whose sides are multiples of r holds the same bits as
 * lr[y/r .. y/r + p, x/r .. x/r + p] and the label likewise. */

#define SRX_ESPCN_EVAL_TILE 16   /* one workgroup builds a tile of this many lr pixels on a side */

typedef struct srx_eval_image {   /* 32 bytes */
    uint64_t offset;              /* arena byte offset of pixel (0,0); rows are width*3 bytes */
    int32_t width, height;        /* of the trimmed image: multiples of r, each >= r */
    uint64_t lr_offset;           /* floats: lr of this image starts at lr + lr_offset, its label at label + lr_offset*r*r */
    uint32_t first_tile;          /* tiles of the images before it */
    uint32_t reserved;            /* 0 */
} srx_eval_image;

/* Pure host code, no GPU call, and the only bound between a table and the kernel's reads and writes: 0 if
 * table_host[0..n) is safe to hand to srx_espcn_eval_pairs with an arena of arena_bytes bytes and outputs of lr_floats
 * and lr_floats r^2 floats, else SRX_ERR_BAD_ARG with the entry and the reason in srx_last_error().  Refused: a null
 * table, n < 1, r outside 2..4, a width or height below r or not a multiple of r, an image that leaves the arena
 * (offset + 3 width height > arena_bytes, formed without overflow), reserved != 0, an lr_offset that is not the sum of
 * 3 (height/r) (width/r) over the entries before it, a first_tile that is not the sum of their tiles
 * (ceil(h'/T) ceil(w'/T), T = SRX_ESPCN_EVAL_TILE) -- the outputs are packed in table order, so no two images' outputs
 * overlap -- more than 2^31 - 1 tiles, and a total of lr floats other than lr_floats. */
int srx_espcn_eval_table_check(const srx_eval_image* table_host, int n, int r, size_t arena_bytes, size_t lr_floats);

/* Host only.  The tiles of table_host[0..n): the sum of ceil(h'/T) ceil(w'/T).  0 with the reason in srx_last_error()
 * for a null table, n < 1, r outside 2..4, a size below r or not a multiple of r, or more than 2^31 - 1 tiles. */
size_t srx_espcn_eval_tiles(const srx_eval_image* table_host, int n, int r);

/* The launch.  arena: the packed uint8 images; table_dev: a DEVICE copy of n records that passed
 * srx_espcn_eval_table_check for this arena, r and the sizes of lr and label (the kernel does not check them again).
 * Each tile of T x T lr pixels of an image is built by one workgroup alone; a workgroup finds a tile's image from
 * first_tile, stages the tile's bytes with a halo of the radius in LDS (indices clamped to the image), and stores only
 * i < h', j < w'.  The table being on the device, the grid has a fixed size and its workgroups stride over the tiles.
 * No atomics, no communication between workgroups, plain vector stores; 1088 + 3 (T r + 2R)^2 + 12 T (r (T-1) + 1 + 2R)
 * bytes of LDS.  Null pointers, n < 1, r outside 2..4 and lr == label are refused before any launch. */
int srx_espcn_eval_pairs(const uint8_t* arena, const srx_eval_image* table_dev, int n, int r,
                         float* lr, float* label, srx_stream_t stream);

/* ---- VDSR's evaluation pairs of a whole image set built on the device (vdsr/vdsr/experiment_evaluate.py:14-33) ----
 * The decoded images of a set lie in one uint8 arena; a record names an image and ONE scaling factor s, so a set that
 * serves x2, x3 and x4 holds three records per image.  One launch writes, for record k of a height x width image, at
 * sd + out_offset and hd + out_offset, two [height, width, 3] fp32 images:
 *   hd = (float)u8 / 255.0f * 2 - 1, the bits of srx_u8_to_unit_float followed by srx_affine(2, -1);
 *   sd = hd_image_to_sd_image (vdsr/vdsr/dataset.py:13-38) of the WHOLE image, times 2 minus 1: gaussian blur with
 *        sigma = 0.5 (s - 1), radius int(4 sigma + 0.5), along H then along W, borders replicated at the image's edge;
 *        bilinear resize to (int(height / s), int(width / s)) and back, half-pixel coordinates clamped to the image --
 *        the arithmetic of srx_gaussian_blur, srx_resize_bilinear and srx_vdsr_patch_pairs (every product and sum
 *        rounded on its own; the coordinates may differ from srx_resize_bilinear's in the last bit).
 * A record's start is rounded up to a multiple of 4 floats, so every record's view is 16-byte aligned when sd and hd
 * are; the padding floats between records are never written. */

#define SRX_VDSR_EVAL_TILE 32    /* one workgroup builds a tile of this many hd pixels on a side */

typedef struct srx_vdsr_eval_image {   /* 32 bytes */
    uint64_t offset;              /* arena byte offset of pixel (0,0); rows are width*3 bytes */
    int32_t width, height;
    uint64_t out_offset;          /* floats: this record's sd starts at sd + out_offset, its hd at hd + out_offset */
    uint32_t first_tile;          /* tiles of the records before it */
    float scaling_factor;         /* this record's s */
} srx_vdsr_eval_image;

/* Pure host code, no GPU call, and the only bound between a table and the kernel's reads and writes: 0 if
 * table_host[0..n) is safe to hand to srx_vdsr_eval_pairs with an arena of arena_bytes bytes and outputs of out_floats
 * floats each, else SRX_ERR_BAD_ARG with the entry and the reason in srx_last_error().  Refused: a null table, n < 1, a
 * width or height below 1, an s that is not finite or outside (1, 8], int(height / s) or int(width / s) below 1, an image
 * that leaves the arena (offset + 3 width height > arena_bytes, formed without overflow), an out_offset that is not the
 * padded running sum (each record's 3 width height floats, its start rounded up to a multiple of 4), a first_tile that is
 * not the sum of ceil(height / T) ceil(width / T) over the records before it (T = SRX_VDSR_EVAL_TILE), more than
 * 2^31 - 1 tiles, a record one of whose tiles reaches more than the kernel's LDS layout holds (every tile row and tile
 * column is walked: ceil(height / T) + ceil(width / T) footprints per record), and a total (the last record's end,
 * unpadded) other than out_floats. */
int srx_vdsr_eval_table_check(const srx_vdsr_eval_image* table_host, int n, size_t arena_bytes, size_t out_floats);

/* Host only.  The tiles of table_host[0..n): the sum of ceil(height / T) ceil(width / T).  0 with the reason in
 * srx_last_error() for a null table, n < 1, a size below 1 or more than 2^31 - 1 tiles. */
size_t srx_vdsr_eval_tiles(const srx_vdsr_eval_image* table_host, int n);

/* Host only, for tests: what tile `tile` of an axis of `side` hd pixels reaches at scaling factor s, by the function the
 * table check and the kernel's pixel loops share.  out = {first, last low-resolution index its up-resize taps name;
 * first, last blurred index the down-resize taps of those name; first, last source index the blur of those reads,
 * clamped to the image}, all inclusive.  tests/test_vdsr_eval_host.py compares it with a brute-force enumeration of
 * every pixel's taps.  SRX_ERR_BAD_ARG for a null out, side < 1, an s outside (1, 8], int(side / s) < 1 or a tile
 * outside 0 .. ceil(side / T) - 1. */
int srx_vdsr_eval_footprint(int side, float s, int tile, int out[6]);

/* The launch.  arena: the packed uint8 images; table_dev: a DEVICE copy of n records that passed
 * srx_vdsr_eval_table_check for this arena and the size of sd and hd (the kernel does not check them again).  Each tile
 * of T x T hd pixels of a record is built by one workgroup alone: it finds the tile's record from first_tile, stages the
 * source bytes the tile reaches in LDS, blurs along H at the rows the down-resize samples, blurs along W at the sampled
 * columns as it forms the tile's low-resolution pixels, and up-resizes those; consecutive lanes store consecutive floats
 * of a row.  The table being on the device, the grid has a fixed size and its workgroups stride over the tiles.  No
 * atomics, no communication between workgroups, plain vector stores; 40 KiB of LDS.  Null pointers, n < 1 and sd == hd
 * are refused before any launch. */
int srx_vdsr_eval_pairs(const uint8_t* arena, const srx_vdsr_eval_image* table_dev, int n,
                        float* sd, float* hd, srx_stream_t stream);

/* ---- EnhanceNet's training batches sampled on the device from a resident image set (enet/enet/datasets.py:79-127) ----
 * S: the side of the hd crop, a multiple of 4 in 4..128 (the reference's 128, :110); s = S / 4 the side of sd.  A table
 * is srx_patch_src records read this way: offset / width / height name the image, (x, y) is the crop's top-left corner
 * (the two np.random.randint(128) of :107-108); flip is a 2-bit field -- bit 1 reverses the crop's rows, bit 0 its columns,
 * the augmentation of the reference's unused build_image_batch_iterator (:66-68), 0 on its used path; scaling_factor
 * holds 4.0f, so a table says what it was built for. */

/* Host only.  The number of int32 words of the coefficient block srx_enet_pairs_tables writes for S, or -1 (S not a
 * multiple of 4 in 4..128). */
int srx_enet_pairs_table_words(int S);

/* Host only, no GPU call: Pillow's coefficients for the two resizes of enet/enet/datasets.py:112-113 in one int32 block
 * of srx_enet_pairs_table_words(S) words at words_host: the S -> s BILINEAR table (imresize(hd, 25): 9 taps), then the
 * s -> S BICUBIC one (imresize(sd, 400, 'bicubic'): 5 taps); each table is its bounds [out][2] = (first input index,
 * count) followed by its kk [out][ksize] -- the arrays of srx_pil_resample_coeffs, which builds them.  A square crop's
 * horizontal and vertical pass share a table.  The caller uploads the block once per S. */
int srx_enet_pairs_tables(int S, int32_t* words_host);

/* Pure host code, no GPU call: 0 if every entry of table_host[0..B) is safe to hand to srx_enet_patch_pairs with an arena
 * of arena_bytes bytes, else SRX_ERR_BAD_ARG with the entry and the reason in srx_last_error().  Refused: a null table,
 * B < 1, S not a multiple of 4 or outside 4..128, a crop that leaves its image (x < 0, y < 0, x + S > width,
 * y + S > height), an image that leaves the arena (offset + 3 width height > arena_bytes, formed without overflow), flip
 * outside 0..3, scaling_factor != 4.  It stands where the reference's numpy slicing stands (enet/enet/datasets.py:107-110);
 * the kernel trusts the table. */
int srx_enet_patch_table_check(const srx_patch_src* table_host, int B, int S, size_t arena_bytes);

/* One launch for a whole batch of (sd, bq, hd) triples, replacing enet/enet/datasets.py:104-125 per image:
 *   hd_u8 = the S x S x 3 crop at (x, y) of the entry's image (:107-110), rows reversed if flip & 2, columns if flip & 1
 *           (:66-68), the flips applied to the crop before anything else;
 *   sd_u8 = Pillow BILINEAR of hd_u8 to s x s (:112, imresize(hd, 25): antialiased, support 4);
 *   bq_u8 = Pillow BICUBIC (a = -0.5) of sd_u8 to S x S (:113, imresize(sd, 400, 'bicubic'));
 *   each resize in Pillow's two passes, horizontal then vertical, each clip8((2^21 + sum kk[k] in[xmin + k]) >> 22) with a
 *   uint8 intermediate: the bytes of srx_resample_u8;
 *   sd [B,s,s,3], bq [B,S,S,3], hd [B,S,S,3] fp32 = (float)u8 / 127.5f - 1.0f, two roundings as srx_u8_to_pm1 (:115-117),
 *   in table order.
 * arena: the packed uint8 images; table_dev: B consecutive DEVICE records of a table that passed
 * srx_enet_patch_table_check for this arena and S; tables_dev: a DEVICE copy of the block srx_enet_pairs_tables wrote
 * for this S.  The kernel checks neither again: it trusts both.  One workgroup per entry, intermediates in LDS (1024 +
 * 28 S + 44 s + 3 S^2 + 6 S s + 3 s^2 bytes: 80.9 KiB at S = 128).  Null pointers, B < 1, S not a multiple of 4 or outside
 * 4..128 and outputs that are not three distinct pointers are refused before any launch. */
int srx_enet_patch_pairs(const uint8_t* arena, const srx_patch_src* table_dev, int B, int S, const int32_t* tables_dev,
                         float* sd, float* bq, float* hd, srx_stream_t stream);

/* ---- EnhanceNet's evaluation pairs of a whole image set built on the device (enet/enet/datasets.py:95-127) ----
 * The training degradation of enet/enet/datasets.py:95-127 applied to WHOLE images: the decoded images of a set lie in one
 * uint8 arena, each already trimmed at the bottom and right to multiples of 4 (the top-left pixel stays).  One launch
 * writes, for record k of a height x width image (h = height / 4, w = width / 4):
 *   hd [height, width, 3] at hd + out_offset: (float)u8 / 127.5f - 1.0f, the two roundings of srx_u8_to_pm1;
 *   sd [h, w, 3] at sd + sd_offset: Pillow BILINEAR (antialiased) of the whole image to (h, w), the same float map;
 *   bq [height, width, 3] at bq + out_offset: Pillow BICUBIC (a = -0.5) of sd's bytes back to (height, width), the same map.
 * Each resize is Pillow's two passes, horizontal then vertical, each clip8((2^21 + sum kk[k] in[first + k]) >> 22) with an
 * arithmetic shift and a uint8 intermediate: the bytes of srx_resample_u8 and of srx_enet_patch_pairs.  A record's start
 * is rounded up to a multiple of 4 floats in all three outputs, so every view is 16-byte aligned when the outputs are; the
 * padding floats between records are never written.
 * The coefficients of an axis of `side` pixels are a BLOCK of int32 words: word 0 holds `side`, then follows the block of
 * srx_enet_pairs_tables' layout for S = side (side -> side / 4 BILINEAR bounds [side/4][2] and kk [side/4][9], then
 * side / 4 -> side BICUBIC bounds [side][2] and kk [side][5]).  A coefficient ARENA is blocks back to back, one per distinct
 * side of a set; a record names the blocks of its width and of its height by their word offsets.  The side in word 0 is how
 * srx_enet_eval_table_check tells that a record's blocks were built for its sides. */

#define SRX_ENET_EVAL_TILE 32    /* one workgroup builds a tile of this many hd pixels on a side; a multiple of 4 */

typedef struct srx_enet_eval_image {   /* 48 bytes */
    uint64_t offset;              /* arena byte offset of pixel (0,0); rows are width*3 bytes */
    int32_t width, height;        /* of the trimmed image: multiples of 4, each >= 12 */
    uint64_t out_offset;          /* floats: this record's hd starts at hd + out_offset, its bq at bq + out_offset */
    uint64_t sd_offset;           /* floats: this record's sd starts at sd + sd_offset */
    uint32_t first_tile;          /* tiles of the records before it */
    uint32_t width_coeffs;        /* word offset in the coefficient arena of the block of `width` */
    uint32_t height_coeffs;       /* word offset of the block of `height` */
    uint32_t reserved;            /* 0 */
} srx_enet_eval_image;

/* Host only (enet/enet/datasets.py:95-127).  The int32 words of the coefficient block of an axis of `side` pixels:
 * 1 + 39 side / 4, or -1 (side not a multiple of 4 in 4..2^20). */
int srx_enet_eval_coeff_words(int side);

/* Host only, no GPU call (enet/enet/datasets.py:95-127: imresize(hd, 25) and imresize(sd, 400, 'bicubic') along one axis).
 * Writes the block of `side` (a multiple of 4 in 4..2^20) at out[0 .. srx_enet_eval_coeff_words(side)): `side`, then the
 * arrays of srx_pil_resample_coeffs in srx_enet_pairs_tables' layout.  Unlike srx_enet_pairs_tables the side is not capped
 * at 128, and an image with height != width uses two blocks.  Refuses if Pillow's window sizes for the ratio 4 are not 9
 * and 5 at this side. */
int srx_enet_eval_coeffs(int side, int32_t* out);

/* Pure host code, no GPU call, and the only bound between a table and the kernel's reads and writes
 * (enet/enet/datasets.py:95-127): 0 if table_host[0..n) is safe to hand to srx_enet_eval_pairs with an arena of arena_bytes
 * bytes, hd and bq of out_floats floats, sd of sd_floats floats and a device copy of the coefficient arena
 * coeffs_host[0..coeff_words), else SRX_ERR_BAD_ARG with the entry and the reason in srx_last_error().  Refused: a null
 * table or arena of coefficients, n < 1, a side below 12, above 2^20 or not a multiple of 4, an image that leaves the arena
 * (offset + 3 width height > arena_bytes, formed without overflow), reserved != 0, an out_offset or sd_offset that is not
 * the padded running sum (each record's floats, its start rounded up to a multiple of 4), a first_tile that is not the sum
 * of ceil(height / T) ceil(width / T) over the records before it (T = SRX_ENET_EVAL_TILE), more than 2^31 - 1 tiles, a
 * coefficient offset whose block leaves coeff_words or whose first word is not the record's side, a block whose bounds
 * are not Pillow's in shape (a count outside 1..ksize, an index outside the input, a first index or an end that decreases),
 * a tile whose footprint leaves the image or does not hold the tile's own pixels, or exceeds the kernel's LDS layout
 * (every tile row and tile column is walked), and totals (the last record's end, unpadded) other than out_floats and
 * sd_floats. */
int srx_enet_eval_table_check(const srx_enet_eval_image* table_host, int n, size_t arena_bytes, size_t out_floats,
                              size_t sd_floats, const int32_t* coeffs_host, size_t coeff_words);

/* Host only (enet/enet/datasets.py:95-127).  The tiles of table_host[0..n): the sum of ceil(height / T) ceil(width / T).
 * 0 with the reason in srx_last_error() for a null table, n < 1, a side that the check refuses or more than 2^31 - 1 tiles. */
size_t srx_enet_eval_tiles(const srx_enet_eval_image* table_host, int n);

/* Host only, for tests (enet/enet/datasets.py:95-127): what tile `tile` of an axis of `side` hd pixels reaches, read from
 * the bounds tables the table check and the kernel's pixel loops use -- nothing is derived in floating point here.
 * out = {first, last sd index the BICUBIC taps of the tile's hd range name; first, last hd index the BILINEAR taps of those
 * name}, all inclusive.  SRX_ERR_BAD_ARG for a null out, a side the check refuses or a tile outside
 * 0 .. ceil(side / T) - 1. */
int srx_enet_eval_footprint(int side, int tile, int out[4]);

/* The launch (enet/enet/datasets.py:95-127 per image, for a whole set).  arena: the packed uint8 images; table_dev: a
 * DEVICE copy of n records that passed srx_enet_eval_table_check for this arena, the sizes of sd, bq and hd and the
 * coefficient arena of which coeffs_dev is a DEVICE copy (the kernel checks none of them again).  Each tile of T x T hd
 * pixels of a record is built by one workgroup alone: it finds the tile's record from first_tile, stages the hd bytes the
 * tile reaches and the coefficient slices of its two axes in LDS, and runs the four passes there; consecutive lanes store
 * consecutive floats of a row.  The table being on the device, the grid has a fixed size and its workgroups stride over
 * the tiles.  No atomics, no communication between workgroups, plain vector stores; 40 KiB of LDS.  Null pointers, n < 1
 * and outputs that are not three distinct pointers are refused before any launch. */
int srx_enet_eval_pairs(const uint8_t* arena, const srx_enet_eval_image* table_dev, int n, const int32_t* coeffs_dev,
                        float* sd, float* bq, float* hd, srx_stream_t stream);

/* ---- SRCNN's training batches sampled on the device from a resident image set (srcnn/srcnn.py:46-93, :132-136) ----
 * S: the side of the crop, 2..256 (the reference's 243); f: the integer upscaling factor, f >= 2 and s = S / f >= 1
 * (integer division) the side of the low-resolution image; border: the margin the VALID network removes from the ground
 * truth, 0 <= 2 border < S (the reference's 6).  A table is srx_patch_src records read this way: offset / width / height
 * name the image, (x, y) is the crop's top-left corner (:60-61), flip 1 reverses the crop's columns (:62);
 * scaling_factor holds (float)f, so a table says what it was built for. */

/* Host only.  The number of output rows one workgroup of srx_srcnn_patch_pairs builds (a band), or -1 (S outside 2..256,
 * f < 2 or S / f < 1).  The bands [k band, min(S, (k + 1) band)) cover [0, S). */
int srx_srcnn_pairs_band(int S, int f);

/* Host only.  The dynamic LDS of one workgroup of srx_srcnn_patch_pairs in bytes, at most 160 KiB, or -1 (as above). */
int srx_srcnn_pairs_lds_bytes(int S, int f);

/* Pure host code, no GPU call: 0 if every entry of table_host[0..B) is safe to hand to srx_srcnn_patch_pairs with an
 * arena of arena_bytes bytes, else SRX_ERR_BAD_ARG with the entry and the reason in srx_last_error().  Refused: a null
 * table, B < 1, S outside 2..256, f < 2 or S / f < 1, border < 0 or 2 border >= S, a crop that leaves its image (x < 0,
 * y < 0, x + S > width, y + S > height), an image that leaves the arena (offset + 3 width height > arena_bytes, formed
 * without overflow), width or height below 1, flip outside {0, 1}, scaling_factor != f.  It stands where the reference's
 * random_crop stands (srcnn/srcnn.py:60-61); the kernel trusts the table. */
int srx_srcnn_patch_table_check(const srx_patch_src* table_host, int B, int S, int f, int border, size_t arena_bytes);

/* One launch for a whole batch of (sd, hd) pairs, replacing per step the host-built batch, its upload, two
 * srx_resize_bicubic_tf launches and the border slice:
 *   crop    = the S x S x 3 bytes at (x, y) of the entry's image, columns reversed if flip;
 *   hd_full = (float)crop / 127.5f - 1.0f, two roundings as srx_u8_to_pm1;
 *   lo      = srx_resize_bicubic_tf(hd_full) to s x s, sd = srx_resize_bicubic_tf(lo) to S x S, bit for bit;
 *   hd      = hd_full without `border` pixels all round (srcnn/srcnn.py:132-136).
 * sd [B,S,S,3] and hd [B,S-2 border,S-2 border,3] fp32 in table order.  arena: the packed uint8 images; table_dev: B
 * consecutive DEVICE records of a table that passed srx_srcnn_patch_table_check for this arena, S, f and border (the
 * kernel does not check them again).  One workgroup per (entry, band of srx_srcnn_pairs_band rows), intermediates in LDS
 * (srx_srcnn_pairs_lds_bytes).  Null pointers, sd == hd, B < 1 and S, f or border outside the limits above are refused
 * before any launch. */
int srx_srcnn_patch_pairs(const uint8_t* arena, const srx_patch_src* table_dev, int B, int S, int f, int border,
                          float* sd, float* hd, srx_stream_t stream);

/* ---- SRCNN's evaluation pairs of a whole image set built on the device (srcnn/srcnn.py:89-93,132-139) ----
 * The in-graph degradation of srcnn/srcnn.py:89-93 applied to WHOLE images, and the margin of :132-139: the decoded images
 * of a set lie in one uint8 arena; f (2..8) is the integer upscaling factor and border >= 0 the margin the VALID network
 * removes (SrcnnModel.crop_side(), 6 for the 9-1-5 network), both the table's.  One launch writes, for record k of a
 * height x width image (h = height / f, w = width / f, integer division; b = border):
 *   sd [height, width, 3] at sd + out_offset: srx_resize_bicubic_tf(srx_resize_bicubic_tf(hd_full, h, w), height, width) of
 *      hd_full = (float)u8 / 127.5f - 1.0f (the two roundings of srx_u8_to_pm1), bit for bit: the network's input;
 *   bq [height - 2 b, width - 2 b, 3] at bq + crop_offset: sd without its margin, contiguous (the reference's sd_images);
 *   hd [height - 2 b, width - 2 b, 3] at hd + crop_offset: hd_full without its margin.
 * A record's start is rounded up to a multiple of 4 floats in all three outputs, so every view is 16-byte aligned when the
 * outputs are; the padding floats between records are never written. */

#ifndef SRX_SRCNN_EVAL_TILE
#define SRX_SRCNN_EVAL_TILE 32   /* one workgroup builds a tile of this many sd pixels on a side */
#endif

typedef struct srx_srcnn_eval_image {  /* 40 bytes */
    uint64_t offset;              /* arena byte offset of pixel (0,0); rows are width*3 bytes */
    int32_t width, height;        /* of the image: each with side / f >= 1 and side > 2 border */
    uint64_t out_offset;          /* floats: this record's sd starts at sd + out_offset */
    uint64_t crop_offset;         /* floats: this record's bq starts at bq + crop_offset, its hd at hd + crop_offset */
    uint32_t first_tile;          /* tiles of the records before it */
    uint32_t reserved;            /* 0 */
} srx_srcnn_eval_image;

/* Pure host code, no GPU call, and the only bound between a table and the kernel's reads and writes
 * (srcnn/srcnn.py:89-93,132-139): 0 if table_host[0..n) is safe to hand to srx_srcnn_eval_pairs with this f and border, an
 * arena of arena_bytes bytes, sd of out_floats floats and bq and hd of crop_floats floats each, else SRX_ERR_BAD_ARG with
 * the entry and the reason in srx_last_error().  Refused: a null table, n < 1, f outside 2..8, border < 0, a side with
 * side / f < 1 or side <= 2 border, an image that leaves the arena (offset + 3 width height > arena_bytes, formed without
 * overflow), reserved != 0, an out_offset or crop_offset that is not the padded running sum (each record's floats, its
 * start rounded up to a multiple of 4), a first_tile that is not the sum of ceil(height / T) ceil(width / T) over the
 * records before it (T = SRX_SRCNN_EVAL_TILE), more than 2^31 - 1 tiles, a record one of whose tiles reaches more than the
 * kernel's LDS layout holds (every tile row and tile column is walked), and totals (the last record's end, unpadded)
 * other than out_floats and crop_floats. */
int srx_srcnn_eval_table_check(const srx_srcnn_eval_image* table_host, int n, int f, int border, size_t arena_bytes,
                               size_t out_floats, size_t crop_floats);

/* Host only (srcnn/srcnn.py:89-93,132-139).  The tiles of table_host[0..n): the sum of ceil(height / T) ceil(width / T).
 * 0 with the reason in srx_last_error() for a null table, n < 1, a side below 1 or more than 2^31 - 1 tiles. */
size_t srx_srcnn_eval_tiles(const srx_srcnn_eval_image* table_host, int n);

/* Host only, for tests (srcnn/srcnn.py:89-93): what tile `tile` of an axis of `side` pixels reaches at the factor f,
 * through the function the table check and the kernel use.  out = {first, last low-resolution index the taps of the
 * tile's pixels name in the side / f -> side pass; first, last source index the taps of those name in the side -> side / f
 * pass}, all inclusive.  SRX_ERR_BAD_ARG for a null out, f outside 2..8, side / f < 1 or a tile outside
 * 0 .. ceil(side / T) - 1. */
int srx_srcnn_eval_footprint(int side, int f, int tile, int out[4]);

/* The launch (srcnn/srcnn.py:89-93,132-139 per image, for a whole set).  arena: the packed uint8 images; table_dev: a
 * DEVICE copy of n records that passed srx_srcnn_eval_table_check for this arena, f, border and the sizes of sd, bq and hd
 * (the kernel checks none of them again).  Each tile of T x T pixels of a record is built by one workgroup alone: it finds
 * the tile's record from first_tile, stages the source bytes the tile reaches and the tap tables of its four ranges in
 * LDS, and runs both resizes separably there; consecutive lanes store consecutive floats of a row.  The table being on
 * the device, the grid has a fixed size and its workgroups stride over the tiles.  No atomics, no communication between
 * workgroups, plain vector stores; 40 KiB of LDS.  Null pointers, n < 1, f outside 2..8, border < 0 and outputs that are
 * not three distinct pointers are refused before any launch. */
int srx_srcnn_eval_pairs(const uint8_t* arena, const srx_srcnn_eval_image* table_dev, int n, int f, int border,
                         float* sd, float* bq, float* hd, srx_stream_t stream);

/* tf.image.resize_bicubic(images, [OH, OW]) with TensorFlow 1.x semantics (align_corners=False, no half-pixel centres:
 * in = out * IN / OUT; cubic kernel A = -0.75 evaluated on TF's 1024-step grid; taps clamped to the image): SRCNN's
 * in-graph degradation, srcnn/srcnn.py:89-93.  [N,H,W,C] -> [N,OH,OW,C].  An integer down-scaling factor is plain
 * decimation (weights 0,1,0,0).  Pinned against the reference's assets/srcnn_00{0,1}.jpg panels. */
int srx_resize_bicubic_tf(const float* in, float* out, int N, int H, int W, int C, int OH, int OW,
                          srx_stream_t stream);

/* tf.image.resize_nearest_neighbor by an integer factor (pixel replication):
 * in [N,H,W,C] -> out [N,H*f,W*f,C].  enet/enet/model_enet.py:78-80. */
int srx_upsample_nearest(const float* in, float* out, int N, int H, int W, int C, int f,
                         srx_stream_t stream);

/* Gradient of srx_upsample_nearest (what TF's ResizeNearestNeighborGrad computes for an integer factor):
 * din[n,h,w,c] = sum of the f x f block of dout.  dout [N,H*f,W*f,C] -> din [N,H,W,C].
 * Backward of enet/enet/model_enet.py:78-80 inside the generator's training graph (:331-337). */
int srx_upsample_nearest_bwd(const float* dout, float* din, int N, int H, int W, int C, int f,
                             srx_stream_t stream);

/* Test aid: fills the LDS of every CU with quiet NaNs (one launch).  A kernel that reads LDS it has not written must not
 * depend on what it finds there; the Python wrappers call this before every entry point when SRX_POISON_LDS=1, which turns such a
 * dependence into NaNs in the parity tests (round 4: conv_pack3_kernel read one float behind its tile).  No reference counterpart. */
int srx_debug_poison_lds(srx_stream_t stream);

/* Gradient through t = relu(x + f(x)) of a residual block (enet/enet/model_enet.py:8-31) where the
 * gradients via the skip path and via the conv path arrive separately:
 * out = (y > 0) ? a + b : 0, y = the block input as saved (post-ReLU).  out may alias a or b. */
int srx_add_relu_grad(const float* a, const float* b, const float* y, float* out, size_t numel,
                      srx_stream_t stream);

/* ---- row A14 / "next" row N4: EnhanceNet-PAT's loss side (discriminator, VGG-19 features, perceptual / texture /
 * adversarial losses: enet/enet/model_enet.py:118-261, enet/enet/model_vgg.py:11-99) -------------------------------- */

/* One launch for a whole 3x3 SAME stride-1 layer wider than 64 channels, on channel-blocked tensors (see
 * srx_conv2d_bwd_data_acc): x [staged_blocks][N,H,W,64] -> y [produced_blocks][N,H,W,64];
 * w = the FORWARD layer's filters as [CIB][COB][3][3][64][64] (block [ib][ob] = HWIO[:, :, 64 ib:64 ib+64, 64 ob:64 ob+64]).
 *   transpose_filters == 0 (forward):  y[ob] = act( sum_ib conv(x[ib], w[ib][ob]) + bias[64 ob ..] ),
 *                                      staged_blocks = CIB, produced_blocks = COB;
 *   transpose_filters != 0 (dgrad):    y[ib] = sum_ob conv(x[ob], flipped / transposed w[ib][ob]),
 *                                      staged_blocks = COB, produced_blocks = CIB, bias NULL, act NONE.
 * mask (nullable, produced-shaped, blocked): y *= act'(mask) with mask_act -- the activation gradient of the layer
 * below fused into a data-gradient launch (ReluGrad / leaky-ReLU gradient on its saved post-activation output).
 * Same arithmetic as the block-pair launches (exact fp32 MFMA); the sum over the staged blocks stays in registers.
 * VGG-19 blocks 2-5 and the discriminator's 128..512-channel layers: enet/enet/model_vgg.py:65-99,
 * enet/enet/model_enet.py:118-146.  act: SRX_ACT_NONE / RELU / LRELU.  Any image width (rows wider than 64 pixels are
 * cut into column strips). */
int srx_conv3x3_blocked(const float* x, const float* w, const float* bias, const float* mask, int mask_act, float* y,
                        int N, int H, int W, int staged_blocks, int produced_blocks, int act,
                        int transpose_filters, srx_stream_t stream);

/* The filter gradient of such a layer (the discriminator's 128..512-channel layers; tf.gradients of
 * tf.layers.conv2d, enet/enet/model_enet.py:118-146, 331-346): x [staged_blocks][N,H,W,64] (the layer's input),
 * dpre [produced_blocks][N,H,W,64] -> dw [CIB][COB][3][3][64][64] (the layout of `w` above), dbias [64 COB] (nullable).
 * Every (input block, output block) pair is a 64 -> 64 problem: ONE launch over all pairs and one reduction of the
 * per-workgroup partial filters (deterministic order) where the linear-walk kernel covers the shape (rows of up to
 * about 120 pixels), otherwise one srx_conv2d_bwd_filter per pair.  Workspace: ..._workspace_bytes, 16-byte aligned. */
size_t srx_conv3x3_blocked_bwd_filter_workspace_bytes(int N, int H, int W, int staged_blocks, int produced_blocks);
int srx_conv3x3_blocked_bwd_filter(const float* x, const float* dpre, float* dw, float* dbias, int N, int H, int W,
                                   int staged_blocks, int produced_blocks, void* ws, size_t ws_bytes, srx_stream_t stream);

/* The two entry points above with a precision (srx_precision).  Precision 0: exactly srx_conv3x3_blocked /
 * srx_conv3x3_blocked_bwd_filter (same kernels, same bits; those two are these at precision 0).  Precision 1 (bf16x3,
 * conv_wide_bf16x3.hip): every product of the layer -- forward x and w, data gradient the staged gradient and w, filter
 * gradient x and dpre -- is hi*hi + hi*lo + lo*hi of the split described at srx_precision, accumulated in fp32; the
 * sum over the staged blocks stays in the fp32 accumulators.  Bias, act, mask / mask_act, the bias gradient (a plain
 * fp32 sum of dpre) and the fixed-order reduction of the per-workgroup partial filters stay exact fp32.  Worst case
 * per output element: |y - exact| <= 2^-13 (|x| (*) |w| + |b|) over all staged blocks.  Forward and data gradient sum
 * every output element in one fixed order (staged block, tap, channel) wherever its pixel lies: image n of a batch
 * gets the same bits as the image run alone; the filter gradient runs all block pairs in one launch with
 * deterministic partials.  Deterministic like precision 0.  Any N, H, W.  act: NONE / RELU / LRELU at both precisions
 * (others SRX_ERR_UNSUPPORTED).  Any other precision is SRX_ERR_BAD_ARG, returned before any launch; the workspace
 * query returns 0 for it.  The workspace of the filter gradient depends on the precision: size it with
 * ..._ex_workspace_bytes at the precision of the call (16-byte aligned). */
int srx_conv3x3_blocked_ex(const float* x, const float* w, const float* bias, const float* mask, int mask_act, float* y,
                           int N, int H, int W, int staged_blocks, int produced_blocks, int act,
                           int transpose_filters, int precision, srx_stream_t stream);
size_t srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes(int N, int H, int W, int staged_blocks, int produced_blocks, int precision);
int srx_conv3x3_blocked_bwd_filter_ex(const float* x, const float* dpre, float* dw, float* dbias, int N, int H, int W,
                                      int staged_blocks, int produced_blocks, int precision, void* ws, size_t ws_bytes,
                                      srx_stream_t stream);

/* The texture-matching statistics of texture_matching_loss (enet/enet/model_enet.py:225-259) in one pass:
 *   gram[n*P + p] = patches_p^T patches_p,   patches = extract_image_patches(16x16, stride 16) of normalize(x)
 *   (normalize: x / (mean over channels + eps), :34-41) -- x [N,H,W,C] -> gram [N*(H/16)*(W/16), C, C].
 * The same numbers as srx_channel_normalize -> srx_extract_patches16 -> srx_gemm(trans_a) without the two feature-sized
 * intermediates; exact-fp32 MFMA.  C = 64, 128 or 256 (VGG-19 block1/2/3_conv1), H and W multiples of 16.
 * _bwd: dx = d loss / d x given dgram = d loss / d gram, SYMMETRIC (the difference of two gram matrices is):
 *   dn = alpha * n dgram (alpha = 2), pushed through the patch permutation and the gradient of normalize. */
int srx_texture_gram(const float* x, float* gram, int N, int H, int W, int C, float eps, srx_stream_t stream);
int srx_texture_gram_bwd(const float* x, const float* dgram, float* dx, int N, int H, int W, int C, float eps, float alpha,
                         srx_stream_t stream);

/* The reference's uint8 image resizes, byte for byte: scipy.misc.imresize (enet/enet/datasets.py:110-111: 25 % bilinear
 * down, 400 % bicubic up; enet/enet/experiment_resolve.py:78-79: 400 % bicubic) is Pillow's Image.resize on the uint8
 * image -- two passes (horizontal, then vertical) of  out = clip8((2^21 + sum_k kk[k] * in[xmin + k]) >> 22)  with
 * integer coefficients (libImaging/Resample.c).  Pinned by the reference's own output, assets/enet_eagle_bq.png.
 *   srx_pil_resample_ksize / _coeffs: the coefficient tables of one axis, computed on the HOST in double precision as
 *     Pillow does: bounds [out_size][2] = (first input index, count), kk [out_size][ksize].
 *   srx_resample_u8: one pass on the device over [outer][in_size][inner] -> [outer][out_size][inner] (horizontal pass of
 *     an [N,H,W,C] image: outer = N*H, inner = C; vertical: outer = N, inner = W*C); bounds / kk are DEVICE copies.
 *   srx_u8_to_pm1: astype(float32) / 127.5 - 1.0 (two roundings). */
typedef enum { SRX_RESAMPLE_BILINEAR = 0, SRX_RESAMPLE_BICUBIC = 1 } srx_resample_filter;
int srx_pil_resample_ksize(int in_size, int out_size, int filter);
int srx_pil_resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk);
int srx_resample_u8(const uint8_t* in, uint8_t* out, long outer, int in_size, int out_size, long inner,
                    const int32_t* bounds, const int32_t* kk, int ksize, srx_stream_t stream);
int srx_u8_to_pm1(const uint8_t* in, float* out, size_t n, srx_stream_t stream);

/* tf.nn.max_pool(ksize 2x2, strides 2x2, padding='SAME') (enet/enet/model_vgg.py:28-36): [N,H,W,C] ->
 * [N,ceil(H/2),ceil(W/2),C], C % 4 == 0.  _bwd = MaxPoolGrad given the forward INPUT x: the gradient of a window goes
 * to its first maximum in scan order. */
int srx_maxpool2x2(const float* in, float* out, int N, int H, int W, int C, srx_stream_t stream);
int srx_maxpool2x2_bwd(const float* x, const float* dout, float* din, int N, int H, int W, int C,
                       srx_stream_t stream);
/* The same with the gradient of the activation that produced x fused in: din *= act'(x) (x is the post-activation
 * tensor; mask_act = SRX_ACT_RELU for VGG-19, whose every pooling layer follows a ReLU convolution:
 * enet/enet/model_vgg.py:11-36).  Same bits as srx_maxpool2x2_bwd followed by srx_act_bwd, one pass instead of two. */
int srx_maxpool2x2_bwd_masked(const float* x, const float* dout, float* din, int N, int H, int W, int C, int mask_act,
                              srx_stream_t stream);

/* out[n,i,j,:] = in[n,2i+oy,2j+ox,:] ([N,H,W,C] -> [N,(H-oy+1)/2,(W-ox+1)/2,C]: the positions oy, oy + 2, ... below H;
 * oy, ox 0 or 1, C % 4 == 0), and its gradient (zero stuffing, H and W the size of din):
 * din[n,h,w,:] = (h%2==oy && w%2==ox) ? dout[n,h/2,w/2,:] : 0.
 * tf.layers.conv2d(kernel_size=3, strides=2, padding='same') on an even-sized image pads 0 before / 1 after
 * (enet/enet/model_enet.py:136-146), i.e. it IS the stride-1 SAME convolution sampled at (oy, ox) = (1, 1); its
 * gradients are the stride-1 gradients of the zero-stuffed upstream gradient.  An odd-sized axis is padded 1 before /
 * 1 after: its offset is 0 and it has (size + 1) / 2 samples. */
int srx_subsample2(const float* in, float* out, int N, int H, int W, int C, int oy, int ox, srx_stream_t stream);
int srx_subsample2_bwd(const float* dout, float* din, int N, int H, int W, int C, int oy, int ox,
                       srx_stream_t stream);

/* Channel-blocked [blocks][pixels][64] <-> NHWC [pixels][blocks*64] (see srx_conv2d_bwd_data_acc). */
int srx_channel_blocks_to_nhwc(const float* blocked, float* plain, size_t pixels, int blocks, srx_stream_t stream);
int srx_nhwc_to_channel_blocks(const float* plain, float* blocked, size_t pixels, int blocks, srx_stream_t stream);

/* normalize() of enet/enet/model_enet.py:34-41: y = x / (mean over channels + eps) per pixel, x [pixels, C]; and its
 * gradient dx = dy / m - sum_c(dy x) / (C m^2), m = mean + eps. */
int srx_channel_normalize(const float* x, float* y, size_t pixels, int C, float eps, srx_stream_t stream);
int srx_channel_normalize_bwd(const float* x, const float* dy, float* dx, size_t pixels, int C, float eps,
                              srx_stream_t stream);

/* tf.extract_image_patches(ksizes 16x16, strides 16x16, 'VALID') + reshape to [N, (H/16)*(W/16), 256, C]
 * (enet/enet/model_enet.py:237-250): x [N,H,W,C] -> patches; inverse != 0: patches (first argument) -> image
 * (second argument), which is also the gradient of the forward map.  H, W multiples of 16, C of 4. */
int srx_extract_patches16(const float* x, float* patches, int N, int H, int W, int C, int inverse,
                          srx_stream_t stream);

/* tf.losses.log_loss(labels = label everywhere, predictions = p, epsilon = eps, reduction=MEAN)
 * (enet/enet/model_enet.py:165-182):
 *   *loss_out (+)= loss_scale * mean_i( -label log(p_i + eps) - (1 - label) log(1 - p_i + eps) )
 *   dp_i = grad_scale / n * ( -label / (p_i + eps) + (1 - label) / (1 - p_i + eps) )       (dp nullable) */
int srx_log_loss(const float* p, float label, int n, float eps, float loss_scale, float grad_scale,
                 float* loss_out, int accumulate, float* dp, srx_stream_t stream);

/* VGG-19's input map (enet/enet/model_enet.py:288-289, enet/enet/model_vgg.py:72-76), [pixels, 3]:
 *   out[..., c] = (in[..., 2-c] * 127.5 + 127.5) - (103.939, 116.779, 123.68)[c]
 * backward != 0: the gradient map din[..., c] = 127.5 * dout[..., 2-c] (in = dout, out = din). */
int srx_vgg_preprocess(const float* in, float* out, size_t pixels, int backward, srx_stream_t stream);

/* out = alpha * a + beta * b (b nullable: out = alpha * a); out may alias a or b.  Sums of gradients that reach one
 * tensor from two consumers (sr_images feeds VGG-19 and the discriminator: enet/enet/model_enet.py:291-298) and the
 * loss weights of :204,:314-317. */
int srx_add_scaled(const float* a, const float* b, float* out, size_t n, float alpha, float beta,
                   srx_stream_t stream);

/* out[j] = sum_i a[i*ld + j]: bias gradient of tf.layers.dense (enet/enet/model_enet.py:148-160). */
int srx_column_sums(const float* a, float* out, int rows, int cols, int ld, srx_stream_t stream);

/* Exact-fp32 batched GEMM with general strides (v_mfma_f32_16x16x4_f32):
 *   C_b(m,n) = act( alpha * sum_k A_b(m,k) B_b(k,n) + bias(n) ) [+ C_b(m,n)]
 *   X_b(i,j) = X[b * x_batch_stride + i * x_row_stride + j * x_col_stride]        (strides in elements)
 * tf.layers.dense forward / backward (enet/enet/model_enet.py:148-160) and the gram matrices tf.matmul(x, x,
 * transpose_a=True) over 16x16 patches and their gradient (:252-255).  bias nullable.  ws: optional workspace of
 * srx_gemm_workspace_bytes() for a deterministic split of K when M*N is small (dense layers with M = batch). */
typedef struct {
    int32_t M, N, K, batch;
    int64_t a_row_stride, a_col_stride, a_batch_stride;
    int64_t b_row_stride, b_col_stride, b_batch_stride;
    int64_t c_row_stride, c_col_stride, c_batch_stride;
    float alpha;
    int32_t act;        /* srx_act */
    int32_t accumulate; /* != 0: add to C */
} srx_gemm_desc;
size_t srx_gemm_workspace_bytes(int M, int N, int K, int batch);
int srx_gemm(const srx_gemm_desc* d, const float* A, const float* B, const float* bias, float* C, void* ws,
             size_t ws_bytes, srx_stream_t stream);

/* Which kernel srx_gemm runs for these arguments: the decision srx_gemm itself makes, by the same code.  Pointers are
 * looked at (alignment, NULL), never read; ws / ws_bytes as srx_gemm gets them.  Host-only, no device needed.
 *   TILE           gemm_mfma_kernel: a 64 x 64 tile of C per workgroup
 *   TILE_SPLITK    the same over *splits K ranges into the workspace + gemm_splitk_finish_kernel (batch 1, K >= 512,
 *                  fewer than 128 tiles, a workspace)
 *   TILE_PER_WAVE  gemm_mfma_w64_kernel: a 64 x 64 tile per wave (M, N >= 48, at least 1024 tiles over all batches)
 *   SKINNY_NN      gemm_skinny_nn_kernel<4/8/16> + the finish kernel (batch 1, M <= 16, K >= 4096, K and N multiples of
 *                  4, N >= 256, B row-major and 16-byte aligned, a workspace, at most 48 KiB of LDS)
 *   SKINNY_NT      gemm_skinny_nt_kernel<4/8/16> (batch 1, M <= 16, N >= 2048, B's rows along K and 16-byte aligned,
 *                  K a multiple of 256, no bias, no activation, at most 48 KiB of LDS)
 * Returns an srx_gemm_route, or a negative srx_status for arguments srx_gemm refuses.  *splits (nullable): K ranges. */
typedef enum { SRX_GEMM_TILE = 0, SRX_GEMM_TILE_SPLITK = 1, SRX_GEMM_TILE_PER_WAVE = 2,
               SRX_GEMM_SKINNY_NN = 3, SRX_GEMM_SKINNY_NT = 4 } srx_gemm_route;
int srx_gemm_route_of(const srx_gemm_desc* d, const float* A, const float* B, const float* bias,
                      const void* ws, size_t ws_bytes, int* splits);

#ifdef __cplusplus
}
#endif
#endif /* SRX_H_ */
