"""
model_espcn.py -- mirror of espcn/espcn/model_espcn.py (reference) on the MI355X engine.

  build_model(lr_source, scaling_factor=3, hr_target=None)
      -> {'lr_source', 'sr_result'} (+ 'hr_target', 'step', 'loss', 'optimizer', 'learning_rate')
  build_test_model(meta_path, ckpt_path) -> {'lr_sources', 'sr_results', 'scaling_factor'}
  extract_weights(meta_path, ckpt_path)  -> {'f1/kernel:0': ndarray, ...}
(reference: model_espcn.py:6,17-19,64,71,91-94,143-147,150-166).

Network (model_espcn.py:30-62 / :117-134): 5x5 conv -> 64 tanh, 3x3 -> 32 tanh, 3x3 -> 3*r*r linear,
all SAME.  `sr_result` stays in sub-pixel space [N,H,W,3*r*r], exactly like the reference; the
depth-to-space map (experiment_test.py:171-177) is either the separate op ops.depth_to_space or -- on the
inference path `super_resolve` -- the STORE MODE of the f3 layer (srx_conv_desc.subpixel_r): three launches,
no intermediate sub-pixel tensor, replayed as one HIP graph per input shape.
Checkpoints: the reference restores a TF bundle + .meta graph; here a checkpoint is an .npz of the
same variable names (`f1/kernel:0` ...), `meta_path` is accepted and ignored.
"""
import collections
import functools
import os
import weakref

import numpy as np
import torch

from .. import _lib, graph, ops
from ..engine import ConvStack, LayerSpec, capture_graph, truncated_normal_


def layer_specs(scaling_factor=3):
    r2 = scaling_factor * scaling_factor
    return [LayerSpec(5, 3, 64, 'same', 'tanh', 'f1'),
            LayerSpec(3, 64, 32, 'same', 'tanh', 'f2'),
            LayerSpec(3, 32, 3 * r2, 'same', None, 'f3')]


RoutePlan = collections.namedtuple('RoutePlan', 'key floats out_shape out_dtype shared shared_out')


@functools.lru_cache(maxsize=32)                        # (asked once per call of a route: a frame of a sequence costs ~135 us)
def route_plan(route, n, h, w, r, single_launch=False, matrix='bt601', full_range=False, pixel_format=None):
    """What tells one inference route at one size from the others, as plain data (a pure function, no torch: checked
    without a GPU); EspcnModel._run does the rest.  route: 'float' (super_resolve), 'u8' (super_resolve_u8), 'yuv420'
    (super_resolve_yuv420) or 'yuv' (super_resolve_yuv, which asks the library's host function for the frame size) on n LR
    frames of h x w at scaling factor r; single_launch, matrix and full_range matter to the last two alone, pixel_format (a
    name of _lib.PIXEL_FORMATS) to 'yuv' alone.
      key         the route's entry in EspcnModel._graphs
      floats      the shapes of the float32 tensors between input and output, in the order its launches take them; None
                  where the route has none (t1 and t2 when one launch runs the network)
      out_shape, out_dtype   of its output
      shared, shared_out     the names of the model's own buffers that stand in for `floats` and the output on the eager path"""
    lr, t1, t2, hr = (n, h, w, 3), (n, h, w, 64), (n, h, w, 32), (n, h * r, w * r, 3)
    if route == 'float':
        return RoutePlan(lr, (t1, t2), hr, 'float32', (('sr', 0), ('sr', 1)), ('sr', 2))
    if route == 'u8':
        return RoutePlan(('u8',) + lr, (lr, t1, t2, hr), hr, 'uint8', (('sr8', 0), ('sr', 0), ('sr', 1), ('sr', 2)), 'sr5')
    if route == 'yuv420':
        single_launch = bool(single_launch)
        return RoutePlan(('yuv420', n, h, w, matrix, bool(full_range), single_launch),
                         (lr, None, None, hr) if single_launch else (lr, t1, t2, hr), (n, _lib.yuv420_frame_bytes(h * r, w * r)), 'uint8',
                         (('sry', 0), ('sr', 0), ('sr', 1), ('sry', 1)), 'sry')
    if route == 'yuv':
        single_launch = bool(single_launch)
        return RoutePlan(('yuv', pixel_format, n, h, w, matrix, bool(full_range), single_launch),
                         (lr, None, None, hr) if single_launch else (lr, t1, t2, hr), (n, _lib.yuv_frame_bytes(h * r, w * r, pixel_format)), 'uint8',
                         (('sry', 0), ('sr', 0), ('sr', 1), ('sry', 1)), 'sry')
    raise ValueError("route must be 'float', 'u8', 'yuv420' or 'yuv', got %r" % (route,))


class EspcnModel(object):
    def __init__(self, scaling_factor=3, device='cuda', seed=None):
        self.scaling_factor = scaling_factor
        self.stack = ConvStack(layer_specs(scaling_factor), device=device, residual=False, weight_decay=0.0)
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        for i in range(3):
            truncated_normal_(self.stack.kernel(i), 0.02, gen)      # model_espcn.py:21; biases zero
        self.placeholders = {}
        # inference path: HIP-graph replay of the three launches (SRX_ESPCN_GRAPH=0: eager launches)
        self.use_graph = os.environ.get('SRX_ESPCN_GRAPH', '1') != '0'
        self._graphs = {}
        self._lut, self._u8_bufs = None, {}             # super_resolve_u8: the byte table and the model-owned byte outputs
        self._yuv_coeff_cache = {}                      # super_resolve_yuv420: (matrix, full_range) -> _lib.Yuv420Coeffs
        self._luts, self._yuv_depth_coeff_cache = {}, {}    # super_resolve_yuv: depth -> table; (matrix, full_range, depth) -> coefficients
        # one launch for the whole net while the problem is latency-bound (SRX_ESPCN_FUSED=0: never)
        self.use_single_launch = os.environ.get('SRX_ESPCN_FUSED', '1') != '0'
        # (measured, round 4 -- tiles of up to 16 x 16, LDS reads a block ahead of the MFMAs -- one launch against the three-launch
        # graph: 28 / 38 / 62 / 89 / 130 us against 67 / 78 / 79 / 102 / 137 us at 16 k / 29 k / 66 k / 90 k / 131 k LR pixels;
        # behind at 230 k: 213 against 181 us.  Round 3, 9 x 9 tiles: level at 46-58 k pixels, behind from 65 k on.)
        self.single_launch_max_pixels = int(os.environ.get('SRX_ESPCN_FUSED_MAX_PIXELS', '131072'))
        self.inference_path = ('<= %d LR pixels: ONE launch, the three layers chained through LDS per <= 16x16 tile with the '
                               'sub-pixel store (srx_espcn_forward); larger: f1, f2, f3 with the sub-pixel store fused into '
                               "f3's epilogue, 3 launches%s" % (self.single_launch_max_pixels,
                                                               ' replayed as one HIP graph' if self.use_graph else ', eager'))

        # the forward pass of a TRAIN step in one launch too (srx_espcn_forward_keep: writes t1, t2 and y for backward);
        # SRX_ESPCN_FUSED_TRAIN=0: three launches (A/B).  Measured (scripts/time_espcn_train.py, whole train step, one launch
        # against three): batch 16 / 32 / 64 of 17 x 17: 119 / 128 / 154 us against 149 / 144 / 169; batch 128 (37 k pixels): level.
        self.use_single_launch_train = os.environ.get('SRX_ESPCN_FUSED_TRAIN', '1') != '0'
        self.single_launch_train_max_pixels = int(os.environ.get('SRX_ESPCN_FUSED_TRAIN_MAX_PIXELS', '30000'))
        # through a weak reference: the stack does not keep its model alive, so a dropped model and its device memory are freed
        # at once, by reference count, not whenever the cyclic collector next runs (tests compare memory_allocated() around a
        # refused call, and a collection that freed an earlier test's model inside that window made them fail).  A stack that
        # outlives its model falls back to the three launches.
        model = weakref.ref(self)
        self.stack.forward_keep_hook = lambda x, outs: model() is not None and model()._forward_keep_one_launch(x, outs)
        # train steps are replayed as a HIP graph for small batches only: measured (bench.py espcn_train_us, scripts/time_espcn_train.py)
        # batch 16 / 32 of 17 x 17: replay 119 / 128 us against 155 / 164 us of eager launches; batch 64: 155 against 148 -- the
        # launches of the larger problem keep the queue fed by themselves
        self.stack.step_graph_max_pixels = int(os.environ.get('SRX_ESPCN_STEP_GRAPH_MAX_PIXELS', '12000'))

    def _forward_keep_one_launch(self, x, outs):
        n, h, w, _ = x.shape
        if not (self.use_single_launch and self.use_single_launch_train and x.is_cuda and n * h * w <= self.single_launch_train_max_pixels
                and 2 <= self.scaling_factor <= 4):
            return False
        ops.espcn_forward_keep(x.contiguous(), self._params(), self.scaling_factor, outs[0], outs[1], outs[2])
        return True

    # ---- eager API -----------------------------------------------------------------------------
    def forward(self, lr_source, keep=False):
        """sr_result in sub-pixel space [N,H,W,3*r*r]."""
        return self.stack.forward(lr_source, keep=keep)

    def super_resolve_two_step(self, lr_source):
        """forward + the standalone depth-to-space pass (4 launches): [N,H,W,3] -> [N,H*r,W*r,3]."""
        return ops.depth_to_space(self.forward(lr_source), self.scaling_factor)

    # ---- the inference routes --------------------------------------------------------------------
    def _params(self):
        st = self.stack
        return [(st.kernel(i), st.bias(i)) for i in range(3)]

    def _layers(self, x, t1, t2, out):
        """f1, f2 and f3 with the sub-pixel store: the three launches every route's per-layer form runs."""
        st = self.stack
        t = ops.conv2d_fwd(x, st.kernel(0), st.bias(0), 'same', 'tanh', out=t1)
        t = ops.conv2d_fwd(t, st.kernel(1), st.bias(1), 'same', 'tanh', out=t2)
        return ops.conv2d_fwd(t, st.kernel(2), st.bias(2), 'same', None, subpixel_r=self.scaling_factor, out=out)

    def _run(self, plan, src, launches, out=None, use_graph=None):
        """Runs one route (plan: its route_plan; launches(src, out, bufs) enqueues it on bufs, the float tensors of
        plan.floats).  Eager (use_graph False, SRX_ESPCN_GRAPH=0, or a CPU tensor): the launches on the model's shared
        buffers, which are replaced when another size comes along.  Else the launches replayed as one HIP graph per plan.key,
        captured on a miss; the static input is copied unless the caller passed the graph's own tensor.  out None: the
        route's own output tensor (the graph's, or the model's), overwritten by the next call; else `out`, returned as given."""
        if not (self.use_graph if use_graph is None else use_graph) or not src.is_cuda:
            bufs = tuple(None if s is None else self.stack._buf(name, s) for name, s in zip(plan.shared, plan.floats))
            if out is None:
                out = self.stack._buf(plan.shared_out, plan.out_shape) if plan.out_dtype == 'float32' else self._u8_buf(plan.shared_out, plan.out_shape)
            return launches(src, out, bufs)
        g = self._graphs.get(plan.key)
        if g is None:
            g = self._graphs[plan.key] = self._capture(plan, src, launches)
        static_in, graph_obj, graph_out = g[:3]
        if src.data_ptr() != static_in.data_ptr():
            static_in.copy_(src)
        graph_obj.replay()
        if out is None:
            return graph_out
        out.view(-1).copy_(graph_out.view(-1))
        return out

    def _capture(self, plan, src, launches):
        """Warm the kernels up on a side stream (function attributes and buffers must exist before capture), then record
        the launches.  Three rules: the oldest graph is evicted before the capture begins, never during it; whatever the
        launches read besides their arguments (the byte table) exists before it; and the graph owns every buffer it points at
        -- its cloned input, its output and the float tensors between them -- because the model's shared ones are replaced
        when another size comes along, and a replay must never write through a dangling pointer.  The weights alone are
        read through the model's pointers: training steps or load_variables() that update them in place are seen by later
        replays."""
        if len(self._graphs) >= 8:                      # a directory of images of many sizes: keep the cache small
            self._graphs.pop(next(iter(self._graphs)))
        dev = src.device
        static_in = src.clone()
        out = torch.empty(plan.out_shape, dtype=getattr(torch, plan.out_dtype), device=dev)
        bufs = tuple(None if s is None else torch.empty(s, dtype=torch.float32, device=dev) for s in plan.floats)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                launches(static_in, out, bufs)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph_obj = torch.cuda.CUDAGraph()
        with capture_graph(graph_obj):
            launches(static_in, out, bufs)
        return static_in, graph_obj, out, bufs          # (the tuple keeps every buffer the graph points at alive)

    def super_resolve(self, lr_source, use_graph=None, single_launch=None):
        """The inference path (espcn/espcn/experiment_test.py:156-181: run the net, then the sub-pixel shuffle):
        [N,H,W,3] -> [N,H*r,W*r,3] in three launches -- the f3 layer stores straight through the depth-to-space map
        (bit-identical to super_resolve_two_step) -- replayed as ONE HIP graph per input shape: the problem is
        launch-latency-bound (0.57 GFLOP at BASELINE configs[1]).  Small problems (<= single_launch_max_pixels LR
        pixels) take ONE launch instead: srx_espcn_forward chains the three layers through LDS per <= 16x16 tile (same
        bits).  The returned tensor is a buffer owned by the model and overwritten by the next call."""
        n, h, w, _ = lr_source.shape
        r = self.scaling_factor
        if single_launch is None:
            single_launch = self.use_single_launch and n * h * w <= self.single_launch_max_pixels
        if single_launch and lr_source.is_cuda:
            return ops.espcn_forward(lr_source.contiguous(), self._params(), r, out=self.stack._buf(('sr1',), (n, h * r, w * r, 3)))
        return self._run(route_plan('float', n, h, w, r), lr_source, lambda src, out, bufs: self._layers(src, bufs[0], bufs[1], out),
                         use_graph=use_graph)

    # ---- bytes in, bytes out ---------------------------------------------------------------------
    @property
    def lut(self):
        """The 256 floats a byte decodes to: the host route's `lr_image / 127.5 - 1.0` (ops.unit_lut), on the model's device."""
        if self._lut is None:
            self._lut = ops.unit_lut(self.stack.device)
        return self._lut

    def _u8_buf(self, key, shape):
        t = self._u8_bufs.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._u8_bufs[key] = torch.empty(shape, dtype=torch.uint8, device=self.stack.device)
        return t

    def super_resolve_u8(self, lr_u8, out=None, single_launch=None, use_graph=None):
        """super_resolve from bytes to bytes (espcn/espcn/experiment_test.py:148-184 with the `/ 127.5 - 1.0` before and the
        `* 0.5 + 0.5`, clip, `* 255.0 + 0.5`, astype(uint8) after the network on the device): [N,H,W,3] uint8 on the device
        -> [N,H*r,W*r,3] uint8, the bytes `(super_resolve_array(model, img) * 255.0 + 0.5).astype(uint8)` gives per image.
        The same window rule as super_resolve: <= single_launch_max_pixels LR pixels take ONE launch
        (srx_espcn_forward_u8); larger frames take five (decode, the three layers, encode), replayed as one HIP graph per
        input shape that owns every buffer it points at.  out: a contiguous uint8 tensor of N*rH*rW*3 elements (returned as
        given); None: a buffer owned by the model and overwritten by the next call."""
        n, h, w, _ = lr_u8.shape
        r = self.scaling_factor
        lut = self.lut                                  # (read here: the table exists before any capture below)
        if single_launch is None:
            single_launch = self.use_single_launch and n * h * w <= self.single_launch_max_pixels
        if single_launch:
            return ops.espcn_forward_u8(lr_u8, lut, self._params(), r,
                                        out=out if out is not None else self._u8_buf('sr1', (n, h * r, w * r, 3)))

        def launches(src, out, bufs):
            lr, t1, t2, hr = bufs
            ops.u8_lut_float(src, lut, out=lr)
            return ops.unit_u8(self._layers(lr, t1, t2, hr), out=out)

        return self._run(route_plan('u8', n, h, w, r), lr_u8, launches, out=out, use_graph=use_graph)

    # ---- planar YUV 4:2:0 in, planar YUV 4:2:0 out ----------------------------------------------
    def _yuv_coeffs(self, matrix, full_range):
        key = (matrix, bool(full_range))
        c = self._yuv_coeff_cache.get(key)
        if c is None:
            c = self._yuv_coeff_cache[key] = ops.yuv420_coeffs(matrix, full_range)
        return c

    def super_resolve_yuv420(self, yuv, height, width, out=None, matrix='bt601', full_range=False, single_launch=None, use_graph=None):
        """super_resolve on planar YUV 4:2:0 frames, the Y4M frame payload: yuv [N, frame_bytes] uint8 on the device, each
        frame Y [height,width] then U and V [(height + 1) // 2, (width + 1) // 2] -> [N, hr_frame_bytes] uint8, the frames of
        height*r x width*r.  Decode (integer matrix, chroma replicated, the byte table of super_resolve_u8), the float
        network, encode (encode_unit_u8, integer matrix, one rounding for the 2 x 2 average): ops.yuv420_lut_float and
        ops.unit_yuv420 state the arithmetic.  matrix 'bt601' / 'bt709'; full_range False: luma 16..235, chroma 16..240.
        The same window rule as super_resolve: <= single_launch_max_pixels LR pixels run srx_espcn_forward between the two
        (three launches), larger frames the three layers (five); either way the launches are replayed as one linear HIP
        graph per (shape, matrix, range) that owns every buffer it points at (use_graph=False: eager launches); the
        coefficients are kernel arguments, recorded by value.  out: a contiguous uint8 tensor of N * hr_frame_bytes elements
        (returned as given); None: a buffer owned by the model and overwritten by the next call."""
        height, width, r = int(height), int(width), self.scaling_factor
        if yuv.dim() != 2 or yuv.shape[1] != ops.yuv420_frame_bytes(height, width):
            raise ValueError('yuv must be [N, %d] for %d x %d 4:2:0 frames, got %s'
                             % (ops.yuv420_frame_bytes(height, width), height, width, tuple(yuv.shape)))
        n = yuv.shape[0]
        coeffs = self._yuv_coeffs(matrix, full_range)
        lut = self.lut                                  # (read here: the table exists before any capture below)
        if single_launch is None:
            single_launch = self.use_single_launch and n * height * width <= self.single_launch_max_pixels

        def launches(src, out, bufs):
            lr, t1, t2, hr = bufs
            ops.yuv420_lut_float(src, n, height, width, coeffs, lut, out=lr)
            if single_launch:
                ops.espcn_forward(lr, self._params(), r, out=hr)
            else:
                self._layers(lr, t1, t2, hr)
            return ops.unit_yuv420(hr, coeffs, out=out)

        return self._run(route_plan('yuv420', n, height, width, r, single_launch, matrix, full_range), yuv, launches, out=out, use_graph=use_graph)

    # ---- planar YUV of any format of _lib.PIXEL_FORMATS in, the same format out -------------------
    def lut_of(self, depth):
        """The 2^depth floats a code of `depth` bits decodes to (ops.unit_lut), on the model's device; depth 8: `lut`."""
        if depth == 8:
            return self.lut
        t = self._luts.get(depth)
        if t is None:
            t = self._luts[depth] = ops.unit_lut(self.stack.device, depth)
        return t

    def super_resolve_yuv(self, yuv, height, width, pixel_format, out=None, matrix='bt601', full_range=False, single_launch=None, use_graph=None):
        """super_resolve_yuv420 for every planar format of _lib.PIXEL_FORMATS ('yuv420p', 'yuv422p', 'yuv444p' and their
        'p10le' / 'p12le' forms): yuv [N, frame_bytes] uint8 on the device, the stream's bytes at every depth (two per sample,
        little-endian, above 8 bits) -> [N, hr_frame_bytes] uint8 in the same format.  ops.yuv_lut_float and ops.unit_yuv state
        the arithmetic; the table has 2^depth floats and the coefficients are those of the depth.  The window rule, the
        launches and the replay are super_resolve_yuv420's, one graph per (format, shape, matrix, range)."""
        height, width, r = int(height), int(width), self.scaling_factor
        depth = _lib.yuv_format(pixel_format).depth
        frame = ops.yuv_frame_bytes(height, width, pixel_format)
        if yuv.dim() != 2 or yuv.shape[1] != frame:
            raise ValueError('yuv must be [N, %d] for %d x %d %s frames, got %s' % (frame, height, width, pixel_format, tuple(yuv.shape)))
        n = yuv.shape[0]
        key = (matrix, bool(full_range), depth)
        coeffs = self._yuv_depth_coeff_cache.get(key)
        if coeffs is None:
            coeffs = self._yuv_depth_coeff_cache[key] = ops.yuv_coeffs(matrix, full_range, depth)
        lut = self.lut_of(depth)                        # (read here: the table exists before any capture below)
        if single_launch is None:
            single_launch = self.use_single_launch and n * height * width <= self.single_launch_max_pixels

        def launches(src, out, bufs):
            lr, t1, t2, hr = bufs
            ops.yuv_lut_float(src, n, height, width, pixel_format, coeffs, lut, out=lr)
            if single_launch:
                ops.espcn_forward(lr, self._params(), r, out=hr)
            else:
                self._layers(lr, t1, t2, hr)
            return ops.unit_yuv(hr, pixel_format, coeffs, out=out)

        return self._run(route_plan('yuv', n, height, width, r, single_launch, matrix, full_range, pixel_format), yuv, launches,
                         out=out, use_graph=use_graph)

    def train_step(self, lr_source, hr_target, learning_rate):
        """MSE in sub-pixel space (hr_target is the space-to-depth label, dataset.py:140-156) + Adam
        with the fed learning rate (model_espcn.py:76-89)."""
        # one replayed HIP graph per batch shape (engine.ConvStack.train_step_replay): a step is a dozen dependent launches
        return self.stack.train_step_replay(lr_source, hr_target, learning_rate)

    # ---- checkpoints ---------------------------------------------------------------------------
    def save(self, path):
        arrays = {k + ':0': v.detach().cpu().numpy() for k, v in self.stack.variables().items()}
        arrays['global_step'] = np.int64(self.stack.global_step)
        np.savez(path, **arrays)

    # ---- Session.run backend -------------------------------------------------------------------
    def run(self, keys, feed_dict):
        dev = self.stack.device
        feeds = {name: feed_dict[ph] for name, ph in self.placeholders.items() if ph in feed_dict}
        # `step` is a variable: the reference reads it with no feed (espcn/espcn/experiment_train.py:92)
        needs_forward = [k for k in keys if k != 'step']
        lr = hr = y = loss = None
        if needs_forward:
            if 'lr_source' not in feeds:
                raise ValueError('lr_source must be fed to fetch %s' % ', '.join(needs_forward))
            lr = graph.to_device(feeds['lr_source'], dev)
            hr = graph.to_device(feeds['hr_target'], dev) if 'hr_target' in feeds else None
            if 'optimizer' in keys:
                if hr is None or 'learning_rate' not in feeds:
                    raise ValueError('hr_target and learning_rate must be fed to run the optimizer')
                loss = self.train_step(lr, hr, float(feeds['learning_rate']))
                y = self.stack.acts[-1]
            else:
                y = self.stack.forward(lr, keep=True)
                if 'loss' in keys:
                    if hr is None:
                        raise ValueError('hr_target must be fed to fetch loss')
                    loss = self.stack.loss
                    ops.mse_fwd_bwd(y, hr, loss, accumulate=False, want_grad=False)
        out = {}
        for k in keys:
            if k == 'optimizer':
                out[k] = None
            elif k == 'loss':
                out[k] = float(loss.item())
            elif k == 'step':
                out[k] = self.stack.global_step
            elif k in ('sr_result', 'sr_results'):
                out[k] = y.detach().cpu().numpy()
            elif k in ('lr_source', 'lr_sources'):
                out[k] = lr.detach().cpu().numpy()
            elif k == 'hr_target':
                out[k] = hr.detach().cpu().numpy()
            else:
                raise KeyError(k)
        return out


def build_model(lr_source, scaling_factor=3, hr_target=None, device='cuda', seed=None):
    """
    lr_source:  source image batch (graph.placeholder) to be super resolved
    hr_target:  target batch as training labels in sub-pixel convolved shape; a partial (test)
                model is built if hr_target is None
    scaling_factor: factor of up scaling; the depth of the final layer is 3 * scaling_factor ** 2
    """
    m = EspcnModel(scaling_factor, device=device, seed=seed)
    m.placeholders['lr_source'] = lr_source
    model = {'lr_source': lr_source, '_model': m}
    model['sr_result'] = graph.Tensor('sr_result', owner=m, key='sr_result')
    if hr_target is None:
        return model
    m.placeholders['hr_target'] = hr_target
    lr = graph.placeholder([], name='learning_rate')         # tf.placeholder(shape=[]) (model_espcn.py:83)
    m.placeholders['learning_rate'] = lr
    model['hr_target'] = hr_target
    model['step'] = graph.Tensor('global_step', owner=m, key='step')
    model['loss'] = graph.Tensor('loss', owner=m, key='loss')
    model['optimizer'] = graph.Tensor('optimizer', owner=m, key='optimizer')
    model['learning_rate'] = lr
    return model


def extract_weights(meta_path, ckpt_path):
    """{variable name: ndarray} for every trainable variable (model_espcn.py:150-166).  `ckpt_path` is either a
    TensorFlow V2 checkpoint prefix (read by tf_bundle, no TensorFlow needed; `meta_path` is not used: the
    trainable variables are the `f{1,2,3}/{kernel,bias}` entries) or an .npz written by EspcnModel.save."""
    from .. import tf_bundle
    if tf_bundle.is_checkpoint_prefix(ckpt_path):
        values = tf_bundle.load_checkpoint(ckpt_path)
        return {k + ':0': v for k, v in values.items()
                if k.count('/') == 1 and k.split('/')[1] in ('kernel', 'bias')}
    z = np.load(ckpt_path)
    return {k: z[k] for k in z.files if k.endswith(':0')}


def build_test_model(meta_path, ckpt_path, device='cuda'):
    """Weights-as-constants inference model with dynamic image size (model_espcn.py:99-147).
    `ckpt_path` may also be an already-loaded {name: array} dict."""
    variables = ckpt_path if isinstance(ckpt_path, dict) else extract_weights(meta_path, ckpt_path)
    scaling_factor = int((np.asarray(variables['f3/bias:0']).size // 3) ** 0.5)      # model_espcn.py:108
    m = EspcnModel(scaling_factor, device=device)
    m.stack.load_variables(variables)
    lr_sources = graph.placeholder([None, None, None, 3], name='lr_sources')
    m.placeholders['lr_source'] = lr_sources
    return {'lr_sources': lr_sources,
            'sr_results': graph.Tensor('sr_results', owner=m, key='sr_results'),
            'scaling_factor': scaling_factor,
            '_model': m}
