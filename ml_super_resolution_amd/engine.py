"""
engine.py -- the layer-stack engine behind the model mirrors.

A `ConvStack` is what the reference's `build_model` functions describe: a chain of stride-1
convolutions with bias + activation (vdsr/vdsr/model_vdsr.py:47-106,
espcn/espcn/model_espcn.py:30-62, srcnn/srcnn.py:100-130), an MSE loss with optional L2
regulariser (model_vdsr.py:120-125), and a TF-semantics Adam / Momentum+clip update
(model_vdsr.py:145-184).  TensorFlow's autodiff is replaced by an explicit backward over the
C-ABI ops: per layer one fused dgrad (+ upstream activation gradient) and one wgrad
(+ bias grad + weight decay).

Memory layout (sized for 288 GB HBM: everything stays resident):
  * all kernels and biases live in ONE flat fp32 buffer: a ConvStack IS a param_pool.ParamPool, which owns the layout,
    the gradient / optimizer-slot buffers that mirror it, the step count, the optimizer launches and the checkpoint walk;
  * every layer's post-activation output is kept for backward (VDSR-20 @ 256x41x41: 2.1 GB);
  * two ping-pong buffers hold the running pre-activation gradient.
"""
import collections
import contextlib
import gc
import math
import os

import torch

from . import ops
from .param_pool import ParamPool


@contextlib.contextmanager
def capture_graph(g):
    """torch.cuda.graph(g) with Python's cyclic collector run before the capture and held off during it.  A model and its
    stack refer to each other (forward_keep_hook), so a dropped model, its captured graphs and their memory pools are
    freed by the collector, whenever its allocation counters say so.  Freeing a graph or device memory is not allowed
    while a stream captures (the process aborts), and torch.cuda.graph no longer collects on entry: so collect what is
    dead now, and let nothing be collected until the capture has ended."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            yield
    finally:
        if was_enabled:
            gc.enable()


class LayerSpec(object):
    """One conv layer.  `scope` is the TF variable scope (`conv2d`, `conv2d_1`, `f1`, ...):
    variables are `<scope>/kernel` and `<scope>/bias`."""

    def __init__(self, ksize, cin, cout, padding='same', act=None, scope=None):
        self.kh, self.kw = (ksize, ksize) if isinstance(ksize, int) else ksize
        self.cin, self.cout = cin, cout
        self.padding = padding.lower()
        self.act = act
        self.scope = scope

    @property
    def kernel_shape(self):
        return (self.kh, self.kw, self.cin, self.cout)

    def out_hw(self, h, w):
        if self.padding == 'same':
            return h, w
        return h - self.kh + 1, w - self.kw + 1


# ---- the schedule of a pass: pure host data --------------------------------------------------------------------------
# A pass is planned as a list of ops, then walked (ConvStack.forward / loss_and_backward).  An op holds layer indices and the keys
# that buffers have in ConvStack._bufs, never a tensor: two plans compare with ==, and tests/test_step_plan_host.py pins them.
Conv = collections.namedtuple('Conv', 'i')                                    # layer i's forward, one launch
Chain = collections.namedtuple('Chain', 'lo hi')                              # the forwards of layers lo .. hi, one launch (srx_conv_chain)
Wgrad = collections.namedtuple('Wgrad', 'i dpre_key')                         # layer i's filter gradient, from the gradient at its output
Dgrad = collections.namedtuple('Dgrad', 'i src_key dst_key')                  # layer i's data gradient: at its output -> at its input
DgradChain = collections.namedtuple('DgradChain', 'hi lo src_key dst_keys')   # those of layers hi, hi - 1 .. lo, one launch (srx_conv_chain)
WgradBatch = collections.namedtuple('WgradBatch', 'lo hi dpre_keys')          # the filter gradients of layers lo .. hi, one call
RUN_MAX = 32    # the most layers one chain or one batch takes: the library's kChainMax


def _runs(start, stop, step, alike):
    """(i, j) per run of like layers: i, i + step .. j - step are the layers k from i on with alike(i, k), at most RUN_MAX of them and
    short of stop.  The first run begins at start, every further one where the last one ended (one layer on when that was empty)."""
    i = start
    while (stop - i) * step > 0:
        j = i
        while (stop - j) * step > 0 and abs(j - i) < RUN_MAX and alike(i, j):
            j += step
        yield i, j
        i = j if j != i else i + step


def _chainable(specs, residual, layer_precision, chain_ok):
    """fn(i, in_shape, op): can layer i's forward (op OP_FWD) or data gradient (OP_BWD_DATA) run inside a chain (srx_conv_chain)?"""
    def chainable(i, in_shape, op):
        s = specs[i]
        # The layer kind, the shape and the activations it is given are the library's to judge (srx_conv_chain_supported).
        # Here: what its descriptor does not carry -- the precision this stack runs the layer at, the residual add of the
        # last layer, and in a data gradient the layer's own activation and the previous layer's.
        if layer_precision[i] != 'highest':
            return False
        if op == ops._lib.OP_FWD:
            if residual and i == len(specs) - 1:
                return False
            act, in_act = s.act, None
        else:
            if i == 0 or s.act not in (None, 'relu') or specs[i - 1].act not in (None, 'relu'):
                return False
            act, in_act = None, specs[i - 1].act
        return chain_ok(i, in_shape, op) if chain_ok else ops.chain_supported(in_shape, s.kernel_shape, op, s.padding, act, in_act)
    return chainable


def plan_forward(specs, residual, layer_precision, in_shapes, chain_ok=None):
    """The forward pass as [Conv(i) | Chain(lo, hi)]: a Chain is a run of two or more layers of one input shape, padding and activation.
    in_shapes: every layer's input shape (tuples), then the output's.  chain_ok(i, in_shape, op): a test's stand-in for ops.chain_supported."""
    chainable = _chainable(specs, residual, layer_precision, chain_ok)

    def alike(i, k):
        return (specs[k].padding == specs[i].padding and specs[k].act == specs[i].act and in_shapes[k] == in_shapes[i] and
                chainable(k, in_shapes[k], ops._lib.OP_FWD))
    return [Chain(i, j - 1) if j > i + 1 else Conv(i) for i, j in _runs(0, len(specs), 1, alike)]


def plan_backward(specs, residual, layer_precision, in_shapes, chain_ok=None, batch_ok=None):
    """The backward pass in launch order, [Wgrad | Dgrad | DgradChain | WgradBatch], for one stream: a layer's dgrad and its wgrad
    (+ partial reduce) are independent, but running the wgrads or the reductions on a side stream measured slower.
    batch_ok(lo, hi): a test's stand-in for ops.bwd_filter_batch_plan (the shape, the layer count and srx_set_wgrad_batch decide)."""
    chainable = _chainable(specs, residual, layer_precision, chain_ok)
    last = len(specs) - 1

    def alike(i, k):
        return (layer_precision[k] == 'highest' and specs[k].kernel_shape == specs[i].kernel_shape and specs[k].padding == specs[i].padding and
                in_shapes[k] == in_shapes[i] and in_shapes[k + 1] == in_shapes[i + 1])
    # the batch: the longest run (the first one among equals) of exact-fp32 layers of one shape and padding that the library takes
    b_lo, b_hi = 0, -1
    for i, j in _runs(0, len(specs), 1, alike):
        if j - i >= 2 and j - i > b_hi - b_lo + 1 and (batch_ok(i, j - 1) if batch_ok else ops.bwd_filter_batch_plan(
                in_shapes[i], specs[i].kernel_shape, j - i, specs[i].padding)[0] > 0):
            b_lo, b_hi = i, j - 1

    def chain_alike(hi, k):
        return (specs[k].padding == specs[hi].padding and specs[k - 1].act == specs[hi - 1].act and in_shapes[k] == in_shapes[hi] and
                chainable(k, in_shapes[k], ops._lib.OP_BWD_DATA))
    # the chain: the highest run of two or more layers below the last one that share the shape, padding and mask activation
    c_lo, c_hi = next(((lo + 1, hi) for hi, lo in _runs(last - 1, 0, -1, chain_alike) if hi - lo >= 2), (0, -1))

    def dpre_key(i):
        """Where the gradient at layer i's output lives: what the loss left or what layer i + 1's data gradient writes.  A buffer of the
        layer's own where a chain writes it or a batch reads it (it must outlive the rotation), else one of three rotating buffers."""
        if i == last:
            return ('dy', 0) if specs[last].act is None else ('dpre_last',)
        if c_lo <= i + 1 <= c_hi or b_lo <= i <= b_hi:
            return ('dpre_chain', i)
        return ('dx', (i + 1) % 3, in_shapes[i + 1][3])
    plan = []
    for i in range(last, -1, -1):
        if i == c_hi:
            plan.append(DgradChain(c_hi, c_lo, dpre_key(c_hi), [dpre_key(k - 1) for k in range(c_hi, c_lo - 1, -1)]))
        if not b_lo <= i <= b_hi:
            plan.append(Wgrad(i, dpre_key(i)))
        elif i == b_lo:
            plan.append(WgradBatch(b_lo, b_hi, [dpre_key(k) for k in range(b_lo, b_hi + 1)]))
        if i > 0 and not c_lo <= i <= c_hi:
            plan.append(Dgrad(i, dpre_key(i), dpre_key(i - 1)))
    return plan


class ConvStack(ParamPool):
    def __init__(self, specs, device='cuda', residual=False, weight_decay=0.0, precision='highest', leaf_names=('kernel', 'bias')):
        """residual: output = input + stack(input) (VDSR, model_vdsr.py:104).
        weight_decay: scale of tf.contrib.layers.l2_regularizer on every kernel.
        precision: 'highest' (exact fp32 products) or 'high' (bf16x3 products on the layers that support them, exact
        fp32 on the others: see set_precision).
        leaf_names: tf.layers.conv2d creates <scope>/kernel, <scope>/bias; tf.contrib.layers.convolution2d (SRCNN,
        srcnn/srcnn.py:100-130) creates <scope>/weights, <scope>/biases."""
        self.specs = list(specs)
        self.residual = residual
        self.weight_decay = float(weight_decay)
        # the pool's variables 2 i and 2 i + 1 are layer i's kernel and bias
        entries = []
        for i, s in enumerate(self.specs):
            scope = s.scope or ('layer%d' % i)
            entries += [('%s/%s' % (scope, leaf_names[0]), s.kernel_shape), ('%s/%s' % (scope, leaf_names[1]), (s.cout,))]
        ParamPool.__init__(self, entries, device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._acts = None
        self.step_graph_max_pixels = None  # optional: input pixels (N*H*W) above which train_step_replay issues eager launches
        self.forward_keep_hook = None      # optional: fn(x, [per-layer output buffers]) -> True when it ran the whole forward pass
        self._bufs = {}
        self._ws = None
        self.grad_hook = None      # called with the flat gradient after backward (DP all-reduce)
        self.loss_kind = 'mse'     # 'mse' (VDSR, ESPCN) or 'rownorm' (SRCNN)
        self._decay_mask = None
        # ---- Adam with its step count and learning rate in device memory, and whole train steps replayed as HIP graphs
        # (train_step_replay): ESPCN / SRCNN steps are a dozen dependent launches of ~10 us each, their recipes run 1.6 M
        # of them (espcn/makefile:30-36).  SRX_STEP_GRAPH=0: every step as eager launches.
        self.use_step_graph = os.environ.get('SRX_STEP_GRAPH', '1') != '0'
        self._step_graphs = {}
        self.on_slot_dropped = self._step_graphs.clear
        self.set_precision(precision)

    # ---- precision -----------------------------------------------------------------------------
    def set_precision(self, precision):
        """'highest': every layer exact fp32.  'high': each layer whose forward, data gradient and filter gradient all run
        at bf16x3 (include/srx.h, srx_conv2d_precision_supported -- VDSR's 3x3 64 -> 64 body layers) uses it for all three
        passes, every other layer stays exact.  Decided here, once per layer, from its spec; `layer_precision` holds the
        choice ('high' / 'highest' per layer).  Parameters, gradients, optimizer slots and checkpoints are fp32 either way."""
        if precision not in ('highest', 'high'):
            raise ValueError("precision must be 'highest' or 'high', got %r" % (precision,))
        self.precision = precision
        choice = []
        last = len(self.specs) - 1
        for i, s in enumerate(self.specs):
            ok = precision == 'high' and not (self.residual and i == last)    # (the residual add is a skip operand: exact path only)
            if ok:
                x_shape = (1, 1, 1, s.cin)
                ok = all(ops.precision_supported(x_shape, s.kernel_shape, op, s.padding, s.act if op == ops._lib.OP_FWD else None,
                                                 precision='high')[0]
                         for op in (ops._lib.OP_FWD, ops._lib.OP_BWD_DATA, ops._lib.OP_BWD_FILTER))
            choice.append('high' if ok else 'highest')
        self.layer_precision = choice
        self._step_graphs.clear()      # a captured step holds the launches of the old choice

    # ---- parameter views -------------------------------------------------------------------
    global_step = property(lambda self: self.t, lambda self, value: setattr(self, 't', value),
                           doc="The pool's step count under the name of the reference's variable.")

    def kernel(self, i, buf=None):
        return self.view(2 * i, buf)

    def bias(self, i, buf=None):
        return self.view(2 * i + 1, buf)

    def set_params(self, pairs):
        """pairs: [(kernel, bias)] per layer (numpy or torch)."""
        for i, (k, b) in enumerate(pairs):
            self.kernel(i).copy_(torch.as_tensor(k, dtype=torch.float32).to(self.device))
            self.bias(i).copy_(torch.as_tensor(b, dtype=torch.float32).to(self.device))

    # ---- buffers ------------------------------------------------------------------------------
    def _buf(self, key, shape):
        t = self._bufs.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            if t is not None:
                self._step_graphs.clear()      # a captured step points at the buffer that is about to be released
            t = torch.empty(shape, dtype=torch.float32, device=self.device)
            self._bufs[key] = t
        return t

    def _shapes(self, x_shape):
        n, h, w, _ = x_shape
        shapes = []
        for s in self.specs:
            h, w = s.out_hw(h, w)
            shapes.append((n, h, w, s.cout))
        return shapes

    # ---- forward ------------------------------------------------------------------------------
    def forward(self, x, keep=True):
        """Returns the stack output; with keep=True every layer's output is kept for backward()
        and exposed through `self.acts` (acts[0] is the input, acts[i+1] layer i's output)."""
        shapes = self._shapes(x.shape)
        if keep and self.forward_keep_hook is not None:
            # a model's one-launch forward pass (ESPCN: srx_espcn_forward_keep) writing the same activation buffers
            outs = [self._buf(('act', i), shapes[i]) for i in range(len(self.specs))]
            if self.forward_keep_hook(x, outs):
                self._acts = self.acts = [x] + outs
                return outs[-1]
        acts = [x]

        def out_buf(i):
            # keep=False: keyed by parity and channel count, not by the full shape: a new image size replaces the old
            # buffer instead of piling up one pair per size (a directory of images of many sizes)
            return self._buf(('act', i) if keep else ('tmp', i & 1, self.specs[i].cout), shapes[i])

        for op in plan_forward(self.specs, self.residual, self.layer_precision, [x.shape] + shapes):
            if type(op) is Chain:
                # body layers lo .. hi in one launch (srx_conv_chain): the same bits as one launch per layer
                ks, s = range(op.lo, op.hi + 1), self.specs[op.lo]
                outs = [out_buf(k) for k in ks]
                ops.conv2d_fwd_chain(acts[-1:] + outs[:-1], [self.kernel(k) for k in ks], [self.bias(k) for k in ks], outs, s.padding, s.act)
                acts.extend(outs)
            else:
                i, s = op.i, self.specs[op.i]
                skip = x if (self.residual and i == len(self.specs) - 1) else None
                acts.append(ops.conv2d_fwd(acts[-1], self.kernel(i), self.bias(i), s.padding, s.act, skip=skip, out=out_buf(i),
                                           precision=self.layer_precision[i]))
        self._acts = acts if keep else None
        self.acts = acts
        return acts[-1]

    # ---- loss + backward ----------------------------------------------------------------------
    def loss_and_backward(self, target, numel_global=None):
        """MSE(output, target) [+ weight decay terms] into self.loss (device scalar) and the full
        gradient into self.grads.  With data parallelism pass nothing: every rank uses its LOCAL
        mean and the hook averages the gradients (identical to the global mean for equal shards;
        the regulariser gradient is the same on every rank, so averaging preserves it)."""
        if self._acts is None:
            raise RuntimeError('forward(keep=True) must run before loss_and_backward')
        acts = self._acts
        y = acts[-1]
        last = len(self.specs) - 1
        inv = 1.0 / (y.numel() if numel_global is None else numel_global)
        dy = self._buf(('dy', 0), y.shape)
        if self.loss_kind == 'rownorm':
            # srcnn/srcnn.py:142-144: mean over rows of ||reshape(diff, [-1, bb*bb])||_2
            row_len = y.shape[1] * y.shape[2]
            ops.rownorm_loss_fwd_bwd(y, target, row_len, self.loss, dpred=dy, norms=self._buf(('rownorms',), (y.numel() // row_len,)))
        else:
            ops.mse_fwd_bwd(y, target, self.loss, inv_numel=inv, accumulate=False, dpred=dy)
        if self.weight_decay:
            self.add_regulariser_loss()
        if self.specs[last].act is not None:
            ops.act_bwd(dy, y, self.specs[last].act, out=self._buf(('dpre_last',), y.shape))
        # the number of partial filters grows with batch and image size: re-query on every call (host-only) and
        # grow the workspace when a larger feed arrives
        prec, shapes = self.layer_precision, [t.shape for t in acts]
        need = max(ops.bwd_filter_workspace_bytes(shapes[i], s.kernel_shape, s.padding, precision=prec[i])
                   for i, s in enumerate(self.specs))
        plan = plan_backward(self.specs, self.residual, prec, shapes)
        for op in plan:
            if type(op) is WgradBatch:
                need = max(need, ops.bwd_filter_batch_workspace_bytes(shapes[op.lo], self.specs[op.lo].kernel_shape, op.hi - op.lo + 1,
                                                                      self.specs[op.lo].padding))
        if self._ws is None or self._ws.numel() * 4 < need:
            self._step_graphs.clear()
            self._ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.device)

        def dpre(i, key):
            return self._buf(key, shapes[i + 1])        # (the gradient at layer i's output)

        for op in plan:
            if type(op) is Wgrad:
                i, s = op.i, self.specs[op.i]
                ops.conv2d_bwd_filter(acts[i], dpre(i, op.dpre_key), s.kernel_shape, s.padding,
                                      w_for_decay=self.kernel(i) if self.weight_decay else None, wd_scale=self.weight_decay,
                                      dw=self.kernel(i, self.grads), dbias=self.bias(i, self.grads), workspace=self._ws, precision=prec[i])
            elif type(op) is Dgrad:
                i, prev_act = op.i, self.specs[op.i - 1].act
                ops.conv2d_bwd_data(dpre(i, op.src_key), self.kernel(i), shapes[i], self.specs[i].padding,
                                    x_in=acts[i] if prev_act is not None else None, in_act=prev_act, out=dpre(i - 1, op.dst_key),
                                    precision=prec[i])
            elif type(op) is DgradChain:
                ks = range(op.hi, op.lo - 1, -1)
                outs = [dpre(k - 1, key) for k, key in zip(ks, op.dst_keys)]
                ops.conv2d_bwd_data_chain([dpre(op.hi, op.src_key)] + outs[:-1], [self.kernel(k) for k in ks], [acts[k] for k in ks],
                                          outs, shapes[op.hi], self.specs[op.hi].padding, in_act=self.specs[op.hi - 1].act)
            else:
                ks = range(op.lo, op.hi + 1)
                ops.conv2d_bwd_filter_batch([acts[k] for k in ks], [dpre(k, key) for k, key in zip(ks, op.dpre_keys)],
                                            [self.kernel(k, self.grads) for k in ks], [self.bias(k, self.grads) for k in ks],
                                            [self.kernel(k) for k in ks] if self.weight_decay else None, self.weight_decay,
                                            self.specs[op.lo].padding, workspace=self._ws)
        if self.grad_hook is not None:
            self.grad_hook(self.grads)
        return self.loss

    def add_regulariser_loss(self):
        """self.loss += weight_decay * sum over kernels of sum(w^2)/2 -- one launch over the flat buffer."""
        if self._decay_mask is None:
            self._decay_mask = torch.zeros_like(self.params)
            for i in range(len(self.specs)):
                self.kernel(i, self._decay_mask).fill_(1.0)
        ops.l2_loss(self.params, self.weight_decay, self.loss, accumulate=True, mask=self._decay_mask)

    # ---- optimizers (ParamPool.adam_step / adam_step_dev / momentum_clip_step) ---------------------
    def train_step_replay(self, x, target, lr, beta1=0.9, beta2=0.999, eps=1e-8, momentum=None, gradient_cap=0.01):
        """forward + loss_and_backward + optimizer as ONE replayed HIP graph per (input shape, target shape, optimizer
        constants).  momentum=None: TF-Adam with the step count and the learning rate in device memory
        (srx_adam_tf_step_dev) -- a changing rate needs no new graph; momentum=m: Momentum on clipped gradients
        (momentum_clip_step), whose rate is a kernel argument: the graph is keyed by it (VDSR's schedule changes it every
        few thousand steps).  The first two steps of a shape run as eager launches (they are real steps: buffers, workspaces
        and kernel attributes come into being), the third is captured -- capturing executes nothing -- and replayed, like
        every step after it.  Eager and replayed steps issue the same kernels with the same arguments: the weights are
        bit-identical either way (tests/test_gpu_models.py).  Falls back to eager launches when a gradient hook (data
        parallelism) is attached or SRX_STEP_GRAPH=0.  Returns the device scalar of the loss."""
        def optimizer_launch():
            if momentum is None:
                self.adam_launch_dev(beta1, beta2, eps)
            else:
                ops.momentum_clip_step(self.params, self.grads, self.opt_m, lr, momentum, gradient_cap / lr)

        def eager(xx, tt):
            self.forward(xx, keep=True)
            self.loss_and_backward(tt)
            if momentum is None:
                self.adam_step_dev(lr, beta1, beta2, eps)
            else:
                self.momentum_clip_step(lr, momentum, gradient_cap)
            return self.loss
        if not self.use_step_graph or self.grad_hook is not None or self.device.type != 'cuda':
            return eager(x, target)
        if self.step_graph_max_pixels is not None and x.shape[0] * x.shape[1] * x.shape[2] > self.step_graph_max_pixels:
            return eager(x, target)          # (measured per model: beyond this size the replay is no faster than the launches)
        opt_key = (float(beta1), float(beta2), float(eps)) if momentum is None else ('momentum', float(lr), float(momentum), float(gradient_cap))
        key = (tuple(x.shape), tuple(target.shape)) + opt_key
        ent = self._step_graphs.get(key)
        if ent is None:
            if len(self._step_graphs) >= 4:
                self._step_graphs.clear()
            ent = self._step_graphs[key] = {'warm': 0, 'graph': None}
        if ent['graph'] is None:
            if ent['warm'] < 2:
                ent['warm'] += 1
                loss = eager(x, target)
                if key not in self._step_graphs:         # (the first step of a new shape replaced buffers: start over, warm)
                    self._step_graphs[key] = ent
                return loss
            self.ensure_slots(2 if momentum is None else 1)
            if momentum is None:
                self.sync_adam_state(lr)
            sx, st = x.clone(), target.clone()
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with capture_graph(g):
                self.forward(sx, keep=True)
                self.loss_and_backward(st)
                optimizer_launch()
            ent.update(graph=g, x=sx, t=st)
        if momentum is None:
            self.sync_adam_state(lr)
        if x.data_ptr() != ent['x'].data_ptr():
            ent['x'].copy_(x)
        if target.data_ptr() != ent['t'].data_ptr():
            ent['t'].copy_(target)
        ent['graph'].replay()
        if momentum is None:
            self.count_dev_step()
        else:
            self.t += 1
        return self.loss

    def static_step_inputs(self, x_shape, target_shape):
        """The input / target tensors a captured train step of these shapes reads (None before it exists): a training loop
        that writes its batches straight into them (the host-to-device copy it makes anyway) and passes them to
        train_step_replay replays without the device-side copies."""
        for key, ent in self._step_graphs.items():
            if ent.get('graph') is not None and key[0] == tuple(x_shape) and key[1] == tuple(target_shape):
                return ent['x'], ent['t']
        return None

    # ---- checkpoint (own format, TF variable names) -----------------------------------------
    def state_dict(self):
        sd = {'global_step': self.global_step, 'params': self.params.detach().cpu()}
        if self.opt_m is not None:
            sd['opt_m'] = self.opt_m.detach().cpu()
        if self.opt_v is not None:
            sd['opt_v'] = self.opt_v.detach().cpu()
        return sd

    # ---- TensorFlow V2 checkpoints (tf.train.Saver format; tf_bundle.py) --------------------------
    def tf_checkpoint_tensors(self, adam_betas=(0.9, 0.999), extra=None):
        """{checkpoint key: ndarray} as tf.train.Saver would write this model: `<scope>/kernel`, `<scope>/bias`,
        `global_step` (int64) and, when an optimizer has run, its slots: Adam `<var>/Adam`, `<var>/Adam_1`,
        `beta1_power`, `beta2_power`; Momentum `<var>/Momentum`.  `extra`: further global variables of the
        reference graph ({name: array}; VDSR's non-trainable `learning_rate`, vdsr/vdsr/model_vdsr.py:136-141 --
        Saver().restore needs every global variable to be present).
        beta powers: TF-1.x AdamOptimizer creates them with the value beta and multiplies them by beta once per
        apply (_finish), so after N steps the checkpoint holds float32(beta) ** (N + 1) (tf_bundle.tf_beta_power).
        UNVERIFIED CONVENTIONS -- TensorFlow's source is not available here and no TF-written checkpoint exists to
        check against; a maintainer holding a real `model.ckpt-25600` should check, in
        this order: (1) the key set of its `.index` (tf_bundle.list_variables) against this function's: the non-slot
        accumulators are expected at top level as `beta1_power` / `beta2_power` (a second optimizer in the same graph:
        `beta1_power_1` / `beta2_power_1`), the slots as `<var>/Adam` (m) and `<var>/Adam_1` (v), Momentum's as
        `<var>/Momentum`; (2) that `beta1_power` equals 0.9 ** (global_step + 1) and not ** global_step; (3) that the
        layer scopes are `conv2d`, `conv2d_1`, ... in creation order (tf.layers' auto-numbering) for VDSR and
        `f1` / `f2` / `f3` for ESPCN; (4) dtype / shape of `global_step` (int64 scalar expected).  The container format
        itself (table blocks, CRCs, BundleEntryProto fields) is checked against published known-answer vectors only."""
        import numpy as np
        from . import tf_bundle
        out = self.tf_tensors()
        out['global_step'] = np.asarray(self.global_step, dtype=np.int64)
        for k, v in (extra or {}).items():
            out[k] = np.asarray(v)
        if self.opt_m is not None and self.opt_v is not None:
            out['beta1_power'] = tf_bundle.tf_beta_power(adam_betas[0], self.global_step)
            out['beta2_power'] = tf_bundle.tf_beta_power(adam_betas[1], self.global_step)
        return out

    def save_tf_checkpoint(self, prefix, adam_betas=(0.9, 0.999), extra=None, write_state=True):
        """Writes `<prefix>.index` + `<prefix>.data-00000-of-00001` and (write_state) the `checkpoint` state file
        (CheckpointState text proto) next to them, which is what tf.train.latest_checkpoint(dir) reads
        (vdsr/vdsr/experiment_train.py:108)."""
        from . import tf_bundle
        tf_bundle.save_checkpoint(prefix, self.tf_checkpoint_tensors(adam_betas, extra))
        if write_state:
            tf_bundle.update_checkpoint_state(prefix)

    def load_tf_checkpoint(self, prefix, with_optimizer=True):
        """Restores kernels / biases (and global_step, optimizer slots when present) from a checkpoint written by
        the reference's `tf.train.Saver` (vdsr/vdsr/experiment_train.py:100-121) or by save_tf_checkpoint."""
        from . import tf_bundle
        values = tf_bundle.load_checkpoint(prefix)
        self.load_tf_tensors(values, 'checkpoint %s' % prefix, with_optimizer)
        if 'global_step' in values:
            self.global_step = int(values['global_step'])

    def load_checkpoint(self, path):
        """`path`: a TensorFlow V2 checkpoint prefix (as the reference's --ckpt_path, e.g. .../model.ckpt-25600)
        or a state dict saved with torch.save(stack.state_dict())."""
        from . import tf_bundle
        if tf_bundle.is_checkpoint_prefix(path):
            self.load_tf_checkpoint(path)
        else:
            self.load_state_dict(torch.load(path))

    def load_state_dict(self, sd):
        self.params.copy_(sd['params'].to(self.device))
        self.global_step = int(sd['global_step'])
        # in place, as in load_tf_checkpoint: captured train steps keep reading the restored slots
        for attr in ('opt_m', 'opt_v'):
            if attr in sd:
                self.restore_slot(attr, lambda buf: buf.copy_(sd[attr].to(self.device)))
        if 'opt_m' in sd and 'opt_v' not in sd:
            self.drop_second_slot()


# ---- initialisers (the reference's; TF's RNG stream itself cannot be reproduced) --------------
def xavier_uniform_(t, generator=None):
    """tf.contrib.layers.xavier_initializer(): U(+-sqrt(6/(fan_in+fan_out))), fan = kh*kw*C.
    vdsr/vdsr/model_vdsr.py:27."""
    kh, kw, cin, cout = t.shape
    lim = math.sqrt(6.0 / (kh * kw * cin + kh * kw * cout))
    t.copy_((torch.rand(t.shape, generator=generator) * 2 - 1).mul_(lim).to(t.device))


def truncated_normal_(t, stddev, generator=None):
    """tf.truncated_normal_initializer(stddev): redraw beyond 2 sigma.
    espcn/espcn/model_espcn.py:21, srcnn/srcnn.py:84."""
    v = torch.randn(t.shape, generator=generator)
    bad = v.abs() > 2
    while bad.any():
        v[bad] = torch.randn(int(bad.sum()), generator=generator)
        bad = v.abs() > 2
    t.copy_(v.mul_(stddev).to(t.device))
