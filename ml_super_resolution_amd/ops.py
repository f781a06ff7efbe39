"""Thin op wrappers over the C ABI.  Tensors are torch CUDA(ROCm) float32, NHWC activations,
HWIO filters.  Every call is asynchronous on torch's current stream."""
import ctypes
import functools
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import ACT_BY_NAME, PAD_BY_NAME, ConvDesc, check
from ._lib import lib as _load_lib

# SRX_POISON_LDS=1 (test aid): every CU's LDS is filled with NaNs before each call into the library, so a kernel that depends on
# LDS bytes it has not written shows up in the parity tests (include/srx.h: srx_debug_poison_lds)
_POISON_LDS = os.environ.get('SRX_POISON_LDS', '0') == '1'


def lib():
    L = _load_lib()
    if _POISON_LDS and torch.cuda.is_available():
        L.srx_debug_poison_lds(_stream())
    return L


def _stream():
    # torch.cuda.current_stream().cuda_stream without building a Stream object per launch (an int: all argument types are declared)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- the argument checks: every tensor whose address reaches the library first passes _chk, _chk_u8, _holds or _out
def _refusal(t, name, dtype, index):
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        return '%s must be a contiguous %s tensor on the GPU' % (name, str(dtype)[6:])
    # (the launch goes to the CURRENT device's stream; one process per GPU: call torch.cuda.set_device(local_rank) first)
    return '%s lives on %s but the current device is cuda:%d' % (name, t.device, index)


def _holds(n, device, *named, dtype=torch.float32, at_least=False):
    """Every tensor of `named` (t, name, t, name, ...; None is skipped) is a contiguous `dtype` tensor on `device` -- that of a
    tensor that has passed already, or None: the current GPU, asked for once -- and holds exactly n elements (at_least: n or
    more; n None: any number).  A name given as (name, n) has a count of its own, and (name, n, _LEAST), (name, n, _REQUIRED)
    or (name, n, _LEAST | _REQUIRED) may hold more / may not be None: so one call, one loop and four attribute reads per tensor
    serve a whole wrapper.  These run in front of every launch."""
    index = None if device is None else device.index
    for k in range(0, len(named), 2):
        t, name, want, least = named[k], named[k + 1], n, at_least
        if type(name) is tuple:
            if len(name) > 2:
                least = name[2] & _LEAST
                if t is None and name[2] & _REQUIRED:
                    raise ValueError('%s is required' % name[0])
            name, want = name[0], name[1]
        if t is None:
            continue
        if index is None:
            index = torch.cuda.current_device() if t.is_cuda else -2
        if t.dtype != dtype or t.get_device() != index or not t.is_contiguous():        # (get_device: -1 off the GPU)
            raise ValueError(_refusal(t, name, dtype, index))
        if want is not None and (t.numel() < want if least else t.numel() != want):
            raise ValueError('%s must hold %s%d elements, got %d' % (name, 'at least ' if least else '', want, t.numel()))


_LEAST, _REQUIRED = 1, 2
_chk = functools.partial(_holds, None, None)                          # n None, device None: any count, on the current GPU
_chk_u8 = functools.partial(_holds, None, None, dtype=torch.uint8)


def _out(out, shape, dtype, device, wrong='%(name)s must hold %(want)d elements, got %(got)d', name='out'):
    """A new tensor of `shape`, or the caller's `out` (under `name`) checked for that kind, `device` (that of a checked input) and
    as many elements: a flat or reshaped buffer of the right size is taken.  wrong: the refusal of another count."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError(_refusal(out, name, dtype, device.index))
    want = math.prod(shape)
    if out.numel() != want:
        raise ValueError(wrong % {'name': name, 'want': want, 'got': out.numel()})
    return out


def precision_code(precision):
    """'highest' -> 0 (exact fp32), 'high' -> 1 (bf16x3: split-bf16 products), or the int itself (torch's names:
    torch.set_float32_matmul_precision)."""
    if isinstance(precision, str):
        if precision not in _lib.PRECISION_BY_NAME:
            raise ValueError("precision must be 'highest', 'high' or an int, got %r" % precision)
        return _lib.PRECISION_BY_NAME[precision]
    return int(precision)


def conv_desc(x_shape, w_shape, padding='same', act=None, post_add_relu=False, subpixel_r=0, stride=1, precision='highest'):
    N, H, W, Cin = x_shape
    KH, KW, wci, Cout = w_shape
    if wci != Cin:
        raise ValueError('filter Cin %d != input channels %d' % (wci, Cin))
    return ConvDesc(N, H, W, Cin, Cout, KH, KW, int(stride), PAD_BY_NAME[padding.lower()],
                    ACT_BY_NAME[act] if not isinstance(act, int) else act, int(post_add_relu), precision_code(precision),
                    int(subpixel_r))


def precision_supported(x_shape, w_shape, op=_lib.OP_FWD, padding='same', act=None, post_add_relu=False, subpixel_r=0, stride=1,
                        precision='high'):
    """(supported, reason) -- srx_conv2d_precision_supported: does `op` (OP_FWD / OP_BWD_DATA / OP_BWD_FILTER) of this
    layer run at `precision`?  reason is srx_last_error() when it does not, else ''.  Host-only."""
    d = conv_desc(x_shape, w_shape, padding, act, post_add_relu, subpixel_r, stride, precision)
    L = _load_lib()
    ok = L.srx_conv2d_precision_supported(ctypes.byref(d), int(op)) == 1
    return ok, ('' if ok else L.srx_last_error().decode())


def out_shape(d):
    """TensorFlow's geometry: SAME ceil(in / stride); VALID (in - k) / stride + 1."""
    s = d.stride
    if d.pad_mode == _lib.PAD_SAME:
        return (d.N, (d.H + s - 1) // s, (d.W + s - 1) // s, d.Cout)
    return (d.N, (d.H - d.KH) // s + 1, (d.W - d.KW) // s + 1, d.Cout)


_scratch = {}


def reduce_scratch(device):
    key = (device.type, device.index)
    if key not in _scratch:
        _scratch[key] = torch.empty(lib().srx_reduce_scratch_bytes() // 4, dtype=torch.float32, device=device)
    return _scratch[key]


def conv2d_fwd(x, w, bias=None, padding='same', act=None, skip=None, post_add_relu=False, out=None, subpixel_r=0, stride=1,
               precision='highest'):
    """act(bias + x (*) w) [+ skip] [relu] -- srx_conv2d_fwd.  subpixel_r > 1: the result is stored through the
    depth-to-space map, [N,OH*r,OW*r,Cout/r^2] (bit-identical to conv2d_fwd + depth_to_space, one launch).
    stride 1 or 2 (tf.layers.conv2d(strides=2, padding='same'): enet/enet/model_enet.py:136-146).
    precision: 'highest' (exact fp32) or 'high' (bf16x3 products; include/srx.h, srx_precision)."""
    _chk(x, 'x', w, 'w', bias, ('bias', w.shape[-1]))
    d = conv_desc(x.shape, w.shape, padding, act, post_add_relu, subpixel_r, stride, precision)
    shape = out_shape(d)
    if subpixel_r > 1:
        r = int(subpixel_r)
        if shape[3] % (r * r):
            raise ValueError('subpixel_r %d: %d output channels are not a multiple of r*r' % (r, shape[3]))
        shape = (shape[0], shape[1] * r, shape[2] * r, shape[3] // (r * r))
    if skip is not None:
        _holds(math.prod(shape), x.device, skip, 'skip')
    if out is not None and tuple(out.shape) != tuple(shape):
        raise ValueError('out has shape %s, expected %s' % (tuple(out.shape), tuple(shape)))
    y = _out(out, shape, torch.float32, x.device)
    check(lib().srx_conv2d_fwd(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(bias), _ptr(skip), _ptr(y), None, 0, _stream()),
          'srx_conv2d_fwd')
    return y


def _dpre_count(x_shape, w_shape, padding):
    """The elements of a stride-1 layer's output, out_shape(d) without reading the descriptor back."""
    (N, H, W, _), (KH, KW, _, Cout) = x_shape, w_shape
    return N * H * W * Cout if padding.lower() == 'same' else N * (H - KH + 1) * (W - KW + 1) * Cout


def conv2d_bwd_data(dpre, w, x_shape, padding='same', x_in=None, in_act=None, out=None, precision='highest'):
    """dx * act'(x_in) -- srx_conv2d_bwd_data."""
    d = conv_desc(x_shape, w.shape, padding, precision=precision)
    _chk(w, 'w', dpre, ('dpre', _dpre_count(x_shape, w.shape, padding)), x_in, ('x_in', math.prod(x_shape)))
    dx = _out(out, tuple(x_shape), torch.float32, w.device)
    check(lib().srx_conv2d_bwd_data(ctypes.byref(d), _ptr(dpre), _ptr(w), _ptr(x_in), ACT_BY_NAME[in_act],
                                    _ptr(dx), None, 0, _stream()), 'srx_conv2d_bwd_data')
    return dx


def chain_supported(x_shape, w_shape, op=_lib.OP_FWD, padding='same', act=None, in_act=None, precision='highest'):
    """srx_conv_chain_supported: does srx_conv_chain take this layer for `op` (OP_FWD / OP_BWD_DATA)?  Host-only."""
    d = conv_desc(x_shape, w_shape, padding, act, precision=precision)
    return lib().srx_conv_chain_supported(ctypes.byref(d), int(op), ACT_BY_NAME[in_act]) == 1


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def conv2d_fwd_chain(xs, ws, biases, outs, padding='same', act=None):
    """outs[l] = act(biases[l] + xs[l] (*) ws[l]) for consecutive layers of one shape in ONE launch -- srx_conv_chain.
    The same bits as one conv2d_fwd per layer; layer l may read what an earlier layer wrote (xs[l] is outs[l - 1]).
    Raises SrxError when the chain is not eligible (chain_supported)."""
    for l in range(len(xs)):
        _chk(xs[l], 'x', ws[l], 'w', outs[l], 'out')
        _holds(ws[l].shape[-1], ws[l].device, biases[l], 'bias')
    d = conv_desc(xs[0].shape, ws[0].shape, padding, act)
    shape = out_shape(d)
    for l in range(len(xs)):
        if tuple(xs[l].shape) != tuple(xs[0].shape) or tuple(ws[l].shape) != tuple(ws[0].shape) or tuple(outs[l].shape) != shape:
            raise ValueError('conv2d_fwd_chain: layer %d does not have the shape of layer 0' % l)
    check(lib().srx_conv_chain(ctypes.byref(d), _lib.OP_FWD, _lib.ACT_NONE, len(xs), _ptr_array(xs), _ptr_array(ws), _ptr_array(biases),
                               None, _ptr_array(outs), _stream()), 'srx_conv_chain')
    return outs[-1]


def conv2d_bwd_data_chain(dpres, ws, x_ins, outs, x_shape, padding='same', in_act=None):
    """outs[l] = dx(dpres[l], ws[l]) * act'(x_ins[l]) for consecutive layers of one shape in ONE launch -- srx_conv_chain.
    The same bits as one conv2d_bwd_data per layer; dpres[l] may be outs[l - 1].  x_ins: None (no mask) or one per layer."""
    masks = x_ins if (x_ins is not None and in_act is not None) else None
    for l in range(len(dpres)):
        _chk(dpres[l], 'dpre', ws[l], 'w', outs[l], 'out')
        if tuple(outs[l].shape) != tuple(x_shape) or tuple(ws[l].shape) != tuple(ws[0].shape) or tuple(dpres[l].shape) != tuple(dpres[0].shape):
            raise ValueError('conv2d_bwd_data_chain: layer %d does not have the shape of layer 0' % l)
        _holds(outs[l].numel(), outs[l].device, None if masks is None else masks[l], 'x_in')
    d = conv_desc(x_shape, ws[0].shape, padding)
    if tuple(dpres[0].shape) != tuple(out_shape(d)):
        raise ValueError('dpre has shape %s, the layer output is %s' % (tuple(dpres[0].shape), tuple(out_shape(d))))
    check(lib().srx_conv_chain(ctypes.byref(d), _lib.OP_BWD_DATA, ACT_BY_NAME[in_act] if masks is not None else _lib.ACT_NONE, len(dpres),
                               _ptr_array(dpres), _ptr_array(ws), None, None if masks is None else _ptr_array(masks),
                               _ptr_array(outs), _stream()), 'srx_conv_chain')
    return outs[-1]


def set_chain(on):
    """srx_set_chain: 1 chains eligible body layers (default), 0 launches them one by one, < 0 the environment's default
    (SRX_CHAIN).  Returns the old value."""
    return lib().srx_set_chain(int(on))


def set_chain_fixed(on):
    """srx_set_chain_fixed: 1 runs chains of 41-pixel rows on the kernel instance with that tile geometry compiled in
    (default), 0 every chain on the generic instance, < 0 the environment's default (SRX_CHAIN_FIXED).  Same bits either
    way.  Returns the old value."""
    return lib().srx_set_chain_fixed(int(on))


def bwd_filter_workspace_bytes(x_shape, w_shape, padding='same', stride=1, precision='highest'):
    d = conv_desc(x_shape, w_shape, padding, stride=stride, precision=precision)
    return lib().srx_conv2d_workspace_bytes(ctypes.byref(d), _lib.OP_BWD_FILTER)


def conv2d_bwd_filter(x, dpre, w_shape, padding='same', w_for_decay=None, wd_scale=0.0, dw=None, dbias=None,
                      want_dbias=True, workspace=None, stride=1, precision='highest'):
    """(dw, dbias) -- srx_conv2d_bwd_filter.  stride 2: dpre is the gradient at the layer's (half-resolution) output."""
    d = conv_desc(x.shape, w_shape, padding, stride=stride, precision=precision)
    need = (lib().srx_conv2d_workspace_bytes(ctypes.byref(d), _lib.OP_BWD_FILTER) + 3) // 4
    _chk(x, 'x', dpre, 'dpre', w_for_decay, ('w_for_decay', math.prod(w_shape)), workspace, ('workspace', need, _LEAST))
    if tuple(dpre.shape) != tuple(out_shape(d)):
        raise ValueError('dpre has shape %s, the layer output is %s' % (tuple(dpre.shape), tuple(out_shape(d))))
    dw = _out(dw, tuple(w_shape), torch.float32, x.device, name='dw')
    if dbias is not None or want_dbias:
        dbias = _out(dbias, (w_shape[3],), torch.float32, x.device, name='dbias')
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=x.device)
    check(lib().srx_conv2d_bwd_filter(ctypes.byref(d), _ptr(x), _ptr(dpre), _ptr(dw), _ptr(dbias),
                                      _ptr(w_for_decay), float(wd_scale), _ptr(workspace),
                                      workspace.numel() * workspace.element_size(), _stream()), 'srx_conv2d_bwd_filter')
    return dw, dbias


def conv2d_bwd_filter_partials(x, dpre, w_shape, padding, workspace, precision='highest'):
    """First half of conv2d_bwd_filter: per-workgroup partial filters into `workspace`; returns their count."""
    d = conv_desc(x.shape, w_shape, padding, precision=precision)
    need = (lib().srx_conv2d_workspace_bytes(ctypes.byref(d), _lib.OP_BWD_FILTER) + 3) // 4
    _chk(x, 'x', dpre, ('dpre', math.prod(out_shape(d))), workspace, ('workspace', need, _LEAST | _REQUIRED))
    n = ctypes.c_int(0)
    check(lib().srx_conv2d_bwd_filter_partials(ctypes.byref(d), _ptr(x), _ptr(dpre), _ptr(workspace),
                                               workspace.numel() * workspace.element_size(), ctypes.byref(n), _stream()),
          'srx_conv2d_bwd_filter_partials')
    return n.value


def conv2d_bwd_filter_reduce(x_shape, w_shape, padding, workspace, n_partials, dw, dbias=None, w_for_decay=None, wd_scale=0.0,
                             precision='highest'):
    """Second half: sums the partials into dw / dbias on the CURRENT stream (the caller orders it after the first half)."""
    d = conv_desc(x_shape, w_shape, padding, precision=precision)
    need = (lib().srx_conv2d_workspace_bytes(ctypes.byref(d), _lib.OP_BWD_FILTER) + 3) // 4
    _holds(math.prod(w_shape), None, dw, ('dw', math.prod(w_shape), _REQUIRED), w_for_decay, 'w_for_decay', dbias, ('dbias', w_shape[3]),
           workspace, ('workspace', need, _LEAST | _REQUIRED))
    check(lib().srx_conv2d_bwd_filter_reduce(ctypes.byref(d), _ptr(workspace), int(n_partials), _ptr(dw), _ptr(dbias),
                                             _ptr(w_for_decay), float(wd_scale), _stream()), 'srx_conv2d_bwd_filter_reduce')
    return dw, dbias


def bwd_filter_batch_plan(x_shape, w_shape, n_layers, padding='same', stride=1, precision='highest'):
    """(workgroups per layer, grid) of conv2d_bwd_filter_batch for n_layers layers of this shape -- (0, 0) when the batch is
    not eligible (srx_conv2d_bwd_filter_batch_plan; the reason is srx_last_error()).  Host-only."""
    d = conv_desc(x_shape, w_shape, padding, stride=stride, precision=precision)
    wpl, grid = ctypes.c_int(0), ctypes.c_int(0)
    _load_lib().srx_conv2d_bwd_filter_batch_plan(ctypes.byref(d), int(n_layers), ctypes.byref(wpl), ctypes.byref(grid))
    return wpl.value, grid.value


def bwd_filter_batch_workspace_bytes(x_shape, w_shape, n_layers, padding='same', stride=1, precision='highest'):
    """Workspace bytes of conv2d_bwd_filter_batch; 0 when the batch is not eligible.  Host-only."""
    d = conv_desc(x_shape, w_shape, padding, stride=stride, precision=precision)
    return _load_lib().srx_conv2d_bwd_filter_batch_workspace_bytes(ctypes.byref(d), int(n_layers))


def conv2d_bwd_filter_batch(xs, dpres, dws, dbiases=None, w_for_decay=None, wd_scale=0.0, padding='same', workspace=None,
                            stride=1, precision='highest'):
    """dws[l], dbiases[l] = the filter and bias gradients of layer l (input xs[l], upstream gradient dpres[l]) for layers of
    ONE shape, in one launch and one reduction -- srx_conv2d_bwd_filter_batch.  dbiases / w_for_decay: None, or one entry
    per layer (entries may be None).  Raises SrxError when the batch is not eligible (bwd_filter_batch_plan)."""
    L = len(xs)
    if not (len(dpres) == len(dws) == L) or (dbiases is not None and len(dbiases) != L) or (w_for_decay is not None and len(w_for_decay) != L):
        raise ValueError('conv2d_bwd_filter_batch: the per-layer lists differ in length')
    for l in range(L):
        _chk(xs[l], 'x', dpres[l], 'dpre', dws[l], 'dw')
    d = conv_desc(xs[0].shape, dws[0].shape, padding, stride=stride, precision=precision)
    for l in range(L):
        if tuple(xs[l].shape) != tuple(xs[0].shape) or tuple(dpres[l].shape) != tuple(out_shape(d)) or tuple(dws[l].shape) != tuple(dws[0].shape):
            raise ValueError('conv2d_bwd_filter_batch: layer %d does not have the shape of layer 0' % l)
        _holds(d.Cout, xs[0].device, None if dbiases is None else dbiases[l], 'dbias')
        _holds(dws[l].numel(), xs[0].device, None if w_for_decay is None else w_for_decay[l], 'w_for_decay')
    need = (_load_lib().srx_conv2d_bwd_filter_batch_workspace_bytes(ctypes.byref(d), L) + 3) // 4
    _holds(need, xs[0].device, workspace, 'workspace', at_least=True)
    if workspace is None:
        workspace = torch.empty(max(need, 4), dtype=torch.float32, device=xs[0].device)
    check(lib().srx_conv2d_bwd_filter_batch(ctypes.byref(d), L, _ptr_array(xs), _ptr_array(dpres), _ptr_array(dws),
                                            None if dbiases is None else _ptr_array(dbiases),
                                            None if w_for_decay is None else _ptr_array(w_for_decay), float(wd_scale),
                                            _ptr(workspace), workspace.numel() * workspace.element_size(), _stream()),
          'srx_conv2d_bwd_filter_batch')
    return dws, dbiases


def set_wgrad_batch(on):
    """srx_set_wgrad_batch: 1 runs eligible runs of layers' filter gradients as one batch (default), 0 launches them one by
    one, < 0 the environment's default (SRX_WGRAD_BATCH).  Returns the old value."""
    return lib().srx_set_wgrad_batch(int(on))


def act_bwd(dy, y, act, out=None):
    _holds(dy.numel(), None, dy, 'dy', y, 'y')
    out = _out(out, dy.shape, torch.float32, dy.device)
    check(lib().srx_act_bwd(_ptr(dy), _ptr(y), _ptr(out), dy.numel(), ACT_BY_NAME[act], _stream()), 'srx_act_bwd')
    return out


def depth_to_space(x, r, out=None):
    """[N,H,W,C*r*r] -> [N,H*r,W*r,C], TF channel order (dy,dx,c)."""
    _chk(x, 'x')
    N, H, W, D = x.shape
    if D % (r * r):
        raise ValueError('depth %d not divisible by r*r=%d' % (D, r * r))
    C = D // (r * r)
    out = _out(out, (N, H * r, W * r, C), torch.float32, x.device)
    check(lib().srx_depth_to_space(_ptr(x), _ptr(out), N, H, W, C, r, _stream()), 'srx_depth_to_space')
    return out


def _espcn_params(params, channels, r, who):
    """The three (kernel, bias) pairs of ESPCN 5-3-3 at scaling factor r for an input of `channels` channels, checked; who:
    the entry point, for the refusal."""
    (w1, b1), (w2, b2), (w3, b3) = params
    _chk(w1, 'kernel', b1, ('bias', 64), w2, 'kernel', b2, ('bias', 32), w3, 'kernel', b3, ('bias', 3 * r * r))
    if channels != 3 or tuple(w1.shape) != (5, 5, 3, 64) or tuple(w2.shape) != (3, 3, 64, 32) or tuple(w3.shape) != (3, 3, 32, 3 * r * r):
        raise ValueError('%s: shapes do not describe ESPCN 5-3-3 with scaling factor %d' % (who, r))
    return params


def espcn_forward(x, params, r, out=None):
    """ESPCN inference in one launch -- srx_espcn_forward.  params = [(w1, b1), (w2, b2), (w3, b3)] (HWIO kernels);
    x [N,H,W,3] -> [N,H*r,W*r,3]."""
    _chk(x, 'x')
    N, H, W, C = x.shape
    (w1, b1), (w2, b2), (w3, b3) = _espcn_params(params, C, r, 'espcn_forward')
    out = _out(out, (N, H * r, W * r, 3), torch.float32, x.device)
    check(lib().srx_espcn_forward(_ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(out),
                                  N, H, W, int(r), _stream()), 'srx_espcn_forward')
    return out


def _chk_lut(lut, n=256):
    _chk(lut, 'lut')
    if lut.numel() != n:
        raise ValueError('lut must hold %d floats, one per %s, got %d' % (n, 'byte value' if n == 256 else 'code', lut.numel()))


def unit_lut(device, depth=8):
    """The 256 floats of the host route's `lr_image / 127.5 - 1.0` (espcn/espcn/experiment_test.py:160): float64
    arithmetic on the uint8 values, then one cast.  depth 10 / 12: the 2^depth floats of the same expression for codes of that
    many bits, `code / (max / 2.0) - 1.0` with max = 2^depth - 1."""
    if depth not in (8, 10, 12):
        raise ValueError('depth must be 8, 10 or 12, got %r' % (depth,))
    return torch.from_numpy((np.arange(1 << depth) / (((1 << depth) - 1) / 2.0) - 1.0).astype(np.float32)).to(device)


def espcn_forward_u8(lr_u8, lut, params, r, out=None):
    """ESPCN inference from bytes to bytes in one launch -- srx_espcn_forward_u8: lr_u8 [N,H,W,3] uint8 read through the
    256-float table lut, [N,H*r,W*r,3] uint8 out (encode_unit_u8 of the floats espcn_forward gives).  out: a contiguous
    uint8 tensor of that many elements at any byte offset, or None for a new one."""
    _chk_u8(lr_u8, 'lr_u8')
    _chk_lut(lut)
    N, H, W, C = lr_u8.shape
    (w1, b1), (w2, b2), (w3, b3) = _espcn_params(params, C, r, 'espcn_forward_u8')
    out = _out(out, (N, H * r, W * r, 3), torch.uint8, lr_u8.device, 'espcn_forward_u8: out must hold %(want)d bytes, got %(got)d')
    check(lib().srx_espcn_forward_u8(_ptr(lr_u8), _ptr(lut), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(out),
                                     N, H, W, int(r), _stream()), 'srx_espcn_forward_u8')
    return out


def u8_lut_float(x_u8, lut, out=None):
    """uint8 -> float32 through a 256-float table (srx_u8_lut_float): out = lut[x_u8], bit for bit."""
    _chk_u8(x_u8, 'x_u8')
    _chk_lut(lut)
    out = _out(out, x_u8.shape, torch.float32, x_u8.device, 'u8_lut_float: sizes differ')
    check(lib().srx_u8_lut_float(_ptr(x_u8), _ptr(lut), _ptr(out), x_u8.numel(), _stream()), 'srx_u8_lut_float')
    return out


def unit_u8(x, out=None):
    """float32 in [-1, 1] -> uint8 as ESPCN's inference script encodes (srx_unit_u8, csrc/u8_encode.h: encode_unit_u8):
    `* 0.5 + 0.5`, clip to [0, 1], `* 255.0 + 0.5`, truncation -- five roundings.  out: a contiguous uint8 tensor of as many
    elements at any byte offset, or None for a new one."""
    _chk(x, 'x')
    out = _out(out, x.shape, torch.uint8, x.device, 'unit_u8: sizes differ')
    check(lib().srx_unit_u8(_ptr(x), _ptr(out), x.numel(), _stream()), 'srx_unit_u8')
    return out


yuv420_frame_bytes = _lib.yuv420_frame_bytes


def yuv420_coeffs(matrix='bt601', full_range=False):
    """The integer coefficients of a matrix ('bt601' / 'bt709') and range as _lib.Yuv420Coeffs, from srx_yuv420_coeffs: the
    library's host function is the one place that computes them.  No GPU call."""
    if matrix not in _lib.YUV_MATRIX_BY_NAME:
        raise ValueError("matrix must be 'bt601' or 'bt709', got %r" % (matrix,))
    c = _lib.Yuv420Coeffs()
    check(_load_lib().srx_yuv420_coeffs(_lib.YUV_MATRIX_BY_NAME[matrix], int(bool(full_range)), ctypes.byref(c)), 'srx_yuv420_coeffs')
    return c


_YUV_HOLDS = '%s must hold %d frames of %d bytes (%d x %d, 4:2:0), got %%(got)d bytes'


def _chk_yuv(t, name, n, height, width):
    _chk_u8(t, name)
    if n < 1 or height < 1 or width < 1:
        raise ValueError('%s: N, height and width must be positive, got %d, %d, %d' % (name, n, height, width))
    if t.numel() != n * yuv420_frame_bytes(height, width):
        raise ValueError(_YUV_HOLDS % (name, n, yuv420_frame_bytes(height, width), height, width) % {'got': t.numel()})


def yuv420_lut_float(yuv, n, height, width, coeffs, lut, out=None):
    """n planar 4:2:0 frames of height x width (uint8, back to back) -> [n,height,width,3] float32: the integer matrix of
    `coeffs` (yuv420_coeffs) with the chroma replicated, then lut[byte] as u8_lut_float (srx_yuv420_lut_float)."""
    _chk_yuv(yuv, 'yuv', n, height, width)
    _chk_lut(lut)
    out = _out(out, (n, height, width, 3), torch.float32, yuv.device, 'yuv420_lut_float: out must hold %(want)d floats, got %(got)d')
    check(lib().srx_yuv420_lut_float(_ptr(yuv), n, height, width, ctypes.byref(coeffs), _ptr(lut), _ptr(out), _stream()), 'srx_yuv420_lut_float')
    return out


def unit_yuv420(x, coeffs, out=None):
    """[N,H,W,3] float32 in [-1, 1] -> N planar 4:2:0 frames [N, frame_bytes] uint8: each float through encode_unit_u8 as
    unit_u8, then the integer matrix of `coeffs` with one rounding for the 2 x 2 average and the chroma rows
    (srx_unit_yuv420).  out: a contiguous uint8 tensor of as many bytes at any byte offset, or None for a new one."""
    _chk(x, 'x')
    if x.dim() != 4 or x.shape[3] != 3:
        raise ValueError('unit_yuv420: x must be [N,H,W,3], got %s' % (tuple(x.shape),))
    n, height, width, _ = x.shape
    frame = yuv420_frame_bytes(height, width)
    out = _out(out, (n, frame), torch.uint8, x.device, _YUV_HOLDS % ('out', n, frame, height, width))
    check(lib().srx_unit_yuv420(_ptr(x), n, height, width, ctypes.byref(coeffs), _ptr(out), _stream()), 'srx_unit_yuv420')
    return out


# ---- planar YUV of every format of _lib.PIXEL_FORMATS: 4:2:0, 4:2:2 and 4:4:4 at 8, 10 and 12 bits.  A frame is a uint8 tensor
# of yuv_frame_bytes bytes at every depth: the bytes are the stream's, and nothing reinterprets them on the host.
yuv_frame_bytes = _lib.yuv_frame_bytes


def yuv_coeffs(matrix='bt601', full_range=False, depth=8):
    """yuv420_coeffs for samples of `depth` bits (8, 10, 12), from srx_yuv_coeffs; depth 8 gives yuv420_coeffs' integers."""
    if matrix not in _lib.YUV_MATRIX_BY_NAME:
        raise ValueError("matrix must be 'bt601' or 'bt709', got %r" % (matrix,))
    if depth not in (8, 10, 12):
        raise ValueError('depth must be 8, 10 or 12, got %r' % (depth,))
    c = _lib.Yuv420Coeffs()
    check(_load_lib().srx_yuv_coeffs(_lib.YUV_MATRIX_BY_NAME[matrix], int(bool(full_range)), int(depth), ctypes.byref(c)), 'srx_yuv_coeffs')
    return c


_YUV_FORMAT_HOLDS = '%s must hold %d frames of %d bytes (%d x %d, %s), got %%(got)d bytes'


def yuv_lut_float(yuv, n, height, width, pixel_format, coeffs, lut, out=None):
    """n planar frames of height x width in `pixel_format` (uint8 bytes, back to back) -> [n,height,width,3] float32: the integer
    matrix of `coeffs` (yuv_coeffs at the format's depth) with the chroma replicated, then lut[code], lut the 2^depth floats
    of unit_lut(device, depth) (srx_yuv_lut_float).  'yuv420p' runs yuv420_lut_float's kernel."""
    fmt = _lib.yuv_format(pixel_format)
    _chk_u8(yuv, 'yuv')
    if n < 1 or height < 1 or width < 1:
        raise ValueError('yuv: N, height and width must be positive, got %d, %d, %d' % (n, height, width))
    frame = yuv_frame_bytes(height, width, pixel_format)
    if yuv.numel() != n * frame:
        raise ValueError(_YUV_FORMAT_HOLDS % ('yuv', n, frame, height, width, pixel_format) % {'got': yuv.numel()})
    _chk_lut(lut, 1 << fmt.depth)
    out = _out(out, (n, height, width, 3), torch.float32, yuv.device, 'yuv_lut_float (%s): out must hold %%(want)d floats, got %%(got)d' % pixel_format)
    check(lib().srx_yuv_lut_float(_ptr(yuv), n, height, width, ctypes.byref(fmt), ctypes.byref(coeffs), _ptr(lut), _ptr(out), _stream()),
          'srx_yuv_lut_float')
    return out


def unit_yuv(x, pixel_format, coeffs, out=None):
    """[N,H,W,3] float32 in [-1, 1] -> N planar frames [N, frame_bytes] uint8 in `pixel_format`: each float through
    encode_unit_bits (unit_u8's five roundings onto 0..2^depth - 1), then the integer matrix of `coeffs` with one rounding for
    the chroma block's average (srx_unit_yuv).  out: a contiguous uint8 tensor of as many bytes -- at any byte offset at 8
    bits, any even one above -- or None for a new one.  'yuv420p' runs unit_yuv420's kernels."""
    fmt = _lib.yuv_format(pixel_format)
    _chk(x, 'x')
    if x.dim() != 4 or x.shape[3] != 3:
        raise ValueError('unit_yuv: x must be [N,H,W,3], got %s' % (tuple(x.shape),))
    n, height, width, _ = x.shape
    frame = yuv_frame_bytes(height, width, pixel_format)
    out = _out(out, (n, frame), torch.uint8, x.device, _YUV_FORMAT_HOLDS % ('out', n, frame, height, width, pixel_format))
    check(lib().srx_unit_yuv(_ptr(x), n, height, width, ctypes.byref(fmt), ctypes.byref(coeffs), _ptr(out), _stream()), 'srx_unit_yuv')
    return out


def espcn_forward_keep(x, params, r, t1, t2, y):
    """ESPCN's forward pass of a train step in one launch -- srx_espcn_forward_keep: writes the activations t1 [N,H,W,64],
    t2 [N,H,W,32] and the output y [N,H,W,3 r^2] (sub-pixel space) into the given tensors.  Returns y."""
    _chk(x, 'x')
    N, H, W, C = x.shape
    (w1, b1), (w2, b2), (w3, b3) = _espcn_params(params, C, r, 'espcn_forward_keep')
    _holds(None, x.device, t1, 't1', t2, 't2', y, 'y')
    for t, c, name in ((t1, 64, 't1'), (t2, 32, 't2'), (y, 3 * r * r, 'y')):
        if tuple(t.shape) != (N, H, W, c):
            raise ValueError('espcn_forward_keep: %s has shape %s, expected %s' % (name, tuple(t.shape), (N, H, W, c)))
    check(lib().srx_espcn_forward_keep(_ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(t1), _ptr(t2),
                                       _ptr(y), N, H, W, int(r), _stream()), 'srx_espcn_forward_keep')
    return y


def srcnn_forward(x, params, out=None):
    """SRCNN 9-1-5 VALID inference in one launch -- srx_srcnn_forward.  params = [(w1, b1), (w2, b2), (w3, b3)] (HWIO kernels);
    x [N,H,W,3] -> [N,H-12,W-12,3]."""
    (w1, b1), (w2, b2), (w3, b3) = params
    _chk(x, 'x', w1, 'kernel', b1, ('bias', 64), w2, 'kernel', b2, ('bias', 32), w3, 'kernel', b3, ('bias', 3))
    N, H, W, C = x.shape
    if C != 3 or tuple(w1.shape) != (9, 9, 3, 64) or tuple(w2.shape) != (1, 1, 64, 32) or tuple(w3.shape) != (5, 5, 32, 3):
        raise ValueError('srcnn_forward: shapes do not describe SRCNN 9-1-5')
    if H < 13 or W < 13:
        raise ValueError('srcnn_forward: image %dx%d smaller than the 13-pixel receptive field' % (H, W))
    out = _out(out, (N, H - 12, W - 12, 3), torch.float32, x.device)
    check(lib().srx_srcnn_forward(_ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(out),
                                  N, H, W, _stream()), 'srx_srcnn_forward')
    return out


def space_to_depth(x, r, out=None):
    """[N,H*r,W*r,C] -> [N,H,W,C*r*r]."""
    _chk(x, 'x')
    N, HR, WR, C = x.shape
    if HR % r or WR % r:
        raise ValueError('spatial dims %dx%d not divisible by r=%d' % (HR, WR, r))
    H, W = HR // r, WR // r
    out = _out(out, (N, H, W, C * r * r), torch.float32, x.device)
    check(lib().srx_space_to_depth(_ptr(x), _ptr(out), N, H, W, C, r, _stream()), 'srx_space_to_depth')
    return out


def _dihedral_group(t, name, shape, like):
    """A caller's buffer of one transform group, held to the full shape, or a new one."""
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError('%s has shape %s, expected %s' % (name, tuple(t.shape), tuple(shape)))
    return _out(t, shape, torch.float32, like.device, name=name)


def dihedral_expand(x, out=None):
    """x [N,H,W,C] (C <= 8) -> (a [4N,H,W,C], b [4N,W,H,C]): the eight flips / transposes of every image, transform-major
    (a[k*N+n] = T_k(x[n]), k = 0..3; b[(k-4)*N+n] = T_k(x[n]), k = 4..7; include/srx.h), one launch
    (srx_dihedral_expand).  out: (a, b) to write into.  The tensors may start at any 4-byte address."""
    _chk(x, 'x')
    if x.dim() != 4:
        raise ValueError('dihedral_expand: x must be [N,H,W,C], got %s' % (tuple(x.shape),))
    N, H, W, C = x.shape
    a, b = out if out is not None else (None, None)
    a = _dihedral_group(a, 'dihedral_expand: out[0]', (4 * N, H, W, C), x)
    b = _dihedral_group(b, 'dihedral_expand: out[1]', (4 * N, W, H, C), x)
    check(lib().srx_dihedral_expand(_ptr(x), _ptr(a), _ptr(b), N, H, W, C, _stream()), 'srx_dihedral_expand')
    return a, b


def dihedral_merge(a, b, out=None):
    """a [4N,H,W,C], b [4N,W,H,C] (the groups of dihedral_expand, e.g. a model's outputs on them) -> [N,H,W,C]: the
    mean of the eight inverse transforms, summed in fp32 in the order k = 0..7 and scaled by 1/8, one launch
    (srx_dihedral_merge)."""
    _chk(a, 'a', b, 'b')
    if a.dim() != 4 or a.shape[0] % 4 or tuple(b.shape) != (a.shape[0], a.shape[2], a.shape[1], a.shape[3]):
        raise ValueError('dihedral_merge: a must be [4N,H,W,C] and b [4N,W,H,C], got %s and %s' % (tuple(a.shape), tuple(b.shape)))
    N4, H, W, C = a.shape
    out = _dihedral_group(out, 'dihedral_merge: out', (N4 // 4, H, W, C), a)
    check(lib().srx_dihedral_merge(_ptr(a), _ptr(b), _ptr(out), N4 // 4, H, W, C, _stream()), 'srx_dihedral_merge')
    return out


def stream_copy(src, dst):
    """Plain streaming copy on the library's own copy kernel (a measurement aid: the ceiling of a byte-moving kernel)."""
    _chk(src, 'src', dst, 'dst')
    if src.numel() != dst.numel():
        raise ValueError('stream_copy: sizes differ')
    check(lib().srx_stream_copy(_ptr(src), _ptr(dst), src.numel() * 4, _stream()), 'srx_stream_copy')
    return dst


def mse_fwd_bwd(pred, target, loss_out, inv_numel=None, accumulate=False, dpred=None, want_grad=True):
    """loss_out (+)= sum((pred-target)^2)*inv_numel; returns dpred = 2*(pred-target)*inv_numel."""
    _holds(pred.numel(), None, pred, 'pred', target, 'target', loss_out, ('loss_out', 1, _LEAST | _REQUIRED))
    if inv_numel is None:
        inv_numel = 1.0 / pred.numel()
    if dpred is not None or want_grad:
        dpred = _out(dpred, pred.shape, torch.float32, pred.device, name='dpred')
    check(lib().srx_mse_fwd_bwd(_ptr(pred), _ptr(target), pred.numel(), float(inv_numel), _ptr(loss_out),
                                int(accumulate), _ptr(dpred), _ptr(reduce_scratch(pred.device)), _stream()),
          'srx_mse_fwd_bwd')
    return dpred


def l2_loss(w, scale, loss_out, accumulate=True, mask=None):
    """loss_out (+)= scale * sum(mask * w^2) / 2; mask selects the regularised elements of a flat buffer."""
    _holds(w.numel(), None, w, 'w', mask, 'mask', loss_out, ('loss_out', 1, _LEAST | _REQUIRED))
    check(lib().srx_l2_loss(_ptr(w), _ptr(mask), w.numel(), float(scale), _ptr(loss_out), int(accumulate),
                            _ptr(reduce_scratch(w.device)), _stream()), 'srx_l2_loss')


def adam_tf_step(w, g, m, v, lr, t, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    _holds(w.numel(), None, w, 'w', g, 'g', m, 'm', v, 'v')
    check(lib().srx_adam_tf_step(_ptr(w), _ptr(g), _ptr(m), _ptr(v), w.numel(), float(lr), float(beta1),
                                 float(beta2), float(eps), int(t), float(grad_scale), _stream()), 'srx_adam_tf_step')


def adam_state(device, t=0, lr=0.0):
    """The 32-byte device block srx_adam_tf_step_dev works on: {int64 t; float lr; float lr_t; uint32 done, pad} (+ padding)."""
    st = torch.zeros(8, dtype=torch.int32, device=device)
    adam_state_set(st, t=t, lr=lr)
    return st


def adam_state_set(st, t=None, lr=None):
    if t is not None:
        st[0:2].copy_(torch.tensor([int(t)], dtype=torch.int64).view(torch.int32))
    if lr is not None:
        st[2:3].copy_(torch.tensor([float(lr)], dtype=torch.float32).view(torch.int32))


def adam_state_get(st):
    """(t, lr, lr_t) -- synchronises; for tests and checkpoints."""
    h = st.cpu()
    return int(h[0:2].view(torch.int64).item()), float(h[2:3].view(torch.float32).item()), float(h[3:4].view(torch.float32).item())


def adam_tf_step_dev(w, g, m, v, state, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    _holds(w.numel(), None, w, 'w', g, 'g', m, 'm', v, 'v')
    _holds(None, w.device, state, ('state', 8, _LEAST | _REQUIRED), dtype=torch.int32)
    check(lib().srx_adam_tf_step_dev(_ptr(w), _ptr(g), _ptr(m), _ptr(v), w.numel(), _ptr(state), float(beta1), float(beta2),
                                     float(eps), float(grad_scale), _stream()), 'srx_adam_tf_step_dev')


def momentum_clip_step(w, g, acc, lr, momentum=0.9, cap=float('inf'), grad_scale=1.0):
    _holds(w.numel(), None, w, 'w', g, 'g', acc, 'acc')
    cap = min(float(cap), 3.0e38)
    check(lib().srx_momentum_clip_step(_ptr(w), _ptr(g), _ptr(acc), w.numel(), float(lr), float(momentum), cap,
                                       float(grad_scale), _stream()), 'srx_momentum_clip_step')


def rownorm_loss_fwd_bwd(pred, target, row_len, loss_out, want_grad=True, dpred=None, norms=None):
    """SRCNN loss: mean over rows of ||reshape(pred-target, [-1,row_len])||_2 (+ its gradient).  dpred / norms: caller-owned
    output / scratch tensors (a captured train step must not allocate)."""
    _holds(pred.numel(), None, pred, 'pred', target, 'target', loss_out, ('loss_out', 1, _LEAST | _REQUIRED))
    rows = pred.numel() // row_len
    if rows * row_len != pred.numel():
        raise ValueError('numel %d not divisible by row_len %d' % (pred.numel(), row_len))
    norms = _out(norms, (rows,), torch.float32, pred.device, name='norms')
    if dpred is not None or want_grad:
        dpred = _out(dpred, pred.shape, torch.float32, pred.device, name='dpred')
    check(lib().srx_rownorm_loss_fwd_bwd(_ptr(pred), _ptr(target), rows, row_len, _ptr(loss_out), _ptr(dpred),
                                         _ptr(norms), _stream()), 'srx_rownorm_loss_fwd_bwd')
    return dpred


def psnr(a, b, max_val):
    _holds(a.numel(), None, a, 'a', b, 'b')
    N = a.shape[0]
    out = torch.empty((N,), dtype=torch.float32, device=a.device)
    check(lib().srx_psnr(_ptr(a), _ptr(b), _ptr(out), N, a.numel() // N, float(max_val), _stream()), 'srx_psnr')
    return out


def ssim(a, b, max_val):
    """tf.image.ssim(a, b, max_val) per image: [N,H,W,C] x2 -> [N]."""
    _holds(a.numel(), None, a, 'a', b, 'b')
    N, H, W, C = a.shape
    out = torch.empty((N,), dtype=torch.float32, device=a.device)
    scratch = torch.empty(lib().srx_ssim_scratch_bytes(N) // 4, dtype=torch.float32, device=a.device)
    check(lib().srx_ssim(_ptr(a), _ptr(b), _ptr(out), N, H, W, C, float(max_val), _ptr(scratch), _stream()), 'srx_ssim')
    return out


_scores_scratch = {}


def image_scores(ref, cands, max_val, space='rgb', unit_clip=False, out=None):
    """PSNR and SSIM of 1..4 candidates against ref, all [N,H,W,C], in two launches (srx_image_scores) -> [n_cand,N,2]
    (psnr, ssim), on the device: nothing here waits for the GPU.  unit_clip: x -> clip(x / 2 + 1 / 2, 0, 1) first;
    space 'y' (C % 3 == 0): the row is read as [W*C/3, 3] and Y is scored (espcn/experiment_test.py:
    scores_in_subpixel_space); 'rgb': the channels as they are.  The scratch is cached per device and grows as needed:
    calls on one stream follow each other, so they may share it."""
    cands = list(cands)
    _chk(ref, 'ref')
    if ref.dim() != 4:
        raise ValueError('image_scores: ref must be [N,H,W,C], got %s' % (tuple(ref.shape),))
    if not 1 <= len(cands) <= _lib.SCORES_MAX_CAND:
        raise ValueError('image_scores: 1..%d candidates, got %d' % (_lib.SCORES_MAX_CAND, len(cands)))
    for k, c in enumerate(cands):
        _holds(None, ref.device, c, 'cands[%d]' % k)
        if tuple(c.shape) != tuple(ref.shape):
            raise ValueError('image_scores: cands[%d] has shape %s, ref %s' % (k, tuple(c.shape), tuple(ref.shape)))
    if space not in _lib.SCORES_SPACE_BY_NAME:
        raise ValueError("image_scores: space must be 'rgb' or 'y', got %r" % (space,))
    N, H, W, C = ref.shape
    d = _lib.ScoresDesc(N, H, W, C, len(cands), _lib.SCORES_SPACE_BY_NAME[space], int(bool(unit_clip)), float(max_val))
    L = lib()
    need = L.srx_image_scores_scratch_bytes(ctypes.byref(d))
    if need == 0:
        raise _lib.SrxError('srx_image_scores_scratch_bytes refused: %s' % L.srx_last_error().decode())
    key = (ref.device.type, ref.device.index)
    scratch = _scores_scratch.get(key)
    if scratch is None or scratch.numel() * 4 < need:
        scratch = _scores_scratch[key] = torch.empty((need + 3) // 4, dtype=torch.float32, device=ref.device)
    shape = (len(cands), N, 2)
    if out is not None and tuple(out.shape) != shape:
        raise ValueError('image_scores: out has shape %s, expected %s' % (tuple(out.shape), shape))
    out = _out(out, shape, torch.float32, ref.device)
    check(L.srx_image_scores(ctypes.byref(d), _ptr(ref), _ptr_array(cands), _ptr(out), _ptr(scratch), _stream()),
          'srx_image_scores')
    return out


def saturate_u8(x):
    _chk(x, 'x')
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib().srx_saturate_u8(_ptr(x), _ptr(out), x.numel(), _stream()), 'srx_saturate_u8')
    return out


FEATURE_MOSAIC_TW = 128     # SRX_FEATURE_MOSAIC_TW (include/srx.h): pixels of an image row one workgroup moves


def feature_mosaic_u8(x, out=None):
    """[N,H,W,64] float32 -> [N,8H,8W] uint8: the 64 maps as an 8 x 8 mosaic (channel k at tile row k // 8, tile column
    k % 8) of saturate_u8's bytes, one launch (srx_feature_mosaic_u8).  out: a contiguous uint8 tensor of N*8H*8W
    elements at any byte offset (returned as given), or None for a new [N,8H,8W] tensor."""
    _chk(x, 'x')
    if x.dim() != 4 or x.shape[-1] != 64:
        raise ValueError('feature_mosaic_u8: x must be [N,H,W,64], got %s' % (tuple(x.shape),))
    N, H, W, _ = x.shape
    out = _out(out, (N, 8 * H, 8 * W), torch.uint8, x.device,
               'feature_mosaic_u8: out must be a contiguous uint8 tensor of %%(want)d elements on %s' % (x.device,))
    check(lib().srx_feature_mosaic_u8(_ptr(x), _ptr(out), N, H, W, _stream()), 'srx_feature_mosaic_u8')
    return out


def _panel_sources(sources, r, who):
    """The srx_panel_src array of a list of [N,H,W_i,3*r*r] float32 views whose rows are dense (a crop of a larger tensor
    is taken as it is: its pitches go into the record)."""
    if not sources:
        raise ValueError('%s: no sources' % who)
    C = 3 * r * r
    N, H = sources[0].shape[0], sources[0].shape[1]
    arr, current = (_lib.PanelSrc * len(sources))(), torch.cuda.current_device()
    for k, t in enumerate(sources):         # pitched views, which _chk would refuse: the one check of its own kind in this module
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or t.shape[3] != C or t.shape[0] != N or t.shape[1] != H:
            raise ValueError('%s: source %d must be a float32 [%d,%d,W,%d] tensor on the GPU, got %s %s'
                             % (who, k, N, H, C, t.dtype, tuple(t.shape)))
        if t.device.index != current:
            raise ValueError('%s: source %d lives on %s but the current device is cuda:%d' % (who, k, t.device, current))
        if t.numel() == 0 or t.stride(3) != 1 or (t.shape[2] > 1 and t.stride(2) != C):
            raise ValueError('%s: the rows of source %d are not dense (strides %s)' % (who, k, t.stride()))
        arr[k] = _lib.PanelSrc(t.data_ptr(), t.shape[2], 0, t.stride(1) if H > 1 else 0, t.stride(0) if N > 1 else 0)
    return arr, N, H


def summary_panel_range(sources, r=1, out=None):
    """{scale, offset} of TensorFlow 1.x's float-image rescale over the finite values of `sources`, left on the device
    (srx_summary_panel_range; include/srx.h) for summary_panel_u8(range=).  Returns the float32 buffer (its first two
    elements are scale and offset); out: one to reuse."""
    arr, N, H = _panel_sources(sources, r, 'summary_panel_range')
    n = lib().srx_summary_panel_range_bytes() // 4
    out = torch.empty(n, dtype=torch.float32, device=sources[0].device) if out is None else out
    _holds(n, sources[0].device, out, 'summary_panel_range: out', at_least=True)
    check(lib().srx_summary_panel_range(ctypes.byref(arr), len(arr), N, H, int(r), _ptr(out), _stream()), 'srx_summary_panel_range')
    return out


def summary_panel_u8(sources, r=1, range=None, out=None):
    """Sources [N,H,W_i,3*r*r] float32 -> the [N*H*r, sum(W_i)*r, 3] uint8 panel of the reference's image summaries, one
    launch (srx_summary_panel_u8; include/srx.h).  range None: saturate_u8's encoding; range: summary_panel_range's
    buffer.  out: a contiguous uint8 tensor of the panel's size at any byte offset (returned as given)."""
    arr, N, H = _panel_sources(sources, r, 'summary_panel_u8')
    rows, cols = N * H * r, sum(t.shape[2] for t in sources) * r
    out = _out(out, (rows, cols, 3), torch.uint8, sources[0].device,
               'summary_panel_u8: out must be a contiguous uint8 tensor of %%(want)d elements on %s' % (sources[0].device,))
    _holds(2, sources[0].device, range, 'summary_panel_u8: range (the buffer summary_panel_range returns)', at_least=True)
    check(lib().srx_summary_panel_u8(ctypes.byref(arr), len(arr), N, H, int(r), _ptr(range), _ptr(out), _stream()), 'srx_summary_panel_u8')
    return out


def affine(x, a, b, out=None):
    _chk(x, 'x')
    out = _out(out, x.shape, torch.float32, x.device)
    check(lib().srx_affine(_ptr(x), _ptr(out), x.numel(), float(a), float(b), _stream()), 'srx_affine')
    return out


def u8_to_unit_float(x):
    """uint8 tensor -> float32 in [0,1] (skimage.util.img_as_float32)."""
    _chk_u8(x, 'x')
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().srx_u8_to_unit_float(_ptr(x), _ptr(out), x.numel(), _stream()), 'srx_u8_to_unit_float')
    return out


# srx_patch_src (include/srx.h) as a numpy record: one patch of a vdsr_patch_pairs table
PATCH_SRC_DTYPE = np.dtype([('offset', '<u8'), ('width', '<i4'), ('height', '<i4'), ('x', '<i4'), ('y', '<i4'),
                            ('flip', '<i4'), ('scaling_factor', '<f4')])
assert PATCH_SRC_DTYPE.itemsize == ctypes.sizeof(_lib.PatchSrc) == 32
_TABLE_SLOTS = 4
_table_rings = {}


def _upload_table(words, device):
    """A host int32 array -> a new device tensor, without stopping the host: the copy goes through a ring of
    _TABLE_SLOTS pinned buffers per device and is asynchronous on the current stream, so a sampler can run ahead of the
    training steps that consume its batches.  A slot is written again only after the copy that last read it has
    finished (its event), which also keeps the host at most _TABLE_SLOTS batches ahead."""
    ring = _table_rings.setdefault(device.index, {'next': 0, 'slots': [None] * _TABLE_SLOTS})
    k = ring['next']
    ring['next'] = (k + 1) % _TABLE_SLOTS
    slot = ring['slots'][k]
    if slot is not None:
        slot[1].synchronize()
    if slot is None or slot[0].numel() < words.size:
        slot = ring['slots'][k] = (torch.empty(max(words.size, 2048), dtype=torch.int32, pin_memory=True), torch.cuda.Event())
    slot[0].numpy()[:words.size] = words
    dev = torch.empty(words.size, dtype=torch.int32, device=device)
    dev.copy_(slot[0][:words.size], non_blocking=True)
    slot[1].record()
    return dev


def patch_table_words(table):
    """A table of srx_patch_src records -- a structured array of PATCH_SRC_DTYPE, or its int32 view [B, 8] -- as one
    contiguous int32 array [B, 8]."""
    table = np.asarray(table)
    if table.dtype == PATCH_SRC_DTYPE:
        words = np.ascontiguousarray(table).reshape(-1).view(np.int32).reshape(-1, 8)
    elif table.dtype == np.int32 and table.ndim == 2 and table.shape[1] == 8:
        words = np.ascontiguousarray(table)
    else:
        raise ValueError('table must be a PATCH_SRC_DTYPE array or its int32 view [B, 8], got %s %s' % (table.dtype, table.shape))
    return words


def _patch_table_check(c_name, table, *params):
    """One of the srx_*_patch_table_check functions (c_name) on a host table with its integer parameters, the arena's
    byte count last: raises SrxError naming the entry and the reason, else returns the table's int32 words [B, 8]."""
    words = patch_table_words(table)
    check(getattr(_load_lib(), c_name)(ctypes.c_void_p(words.ctypes.data), words.shape[0], *map(int, params)), c_name)
    return words


def vdsr_patch_table_check(table, S, arena_bytes):
    """srx_vdsr_patch_table_check on a host table: raises SrxError naming the entry and the reason, else returns the
    table's int32 words [B, 8].  Host only."""
    return _patch_table_check('srx_vdsr_patch_table_check', table, S, arena_bytes)


def vdsr_patch_pairs(arena, table, S):
    """VDSR training pairs from a resident image set, one launch (srx_vdsr_patch_pairs).  arena: the packed uint8 images
    on the GPU (1-D, contiguous); table: a HOST table of srx_patch_src records (PATCH_SRC_DTYPE, or its int32 view
    [B, 8]).  The table is always checked first (srx_vdsr_patch_table_check: SrxError with the entry and the reason),
    then uploaded, then the kernel runs.  Returns (sd, hd), float32 [B,S,S,3] in [-1, 1], in table order."""
    _chk_u8(arena, 'arena')
    words = vdsr_patch_table_check(table, S, arena.numel())
    B, S = words.shape[0], int(S)
    table_dev = _upload_table(words.reshape(-1), arena.device)
    sd = torch.empty((B, S, S, 3), dtype=torch.float32, device=arena.device)
    hd = torch.empty_like(sd)
    check(lib().srx_vdsr_patch_pairs(_ptr(arena), ctypes.c_void_p(table_dev.data_ptr()), B, S, _ptr(sd),
                                     _ptr(hd), _stream()), 'srx_vdsr_patch_pairs')
    return sd, hd


class EspcnPatchTable:
    """A checked table of ESPCN patch records on the device: `words` int32 [n, 8] (srx_patch_src rows), with the r, p and
    arena_bytes it was checked for.  Built by espcn_patch_table only; `permuted` gathers rows of a checked table, which
    stay rows of a checked table."""

    def __init__(self, words, r, p, arena_bytes):
        self.words, self.r, self.p, self.arena_bytes = words, r, p, arena_bytes

    def __len__(self):
        return self.words.shape[0]

    def permuted(self, perm_dev):
        """The table whose row k is this table's row perm_dev[k] (a device index tensor; torch checks its bounds)."""
        return EspcnPatchTable(self.words[perm_dev].contiguous(), self.r, self.p, self.arena_bytes)

    def rows(self, start, k):
        """Rows [start, start + k) as a table (a view)."""
        if start < 0 or k < 1 or start + k > len(self):
            raise ValueError('rows [%d, %d) are outside the table of %d' % (start, start + k, len(self)))
        return EspcnPatchTable(self.words[start:start + k], self.r, self.p, self.arena_bytes)

    @staticmethod
    def concat(tables):
        """Tables checked for the same arena, r and p, joined on their device in the order given."""
        t0 = tables[0]
        if any((t.r, t.p, t.arena_bytes) != (t0.r, t0.p, t0.arena_bytes) for t in tables):
            raise ValueError('the tables were checked for different r, p or arenas')
        return EspcnPatchTable(torch.cat([t.words for t in tables]), t0.r, t0.p, t0.arena_bytes)


def espcn_patch_table(table, r, p, arena):
    """Check a HOST table of srx_patch_src records (PATCH_SRC_DTYPE, or its int32 view [n, 8]) for `arena`, r and p
    (srx_espcn_patch_table_check: SrxError with the entry and the reason, before any upload), then upload it once."""
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous():
        raise ValueError('arena must be a contiguous 1-D uint8 tensor')
    words = patch_table_words(table)
    r, p = int(r), int(p)
    check(_load_lib().srx_espcn_patch_table_check(ctypes.c_void_p(words.ctypes.data), words.shape[0], r, p, arena.numel()),
          'srx_espcn_patch_table_check')
    return EspcnPatchTable(torch.from_numpy(words).to(arena.device), r, p, arena.numel())


def espcn_patch_pairs(arena, tab, start, B):
    """ESPCN training pairs from a resident image set, one launch and no host-to-device copy (srx_espcn_patch_pairs), for
    rows [start, start + B) of `tab` (an EspcnPatchTable built for this arena).  Returns (lr [B,p,p,3], label
    [B,p,p,3 r^2]), float32, in row order."""
    _chk_u8(arena, 'arena')
    if not isinstance(tab, EspcnPatchTable) or tab.words.device != arena.device or tab.arena_bytes != arena.numel():
        raise ValueError('tab must be an EspcnPatchTable built for this arena (ops.espcn_patch_table)')
    _holds(8 * len(tab), arena.device, tab.words, 'tab.words', dtype=torch.int32)
    start, B = int(start), int(B)
    if start < 0 or B < 1 or start + B > len(tab):
        raise ValueError('rows [%d, %d) are outside the table of %d' % (start, start + B, len(tab)))
    r, p = tab.r, tab.p
    lr = torch.empty((B, p, p, 3), dtype=torch.float32, device=arena.device)
    label = torch.empty((B, p, p, 3 * r * r), dtype=torch.float32, device=arena.device)
    check(lib().srx_espcn_patch_pairs(_ptr(arena), ctypes.c_void_p(tab.words.data_ptr() + 32 * start), B, r, p,
                                      _ptr(lr), _ptr(label), _stream()), 'srx_espcn_patch_pairs')
    return lr, label


# ---- whole-image evaluation pairs, ESPCN's (lr, label), VDSR's (sd, hd), EnhanceNet's and SRCNN's (sd, bq, hd): what the
# four share.  The record layouts, the size rules and views() are each model's own.
class _EvalTable:
    """Checked whole-image records on the device (`words`, int32 [n, record size / 4]), their host copy and the arena they
    were checked for."""

    def __init__(self, words, records, arena_bytes):
        self.words, self.records, self.arena_bytes = words, records, arena_bytes

    def __len__(self):
        return len(self.records)


class _EvalPairs:
    """Flat float32 device tensors, one per name of `_fields`, holding every record's pair in the order of `table`."""

    def __init__(self, *tensors_then_table):
        *tensors, self.table = tensors_then_table
        self._pair = tuple(tensors)
        for name, tensor in zip(self._fields, self._pair):
            setattr(self, name, tensor)

    def __iter__(self):
        return iter(self._pair)

    def __len__(self):
        return len(self.table)


def _eval_table_upload(cls, c_name, records, dtype, dtype_name, arena, floats_of, *params, tail=()):
    """Check a HOST array of `dtype` records for `arena` with the C function c_name and its integer parameters (SrxError
    with the entry and the reason, before any upload), then upload it once, as a `cls`.  The outputs' size is the table's
    own total, floats_of(records, *params) -- one number, or a tuple where the outputs differ in size -- which the check
    holds every entry to.  `tail`: further arguments of the C function, after the sizes."""
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous():
        raise ValueError('arena must be a contiguous 1-D uint8 tensor')
    records = np.ascontiguousarray(records)
    if records.dtype != dtype or records.ndim != 1:
        raise ValueError('records must be a 1-D %s array, got %s %s' % (dtype_name, records.dtype, records.shape))
    params = [int(v) for v in params]
    floats = floats_of(records, *params)
    sizes = floats if isinstance(floats, tuple) else (floats,)
    check(getattr(_load_lib(), c_name)(ctypes.c_void_p(records.ctypes.data), len(records), *params, arena.numel(), *sizes, *tail), c_name)
    words = torch.from_numpy(records.view(np.int32).reshape(len(records), -1).copy()).to(arena.device)
    return cls(words, records.copy(), *params, arena.numel(), *sizes)


def _packed_starts(floats, pad):
    """Where each record of a packed output starts: the running sum of `floats` (an int64 array, one size per record) with
    every start rounded up to a multiple of `pad` floats (4: the outputs whose records start 16-byte aligned; 1: back to back)."""
    padded = (floats + pad - 1) // pad * pad
    return np.cumsum(padded) - padded


def _first_tiles(heights, widths, T):
    """The running sum of ceil(h / T) ceil(w / T): the tiles of the records before each one."""
    tiles = -(-heights // T) * -(-widths // T)
    return np.cumsum(tiles) - tiles


def _packed_ends(records, fields, floats_of):
    """Where the last record of a packed table ends in the outputs whose offsets are `fields`: its offsets plus
    floats_of(height, width), the sides clamped at 0; zeros for an empty table."""
    if len(records) == 0:
        return (0,) * len(fields)
    last = records[-1]
    sizes = floats_of(max(int(last['height']), 0), max(int(last['width']), 0))
    return tuple(int(last[field]) + n for field, n in zip(fields, sizes))


def _eval_table_for(arena, table, cls, refusal):
    """The preamble of the four *_eval_pairs: a checked arena, and a `cls` table built for it (else ValueError `refusal`)."""
    _chk_u8(arena, 'arena')
    if not isinstance(table, cls) or table.words.device != arena.device or table.arena_bytes != arena.numel():
        raise ValueError(refusal)
    _holds(None, arena.device, table.words, 'table.words', table.coeffs if hasattr(table, 'coeffs') else None, 'table.coeffs', dtype=torch.int32)


def _eval_out(out, names, sizes, device, refusal):
    """The flat float32 tensors of `sizes` a pairs launch writes: `out` if it fits (else ValueError `refusal`), or new ones."""
    out = (None,) * len(sizes) if out is None else tuple(out)
    if len(out) != len(sizes) or any(tensor is not None and tensor.dim() != 1 for tensor in out):
        raise ValueError(refusal)
    return tuple(_out(tensor, (n,), torch.float32, device, refusal, name) for tensor, name, n in zip(out, names, sizes))


# srx_eval_image (include/srx.h) as a numpy record: one image of an espcn_eval_pairs table
EVAL_IMAGE_DTYPE = np.dtype([('offset', '<u8'), ('width', '<i4'), ('height', '<i4'), ('lr_offset', '<u8'),
                             ('first_tile', '<u4'), ('reserved', '<u4')])
assert EVAL_IMAGE_DTYPE.itemsize == ctypes.sizeof(_lib.EvalImage) == 32


def espcn_eval_records(heights, widths, offsets, r):
    """The srx_eval_image records (EVAL_IMAGE_DTYPE) of a set of TRIMMED images -- arrays of heights, widths (multiples of
    r) and arena byte offsets -- with the outputs packed in that order: lr_offset and first_tile are the running sums of
    3 h' w' and of ceil(h' / T) ceil(w' / T), T = _lib.ESPCN_EVAL_TILE.  Host only; the check is espcn_eval_table's."""
    heights, widths = np.asarray(heights, np.int64), np.asarray(widths, np.int64)
    r, T = int(r), _lib.ESPCN_EVAL_TILE
    hp, wp = heights // r, widths // r
    records = np.zeros(len(heights), EVAL_IMAGE_DTYPE)
    records['offset'], records['width'], records['height'] = np.asarray(offsets, np.uint64), widths, heights
    records['lr_offset'] = _packed_starts(3 * hp * wp, 1)
    records['first_tile'] = _first_tiles(hp, wp, T)
    return records


def _espcn_eval_lr_floats(records, r):
    return max(int((3 * (records['height'].astype(np.int64) // max(r, 1)) * (records['width'].astype(np.int64) // max(r, 1))).sum()), 0)


class EspcnEvalTable(_EvalTable):
    """A checked table of srx_eval_image records on the device (`words`, int32 [n, 8]) with its host copy (`records`) and
    the r, arena_bytes and lr_floats it was checked for.  Built by espcn_eval_table only."""

    def __init__(self, words, records, r, arena_bytes, lr_floats):
        super().__init__(words, records, arena_bytes)
        self.r, self.lr_floats = r, lr_floats


def espcn_eval_table(records, r, arena):
    """Check a HOST table of srx_eval_image records (EVAL_IMAGE_DTYPE) for `arena` and r (srx_espcn_eval_table_check:
    SrxError with the entry and the reason, before any upload), then upload it once.  The outputs' size is the table's
    own total, 3 h' w' summed, which the check holds every entry to."""
    return _eval_table_upload(EspcnEvalTable, 'srx_espcn_eval_table_check', records, EVAL_IMAGE_DTYPE, 'EVAL_IMAGE_DTYPE', arena,
                              _espcn_eval_lr_floats, r)


class EspcnEvalPairs(_EvalPairs):
    """What espcn_eval_pairs returns: `lr` and `label`, two flat float32 device tensors holding every image's pair back to
    back in table order, and `views(k)`: image k's ([1,h',w',3], [1,h',w',3 r^2]) as views of them (no copy).  Unpacks as
    (lr, label)."""
    _fields = ('lr', 'label')

    def views(self, k):
        rec, r = self.table.records[k], self.table.r
        hp, wp, at = int(rec['height']) // r, int(rec['width']) // r, int(rec['lr_offset'])
        n = 3 * hp * wp
        return (self.lr[at:at + n].view(1, hp, wp, 3), self.label[at * r * r:(at + n) * r * r].view(1, hp, wp, 3 * r * r))


def espcn_eval_pairs(arena, table, out=None):
    """ESPCN's evaluation pairs of a whole resident image set, one launch and no host-to-device copy
    (srx_espcn_eval_pairs), for `table` (an EspcnEvalTable built for this arena).  Returns an EspcnEvalPairs: (lr, label)
    flat float32, and .views(k).  out: (lr, label) tensors of the table's sizes to write into."""
    _eval_table_for(arena, table, EspcnEvalTable, 'table must be an EspcnEvalTable built for this arena (ops.espcn_eval_table)')
    r, n = table.r, table.lr_floats
    lr, label = _eval_out(out, ('lr', 'label'), (n, n * r * r), arena.device,
                          'out must be flat tensors of %d and %d floats' % (n, n * r * r))
    check(lib().srx_espcn_eval_pairs(_ptr(arena), ctypes.c_void_p(table.words.data_ptr()), len(table), r,
                                     _ptr(lr), _ptr(label), _stream()), 'srx_espcn_eval_pairs')
    return EspcnEvalPairs(lr, label, table)


# srx_vdsr_eval_image (include/srx.h) as a numpy record: one (image, scaling factor) of a vdsr_eval_pairs table
VDSR_EVAL_IMAGE_DTYPE = np.dtype([('offset', '<u8'), ('width', '<i4'), ('height', '<i4'), ('out_offset', '<u8'),
                                  ('first_tile', '<u4'), ('scaling_factor', '<f4')])
assert VDSR_EVAL_IMAGE_DTYPE.itemsize == ctypes.sizeof(_lib.VdsrEvalImage) == 32


def vdsr_eval_records(heights, widths, offsets, factors):
    """The srx_vdsr_eval_image records (VDSR_EVAL_IMAGE_DTYPE) of a list of (image, scaling factor) pairs -- arrays of
    heights, widths, arena byte offsets and factors of one length; an image may appear at several factors -- with the
    outputs in that order: out_offset is the running sum of 3 h w with every record's start rounded up to a multiple of 4
    floats, first_tile the running sum of ceil(h / T) ceil(w / T), T = _lib.VDSR_EVAL_TILE.  Host only; the check is
    vdsr_eval_table's."""
    heights, widths = np.asarray(heights, np.int64), np.asarray(widths, np.int64)
    records = np.zeros(len(heights), VDSR_EVAL_IMAGE_DTYPE)
    records['offset'], records['width'], records['height'] = np.asarray(offsets, np.uint64), widths, heights
    records['scaling_factor'] = np.asarray(factors, np.float32)
    records['out_offset'] = _packed_starts(3 * heights * widths, 4)
    records['first_tile'] = _first_tiles(heights, widths, _lib.VDSR_EVAL_TILE)
    return records


def _vdsr_eval_out_floats(records):
    """Where the last record of a packed table ends: the size of sd and of hd."""
    return _packed_ends(records, ('out_offset',), lambda h, w: (3 * h * w,))[0]


class VdsrEvalTable(_EvalTable):
    """A checked table of srx_vdsr_eval_image records on the device (`words`, int32 [n, 8]) with its host copy (`records`)
    and the arena_bytes and out_floats it was checked for.  Built by vdsr_eval_table only."""

    def __init__(self, words, records, arena_bytes, out_floats):
        super().__init__(words, records, arena_bytes)
        self.out_floats = out_floats


def vdsr_eval_table(records, arena):
    """Check a HOST table of srx_vdsr_eval_image records (VDSR_EVAL_IMAGE_DTYPE) for `arena` (srx_vdsr_eval_table_check:
    SrxError with the entry and the reason, before any upload), then upload it once.  The outputs' size is where the
    table's last record ends, which the check holds every entry to."""
    return _eval_table_upload(VdsrEvalTable, 'srx_vdsr_eval_table_check', records, VDSR_EVAL_IMAGE_DTYPE, 'VDSR_EVAL_IMAGE_DTYPE',
                              arena, _vdsr_eval_out_floats)


class VdsrEvalPairs(_EvalPairs):
    """What vdsr_eval_pairs returns: `sd` and `hd`, two flat float32 device tensors holding every record's pair in table
    order (a record starts at a multiple of 4 floats; the floats of a gap are never written), and `views(k)`: record k's
    ([1,h,w,3], [1,h,w,3]) as views of them (no copy, 16-byte aligned).  Unpacks as (sd, hd)."""
    _fields = ('sd', 'hd')

    def views(self, k):
        rec = self.table.records[k]
        h, w, at = int(rec['height']), int(rec['width']), int(rec['out_offset'])
        n = 3 * h * w
        return self.sd[at:at + n].view(1, h, w, 3), self.hd[at:at + n].view(1, h, w, 3)


def vdsr_eval_pairs(arena, table, out=None):
    """VDSR's evaluation pairs of a whole resident image set, one launch and no host-to-device copy (srx_vdsr_eval_pairs),
    for `table` (a VdsrEvalTable built for this arena).  Returns a VdsrEvalPairs: (sd, hd) flat float32 in [-1, 1], and
    .views(k).  out: (sd, hd) tensors of the table's size to write into."""
    _eval_table_for(arena, table, VdsrEvalTable, 'table must be a VdsrEvalTable built for this arena (ops.vdsr_eval_table)')
    n = table.out_floats
    sd, hd = _eval_out(out, ('sd', 'hd'), (n, n), arena.device, 'out must be two flat tensors of %d floats' % n)
    check(lib().srx_vdsr_eval_pairs(_ptr(arena), ctypes.c_void_p(table.words.data_ptr()), len(table),
                                    _ptr(sd), _ptr(hd), _stream()), 'srx_vdsr_eval_pairs')
    return VdsrEvalPairs(sd, hd, table)


RESAMPLE_FILTERS = {'bilinear': 0, 'bicubic': 1}
_resample_tables = {}


def pil_resample_coeffs(in_size, out_size, filt):
    """Pillow's coefficient tables for one axis (srx_pil_resample_coeffs): (bounds int32 [out, 2], kk int32 [out, ksize])."""
    f = RESAMPLE_FILTERS[filt]
    ksize = lib().srx_pil_resample_ksize(in_size, out_size, f)
    if ksize < 0:
        raise ValueError('bad resample sizes %d -> %d' % (in_size, out_size))
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    check(lib().srx_pil_resample_coeffs(in_size, out_size, f, ctypes.c_void_p(bounds.ctypes.data), ctypes.c_void_p(kk.ctypes.data)),
          'srx_pil_resample_coeffs')
    return bounds, kk


def _device_tables(in_size, out_size, filt, device):
    key = (in_size, out_size, filt, str(device))
    t = _resample_tables.get(key)
    if t is None:
        b, k = pil_resample_coeffs(in_size, out_size, filt)
        t = _resample_tables[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), k.shape[1])
    return t


_enet_pairs_blocks = {}


def enet_pairs_tables(S):
    """The coefficient block of srx_enet_pairs_tables for a crop side S, on the host: int32 [srx_enet_pairs_table_words(S)]
    -- bounds [s, 2] and kk [s, 9] of the S -> s BILINEAR table, then bounds [S, 2] and kk [S, 5] of the s -> S BICUBIC one."""
    S = int(S)
    n = _load_lib().srx_enet_pairs_table_words(S)
    if n < 0:
        raise _lib.SrxError('srx_enet_pairs_table_words failed: %s' % _load_lib().srx_last_error().decode())
    words = np.zeros(n, np.int32)
    check(_load_lib().srx_enet_pairs_tables(S, ctypes.c_void_p(words.ctypes.data)), 'srx_enet_pairs_tables')
    return words


def _enet_pairs_block(S, device):
    """The block on the device: uploaded once per (S, device), like _device_tables."""
    key = (S, str(device))
    t = _enet_pairs_blocks.get(key)
    if t is None:
        t = _enet_pairs_blocks[key] = torch.from_numpy(enet_pairs_tables(S)).to(device)
    return t


def enet_patch_table_check(table, S, arena_bytes):
    """srx_enet_patch_table_check on a host table: raises SrxError naming the entry and the reason, else returns the
    table's int32 words [B, 8].  Host only."""
    return _patch_table_check('srx_enet_patch_table_check', table, S, arena_bytes)


def enet_patch_pairs(arena, table, S):
    """EnhanceNet training batches from a resident image set, one launch (srx_enet_patch_pairs).  arena: the packed uint8
    images on the GPU (1-D, contiguous); table: a HOST table of srx_patch_src records (PATCH_SRC_DTYPE, or its int32 view
    [B, 8]) with scaling_factor 4.  The table is always checked first (srx_enet_patch_table_check: SrxError with the entry
    and the reason, before anything is allocated), then uploaded through the pinned ring, then the kernel runs: the host
    does not wait for the device.  Returns (sd [B,S/4,S/4,3], bq [B,S,S,3], hd [B,S,S,3]), float32 in [-1, 1], in table
    order: byte for byte datasets.degrade_on_device of the flipped crops."""
    _chk_u8(arena, 'arena')
    words = enet_patch_table_check(table, S, arena.numel())
    B, S = words.shape[0], int(S)
    block = _enet_pairs_block(S, arena.device)
    table_dev = _upload_table(words.reshape(-1), arena.device)
    sd = torch.empty((B, S // 4, S // 4, 3), dtype=torch.float32, device=arena.device)
    bq = torch.empty((B, S, S, 3), dtype=torch.float32, device=arena.device)
    hd = torch.empty_like(bq)
    check(lib().srx_enet_patch_pairs(_ptr(arena), ctypes.c_void_p(table_dev.data_ptr()), B, S,
                                     ctypes.c_void_p(block.data_ptr()), _ptr(sd), _ptr(bq), _ptr(hd), _stream()), 'srx_enet_patch_pairs')
    return sd, bq, hd


# srx_enet_eval_image (include/srx.h) as a numpy record: one trimmed image of an enet_eval_pairs table
ENET_EVAL_IMAGE_DTYPE = np.dtype([('offset', '<u8'), ('width', '<i4'), ('height', '<i4'), ('out_offset', '<u8'), ('sd_offset', '<u8'),
                                  ('first_tile', '<u4'), ('width_coeffs', '<u4'), ('height_coeffs', '<u4'), ('reserved', '<u4')])
assert ENET_EVAL_IMAGE_DTYPE.itemsize == ctypes.sizeof(_lib.EnetEvalImage) == 48

_enet_eval_coeff_arenas = {}


def enet_eval_coeffs(side):
    """The coefficient block of srx_enet_eval_coeffs for an axis of `side` pixels, on the host: int32
    [srx_enet_eval_coeff_words(side)] -- `side`, then bounds [side/4, 2] and kk [side/4, 9] of the side -> side/4 BILINEAR
    table, then bounds [side, 2] and kk [side, 5] of the side/4 -> side BICUBIC one."""
    side = int(side)
    n = _load_lib().srx_enet_eval_coeff_words(side)
    if n < 0:
        raise _lib.SrxError('srx_enet_eval_coeff_words failed: %s' % _load_lib().srx_last_error().decode())
    words = np.zeros(n, np.int32)
    check(_load_lib().srx_enet_eval_coeffs(side, ctypes.c_void_p(words.ctypes.data)), 'srx_enet_eval_coeffs')
    return words


def _enet_eval_sides(records):
    """The distinct sides of a table, sorted: the order of the blocks in its coefficient arena."""
    return tuple(int(s) for s in np.unique(np.concatenate([records['width'], records['height']])))


def _enet_eval_coeff_offsets(sides):
    """{side: word offset of its block} in the coefficient arena of `sides`, and the arena's length.  A side no block can be
    built for (the table check refuses its record) gets a block of no words."""
    at, total = {}, 0
    for side in sides:
        at[side] = total
        total += max(_load_lib().srx_enet_eval_coeff_words(side), 0)
    return at, total


def _enet_eval_coeff_arena(sides, device=None):
    """The coefficient arena of `sides` (one block per distinct side, in that order): the host array, and with `device` its
    copy there, each built once per sides (and device)."""
    host = _enet_eval_coeff_arenas.get(sides)
    if host is None:
        at, total = _enet_eval_coeff_offsets(sides)
        host = np.zeros(max(total, 1), np.int32)
        for side in sides:
            if _load_lib().srx_enet_eval_coeff_words(side) > 0:
                block = enet_eval_coeffs(side)
                host[at[side]:at[side] + len(block)] = block
        _enet_eval_coeff_arenas[sides] = host
    if device is None:
        return host
    key = (sides, str(device))
    dev = _enet_eval_coeff_arenas.get(key)
    if dev is None:
        dev = _enet_eval_coeff_arenas[key] = torch.from_numpy(host).to(device)
    return dev


def enet_eval_records(sizes, offsets=None):
    """The srx_enet_eval_image records (ENET_EVAL_IMAGE_DTYPE) of a set of TRIMMED images -- `sizes`: their (height, width),
    multiples of 4; `offsets`: their arena byte offsets, by default back to back as image_arena.pack lays them -- with the
    outputs in that order: out_offset and sd_offset are the running sums of 3 h w and of 3 (h/4) (w/4) with every record's
    start rounded up to a multiple of 4 floats, first_tile the running sum of ceil(h / T) ceil(w / T), T =
    _lib.ENET_EVAL_TILE; width_coeffs and height_coeffs name the blocks of the coefficient arena enet_eval_table builds: one
    per distinct side, in increasing order of the sides.  Host only; the check is enet_eval_table's."""
    sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
    heights, widths = sizes[:, 0], sizes[:, 1]
    records = np.zeros(len(sizes), ENET_EVAL_IMAGE_DTYPE)
    nbytes = 3 * heights * widths
    records['offset'] = np.cumsum(nbytes) - nbytes if offsets is None else np.asarray(offsets, np.uint64)
    records['width'], records['height'] = widths, heights
    records['out_offset'] = _packed_starts(3 * heights * widths, 4)
    records['sd_offset'] = _packed_starts(3 * (heights // 4) * (widths // 4), 4)
    records['first_tile'] = _first_tiles(heights, widths, _lib.ENET_EVAL_TILE)
    at, _ = _enet_eval_coeff_offsets(_enet_eval_sides(records))
    records['width_coeffs'] = [at[int(w)] for w in widths]
    records['height_coeffs'] = [at[int(h)] for h in heights]
    return records


def _enet_eval_floats(records):
    """Where the last record of a packed table ends in hd / bq and in sd: the sizes of the outputs."""
    return _packed_ends(records, ('out_offset', 'sd_offset'), lambda h, w: (3 * h * w, 3 * (h // 4) * (w // 4)))


class EnetEvalTable(_EvalTable):
    """A checked table of srx_enet_eval_image records on the device (`words`, int32 [n, 12]) with its host copy (`records`),
    the arena_bytes, out_floats and sd_floats it was checked for and `coeffs`, the coefficient arena on the device it was
    checked against.  Built by enet_eval_table only."""

    def __init__(self, words, records, arena_bytes, out_floats, sd_floats):
        super().__init__(words, records, arena_bytes)
        self.out_floats, self.sd_floats, self.coeffs = out_floats, sd_floats, None


def enet_eval_table(records, arena):
    """Check a HOST table of srx_enet_eval_image records (ENET_EVAL_IMAGE_DTYPE) for `arena` and for the coefficient arena
    of its distinct sides (srx_enet_eval_table_check: SrxError with the entry and the reason, before any upload), then
    upload the table once; the coefficient arena is built and uploaded once per (sides, device).  The outputs' sizes are
    where the table's last record ends, which the check holds every entry to."""
    records = np.ascontiguousarray(records)
    if records.dtype != ENET_EVAL_IMAGE_DTYPE or records.ndim != 1:
        raise ValueError('records must be a 1-D ENET_EVAL_IMAGE_DTYPE array, got %s %s' % (records.dtype, records.shape))
    sides = _enet_eval_sides(records)
    host = _enet_eval_coeff_arena(sides)
    table = _eval_table_upload(EnetEvalTable, 'srx_enet_eval_table_check', records, ENET_EVAL_IMAGE_DTYPE, 'ENET_EVAL_IMAGE_DTYPE',
                               arena, _enet_eval_floats, tail=(ctypes.c_void_p(host.ctypes.data), len(host)))
    table.coeffs = _enet_eval_coeff_arena(sides, arena.device)
    return table


class EnetEvalPairs(_EvalPairs):
    """What enet_eval_pairs returns: `sd`, `bq` and `hd`, three flat float32 device tensors holding every record's images in
    table order (a record starts at a multiple of 4 floats; the floats of a gap are never written), and `views(k)`: record
    k's ([1,h/4,w/4,3], [1,h,w,3], [1,h,w,3]) as views of them (no copy, 16-byte aligned).  Unpacks as (sd, bq, hd)."""
    _fields = ('sd', 'bq', 'hd')

    def views(self, k):
        rec = self.table.records[k]
        h, w, at, sd_at = int(rec['height']), int(rec['width']), int(rec['out_offset']), int(rec['sd_offset'])
        n, m = 3 * h * w, 3 * (h // 4) * (w // 4)
        return (self.sd[sd_at:sd_at + m].view(1, h // 4, w // 4, 3), self.bq[at:at + n].view(1, h, w, 3),
                self.hd[at:at + n].view(1, h, w, 3))


def enet_eval_pairs(arena, table, out=None):
    """EnhanceNet's evaluation pairs of a whole resident image set, one launch and no host-to-device copy
    (srx_enet_eval_pairs), for `table` (an EnetEvalTable built for this arena).  Returns an EnetEvalPairs: (sd, bq, hd) flat
    float32 in [-1, 1], and .views(k): byte for byte datasets.degrade_on_device of each trimmed image.  out: (sd, bq, hd)
    tensors of the table's sizes to write into."""
    _eval_table_for(arena, table, EnetEvalTable, 'table must be an EnetEvalTable built for this arena (ops.enet_eval_table)')
    n, m = table.out_floats, table.sd_floats
    sd, bq, hd = _eval_out(out, ('sd', 'bq', 'hd'), (m, n, n), arena.device,
                           'out must be three flat tensors of %d, %d and %d floats' % (m, n, n))
    check(lib().srx_enet_eval_pairs(_ptr(arena), ctypes.c_void_p(table.words.data_ptr()), len(table),
                                    ctypes.c_void_p(table.coeffs.data_ptr()), _ptr(sd), _ptr(bq), _ptr(hd), _stream()),
          'srx_enet_eval_pairs')
    return EnetEvalPairs(sd, bq, hd, table)


def srcnn_patch_table_check(table, S, f, border, arena_bytes):
    """srx_srcnn_patch_table_check on a host table: raises SrxError naming the entry and the reason, else returns the
    table's int32 words [B, 8].  Host only."""
    return _patch_table_check('srx_srcnn_patch_table_check', table, S, f, border, arena_bytes)


def srcnn_patch_pairs(arena, table, S, f, border):
    """SRCNN training batches from a resident image set, one launch (srx_srcnn_patch_pairs).  arena: the packed uint8
    images on the GPU (1-D, contiguous); table: a HOST table of srx_patch_src records (PATCH_SRC_DTYPE, or its int32 view
    [B, 8]) with scaling_factor f.  The table is always checked first (srx_srcnn_patch_table_check: SrxError with the entry
    and the reason, before anything is allocated), then uploaded through the pinned ring, then the kernel runs: the host
    does not wait for the device.  Returns (sd [B,S,S,3], hd [B,S-2*border,S-2*border,3]), float32 in table order: sd bit
    for bit SrcnnModel.degrade of the flipped crops / 127.5 - 1, hd those crops without `border` pixels all round."""
    _chk_u8(arena, 'arena')
    words = srcnn_patch_table_check(table, S, f, border, arena.numel())
    B, S, f, border = words.shape[0], int(S), int(f), int(border)
    table_dev = _upload_table(words.reshape(-1), arena.device)
    sd = torch.empty((B, S, S, 3), dtype=torch.float32, device=arena.device)
    hd = torch.empty((B, S - 2 * border, S - 2 * border, 3), dtype=torch.float32, device=arena.device)
    check(lib().srx_srcnn_patch_pairs(_ptr(arena), ctypes.c_void_p(table_dev.data_ptr()), B, S, f, border,
                                      _ptr(sd), _ptr(hd), _stream()), 'srx_srcnn_patch_pairs')
    return sd, hd


# srx_srcnn_eval_image (include/srx.h) as a numpy record: one image of a srcnn_eval_pairs table
SRCNN_EVAL_IMAGE_DTYPE = np.dtype([('offset', '<u8'), ('width', '<i4'), ('height', '<i4'), ('out_offset', '<u8'), ('crop_offset', '<u8'),
                                   ('first_tile', '<u4'), ('reserved', '<u4')])
assert SRCNN_EVAL_IMAGE_DTYPE.itemsize == ctypes.sizeof(_lib.SrcnnEvalImage) == 40


def srcnn_eval_records(heights, widths, offsets, f, border):
    """The srx_srcnn_eval_image records (SRCNN_EVAL_IMAGE_DTYPE) of a set of images -- arrays of heights, widths and arena
    byte offsets -- with the outputs in that order: out_offset and crop_offset are the running sums of 3 h w and of
    3 (h - 2 border) (w - 2 border) with every record's start rounded up to a multiple of 4 floats, first_tile the running
    sum of ceil(h / T) ceil(w / T), T = _lib.SRCNN_EVAL_TILE.  f is not part of a record (it is the table's); it is taken so
    that the builders of the four models read alike.  Host only; the check is srcnn_eval_table's."""
    heights, widths = np.asarray(heights, np.int64), np.asarray(widths, np.int64)
    border = int(border)
    records = np.zeros(len(heights), SRCNN_EVAL_IMAGE_DTYPE)
    records['offset'], records['width'], records['height'] = np.asarray(offsets, np.uint64), widths, heights
    records['out_offset'] = _packed_starts(np.maximum(3 * heights * widths, 0), 4)
    records['crop_offset'] = _packed_starts(np.maximum(3 * (heights - 2 * border) * (widths - 2 * border), 0), 4)
    records['first_tile'] = _first_tiles(heights, widths, _lib.SRCNN_EVAL_TILE)
    return records


def _srcnn_eval_floats(records, f, border):
    """Where the last record of a packed table ends in sd and in bq / hd: the sizes of the outputs."""
    return _packed_ends(records, ('out_offset', 'crop_offset'), lambda h, w: (3 * h * w, 3 * max(h - 2 * border, 0) * max(w - 2 * border, 0)))


class SrcnnEvalTable(_EvalTable):
    """A checked table of srx_srcnn_eval_image records on the device (`words`, int32 [n, 10]) with its host copy (`records`)
    and the f, border, arena_bytes, out_floats and crop_floats it was checked for.  Built by srcnn_eval_table only."""

    def __init__(self, words, records, f, border, arena_bytes, out_floats, crop_floats):
        super().__init__(words, records, arena_bytes)
        self.f, self.border, self.out_floats, self.crop_floats = f, border, out_floats, crop_floats


def srcnn_eval_table(records, f, border, arena):
    """Check a HOST table of srx_srcnn_eval_image records (SRCNN_EVAL_IMAGE_DTYPE) for `arena`, f and border
    (srx_srcnn_eval_table_check: SrxError with the entry and the reason, before any upload), then upload it once.  The
    outputs' sizes are where the table's last record ends, which the check holds every entry to."""
    return _eval_table_upload(SrcnnEvalTable, 'srx_srcnn_eval_table_check', records, SRCNN_EVAL_IMAGE_DTYPE, 'SRCNN_EVAL_IMAGE_DTYPE',
                              arena, _srcnn_eval_floats, f, border)


class SrcnnEvalPairs(_EvalPairs):
    """What srcnn_eval_pairs returns: `sd`, `bq` and `hd`, three flat float32 device tensors holding every record's images in
    table order (a record starts at a multiple of 4 floats; the floats of a gap are never written), and `views(k)`: record
    k's ([1,H,W,3], [1,H-2b,W-2b,3], [1,H-2b,W-2b,3]) as views of them (no copy, 16-byte aligned).  Unpacks as (sd, bq, hd)."""
    _fields = ('sd', 'bq', 'hd')

    def views(self, k):
        rec, b = self.table.records[k], self.table.border
        h, w, at, crop_at = int(rec['height']), int(rec['width']), int(rec['out_offset']), int(rec['crop_offset'])
        hc, wc = h - 2 * b, w - 2 * b
        return (self.sd[at:at + 3 * h * w].view(1, h, w, 3), self.bq[crop_at:crop_at + 3 * hc * wc].view(1, hc, wc, 3),
                self.hd[crop_at:crop_at + 3 * hc * wc].view(1, hc, wc, 3))


def srcnn_eval_pairs(arena, table, out=None):
    """SRCNN's evaluation pairs of a whole resident image set, one launch and no host-to-device copy
    (srx_srcnn_eval_pairs), for `table` (a SrcnnEvalTable built for this arena).  Returns a SrcnnEvalPairs: (sd, bq, hd)
    flat float32 in [-1, 1], and .views(k): sd bit for bit SrcnnModel.degrade of image k / 127.5 - 1, bq that without the
    table's border all round, hd the image without it.  out: (sd, bq, hd) tensors of the table's sizes to write into."""
    _eval_table_for(arena, table, SrcnnEvalTable, 'table must be a SrcnnEvalTable built for this arena (ops.srcnn_eval_table)')
    n, m = table.out_floats, table.crop_floats
    sd, bq, hd = _eval_out(out, ('sd', 'bq', 'hd'), (n, m, m), arena.device,
                           'out must be three flat tensors of %d, %d and %d floats' % (n, m, m))
    check(lib().srx_srcnn_eval_pairs(_ptr(arena), ctypes.c_void_p(table.words.data_ptr()), len(table),
                                     table.f, table.border, _ptr(sd), _ptr(bq), _ptr(hd), _stream()), 'srx_srcnn_eval_pairs')
    return SrcnnEvalPairs(sd, bq, hd, table)


def resize_pil_u8(x, out_h, out_w, filt='bicubic'):
    """scipy.misc.imresize / PIL.Image.resize of uint8 images on the GPU, byte for byte: x [N,H,W,C] uint8 ->
    [N,out_h,out_w,C] uint8; two passes of srx_resample_u8 (horizontal, then vertical), the intermediate in uint8."""
    _chk_u8(x, 'x')
    if x.dim() != 4:
        raise ValueError('x must be a contiguous uint8 [N,H,W,C] tensor on the GPU')
    N, H, W, C = x.shape
    t = x
    if out_w != W:
        b, k, ks = _device_tables(W, out_w, filt, x.device)
        t2 = torch.empty((N, H, out_w, C), dtype=torch.uint8, device=x.device)
        check(lib().srx_resample_u8(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(t2.data_ptr()), N * H, W, out_w, C,
                                    ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(k.data_ptr()), ks, _stream()), 'srx_resample_u8')
        t = t2
    if out_h != H:
        b, k, ks = _device_tables(H, out_h, filt, x.device)
        t2 = torch.empty((N, out_h, t.shape[2], C), dtype=torch.uint8, device=x.device)
        check(lib().srx_resample_u8(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(t2.data_ptr()), N, H, out_h, t.shape[2] * C,
                                    ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(k.data_ptr()), ks, _stream()), 'srx_resample_u8')
        t = t2
    return t if t is not x else x.clone()


def u8_to_pm1(x):
    """uint8 -> float32 in [-1, 1]: astype(float32) / 127.5 - 1.0 (two roundings), as the reference's data pipelines do."""
    _chk_u8(x, 'x')
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().srx_u8_to_pm1(_ptr(x), _ptr(out), x.numel(), _stream()), 'srx_u8_to_pm1')
    return out


def gaussian_blur(x, sigma):
    """skimage.filters.gaussian(x, sigma, mode='nearest') on [N,H,W,C]."""
    _chk(x, 'x')
    N, H, W, C = x.shape
    out, tmp = torch.empty_like(x), torch.empty_like(x)
    check(lib().srx_gaussian_blur(_ptr(x), _ptr(out), _ptr(tmp), N, H, W, C, float(sigma), _stream()), 'srx_gaussian_blur')
    return out


def resize_bilinear(x, oh, ow):
    """skimage.transform.resize(x, [oh, ow], mode='edge', anti_aliasing=False), order 1."""
    _chk(x, 'x')
    N, H, W, C = x.shape
    out = torch.empty((N, oh, ow, C), dtype=torch.float32, device=x.device)
    check(lib().srx_resize_bilinear(_ptr(x), _ptr(out), N, H, W, C, int(oh), int(ow), _stream()), 'srx_resize_bilinear')
    return out


def resize_bicubic_tf(x, oh, ow):
    """tf.image.resize_bicubic(x, [oh, ow]) with TensorFlow 1.x semantics (srcnn/srcnn.py:89-93)."""
    _chk(x, 'x')
    N, H, W, C = x.shape
    out = torch.empty((N, int(oh), int(ow), C), dtype=torch.float32, device=x.device)
    check(lib().srx_resize_bicubic_tf(_ptr(x), _ptr(out), N, H, W, C, int(oh), int(ow), _stream()), 'srx_resize_bicubic_tf')
    return out


def upsample_nearest(x, f):
    _chk(x, 'x')
    N, H, W, C = x.shape
    out = torch.empty((N, H * f, W * f, C), dtype=torch.float32, device=x.device)
    check(lib().srx_upsample_nearest(_ptr(x), _ptr(out), N, H, W, C, f, _stream()), 'srx_upsample_nearest')
    return out


def upsample_nearest_bwd(dout, f, out=None):
    """Gradient of upsample_nearest: sums each f x f block.  dout [N,H*f,W*f,C] -> [N,H,W,C]."""
    _chk(dout, 'dout')
    N, HF, WF, C = dout.shape
    if HF % f or WF % f:
        raise ValueError('upsample_nearest_bwd: %dx%d is not a multiple of the factor %d' % (HF, WF, f))
    out = _out(out, (N, HF // f, WF // f, C), torch.float32, dout.device)
    check(lib().srx_upsample_nearest_bwd(_ptr(dout), _ptr(out), N, HF // f, WF // f, C, f, _stream()), 'srx_upsample_nearest_bwd')
    return out


def add_relu_grad(a, b, y, out=None):
    """(y > 0) ? a + b : 0 -- the gradient at the input of a residual block's closing ReLU chain."""
    _chk(a, 'a', b, 'b', y, 'y')
    if a.shape != b.shape or a.shape != y.shape:
        raise ValueError('add_relu_grad: shapes differ')
    out = _out(out, a.shape, torch.float32, a.device)
    check(lib().srx_add_relu_grad(_ptr(a), _ptr(b), _ptr(y), _ptr(out), a.numel(), _stream()), 'srx_add_relu_grad')
    return out


# ---- EnhanceNet-PAT's loss side ------------------------------------------------------------
def conv2d_bwd_data_acc(dpre, w, x_shape, dx_acc, padding='same', out=None):
    """dx_acc + Conv2DBackpropInput(dpre, w) -- srx_conv2d_bwd_data_acc (out may be dx_acc itself)."""
    d = conv_desc(x_shape, w.shape, padding)
    _chk(w, 'w', dpre, ('dpre', _dpre_count(x_shape, w.shape, padding)), dx_acc, ('dx_acc', math.prod(x_shape)))
    dx = _out(out, tuple(x_shape), torch.float32, w.device)
    check(lib().srx_conv2d_bwd_data_acc(ctypes.byref(d), _ptr(dpre), _ptr(w), _ptr(dx_acc), _ptr(dx), None, 0, _stream()),
          'srx_conv2d_bwd_data_acc')
    return dx


def conv3x3_blocked(x, w, bias=None, act=None, transpose=False, out=None, mask=None, mask_act=None, precision='highest'):
    """A whole 3x3 SAME layer wider than 64 channels in one launch -- srx_conv3x3_blocked_ex.
    x [SB, N, H, W, 64]; w [CIB, COB, 3, 3, 64, 64] (the forward layer's filters); forward: SB = CIB, result
    [COB, N, H, W, 64] = act(sum + bias); transpose=True (data gradient): SB = COB, result [CIB, N, H, W, 64].
    precision: 'highest' (exact fp32) or 'high' (bf16x3 products; include/srx.h, srx_conv3x3_blocked_ex)."""
    prec = precision_code(precision)
    _chk(x, 'x', w, 'w', mask, 'mask')
    sb, n, h, wd, c = x.shape
    cib, cob = w.shape[0], w.shape[1]
    if c != 64 or tuple(w.shape[2:]) != (3, 3, 64, 64) or sb != (cob if transpose else cib):
        raise ValueError('conv3x3_blocked: x %s does not fit filters %s' % (tuple(x.shape), tuple(w.shape)))
    pb = cib if transpose else cob
    _holds(64 * pb, x.device, bias, 'bias')
    out = _out(out, (pb, n, h, wd, 64), torch.float32, x.device)
    if mask is not None and tuple(mask.shape) != tuple(out.shape):
        raise ValueError('conv3x3_blocked: mask %s does not have the result shape %s' % (tuple(mask.shape), tuple(out.shape)))
    check(lib().srx_conv3x3_blocked_ex(_ptr(x), _ptr(w), _ptr(bias), _ptr(mask), ACT_BY_NAME[mask_act], _ptr(out), n, h, wd, sb,
                                       pb, ACT_BY_NAME[act], int(transpose), prec, _stream()), 'srx_conv3x3_blocked_ex')
    return out


def conv3x3_blocked_bwd_filter_workspace_bytes(n, h, w, cib, cob, precision='highest'):
    return int(lib().srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes(n, h, w, cib, cob, precision_code(precision)))


def conv3x3_blocked_bwd_filter(x, dpre, dw, dbias=None, workspace=None, precision='highest'):
    """Filter gradient of a 3x3 SAME layer wider than 64 channels -- srx_conv3x3_blocked_bwd_filter_ex: all block pairs in
    one launch + one reduction.  x [CIB, N, H, W, 64], dpre [COB, N, H, W, 64] -> dw [CIB, COB, 3, 3, 64, 64], dbias [64 COB].
    precision: 'highest' or 'high' (as conv3x3_blocked)."""
    prec = precision_code(precision)
    _chk(x, 'x', dpre, 'dpre', dw, 'dw', dbias, 'dbias')
    cib, n, h, w, c = x.shape
    cob = dpre.shape[0]
    if c != 64 or tuple(dpre.shape[1:]) != (n, h, w, 64) or tuple(dw.shape) != (cib, cob, 3, 3, 64, 64) or \
            (dbias is not None and dbias.numel() != 64 * cob):
        raise ValueError('conv3x3_blocked_bwd_filter: x %s, dpre %s, dw %s do not fit' % (tuple(x.shape), tuple(dpre.shape), tuple(dw.shape)))
    need = conv3x3_blocked_bwd_filter_workspace_bytes(n, h, w, cib, cob, prec)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((max(need, 16) + 3) // 4, dtype=torch.float32, device=x.device)
    _holds(None, x.device, workspace, 'workspace')       # (one too small is replaced, as ever: only its kind can be wrong)
    check(lib().srx_conv3x3_blocked_bwd_filter_ex(_ptr(x), _ptr(dpre), _ptr(dw), _ptr(dbias), n, h, w, cib, cob, prec,
                                                  _ptr(workspace), workspace.numel() * workspace.element_size(), _stream()),
          'srx_conv3x3_blocked_bwd_filter_ex')
    return dw


def texture_gram(x, eps=1e-6, out=None):
    """Gram matrices of the 16x16 patches of normalize(x) -- srx_texture_gram: [N,H,W,C] -> [N*(H/16)*(W/16), C, C]."""
    _chk(x, 'x')
    n, h, w, c = x.shape
    out = _out(out, (n * (h // 16) * (w // 16), c, c), torch.float32, x.device)
    check(lib().srx_texture_gram(_ptr(x), _ptr(out), n, h, w, c, eps, _stream()), 'srx_texture_gram')
    return out


def texture_gram_bwd(x, dgram, eps=1e-6, alpha=2.0, out=None):
    """d loss / d x of texture_gram given the (symmetric) d loss / d gram -- srx_texture_gram_bwd."""
    _chk(x, 'x', dgram, 'dgram')
    n, h, w, c = x.shape
    if tuple(dgram.shape) != (n * (h // 16) * (w // 16), c, c):
        raise ValueError('texture_gram_bwd: dgram %s does not fit x %s' % (tuple(dgram.shape), tuple(x.shape)))
    out = _out(out, x.shape, torch.float32, x.device)
    check(lib().srx_texture_gram_bwd(_ptr(x), _ptr(dgram), _ptr(out), n, h, w, c, eps, alpha, _stream()), 'srx_texture_gram_bwd')
    return out


def maxpool2x2(x, out=None):
    """tf.nn.max_pool(ksize 2, strides 2, 'SAME'): [N,H,W,C] -> [N,ceil(H/2),ceil(W/2),C]."""
    _chk(x, 'x')
    N, H, W, C = x.shape
    out = _out(out, (N, (H + 1) // 2, (W + 1) // 2, C), torch.float32, x.device)
    check(lib().srx_maxpool2x2(_ptr(x), _ptr(out), N, H, W, C, _stream()), 'srx_maxpool2x2')
    return out


def maxpool2x2_bwd(x, dout, out=None, mask_act=None):
    """Gradient of 2x2 / 2 SAME max-pooling w.r.t. its input x; mask_act: also multiply by act'(x), the gradient of the
    activation that produced x (one pass instead of maxpool2x2_bwd + act_bwd, same bits)."""
    _chk(x, 'x')
    N, H, W, C = x.shape
    _holds(N * ((H + 1) // 2) * ((W + 1) // 2) * C, x.device, dout, 'dout')
    out = _out(out, x.shape, torch.float32, x.device)
    check(lib().srx_maxpool2x2_bwd_masked(_ptr(x), _ptr(dout), _ptr(out), N, H, W, C, ACT_BY_NAME[mask_act], _stream()),
          'srx_maxpool2x2_bwd_masked')
    return out


def subsample2(x, oy=1, ox=1, out=None):
    """x[:, oy::2, ox::2, :] -- a stride-1 SAME 3x3 convolution's output -> the stride-2 layer's: offset 1 on an even-sized
    axis, 0 on an odd-sized one (TensorFlow pads 0 before / 1 after there, 1 / 1 here)."""
    _chk(x, 'x')
    N, H, W, C = x.shape
    shape = (N, (H - oy + 1) // 2, (W - ox + 1) // 2, C)
    if out is not None and tuple(out.shape) != shape:
        raise ValueError('subsample2: out has shape %s, expected %s' % (tuple(out.shape), shape))
    out = _out(out, shape, torch.float32, x.device)
    check(lib().srx_subsample2(_ptr(x), _ptr(out), N, H, W, C, oy, ox, _stream()), 'srx_subsample2')
    return out


def subsample2_bwd(dout, oy=1, ox=1, out=None, in_hw=None):
    """Zero stuffing: [N,h,w,C] -> [N,H,W,C] with dout at the positions (oy + 2i, ox + 2j).  in_hw: (H, W), by default
    (2h, 2w); an odd size (2h - 1 with offset 0) is what subsample2 maps to h samples as well."""
    _chk(dout, 'dout')
    N, h, w, C = dout.shape
    H, W = (2 * h, 2 * w) if in_hw is None else (int(in_hw[0]), int(in_hw[1]))
    if ((H - oy + 1) // 2, (W - ox + 1) // 2) != (h, w):
        raise ValueError('subsample2_bwd: %dx%d at offsets (%d, %d) does not have %dx%d samples' % (H, W, oy, ox, h, w))
    if out is not None and tuple(out.shape) != (N, H, W, C):
        raise ValueError('subsample2_bwd: out has shape %s, expected %s' % (tuple(out.shape), (N, H, W, C)))
    out = _out(out, (N, H, W, C), torch.float32, dout.device)
    check(lib().srx_subsample2_bwd(_ptr(dout), _ptr(out), N, H, W, C, oy, ox, _stream()), 'srx_subsample2_bwd')
    return out


def blocks_to_nhwc(blocked, out=None):
    """[CB, N, H, W, 64] -> [N, H, W, CB*64]."""
    _chk(blocked, 'blocked')
    CB, N, H, W, cb = blocked.shape
    if CB == 1:
        return blocked[0]
    if cb != 64:
        raise ValueError('channel blocks must hold 64 channels')
    out = _out(out, (N, H, W, CB * 64), torch.float32, blocked.device)
    check(lib().srx_channel_blocks_to_nhwc(_ptr(blocked), _ptr(out), N * H * W, CB, _stream()), 'srx_channel_blocks_to_nhwc')
    return out


def nhwc_to_blocks(plain, out=None):
    """[N, H, W, C] -> [C/64, N, H, W, 64] (C <= 64: a view [1, N, H, W, C])."""
    _chk(plain, 'plain')
    N, H, W, C = plain.shape
    if C <= 64:
        return plain.view(1, N, H, W, C)
    if C % 64:
        raise ValueError('more than 64 channels must come in multiples of 64')
    out = _out(out, (C // 64, N, H, W, 64), torch.float32, plain.device)
    check(lib().srx_nhwc_to_channel_blocks(_ptr(plain), _ptr(out), N * H * W, C // 64, _stream()), 'srx_nhwc_to_channel_blocks')
    return out


def channel_normalize(x, eps=1e-6, out=None):
    """enet normalize(): x / (mean over the last axis + eps)."""
    _chk(x, 'x')
    C = x.shape[-1]
    out = _out(out, x.shape, torch.float32, x.device)
    check(lib().srx_channel_normalize(_ptr(x), _ptr(out), x.numel() // C, C, float(eps), _stream()), 'srx_channel_normalize')
    return out


def channel_normalize_bwd(x, dy, eps=1e-6, out=None):
    _holds(x.numel(), None, x, 'x', dy, 'dy')
    C = x.shape[-1]
    out = _out(out, x.shape, torch.float32, x.device)
    check(lib().srx_channel_normalize_bwd(_ptr(x), _ptr(dy), _ptr(out), x.numel() // C, C, float(eps), _stream()),
          'srx_channel_normalize_bwd')
    return out


def extract_patches16(x, out=None):
    """[N,H,W,C] -> [N, (H/16)*(W/16), 256, C] (tf.extract_image_patches 16x16 / 16, reshaped)."""
    _chk(x, 'x')
    N, H, W, C = x.shape
    out = _out(out, (N, (H // 16) * (W // 16), 256, C), torch.float32, x.device)
    check(lib().srx_extract_patches16(_ptr(x), _ptr(out), N, H, W, C, 0, _stream()), 'srx_extract_patches16')
    return out


def extract_patches16_bwd(dpatches, image_shape, out=None):
    N, H, W, C = image_shape
    _holds(N * (H // 16) * (W // 16) * 256 * C, None, dpatches, 'dpatches')
    out = _out(out, (N, H, W, C), torch.float32, dpatches.device)
    check(lib().srx_extract_patches16(_ptr(dpatches), _ptr(out), N, H, W, C, 1, _stream()), 'srx_extract_patches16')
    return out


def log_loss(p, label, loss_out, loss_scale=1.0, grad_scale=1.0, accumulate=False, want_grad=True, eps=1e-7):
    """loss_out (+)= loss_scale * tf.losses.log_loss(label, p); returns dp * grad_scale (or None)."""
    _chk(p, 'p', loss_out, ('loss_out', 1, _LEAST | _REQUIRED))
    dp = torch.empty_like(p) if want_grad else None
    check(lib().srx_log_loss(_ptr(p), float(label), p.numel(), float(eps), float(loss_scale), float(grad_scale),
                             _ptr(loss_out), int(accumulate), _ptr(dp), _stream()), 'srx_log_loss')
    return dp


def vgg_preprocess(x, backward=False, out=None):
    """[N,H,W,3] in [-1,1] RGB -> BGR 0..255 minus the ImageNet means; backward=True maps the gradient back."""
    _chk(x, 'x')
    out = _out(out, x.shape, torch.float32, x.device)
    check(lib().srx_vgg_preprocess(_ptr(x), _ptr(out), x.numel() // 3, int(backward), _stream()), 'srx_vgg_preprocess')
    return out


def add_scaled(a, b=None, alpha=1.0, beta=1.0, out=None):
    """alpha * a + beta * b (b None: alpha * a); out may be a or b."""
    _chk(a, 'a', b, 'b')
    if b is not None and a.shape != b.shape:
        raise ValueError('add_scaled: shapes differ')
    out = _out(out, a.shape, torch.float32, a.device)
    check(lib().srx_add_scaled(_ptr(a), _ptr(b), _ptr(out), a.numel(), float(alpha), float(beta), _stream()), 'srx_add_scaled')
    return out


def column_sums(a, out=None):
    _chk(a, 'a')
    rows, cols = a.shape
    out = _out(out, (cols,), torch.float32, a.device)
    check(lib().srx_column_sums(_ptr(a), _ptr(out), rows, cols, cols, _stream()), 'srx_column_sums')
    return out


_gemm_ws = {}


def _gemm_desc(a_shape, b_shape, act, alpha, trans_a, trans_b, accumulate):
    """The srx_gemm_desc of gemm() / gemm_route() for operands of these shapes, and the shape of C."""
    batched = len(a_shape) == 3
    if batched != (len(b_shape) == 3):
        raise ValueError('A and B must both be batched or both be matrices')
    a2, b2 = (a_shape[1:], b_shape[1:]) if batched else (a_shape, b_shape)
    M, K = (a2[1], a2[0]) if trans_a else (a2[0], a2[1])
    Kb, N = (b2[1], b2[0]) if trans_b else (b2[0], b2[1])
    if K != Kb:
        raise ValueError('inner dimensions differ: %d vs %d' % (K, Kb))
    batch = a_shape[0] if batched else 1
    d = _lib.GemmDesc(M, N, K, batch,
                      1 if trans_a else a2[1], a2[1] if trans_a else 1, a2[0] * a2[1] if batched else 0,
                      1 if trans_b else b2[1], b2[1] if trans_b else 1, b2[0] * b2[1] if batched else 0,
                      N, 1, M * N if batched else 0, float(alpha), ACT_BY_NAME[act], int(accumulate))
    return d, ((batch, M, N) if batched else (M, N))


def _gemm_workspace(d, device):
    """The split-K workspace gemm() passes for this descriptor: one per (device, stream), grown on demand; None where
    srx_gemm_workspace_bytes asks for none."""
    need = lib().srx_gemm_workspace_bytes(d.M, d.N, d.K, d.batch)
    if not need:
        return None
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _gemm_ws.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = _gemm_ws[key] = torch.empty((need + 3) // 4, dtype=torch.float32, device=device)
    return ws


def gemm(A, B, bias=None, act=None, alpha=1.0, trans_a=False, trans_b=False, out=None, accumulate=False):
    """C = act(alpha * op(A) @ op(B) + bias); A, B 2-D, or 3-D with a leading batch dimension (same batch count).
    Exact fp32 on the MFMA unit -- srx_gemm."""
    _chk(A, 'A', B, 'B')
    d, shape = _gemm_desc(tuple(A.shape), tuple(B.shape), act, alpha, trans_a, trans_b, accumulate)
    _holds(d.N, A.device, bias, 'bias')
    if out is not None and tuple(out.shape) != shape:
        raise ValueError('out has shape %s, expected %s' % (tuple(out.shape), shape))
    out = _out(out, shape, torch.float32, A.device)
    ws = _gemm_workspace(d, A.device)
    check(lib().srx_gemm(ctypes.byref(d), _ptr(A), _ptr(B), _ptr(bias), _ptr(out), _ptr(ws),
                         ws.numel() * ws.element_size() if ws is not None else 0, _stream()), 'srx_gemm')
    return out


GEMM_ROUTES = ('tile', 'tile_splitk', 'tile_per_wave', 'skinny_nn', 'skinny_nt')      # srx_gemm_route, by value


def gemm_route(A, B, bias=None, act=None, alpha=1.0, trans_a=False, trans_b=False, accumulate=False, workspace='gemm'):
    """(route, K ranges) of the gemm() call with these arguments -- srx_gemm_route_of, the decision srx_gemm makes; route is
    one of GEMM_ROUTES.  Host-only: an operand is a tensor, or (shape, address) for a decision without a device; bias a
    tensor, an address or None.  workspace: 'gemm' (what gemm() would pass; needs the device), None, or (address, bytes)."""
    shape_of = lambda t: tuple(t[0]) if isinstance(t, tuple) else tuple(t.shape)
    addr_of = lambda t: t if t is None or isinstance(t, int) else (t[1] if isinstance(t, tuple) else t.data_ptr())
    d, _ = _gemm_desc(shape_of(A), shape_of(B), act, alpha, trans_a, trans_b, accumulate)
    if workspace == 'gemm':
        ws = _gemm_workspace(d, A.device)
        workspace = None if ws is None else (ws.data_ptr(), ws.numel() * 4)
    ws_addr, ws_bytes = workspace if workspace is not None else (None, 0)
    splits = ctypes.c_int(0)
    rc = _load_lib().srx_gemm_route_of(ctypes.byref(d), addr_of(A), addr_of(B), addr_of(bias), ws_addr, ws_bytes, ctypes.byref(splits))
    if rc < 0:
        check(rc, 'srx_gemm_route_of')
    return GEMM_ROUTES[rc], splits.value
