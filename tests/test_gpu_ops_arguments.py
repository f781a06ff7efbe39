"""ops.py checks every tensor it hands to the library ("Argument checks"): one row per wrapper that takes a result, a
required output, a workspace or an operand whose size the library derives from another argument.  Each such argument is
refused -- ValueError naming it, never SrxError, which would mean the call got as far as the library -- when it has another
element count, is a transposed view of the right count, has another dtype or lives on the CPU.  No refusal launches
anything.  The positive case: a flat buffer of exactly the right count (the full shape where the wrapper insists on it) is
accepted, and a result written into it equals the one the wrapper allocates."""
import math
import re

import numpy as np
import pytest
import torch

from ml_super_resolution_amd import ops

pytestmark = pytest.mark.gpu


def f32(*shape):
    n = math.prod(shape)
    return ((torch.arange(n, dtype=torch.float32) * 37 % 23 - 11) / 8).reshape(shape).cuda()


def u8(*shape):
    return (torch.arange(math.prod(shape)) * 37 % 251).to(torch.uint8).reshape(shape).cuda()


def empty(*shape):
    return torch.empty(shape, dtype=torch.float32, device='cuda')


def words(nbytes):
    return empty((max(nbytes, 16) + 3) // 4)


class Row:
    """call(**args) is the valid call.  results: {argument: the part of call's return value it receives}, checked and compared;
    required: {argument: a good tensor} the caller must give (in args already, or optional operands named here), checked only.
    full: the arguments held to their full shape (the others are taken flat).  least: those that may be larger than needed;
    replaced: those the wrapper replaces when they are too small.  unrun: optional operands that are only refused here (their
    valid calls belong to the kernels' own tests).  names: what the refusal names an argument by, where not by its own name:
    one text, or several where an older refusal, kept as it was, words a wrong shape in its own way.  valid=False: only the
    refusals (a chain takes batches that are a multiple of its grid: its valid calls are test_gpu_chain_fixed's; a patch table's
    are test_gpu_espcn_pairs', the two-call filter gradient's test_gpu_ops').  The four *_eval_pairs get a
    table object made here; their valid calls are test_gpu_*_eval.py's."""

    def __init__(self, id, call, args, results=None, required=None, full=(), least=(), replaced=(), unrun=(), names=None, valid=True):
        self.id, self.call, self.args, self.results, self.required = id, call, args, results or {}, required or (lambda: {})
        self.full, self.least, self.replaced, self.unrun, self.names, self.valid = full, least, replaced, unrun, names or {}, valid


whole = lambda r: r
ESPCN = lambda: [(f32(5, 5, 3, 64), f32(64)), (f32(3, 3, 64, 32), f32(32)), (f32(3, 3, 32, 12), f32(12))]
SRCNN = lambda: [(f32(9, 9, 3, 64), f32(64)), (f32(1, 1, 64, 32), f32(32)), (f32(5, 5, 32, 3), f32(3))]
XS, WS, BODY = (1, 4, 4, 3), (3, 3, 3, 64), (1, 41, 41, 64)
WGRAD_BYTES = lambda: ops.bwd_filter_workspace_bytes(XS, WS, 'same')
BATCH_BYTES = lambda: ops.bwd_filter_batch_workspace_bytes(BODY, (3, 3, 64, 64), 2)
BLOCKED_BYTES = lambda: ops.conv3x3_blocked_bwd_filter_workspace_bytes(1, 4, 4, 2, 2)



def eval_table(cls, dtype, arena, *checked_for):
    """A table object of one record as the *_eval_table builders make it, for the refusals in front of the launch only."""
    params, sizes = checked_for[:-1], checked_for[-1]
    return cls(torch.zeros((1, dtype.itemsize // 4), dtype=torch.int32, device='cuda'), np.zeros(1, dtype), *params, arena.numel(), *sizes)


EVAL_OUT = {name: (name, 'out') for name in ('lr', 'label', 'sd', 'bq', 'hd')}      # the count refusals speak of `out`
ROWS = [
    Row('espcn_eval_pairs', lambda arena, lr, label: ops.espcn_eval_pairs(arena, eval_table(ops.EspcnEvalTable, ops.EVAL_IMAGE_DTYPE, arena, 3, (12,)), out=(lr, label)),
        lambda: dict(arena=u8(64), lr=empty(12), label=empty(108)), None, lambda: dict(lr=empty(12), label=empty(108)), names=EVAL_OUT, valid=False),
    Row('vdsr_eval_pairs', lambda arena, sd, hd: ops.vdsr_eval_pairs(arena, eval_table(ops.VdsrEvalTable, ops.VDSR_EVAL_IMAGE_DTYPE, arena, (12,)), out=(sd, hd)),
        lambda: dict(arena=u8(64), sd=empty(12), hd=empty(12)), None, lambda: dict(sd=empty(12), hd=empty(12)), names=EVAL_OUT, valid=False),
    Row('enet_eval_pairs', lambda arena, sd, bq, hd: ops.enet_eval_pairs(arena, eval_table(ops.EnetEvalTable, ops.ENET_EVAL_IMAGE_DTYPE, arena, (48, 6)), out=(sd, bq, hd)),
        lambda: dict(arena=u8(64), sd=empty(6), bq=empty(48), hd=empty(48)), None, lambda: dict(sd=empty(6), bq=empty(48), hd=empty(48)),
        names=EVAL_OUT, valid=False),
    Row('srcnn_eval_pairs', lambda arena, sd, bq, hd: ops.srcnn_eval_pairs(arena, eval_table(ops.SrcnnEvalTable, ops.SRCNN_EVAL_IMAGE_DTYPE, arena, 3, 6, (48, 12)), out=(sd, bq, hd)),
        lambda: dict(arena=u8(64), sd=empty(48), bq=empty(12), hd=empty(12)), None, lambda: dict(sd=empty(48), bq=empty(12), hd=empty(12)),
        names=EVAL_OUT, valid=False),
    Row('conv2d_fwd', lambda x, w, bias, skip=None, out=None: ops.conv2d_fwd(x, w, bias, skip=skip, out=out),
        lambda: dict(x=f32(*XS), w=f32(*WS), bias=f32(64)), {'out': whole}, lambda: dict(bias=f32(64), skip=f32(1, 4, 4, 64)), full=('out',), unrun=('skip',)),
    Row('conv2d_bwd_data', lambda dpre, w, x_in=None, out=None: ops.conv2d_bwd_data(dpre, w, (1, 4, 4, 64), x_in=x_in, in_act='relu' if x_in is not None else None, out=out),
        lambda: dict(dpre=f32(1, 4, 4, 64), w=f32(3, 3, 64, 64)), {'out': whole}, lambda: dict(dpre=f32(1, 4, 4, 64), x_in=f32(1, 4, 4, 64))),
    Row('conv2d_bwd_data_acc', lambda dpre, w, dx_acc, out=None: ops.conv2d_bwd_data_acc(dpre, w, (1, 4, 4, 64), dx_acc, out=out),
        lambda: dict(dpre=f32(1, 4, 4, 64), w=f32(3, 3, 64, 64), dx_acc=f32(1, 4, 4, 64)), {'out': whole},
        lambda: dict(dpre=f32(1, 4, 4, 64), dx_acc=f32(1, 4, 4, 64))),
    Row('conv2d_bwd_filter', lambda x, dpre, **kw: ops.conv2d_bwd_filter(x, dpre, WS, wd_scale=0.5 if 'w_for_decay' in kw else 0.0, **kw),
        lambda: dict(x=f32(*XS), dpre=f32(1, 4, 4, 64)), {'dw': lambda r: r[0], 'dbias': lambda r: r[1]},
        lambda: dict(w_for_decay=f32(*WS), workspace=empty((WGRAD_BYTES() + 3) // 4)), least=('workspace',)),
    Row('conv2d_bwd_filter_partials', lambda x, dpre, workspace: ops.conv2d_bwd_filter_partials(x, dpre, WS, 'same', workspace),
        lambda: dict(x=f32(*XS), dpre=f32(1, 4, 4, 64), workspace=empty((WGRAD_BYTES() + 3) // 4)), None,
        lambda: dict(dpre=f32(1, 4, 4, 64), workspace=empty((WGRAD_BYTES() + 3) // 4)), least=('workspace',)),
    Row('conv2d_bwd_filter_reduce', lambda workspace, dw, dbias=None, w_for_decay=None: ops.conv2d_bwd_filter_reduce(XS, WS, 'same', workspace, 1, dw, dbias, w_for_decay, 0.5),
        lambda: dict(workspace=empty((WGRAD_BYTES() + 3) // 4), dw=empty(*WS)), None,
        lambda: dict(workspace=empty((WGRAD_BYTES() + 3) // 4), dw=empty(*WS), dbias=empty(64), w_for_decay=f32(*WS)), least=('workspace',), valid=False),
    Row('espcn_patch_pairs', lambda arena, words: ops.espcn_patch_pairs(arena, ops.EspcnPatchTable(words, 3, 17, arena.numel()), 0, 1),
        lambda: dict(arena=u8(64), words=torch.zeros((2, 8), dtype=torch.int32, device='cuda')), None,
        lambda: dict(words=torch.zeros((2, 8), dtype=torch.int32, device='cuda')), names={'words': ('tab.words', 'tab must be')}, valid=False),
    Row('conv2d_fwd_chain', lambda x, w, bias, out0, out1: ops.conv2d_fwd_chain([x, out0], [w, w], [bias, bias], [out0, out1], act='relu'),
        lambda: dict(x=f32(*BODY), w=f32(3, 3, 64, 64) / 64, bias=f32(64), out0=empty(*BODY), out1=empty(*BODY)), None,
        lambda: dict(bias=f32(64), out1=empty(*BODY)), full=('out1',), names={'out1': ('out', 'layer 1')}, valid=False),
    Row('conv2d_bwd_data_chain', lambda dpre, w, mask, out0, out1: ops.conv2d_bwd_data_chain([dpre, out0], [w, w], [mask, mask], [out0, out1], BODY, in_act='relu'),
        lambda: dict(dpre=f32(*BODY), w=f32(3, 3, 64, 64) / 64, mask=f32(*BODY), out0=empty(*BODY), out1=empty(*BODY)), None,
        lambda: dict(mask=f32(*BODY), out1=empty(*BODY)), full=('out1',), names={'out1': ('out', 'layer 1'), 'mask': 'x_in'}, valid=False),
    Row('conv2d_bwd_filter_batch', lambda x, dpre, dw, dbias, workspace, decay=None: ops.conv2d_bwd_filter_batch(
            [x, x], [dpre, dpre], [empty(3, 3, 64, 64), dw], [empty(64), dbias], None if decay is None else [None, decay], 0.5, workspace=workspace),
        lambda: dict(x=f32(*BODY), dpre=f32(*BODY), dw=empty(3, 3, 64, 64), dbias=empty(64), workspace=empty((BATCH_BYTES() + 3) // 4)), None,
        lambda: dict(dw=empty(3, 3, 64, 64), dbias=empty(64), decay=f32(3, 3, 64, 64), workspace=empty((BATCH_BYTES() + 3) // 4)),
        full=('dw',), least=('workspace',), names={'dw': ('dw', 'layer 1'), 'decay': 'w_for_decay'}),
    Row('conv3x3_blocked', lambda x, w, bias=None, mask=None, out=None: ops.conv3x3_blocked(x, w, bias, out=out, mask=mask, mask_act=None if mask is None else 'relu'),
        lambda: dict(x=f32(2, 1, 4, 4, 64), w=f32(2, 2, 3, 3, 64, 64) / 64), {'out': whole}, lambda: dict(bias=f32(128), mask=f32(2, 1, 4, 4, 64)), full=('mask',)),
    Row('conv3x3_blocked_bwd_filter', lambda x, dpre, dw, dbias, workspace=None: ops.conv3x3_blocked_bwd_filter(x, dpre, dw, dbias, workspace),
        lambda: dict(x=f32(2, 1, 4, 4, 64), dpre=f32(2, 1, 4, 4, 64), dw=empty(2, 2, 3, 3, 64, 64), dbias=empty(128)), None,
        lambda: dict(dw=empty(2, 2, 3, 3, 64, 64), dbias=empty(128), workspace=words(BLOCKED_BYTES())), full=('dw',),
        least=('workspace',), replaced=('workspace',), names={'dbias': ('dbias', 'dw')}),
    Row('act_bwd', lambda dy, y, out=None: ops.act_bwd(dy, y, 'relu', out=out), lambda: dict(dy=f32(8), y=f32(8)), {'out': whole}, lambda: dict(y=f32(8))),
    Row('depth_to_space', lambda x, out=None: ops.depth_to_space(x, 2, out=out), lambda: dict(x=f32(1, 2, 2, 4)), {'out': whole}),
    Row('space_to_depth', lambda x, out=None: ops.space_to_depth(x, 2, out=out), lambda: dict(x=f32(1, 4, 4, 1)), {'out': whole}),
    Row('espcn_forward', lambda x, out=None: ops.espcn_forward(x, ESPCN(), 2, out=out), lambda: dict(x=f32(1, 4, 4, 3)), {'out': whole}),
    Row('espcn_forward_u8', lambda x, out=None: ops.espcn_forward_u8(x, ops.unit_lut(x.device), ESPCN(), 2, out=out), lambda: dict(x=u8(1, 4, 4, 3)), {'out': whole}),
    Row('espcn_forward_keep', lambda x, t1, t2, y: ops.espcn_forward_keep(x, ESPCN(), 2, t1, t2, y),
        lambda: dict(x=f32(1, 4, 4, 3), t1=empty(1, 4, 4, 64), t2=empty(1, 4, 4, 32), y=empty(1, 4, 4, 12)), None,
        lambda: dict(t1=empty(1, 4, 4, 64), t2=empty(1, 4, 4, 32), y=empty(1, 4, 4, 12)), full=('t1', 't2', 'y')),
    Row('u8_lut_float', lambda x, out=None: ops.u8_lut_float(x, ops.unit_lut(x.device), out=out), lambda: dict(x=u8(9)), {'out': whole}, names={'out': ('out', 'sizes differ')}),
    Row('unit_u8', lambda x, out=None: ops.unit_u8(x, out=out), lambda: dict(x=f32(9)), {'out': whole}, names={'out': ('out', 'sizes differ')}),
    Row('yuv420_lut_float', lambda yuv, out=None: ops.yuv420_lut_float(yuv, 2, 2, 2, ops.yuv420_coeffs(), ops.unit_lut(yuv.device), out=out),
        lambda: dict(yuv=u8(12)), {'out': whole}),
    Row('unit_yuv420', lambda x, out=None: ops.unit_yuv420(x, ops.yuv420_coeffs(), out=out), lambda: dict(x=f32(2, 2, 2, 3)), {'out': whole}),
    Row('srcnn_forward', lambda x, out=None: ops.srcnn_forward(x, SRCNN(), out=out), lambda: dict(x=f32(1, 13, 13, 3)), {'out': whole}),
    Row('dihedral_expand', lambda x, a=None, b=None: ops.dihedral_expand(x, out=None if a is None and b is None else (a, b)),
        lambda: dict(x=f32(1, 2, 3, 3)), {'a': lambda r: r[0], 'b': lambda r: r[1]}, full=('a', 'b'), names={'a': 'out[0]', 'b': 'out[1]'}),
    Row('dihedral_merge', lambda a, b, out=None: ops.dihedral_merge(a, b, out=out), lambda: dict(a=f32(4, 2, 3, 3), b=f32(4, 3, 2, 3)), {'out': whole}, full=('out',)),
    Row('stream_copy', lambda src, dst: ops.stream_copy(src, dst), lambda: dict(src=f32(8), dst=empty(8)), None, lambda: dict(dst=empty(8)), names={'dst': ('dst', 'sizes differ')}),
    Row('mse_fwd_bwd', lambda pred, target, loss_out, dpred=None: ops.mse_fwd_bwd(pred, target, loss_out, dpred=dpred),
        lambda: dict(pred=f32(8), target=f32(8) / 2, loss_out=empty(1)), {'dpred': whole}, lambda: dict(target=f32(8), loss_out=empty(1)), least=('loss_out',)),
    Row('l2_loss', lambda w, loss_out, mask=None: ops.l2_loss(w, 0.5, loss_out, accumulate=False, mask=mask),
        lambda: dict(w=f32(8), loss_out=empty(1)), None, lambda: dict(mask=f32(8), loss_out=empty(1)), least=('loss_out',)),
    Row('adam_tf_step', lambda w, g, m, v: ops.adam_tf_step(w, g, m, v, 1e-3, 1), lambda: dict(w=f32(8), g=f32(8), m=f32(8), v=f32(8).abs()), None,
        lambda: dict(g=f32(8), m=f32(8), v=f32(8))),
    Row('adam_tf_step_dev', lambda w, g, m, v, state: ops.adam_tf_step_dev(w, g, m, v, state),
        lambda: dict(w=f32(8), g=f32(8), m=f32(8), v=f32(8).abs(), state=ops.adam_state(torch.device('cuda'), lr=1e-3)), None,
        lambda: dict(g=f32(8), m=f32(8), v=f32(8), state=ops.adam_state(torch.device('cuda'))), least=('state',)),
    Row('momentum_clip_step', lambda w, g, acc: ops.momentum_clip_step(w, g, acc, 1e-3), lambda: dict(w=f32(8), g=f32(8), acc=f32(8)), None,
        lambda: dict(g=f32(8), acc=f32(8))),
    Row('rownorm_loss_fwd_bwd', lambda pred, target, loss_out, dpred=None, norms=None: ops.rownorm_loss_fwd_bwd(pred, target, 4, loss_out, dpred=dpred, norms=norms),
        lambda: dict(pred=f32(8), target=f32(8) / 2, loss_out=empty(1)), {'dpred': whole},
        lambda: dict(target=f32(8), loss_out=empty(1), norms=empty(2)), least=('loss_out',)),
    Row('log_loss', lambda p, loss_out: ops.log_loss(p, 1.0, loss_out), lambda: dict(p=f32(8).abs() / 4 + 0.1, loss_out=empty(1)), None,
        lambda: dict(loss_out=empty(1)), least=('loss_out',)),
    Row('psnr', lambda a, b: ops.psnr(a, b, 2.0), lambda: dict(a=f32(1, 2, 2, 3), b=f32(1, 2, 2, 3) / 2), None, lambda: dict(b=f32(1, 2, 2, 3))),
    Row('ssim', lambda a, b: ops.ssim(a, b, 2.0), lambda: dict(a=f32(1, 11, 11, 1), b=f32(1, 11, 11, 1) / 2), None, lambda: dict(b=f32(1, 11, 11, 1))),
    Row('image_scores', lambda ref, c, out=None: ops.image_scores(ref, [c], 2.0, out=out), lambda: dict(ref=f32(1, 11, 11, 3), c=f32(1, 11, 11, 3) / 2),
        {'out': whole}, lambda: dict(c=f32(1, 11, 11, 3)), full=('out', 'c'), names={'c': 'cands[0]'}),
    Row('feature_mosaic_u8', lambda x, out=None: ops.feature_mosaic_u8(x, out=out), lambda: dict(x=f32(1, 2, 2, 64)), {'out': whole}),
    Row('summary_panel_range', lambda x, out=None: ops.summary_panel_range([x], out=out), lambda: dict(x=f32(1, 2, 2, 3)), {'out': whole}, least=('out',)),
    Row('summary_panel_u8', lambda x, range=None, out=None: ops.summary_panel_u8([x], range=range, out=out), lambda: dict(x=f32(1, 2, 2, 3)), {'out': whole},
        lambda: dict(range=ops.summary_panel_range([f32(1, 2, 2, 3)])[:2]), least=('range',)),
    Row('affine', lambda x, out=None: ops.affine(x, 2.0, 1.0, out=out), lambda: dict(x=f32(8)), {'out': whole}),
    Row('upsample_nearest_bwd', lambda dout, out=None: ops.upsample_nearest_bwd(dout, 2, out=out), lambda: dict(dout=f32(1, 4, 4, 64)), {'out': whole}),
    Row('add_relu_grad', lambda a, b, y, out=None: ops.add_relu_grad(a, b, y, out=out), lambda: dict(a=f32(8), b=f32(8) / 2, y=f32(8)), {'out': whole}),
    Row('texture_gram', lambda x, out=None: ops.texture_gram(x, out=out), lambda: dict(x=f32(1, 16, 16, 64).abs()), {'out': whole}),
    Row('texture_gram_bwd', lambda x, dgram, out=None: ops.texture_gram_bwd(x, dgram, out=out), lambda: dict(x=f32(1, 16, 16, 64).abs(), dgram=f32(1, 64, 64)),
        {'out': whole}, lambda: dict(dgram=f32(1, 64, 64)), full=('dgram',)),
    Row('maxpool2x2', lambda x, out=None: ops.maxpool2x2(x, out=out), lambda: dict(x=f32(1, 3, 3, 64)), {'out': whole}),
    Row('maxpool2x2_bwd', lambda x, dout, out=None: ops.maxpool2x2_bwd(x, dout, out=out), lambda: dict(x=f32(1, 3, 3, 64), dout=f32(1, 2, 2, 64)), {'out': whole},
        lambda: dict(dout=f32(1, 2, 2, 64))),
    Row('subsample2', lambda x, out=None: ops.subsample2(x, out=out), lambda: dict(x=f32(1, 4, 4, 64)), {'out': whole}, full=('out',)),
    Row('subsample2_bwd', lambda dout, out=None: ops.subsample2_bwd(dout, out=out), lambda: dict(dout=f32(1, 2, 2, 64)), {'out': whole}, full=('out',)),
    Row('blocks_to_nhwc', lambda blocked, out=None: ops.blocks_to_nhwc(blocked, out=out), lambda: dict(blocked=f32(2, 1, 2, 2, 64)), {'out': whole}),
    Row('nhwc_to_blocks', lambda plain, out=None: ops.nhwc_to_blocks(plain, out=out), lambda: dict(plain=f32(1, 2, 2, 128)), {'out': whole}),
    Row('channel_normalize', lambda x, out=None: ops.channel_normalize(x, out=out), lambda: dict(x=f32(2, 64).abs() + 1), {'out': whole}),
    Row('channel_normalize_bwd', lambda x, dy, out=None: ops.channel_normalize_bwd(x, dy, out=out), lambda: dict(x=f32(2, 64).abs() + 1, dy=f32(2, 64)), {'out': whole},
        lambda: dict(dy=f32(2, 64))),
    Row('extract_patches16', lambda x, out=None: ops.extract_patches16(x, out=out), lambda: dict(x=f32(1, 16, 16, 64)), {'out': whole}),
    Row('extract_patches16_bwd', lambda dpatches, out=None: ops.extract_patches16_bwd(dpatches, (1, 16, 16, 64), out=out), lambda: dict(dpatches=f32(1, 1, 256, 64)),
        {'out': whole}, lambda: dict(dpatches=f32(1, 1, 256, 64))),
    Row('vgg_preprocess', lambda x, out=None: ops.vgg_preprocess(x, out=out), lambda: dict(x=f32(1, 2, 2, 3)), {'out': whole}),
    Row('add_scaled', lambda a, b, out=None: ops.add_scaled(a, b, 0.5, 2.0, out=out), lambda: dict(a=f32(8), b=f32(8) / 2), {'out': whole}),
    Row('column_sums', lambda a, out=None: ops.column_sums(a, out=out), lambda: dict(a=f32(3, 4)), {'out': whole}),
    Row('gemm', lambda A, B, bias=None, out=None: ops.gemm(A, B, bias, out=out), lambda: dict(A=f32(4, 8), B=f32(8, 4)), {'out': whole},
        lambda: dict(bias=f32(4)), full=('out',)),
]


def names(text, message):
    """`message` names `text` as a word of its own ('m' is not named by 'must')."""
    return re.search(r'(?<![\w.])%s(?!\w)' % re.escape(text), message) is not None


def transposed(n, dtype):
    """A 2-D transposed view of n elements, or None where n has no two factors above 1."""
    for rows in range(2, n):
        if n % rows == 0:
            return torch.empty((n // rows, rows), dtype=dtype, device='cuda').t()
    return None


def wrong(good, least, replaced):
    """(what, tensor): the four ways `good` can be wrong.  least: one that may be larger is given one element fewer, and
    its transposed view twice as many; replaced: too few elements are no mistake."""
    n = good.numel()
    if not replaced:
        yield 'count', torch.empty(n - 1, dtype=good.dtype, device='cuda')
    view = transposed(2 * max(n, 2) if least else n, good.dtype)
    if view is not None:
        yield 'transposed', view
    yield 'dtype', good.to(torch.float64 if good.dtype == torch.float32 else torch.float32)
    yield 'cpu', good.cpu()


@pytest.mark.parametrize('row', ROWS, ids=[r.id for r in ROWS])
def test_wrong_tensors_are_refused_and_flat_results_taken(row):
    args = row.args()
    ref = row.call(**args) if row.valid else None                            # the valid call, the wrapper allocating
    torch.cuda.synchronize()
    goods = dict(row.required(), **{name: part(ref) for name, part in row.results.items()})
    assert goods, 'a row checks at least one argument'
    for name, good in goods.items():
        assert good.numel() >= 1
        named = row.names.get(name, name)
        for what, bad in wrong(good, name in row.least, name in row.replaced):
            assert what != 'transposed' or not bad.is_contiguous()
            with pytest.raises(ValueError) as refusal:
                row.call(**dict(args, **{name: bad}))
            assert any(names(text, str(refusal.value)) for text in ((named,) if isinstance(named, str) else named)), (name, what, str(refusal.value))
    for name, part in row.results.items():                                  # a flat buffer of the right count is a valid result
        want = part(ref)
        buf = torch.full(want.shape if name in row.full else (want.numel(),), 7, dtype=want.dtype, device='cuda')
        got = part(row.call(**dict(args, **{name: buf})))
        assert got.data_ptr() == buf.data_ptr()
        if name not in row.least:
            assert torch.equal(got.reshape(-1), want.reshape(-1)), (row.id, name)
    for name, good in row.required().items():                               # and so is a required tensor of exactly the count
        if row.valid and name not in row.full and name not in row.results and name not in row.unrun:
            row.call(**dict(args, **{name: good.reshape(-1)}))
    torch.cuda.synchronize()
