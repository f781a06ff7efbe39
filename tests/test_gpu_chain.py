"""Chained body layers (srx_conv_chain, conv_chain.hip) on the MI355X: one launch per pass for VDSR's 3x3 64 -> 64 layers
gives the same bits as one launch per layer (srx_set_chain(0)).  Every buffer a chained call writes is filled with NaN
before the call, so a skipped store or a stale read cannot pass."""
import numpy as np
import pytest
import torch

from ml_super_resolution_amd import _lib, ops
from ml_super_resolution_amd.vdsr import model_vdsr

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    d = torch.device('cuda', 0)
    torch.cuda.set_device(d)
    return d


class chain_off(object):
    def __enter__(self):
        self.old = ops.set_chain(0)

    def __exit__(self, *exc):
        ops.set_chain(self.old)


def _patches(dev, n, h, w, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    hd = torch.rand((n, h, w, 3), device=dev, generator=g) * 2 - 1
    sd = (hd + 0.1 * torch.randn((n, h, w, 3), device=dev, generator=g)).clamp(-1, 1)
    return sd, hd


def _nan_bufs(stack):
    for t in stack._bufs.values():
        t.fill_(float('nan'))


def _grid():
    # the pipelined grid is the compute-unit count (<= 256); batches that are multiples of it chain
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_host_query_matches_shapes(dev):
    G = min(_grid(), 256)
    w = (3, 3, 64, 64)
    assert ops.chain_supported((G, 41, 41, 64), w, _lib.OP_FWD, act='relu')
    assert ops.chain_supported((G, 41, 41, 64), w, _lib.OP_BWD_DATA, in_act='relu')
    assert not ops.chain_supported((16, 41, 41, 64), w, _lib.OP_FWD, act='relu')
    assert not ops.chain_supported((G + 44, 41, 41, 64), w, _lib.OP_FWD, act='relu')
    assert not ops.chain_supported((4, 128, 128, 64), w, _lib.OP_FWD, act='relu')    # column strips
    with chain_off():
        assert not ops.chain_supported((G, 41, 41, 64), w, _lib.OP_FWD, act='relu')


@pytest.mark.parametrize('n_per_cu,hw', [(1, 41), (2, 41), (1, 33)])
def test_substages_match_per_layer_kernels(dev, n_per_cu, hw):
    """Each chained pass against its unfused kernel, layer by layer, at the scale of that layer."""
    n = n_per_cu * min(_grid(), 256)
    shape = (n, hw, hw, 64)
    if not ops.chain_supported(shape, (3, 3, 64, 64), _lib.OP_FWD, act='relu'):
        pytest.skip('%s does not take the chained route' % (shape,))
    g = torch.Generator(device=dev).manual_seed(11 + hw)
    L = 5
    ws = [torch.randn((3, 3, 64, 64), device=dev, generator=g) * 0.06 for _ in range(L)]
    bs = [torch.randn((64,), device=dev, generator=g) * 0.1 for _ in range(L)]
    x = torch.randn(shape, device=dev, generator=g)
    # forward: 5 ReLU layers in one launch
    outs = [torch.full(shape, float('nan'), device=dev) for _ in range(L)]
    ops.conv2d_fwd_chain([x] + outs[:-1], ws, bs, outs, 'same', 'relu')
    t = x
    for l in range(L):
        t = ops.conv2d_fwd(t, ws[l], bs[l], 'same', 'relu')
        assert torch.equal(outs[l], t), 'forward layer %d' % l
    # data gradient with the ReLU-gradient masks of the forward activations
    acts = [x] + outs
    dy = torch.randn(shape, device=dev, generator=g) * 1e-3
    douts = [torch.full(shape, float('nan'), device=dev) for _ in range(L - 1)]
    order = list(range(L - 1, 0, -1))      # layers 4 .. 1
    ops.conv2d_bwd_data_chain([dy] + douts[:-1], [ws[k] for k in order], [acts[k] for k in order], douts, shape, 'same', 'relu')
    d = dy
    for j, k in enumerate(order):
        d = ops.conv2d_bwd_data(d, ws[k], shape, 'same', x_in=acts[k], in_act='relu')
        assert torch.equal(douts[j], d), 'data gradient of layer %d' % k
    # and without masks
    douts2 = [torch.full(shape, float('nan'), device=dev) for _ in range(2)]
    ops.conv2d_bwd_data_chain([dy, douts2[0]], ws[:2], None, douts2, shape, 'same', None)
    d = ops.conv2d_bwd_data(ops.conv2d_bwd_data(dy, ws[0], shape, 'same'), ws[1], shape, 'same')
    assert torch.equal(douts2[1], d)


@pytest.mark.parametrize('n_per_cu,hw', [(1, 41), (2, 41), (1, 33)])
@pytest.mark.parametrize('keep', [True, False])
def test_vdsr_forward_chained_equals_per_layer(dev, n_per_cu, hw, keep):
    n = n_per_cu * min(_grid(), 256)
    sd, _ = _patches(dev, n, hw, hw, 5)
    m = model_vdsr.VdsrModel(num_layers=20, use_adam=True, device=dev, seed=31)
    with chain_off():
        ref = m.forward(sd, keep=keep).clone()
        ref_acts = [a.clone() for a in m.stack.acts[1:]] if keep else None
    _nan_bufs(m.stack)
    got = m.forward(sd, keep=keep)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    if keep:
        for i, (a, r) in enumerate(zip(m.stack.acts[1:], ref_acts)):
            assert torch.equal(a, r), 'activation %d' % i


def _train(dev, n, chained, replay, steps=3):
    sd, hd = _patches(dev, n, 41, 41, 7)
    m = model_vdsr.VdsrModel(num_layers=20, use_adam=True, device=dev, seed=41)
    old = ops.set_chain(1 if chained else 0)
    try:
        losses = []
        for _ in range(steps):
            _nan_bufs(m.stack)
            if replay:
                loss = m.stack.train_step_replay(sd, hd, 5e-5)
            else:
                loss = m.train_step(sd, hd, 5e-5)
            losses.append(loss.clone())
        torch.cuda.synchronize()
    finally:
        ops.set_chain(old)
    return torch.cat(losses), m.stack.grads.clone(), m.stack.params.clone(), m.stack.acts[-1].clone()


@pytest.mark.parametrize('replay', [False, True])
def test_vdsr_train_steps_chained_equal_per_layer(dev, replay):
    n = min(_grid(), 256)
    assert ops.chain_supported((n, 41, 41, 64), (3, 3, 64, 64), _lib.OP_BWD_DATA, in_act='relu')
    ref = _train(dev, n, False, replay)
    got = _train(dev, n, True, replay)
    for name, a, b in zip(('loss', 'grads', 'params', 'sr'), got, ref):
        assert torch.equal(a, b), name
    assert np.isfinite(got[1].cpu().numpy()).all()


@pytest.mark.parametrize('shape', [(16, 41, 41), (300, 41, 41), (4, 128, 128)])
def test_ineligible_shapes_take_the_per_layer_route(dev, shape):
    n, h, w = shape
    assert not ops.chain_supported((n, h, w, 64), (3, 3, 64, 64), _lib.OP_FWD, act='relu')
    sd, hd = _patches(dev, n, h, w, 9)
    res = []
    for chained in (False, True):
        m = model_vdsr.VdsrModel(num_layers=6, use_adam=True, device=dev, seed=43)
        old = ops.set_chain(1 if chained else 0)
        try:
            loss = m.train_step(sd, hd, 5e-5)
            res.append((loss.clone(), m.stack.grads.clone(), m.forward(sd).clone()))
        finally:
            ops.set_chain(old)
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
