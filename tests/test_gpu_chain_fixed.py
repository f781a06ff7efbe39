"""The fixed-geometry instances of the chained body kernels (conv_chain.hip, Geo41) on the MI355X: at 41 x 41 x 64 they give
the bits of the generic instances (srx_set_chain_fixed(0)) and, on small-integer data, of the float64 oracle; every other
chain-eligible shape still runs the generic instance and matches the per-layer kernels.  Every buffer a chained call writes is
filled with NaN before the call, so a skipped store or a stale read cannot pass.

N = 2 x grid makes a workgroup's range two images: the 1-row tile that ends one image is followed by a 5-row tile of the
next, where a constant-folded tile descriptor can go wrong."""
import numpy as np
import pytest
import torch

from ml_super_resolution_amd import _lib, ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu

WSHAPE = (3, 3, 64, 64)
NAN = float('nan')


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    d = torch.device('cuda', 0)
    torch.cuda.set_device(d)
    return d


class chain_fixed(object):
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = ops.set_chain_fixed(self.on)

    def __exit__(self, *exc):
        ops.set_chain_fixed(self.old)


def _grid():
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 256)


_CASES = {}


def _case(dev, n_per_cu, h=41, w=41):
    """Random inputs of one shape, made once and never written again: x, three layers' filters and biases, an upstream gradient."""
    key = (n_per_cu, h, w)
    if key not in _CASES:
        shape = (n_per_cu * _grid(), h, w, 64)
        g = torch.Generator(device=dev).manual_seed(101 + 7 * n_per_cu + h + w)
        ws = [torch.randn(WSHAPE, device=dev, generator=g) * 0.06 for _ in range(3)]
        bs = [torch.randn((64,), device=dev, generator=g) * 0.1 for _ in range(3)]
        x = torch.randn(shape, device=dev, generator=g)
        dy = torch.randn(shape, device=dev, generator=g) * 1e-3
        masks = [torch.randn(shape, device=dev, generator=g) for _ in range(3)]
        _CASES[key] = (shape, x, ws, bs, dy, masks)
    return _CASES[key]


def _nan(shape, dev, count):
    return [torch.full(shape, NAN, device=dev) for _ in range(count)]


def _forward(case, dev, L, rotating):
    shape, x, ws, bs, _, _ = case
    if rotating:
        # two buffers in turn, as a forward pass that keeps no activations runs: layer l reads what layer l - 1 wrote
        a, b = _nan(shape, dev, 2)
        outs = [a, b, a][:L]
    else:
        outs = _nan(shape, dev, L)
    ops.conv2d_fwd_chain([x] + outs[:-1], ws[:L], bs[:L], outs, 'same', 'relu')
    return outs[-2:] if rotating else outs


def _dgrad(case, dev, L, masked):
    shape, _, ws, _, dy, masks = case
    outs = _nan(shape, dev, L)
    ops.conv2d_bwd_data_chain([dy] + outs[:-1], ws[:L], masks[:L] if masked else None, outs, shape, 'same', 'relu' if masked else None)
    return outs


@pytest.mark.parametrize('kind', ['fwd', 'fwd_rotating', 'dgrad_masked', 'dgrad'])
@pytest.mark.parametrize('L', [2, 3])
@pytest.mark.parametrize('n_per_cu', [1, 2])
def test_fixed_instance_equals_generic_instance(dev, n_per_cu, L, kind):
    case = _case(dev, n_per_cu)
    assert ops.chain_supported(case[0], WSHAPE, _lib.OP_FWD, act='relu')
    res = []
    for on in (0, 1):
        with chain_fixed(on):
            if kind.startswith('fwd'):
                res.append(_forward(case, dev, L, kind == 'fwd_rotating'))
            else:
                res.append(_dgrad(case, dev, L, kind == 'dgrad_masked'))
    torch.cuda.synchronize()
    for l, (a, b) in enumerate(zip(res[0], res[1])):
        assert not torch.isnan(b).any(), 'buffer %d: something was not written' % l
        assert torch.equal(a, b), 'buffer %d' % l


def _int_case(n, seed):
    """Small integers: every product and every partial sum of two chained layers is an integer below 2^24 (|x| <= 3, |w| <= 1:
    layer 1 at most 576 * 3, layer 2 at most 576 * 1731), so fp32 is exact in any order."""
    rng = np.random.RandomState(seed)
    shape = (n, 41, 41, 64)
    x = rng.randint(-3, 4, shape).astype(np.float32)
    ws = [rng.randint(-1, 2, WSHAPE).astype(np.float32) for _ in range(2)]
    bs = [rng.randint(-3, 4, (64,)).astype(np.float32) for _ in range(2)]
    masks = [rng.randint(-2, 3, shape).astype(np.float32) for _ in range(2)]
    return shape, x, ws, bs, masks


def _oracle_images(n):
    # the images of the first, a middle and the last workgroup (two each at N = 2 x grid)
    return sorted(set([0, 1, 2, 3, n // 2, n // 2 + 1, n - 2, n - 1]))


def test_forward_equals_the_oracle_on_integers(dev):
    n = 2 * _grid()
    shape, x, ws, bs, _ = _int_case(n, 5)
    t = lambda a: torch.from_numpy(a).to(dev)
    outs = _nan(shape, dev, 2)
    with chain_fixed(1):
        ops.conv2d_fwd_chain([t(x), outs[0]], [t(w) for w in ws], [t(b) for b in bs], outs, 'same', 'relu')
    idx = _oracle_images(n)
    r1 = O.conv2d_fwd(x[idx], ws[0], bs[0], 'SAME', 'relu')
    r2 = O.conv2d_fwd(r1, ws[1], bs[1], 'SAME', 'relu')
    assert np.abs(r2).max() < 2 ** 24
    assert np.array_equal(outs[0][idx].cpu().numpy().astype(np.float64), r1), 'layer 1'
    assert np.array_equal(outs[1][idx].cpu().numpy().astype(np.float64), r2), 'layer 2'


def test_masked_dgrad_equals_the_oracle_on_integers(dev):
    n = 2 * _grid()
    shape, dy, ws, _, masks = _int_case(n, 6)
    t = lambda a: torch.from_numpy(a).to(dev)
    outs = _nan(shape, dev, 2)
    with chain_fixed(1):
        ops.conv2d_bwd_data_chain([t(dy), outs[0]], [t(w) for w in ws], [t(m) for m in masks], outs, shape, 'same', 'relu')
    idx = _oracle_images(n)
    r1 = O.conv2d_bwd_data(dy[idx], ws[0], (41, 41), 'SAME') * (masks[0][idx] > 0)
    r2 = O.conv2d_bwd_data(r1, ws[1], (41, 41), 'SAME') * (masks[1][idx] > 0)
    assert np.abs(r2).max() < 2 ** 24
    assert np.array_equal(outs[0][idx].cpu().numpy().astype(np.float64), r1), 'layer 1'
    assert np.array_equal(outs[1][idx].cpu().numpy().astype(np.float64), r2), 'layer 2'


@pytest.mark.parametrize('hw', [(33, 33), (41, 40)])
def test_other_shapes_run_the_generic_instance(dev, hw):
    """With the switch at 1, a chain whose plan is not the fixed geometry's still equals the per-layer kernels."""
    case = _case(dev, 1, hw[0], hw[1])
    shape, x, ws, bs, dy, masks = case
    assert ops.chain_supported(shape, WSHAPE, _lib.OP_FWD, act='relu'), shape
    with chain_fixed(1):
        outs = _forward(case, dev, 3, False)
        douts = _dgrad(case, dev, 3, True)
        douts0 = _dgrad(case, dev, 2, False)
    v = x
    for l in range(3):
        v = ops.conv2d_fwd(v, ws[l], bs[l], 'same', 'relu')
        assert torch.equal(outs[l], v), 'forward layer %d' % l
    d = dy
    for l in range(3):
        d = ops.conv2d_bwd_data(d, ws[l], shape, 'same', x_in=masks[l], in_act='relu')
        assert torch.equal(douts[l], d), 'masked data gradient %d' % l
    d = dy
    for l in range(2):
        d = ops.conv2d_bwd_data(d, ws[l], shape, 'same')
        assert torch.equal(douts0[l], d), 'data gradient %d' % l
