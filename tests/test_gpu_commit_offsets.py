"""Staging writes at constant LDS slots on the MI355X: the straight-line full tile of the fixed-geometry
chain kernels and the exact-row filter gradient write a staging pass to `per-lane base + immediate` instead of an address
computed from a cursor, and the filter gradient sums its bias gradient before the window handover.  Nothing arithmetic
changed, so every check is for equal bits.

Every case runs plain and with every CU's LDS filled with NaN before each call (ops._POISON_LDS): a pass written to a wrong
slot, or not written, then leaves NaN where the kernel reads, not stale but plausible data of the previous call.

Chain, N = grid and N = 2 x grid, 41 x 41 x 64, L = 2: at 2 x grid a full tile stages the next image's first tile, whose first
passes lie above the image; a full tile also stages the 1-row tile (9 of the 24 passes the groups carry) and, at the
layer's end, nothing.  Filter gradient: ranges of one row, ranges that cut 3-row units, ranges that cross image ends."""
import numpy as np
import pytest
import torch

from ml_super_resolution_amd import ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu

WSHAPE = (3, 3, 64, 64)
NAN = float('nan')
KINDS = ['fwd', 'fwd_rotating', 'dgrad_masked', 'dgrad']


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    d = torch.device('cuda', 0)
    torch.cuda.set_device(d)
    return d


@pytest.fixture(params=[False, True], ids=['plain', 'poisoned_lds'])
def poison(request, monkeypatch):
    monkeypatch.setattr(ops, '_POISON_LDS', request.param)
    return request.param


class switch(object):
    def __init__(self, setter, on):
        self.setter, self.on = setter, on

    def __enter__(self):
        self.old = self.setter(self.on)

    def __exit__(self, *exc):
        self.setter(self.old)


def _grid():
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 256)


def _nan(shape, dev, count):
    return [torch.full(shape, NAN, device=dev) for _ in range(count)]


# ---- chain ------------------------------------------------------------------------------------------------------------------
_CHAIN = {}


def _chain_case(dev, n_per_cu):
    """Random inputs and what the generic instance and the per-layer kernels make of them (plain LDS), made once, never written
    again: {kind: (generic instance's buffers, per-layer kernels' buffers)}."""
    if n_per_cu not in _CHAIN:
        poisoned, ops._POISON_LDS = ops._POISON_LDS, False       # (the references come from plain calls)
        shape = (n_per_cu * _grid(), 41, 41, 64)
        g = torch.Generator(device=dev).manual_seed(311 + n_per_cu)
        ws = [torch.randn(WSHAPE, device=dev, generator=g) * 0.06 for _ in range(2)]
        bs = [torch.randn((64,), device=dev, generator=g) * 0.1 for _ in range(2)]
        x = torch.randn(shape, device=dev, generator=g)
        dy = torch.randn(shape, device=dev, generator=g) * 1e-3
        masks = [torch.randn(shape, device=dev, generator=g) for _ in range(2)]
        case = dict(shape=shape, x=x, ws=ws, bs=bs, dy=dy, masks=masks)
        refs = {}
        with switch(ops.set_chain_fixed, 0):
            for kind in KINDS:
                refs[kind] = [_chain_run(case, dev, kind)]
        with switch(ops.set_chain, 0):
            f1 = ops.conv2d_fwd(x, ws[0], bs[0], 'same', 'relu')
            f2 = ops.conv2d_fwd(f1, ws[1], bs[1], 'same', 'relu')
            m1 = ops.conv2d_bwd_data(dy, ws[0], shape, 'same', x_in=masks[0], in_act='relu')
            m2 = ops.conv2d_bwd_data(m1, ws[1], shape, 'same', x_in=masks[1], in_act='relu')
            d1 = ops.conv2d_bwd_data(dy, ws[0], shape, 'same')
            d2 = ops.conv2d_bwd_data(d1, ws[1], shape, 'same')
        refs['fwd'].append([f1, f2]); refs['fwd_rotating'].append([f1, f2])
        refs['dgrad_masked'].append([m1, m2]); refs['dgrad'].append([d1, d2])
        torch.cuda.synchronize()
        ops._POISON_LDS = poisoned
        case['refs'] = refs
        _CHAIN[n_per_cu] = case
    return _CHAIN[n_per_cu]


def _chain_run(case, dev, kind):
    """Two chained layers into NaN-filled buffers -> [layer 1's output, layer 2's output]."""
    shape = case['shape']
    outs = _nan(shape, dev, 2)       # (rotating: two buffers in turn are, at L = 2, the same two buffers)
    if kind.startswith('fwd'):
        ops.conv2d_fwd_chain([case['x'], outs[0]], case['ws'], case['bs'], outs, 'same', 'relu')
    else:
        masked = kind == 'dgrad_masked'
        ops.conv2d_bwd_data_chain([case['dy'], outs[0]], case['ws'], case['masks'] if masked else None, outs, shape, 'same',
                                  'relu' if masked else None)
    return outs


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n_per_cu', [1, 2])
def test_chain_equals_the_cursor_form_and_the_per_layer_kernels(dev, poison, n_per_cu, kind):
    case = _chain_case(dev, n_per_cu)
    with switch(ops.set_chain_fixed, 1):
        got = _chain_run(case, dev, kind)
    torch.cuda.synchronize()
    generic, per_layer = case['refs'][kind]
    for l in range(2):
        assert not torch.isnan(got[l]).any(), 'layer %d: NaN (a staging slot not written, or a store skipped)' % (l + 1)
        assert torch.equal(got[l], generic[l]), 'layer %d against the generic instance' % (l + 1)
        assert torch.equal(got[l], per_layer[l]), 'layer %d against the per-layer kernels' % (l + 1)


_INT = {}


def _int_case(n_per_cu):
    """Small integers: every product and every partial sum of two chained layers is an integer below 2^24 (|x| <= 3, |w| <= 1:
    layer 1 at most 576 * 3 + 3, layer 2 at most 576 * 1731 + 3), so fp32 is exact in any order.  The oracle for the images of the
    first, a middle and the last workgroup."""
    if n_per_cu not in _INT:
        n = n_per_cu * _grid()
        rng = np.random.RandomState(50 + n_per_cu)
        shape = (n, 41, 41, 64)
        x = rng.randint(-3, 4, shape).astype(np.float32)
        ws = [rng.randint(-1, 2, WSHAPE).astype(np.float32) for _ in range(2)]
        bs = [rng.randint(-3, 4, (64,)).astype(np.float32) for _ in range(2)]
        masks = [rng.randint(-2, 3, shape).astype(np.float32) for _ in range(2)]
        idx = sorted(set([0, 1, n // 2, n // 2 + 1, n - 2, n - 1]))
        f1 = O.conv2d_fwd(x[idx], ws[0], bs[0], 'SAME', 'relu')
        f2 = O.conv2d_fwd(f1, ws[1], bs[1], 'SAME', 'relu')
        d1 = O.conv2d_bwd_data(x[idx], ws[0], (41, 41), 'SAME')
        d2 = O.conv2d_bwd_data(d1, ws[1], (41, 41), 'SAME')
        m1 = d1 * (masks[0][idx] > 0)
        m2 = O.conv2d_bwd_data(m1, ws[1], (41, 41), 'SAME') * (masks[1][idx] > 0)
        assert max(np.abs(f2).max(), np.abs(d2).max()) < 2 ** 24
        ref = {'fwd': (f1, f2), 'fwd_rotating': (f1, f2), 'dgrad': (d1, d2), 'dgrad_masked': (m1, m2)}
        _INT[n_per_cu] = dict(shape=shape, x=x, ws=ws, bs=bs, masks=masks, idx=idx, ref=ref)
    return _INT[n_per_cu]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n_per_cu', [1, 2])
def test_chain_equals_the_oracle_on_integers(dev, poison, n_per_cu, kind):
    c = _int_case(n_per_cu)
    t = lambda a: torch.from_numpy(a).to(dev)
    case = dict(shape=c['shape'], x=t(c['x']), dy=t(c['x']), ws=[t(w) for w in c['ws']], bs=[t(b) for b in c['bs']],
                masks=[t(m) for m in c['masks']])
    with switch(ops.set_chain_fixed, 1):
        got = _chain_run(case, dev, kind)
    torch.cuda.synchronize()
    for l in range(2):
        assert np.array_equal(got[l][c['idx']].cpu().numpy().astype(np.float64), c['ref'][kind][l]), 'layer %d' % (l + 1)


# ---- filter gradient ------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


_WG = {}


def _wgrad_case(dev, L, N, kind):
    """Inputs on the device and the float64 oracle, computed once and never written again."""
    key = (L, N, kind)
    if key not in _WG:
        rng = np.random.RandomState(2000 * L + N + (7 if kind == 'int' else 0))
        shape = (L, N, 41, 41, 64)
        if kind == 'int':
            # |x|, |dpre| <= 3: every partial sum is an integer of magnitude <= 9 N 1681 < 2^24, so every fp32 sum is exact
            x = rng.randint(-3, 4, shape).astype(np.float32)
            dp = rng.randint(-3, 4, shape).astype(np.float32)
            ref = [O.conv2d_bwd_filter(x[l], dp[l], (3, 3)) for l in range(L)]
        else:
            x = rng.standard_normal(shape).astype(np.float32)
            dp = (rng.standard_normal(shape) * 0.05).astype(np.float32)
            ref = None
        _WG[key] = dict(x=[torch.from_numpy(x[l]).to(dev) for l in range(L)], dp=[torch.from_numpy(dp[l]).to(dev) for l in range(L)],
                        ref=ref)
    return _WG[key]


def _per_layer(dev, c, l):
    dw, db = torch.full(WSHAPE, NAN, device=dev), torch.full((64,), NAN, device=dev)
    ops.conv2d_bwd_filter(c['x'][l], c['dp'][l], WSHAPE, dw=dw, dbias=db)
    return dw, db


def _batched(dev, c, L, N):
    dws = [torch.full(WSHAPE, NAN, device=dev) for _ in range(L)]
    dbs = [torch.full((64,), NAN, device=dev) for _ in range(L)]
    need = ops.bwd_filter_batch_workspace_bytes((N, 41, 41, 64), WSHAPE, L)
    ws = torch.full((need // 4,), NAN, device=dev)
    with switch(ops.set_wgrad_batch, 1):
        ops.conv2d_bwd_filter_batch(c['x'], c['dp'], dws, dbs, workspace=ws)
    torch.cuda.synchronize()
    return dws, dbs


@pytest.mark.parametrize('N', [1, 7, 16])
def test_per_layer_filter_gradient(dev, poison, N):
    """Integer data: dw and dbias EQUAL the float64 oracle.  Random data: two runs give the same bits."""
    c = _wgrad_case(dev, 1, N, 'int')
    dw, db = _per_layer(dev, c, 0)
    rw, rb = c['ref'][0]
    assert np.array_equal(dw.cpu().numpy().astype(np.float64), rw), 'dw against the oracle'
    assert np.array_equal(db.cpu().numpy().astype(np.float64), rb), 'dbias against the oracle'
    r = _wgrad_case(dev, 1, N, 'float')
    a, b = _per_layer(dev, r, 0), _per_layer(dev, r, 0)
    assert not torch.isnan(a[0]).any() and not torch.isnan(a[1]).any()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'two calls differ'


@pytest.mark.parametrize('L,N', [(2, 1), (3, 3), (18, 7)])
def test_batched_filter_gradient(dev, poison, L, N):
    """Integer data: every layer's dw and dbias EQUAL the float64 oracle.  Random data: two runs give the same bits, and batched
    and per-layer results differ by at most 2 gamma(K + 258) S (1 + gamma) per element (tests/test_gpu_wgrad_batch.py: each
    side is within gamma(K + its number of partials + 2) S of the exact sum; S = the filter gradient of |x| and |dpre|,
    K = 1681 N)."""
    c = _wgrad_case(dev, L, N, 'int')
    dws, dbs = _batched(dev, c, L, N)
    for l in range(L):
        rw, rb = c['ref'][l]
        assert np.array_equal(dws[l].cpu().numpy().astype(np.float64), rw), 'dw of layer %d against the oracle' % l
        assert np.array_equal(dbs[l].cpu().numpy().astype(np.float64), rb), 'dbias of layer %d against the oracle' % l
    r = _wgrad_case(dev, L, N, 'float')
    a, b = _batched(dev, r, L, N), _batched(dev, r, L, N)
    g = gamma(1681 * N + 258)
    for l in range(L):
        assert torch.equal(a[0][l], b[0][l]) and torch.equal(a[1][l], b[1][l]), 'layer %d: two calls differ' % l
        pw, pb = _per_layer(dev, r, l)
        sw, sb = ops.conv2d_bwd_filter(r['x'][l].abs(), r['dp'][l].abs(), WSHAPE)
        for got, per, s in ((a[0][l], pw, sw), (a[1][l], pb, sb)):
            err = (got.double() - per.double()).abs()
            assert bool((err <= 2 * g * s.double() * (1 + g)).all()), 'layer %d: batched against per-layer' % l
