"""Precision 1 (bf16x3) of the channel-blocked 3x3 layers wider than 64 channels (srx_conv3x3_blocked_ex,
srx_conv3x3_blocked_bwd_filter_ex) on the MI355X: the worst-case bound and the three-term calibration against the float64
oracle, that the fast kernels ran, determinism, batch invariance, NaN propagation, and precision 0 through the _ex
entry points against the old ones."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle_enet as OE

pytestmark = pytest.mark.gpu

BLOCKS = [(1, 2), (2, 2), (2, 4), (4, 4), (8, 8)]
SHAPES = [(1, 1, 1), (2, 5, 7), (3, 16, 16), (1, 8, 130), (2, 64, 64)]
BOUND = 2.0 ** -13


def _dev():
    return torch.device('cuda', 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


# blocked <-> NHWC / HWIO on the host (numpy): the oracle side does not go through the library
def to_nhwc(b):
    cb, n, h, w, c = b.shape
    return b.transpose(1, 2, 3, 0, 4).reshape(n, h, w, cb * c)


def to_blocked(a, cb):
    n, h, w, c = a.shape
    return a.reshape(n, h, w, cb, c // cb).transpose(3, 0, 1, 2, 4)


def w_hwio(wb):
    cib, cob = wb.shape[:2]
    return wb.transpose(2, 3, 0, 4, 1, 5).reshape(3, 3, cib * 64, cob * 64)


def w_blocked(k, cib, cob):
    return k.reshape(3, 3, cib, 64, cob, 64).transpose(2, 4, 0, 1, 3, 5)


def _data(cib, cob, N, H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(cib, N, H, W, 64)).astype(np.float32)
    w = (rng.normal(size=(cib, cob, 3, 3, 64, 64)) * (0.5 / np.sqrt(9 * 64 * cib))).astype(np.float32)
    b = rng.normal(size=(cob * 64,)).astype(np.float32)
    dpre = rng.normal(size=(cob, N, H, W, 64)).astype(np.float32)
    mask = rng.normal(size=(cib, N, H, W, 64)).astype(np.float32)
    return x, w, b, dpre, mask


def _fwd(x, w, b, act, precision):
    from ml_super_resolution_amd import ops
    return ops.conv3x3_blocked(_t(x), _t(w), None if b is None else _t(b), act, precision=precision).cpu().numpy()


def _dgrad(dpre, w, mask, mask_act, precision):
    from ml_super_resolution_amd import ops
    return ops.conv3x3_blocked(_t(dpre), _t(w), None, None, transpose=True, mask=None if mask is None else _t(mask),
                               mask_act=mask_act, precision=precision).cpu().numpy()


def _wgrad(x, dpre, precision):
    from ml_super_resolution_amd import ops
    cib, cob = x.shape[0], dpre.shape[0]
    dw = torch.empty((cib, cob, 3, 3, 64, 64), dtype=torch.float32, device=_dev())
    db = torch.empty((cob * 64,), dtype=torch.float32, device=_dev())
    ops.conv3x3_blocked_bwd_filter(_t(x), _t(dpre), dw, db, precision=precision)
    return dw.cpu().numpy(), db.cpu().numpy()


def _act(v, act):
    if act == 'relu':
        return np.maximum(v, 0)
    if act == 'lrelu':
        return np.where(v > 0, v, 0.2 * v)
    return v


def _mask_grad(v, m, mask_act):
    if mask_act == 'relu':
        return np.where(m > 0, v, 0)
    return np.where(m > 0, v, 0.2 * v)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('blocks', BLOCKS)
def test_worst_case_bound(blocks, shape):
    """Every element of the forward pass (three activations), the data gradient (no mask, ReLU and leaky-ReLU masks) and
    the filter gradient of all pairs within 2^-13 (|x| (*) |w| + |b|) of float64; one oracle pass per op."""
    cib, cob = blocks
    x, w, b, dpre, mask = _data(cib, cob, *shape, seed=1)
    k = w_hwio(w)
    # forward
    pre = to_blocked(OE.conv2d_same_fwd(to_nhwc(x), k, b), cob)
    bound = BOUND * to_blocked(OE.conv2d_same_fwd(np.abs(to_nhwc(x)), np.abs(k), np.abs(b)), cob)
    for act in (None, 'relu', 'lrelu'):
        y = _fwd(x, w, b, act, 'high')
        assert np.all(np.isfinite(y))
        err = np.abs(y - _act(pre, act))
        assert np.all(err <= bound), (act, np.max(err / bound))
    # data gradient
    x0 = np.zeros(to_nhwc(mask).shape, np.float32)
    ref = to_blocked(OE.conv2d_same_bwd(x0, k, to_nhwc(dpre))[0], cib)
    bound = BOUND * to_blocked(OE.conv2d_same_bwd(x0, np.abs(k), np.abs(to_nhwc(dpre)))[0], cib)
    for mask_act in (None, 'relu', 'lrelu'):
        dx = _dgrad(dpre, w, None if mask_act is None else mask, mask_act, 'high')
        r = ref if mask_act is None else _mask_grad(ref, mask, mask_act)
        err = np.abs(dx - r)
        assert np.all(err <= bound), (mask_act, np.max(err - bound))
    # filter gradient of all pairs; the bias gradient is a plain fp32 sum
    dw, db = _wgrad(x, dpre, 'high')
    _, ref_dw, ref_db = OE.conv2d_same_bwd(to_nhwc(x), k, to_nhwc(dpre), want_dx=False)
    _, abs_dw, abs_db = OE.conv2d_same_bwd(np.abs(to_nhwc(x)), k, np.abs(to_nhwc(dpre)), want_dx=False)
    err = np.abs(dw - w_blocked(ref_dw, cib, cob))
    assert np.all(err <= BOUND * w_blocked(abs_dw, cib, cob)), np.max(err - BOUND * w_blocked(abs_dw, cib, cob))
    assert np.all(np.abs(db - ref_db) <= 1e-5 * abs_db + 1e-6)


def _split(a):
    t = torch.from_numpy(np.asarray(a, np.float32))
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi.numpy().astype(np.float64), lo.numpy().astype(np.float64)


def _bf16(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def _rel_rms(y, ref):
    return float(np.sqrt(np.mean((np.asarray(y, np.float64) - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


def _check_calibrated(got, ref, emu3, emu1):
    e_got, e3, e1 = _rel_rms(got, ref), _rel_rms(emu3, ref), _rel_rms(emu1, ref)
    assert e_got <= 2 * e3 + 2e-6, (e_got, e3)
    assert e_got <= 0.05 * e1, (e_got, e1)


@pytest.mark.parametrize('blocks,shape', [((2, 2), (2, 5, 7)), ((2, 4), (3, 16, 16)), ((4, 4), (1, 8, 130))])
def test_calibrated_three_terms(blocks, shape):
    """The error is that of hi*hi + hi*lo + lo*hi, not of a one-pass bf16 product."""
    cib, cob = blocks
    x, w, _, dpre, _ = _data(cib, cob, *shape, seed=6)
    xn, k, dn = to_nhwc(x), w_hwio(w), to_nhwc(dpre)
    xh, xl = _split(xn)
    wh, wl = _split(k)
    dh, dl = _split(dn)
    f = lambda a, c: to_blocked(OE.conv2d_same_fwd(a, c, np.zeros(cob * 64)), cob)
    _check_calibrated(_fwd(x, w, None, None, 'high'), f(xn, k), f(xh, wh) + f(xh, wl) + f(xl, wh), f(_bf16(xn), _bf16(k)))
    x0 = np.zeros(xn.shape)
    g = lambda a, c: to_blocked(OE.conv2d_same_bwd(x0, c, a)[0], cib)
    _check_calibrated(_dgrad(dpre, w, None, None, 'high'), g(dn, k), g(dh, wh) + g(dh, wl) + g(dl, wh), g(_bf16(dn), _bf16(k)))
    h = lambda a, c: w_blocked(OE.conv2d_same_bwd(a, k, c, want_dx=False)[1], cib, cob)
    _check_calibrated(_wgrad(x, dpre, 'high')[0], h(xn, dn), h(xh, dh) + h(xh, dl) + h(xl, dh), h(_bf16(xn), _bf16(dn)))


@pytest.mark.parametrize('blocks,shape', [((2, 4), (3, 16, 16)), ((4, 2), (2, 64, 64)), ((2, 2), (1, 8, 130))])
def test_fast_path_ran_and_is_deterministic(blocks, shape):
    x, w, b, dpre, mask = _data(*blocks, *shape, seed=8)
    y1, y2, y0 = _fwd(x, w, b, 'lrelu', 'high'), _fwd(x, w, b, 'lrelu', 'high'), _fwd(x, w, b, 'lrelu', 'highest')
    assert np.array_equal(y1, y2) and not np.array_equal(y1, y0)
    d1, d2, d0 = (_dgrad(dpre, w, mask, 'relu', p) for p in ('high', 'high', 'highest'))
    assert np.array_equal(d1, d2) and not np.array_equal(d1, d0)
    (w1, b1), (w2, b2), (w0, b0) = (_wgrad(x, dpre, p) for p in ('high', 'high', 'highest'))
    assert np.array_equal(w1, w2) and np.array_equal(b1, b2) and not np.array_equal(w1, w0)


@pytest.mark.parametrize('hw', [(16, 16), (23, 37), (9, 130)])
def test_batch_invariance(hw):
    x, w, b, dpre, mask = _data(2, 2, 6, hw[0], hw[1], seed=10)
    y = _fwd(x, w, b, 'relu', 'high')
    dx = _dgrad(dpre, w, mask, 'lrelu', 'high')
    for n in (0, 2, 5):
        sl = slice(n, n + 1)
        assert np.array_equal(y[:, sl], _fwd(x[:, sl], w, b, 'relu', 'high'))
        assert np.array_equal(dx[:, sl], _dgrad(dpre[:, sl], w, mask[:, sl], 'lrelu', 'high'))


def test_nan_propagates_to_its_window_only():
    x, w, b, _, _ = _data(2, 2, 2, 9, 11, seed=12)
    x[1, 1, 4, 6, 5] = np.nan
    y = _fwd(x, w, b, None, 'high')
    expect = np.zeros(y.shape, bool)
    expect[:, 1, 3:6, 5:8, :] = True
    assert np.array_equal(np.isnan(y), expect)


@pytest.mark.parametrize('blocks,shape', [((2, 4), (3, 16, 16)), ((1, 2), (1, 8, 130)), ((4, 4), (2, 5, 7))])
def test_precision_zero_through_ex_is_the_old_entry(blocks, shape):
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd._lib import lib, ACT_BY_NAME
    cib, cob = blocks
    N, H, W = shape
    x, w, b, dpre, mask = (_t(a) for a in _data(cib, cob, N, H, W, seed=14))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    y_old = torch.empty((cob, N, H, W, 64), dtype=torch.float32, device=_dev())
    assert lib().srx_conv3x3_blocked(p(x), p(w), p(b), None, 0, p(y_old), N, H, W, cib, cob, ACT_BY_NAME['lrelu'], 0, s) == 0
    assert torch.equal(y_old, ops.conv3x3_blocked(x, w, b, 'lrelu', precision='highest'))
    d_old = torch.empty((cib, N, H, W, 64), dtype=torch.float32, device=_dev())
    assert lib().srx_conv3x3_blocked(p(dpre), p(w), None, p(mask), ACT_BY_NAME['relu'], p(d_old), N, H, W, cob, cib, 0, 1, s) == 0
    assert torch.equal(d_old, ops.conv3x3_blocked(dpre, w, None, None, transpose=True, mask=mask, mask_act='relu'))
    need = lib().srx_conv3x3_blocked_bwd_filter_workspace_bytes(N, H, W, cib, cob)
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=_dev())
    dw_old = torch.empty((cib, cob, 3, 3, 64, 64), dtype=torch.float32, device=_dev())
    db_old = torch.empty((cob * 64,), dtype=torch.float32, device=_dev())
    assert lib().srx_conv3x3_blocked_bwd_filter(p(x), p(dpre), p(dw_old), p(db_old), N, H, W, cib, cob, p(ws), need, s) == 0
    dw, db = torch.empty_like(dw_old), torch.empty_like(db_old)
    ops.conv3x3_blocked_bwd_filter(x, dpre, dw, db, precision='highest')
    assert torch.equal(dw_old, dw) and torch.equal(db_old, db)
