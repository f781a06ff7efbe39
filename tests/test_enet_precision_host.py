"""Host-side checks of precision 1 (bf16x3) on the channel-blocked layers (srx_conv3x3_blocked_ex,
srx_conv3x3_blocked_bwd_filter_ex) and of the precision argument of the Python layers above them, without a GPU."""
import ctypes

import numpy as np
import pytest

from ml_super_resolution_amd import _lib

BAD_ARG, UNSUPPORTED = -1, -2


def _host(n):
    # 16-byte aligned host memory: the checks under test come before any launch
    a = np.zeros(n + 4, np.float32)
    off = (-a.ctypes.data % 16) // 4
    return a, ctypes.c_void_p(a.ctypes.data + 4 * off)


def _fwd_ex(precision, act=_lib.ACT_RELU, transpose=0):
    L = _lib.lib()
    N, H, W, sb, pb = 1, 4, 4, 2, 2
    keep = [_host(sb * N * H * W * 64), _host(sb * pb * 9 * 64 * 64), _host(pb * N * H * W * 64)]
    (_, x), (_, w), (_, y) = keep
    rc = L.srx_conv3x3_blocked_ex(x, w, None, None, 0, y, N, H, W, sb, pb, act, transpose, precision, None)
    return rc, L.srx_last_error().decode()


def _wgrad_ex(precision):
    L = _lib.lib()
    N, H, W, cib, cob = 1, 4, 4, 2, 2
    keep = [_host(cib * N * H * W * 64), _host(cob * N * H * W * 64), _host(cib * cob * 9 * 64 * 64), _host(1 << 16)]
    (_, x), (_, d), (_, dw), (_, ws) = keep
    rc = L.srx_conv3x3_blocked_bwd_filter_ex(x, d, dw, None, N, H, W, cib, cob, precision, ws, 1 << 18, None)
    return rc, L.srx_last_error().decode()


def test_symbols_are_exported():
    L = _lib.lib()
    for name in ('srx_conv3x3_blocked_ex', 'srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes',
                 'srx_conv3x3_blocked_bwd_filter_ex'):
        assert name in _lib.EXPORTS and hasattr(L, name)


@pytest.mark.parametrize('precision', [2, -1, 7])
def test_bad_precision_is_a_bad_argument(precision):
    for transpose in (0, 1):
        rc, msg = _fwd_ex(precision, transpose=transpose)
        assert rc == BAD_ARG and 'precision' in msg
    rc, msg = _wgrad_ex(precision)
    assert rc == BAD_ARG and 'precision' in msg
    assert _lib.lib().srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes(2, 8, 8, 2, 2, precision) == 0


@pytest.mark.parametrize('precision', [0, 1])
@pytest.mark.parametrize('act', [_lib.ACT_TANH, _lib.ACT_SIGMOID])
def test_other_activations_are_unsupported(precision, act):
    rc, msg = _fwd_ex(precision, act=act)
    assert rc == UNSUPPORTED and 'activation' in msg


@pytest.mark.parametrize('shape', [(1, 1, 1, 1, 2), (2, 5, 7, 2, 2), (64, 16, 16, 4, 8), (2, 64, 64, 8, 8), (1, 8, 130, 2, 4)])
def test_precision_one_workspace(shape):
    L = _lib.lib()
    ws1 = L.srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes(*shape, 1)
    assert ws1 > 0 and ws1 % 16 == 0
    # one fp32 partial filter (+ bias) per (pair, workgroup)
    per = (9 * 64 * 64 + 64) * 4
    assert ws1 % per == 0
    # precision 0 through _ex is the old query
    assert L.srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes(*shape, 0) == L.srx_conv3x3_blocked_bwd_filter_workspace_bytes(*shape)


def test_python_names():
    from ml_super_resolution_amd import ops
    n, h, w = 2, 8, 8
    assert ops.conv3x3_blocked_bwd_filter_workspace_bytes(n, h, w, 2, 2, precision='high') > 0
    assert ops.conv3x3_blocked_bwd_filter_workspace_bytes(n, h, w, 2, 2, precision='highest') == \
        ops.conv3x3_blocked_bwd_filter_workspace_bytes(n, h, w, 2, 2)
    with pytest.raises(ValueError):
        ops.conv3x3_blocked_bwd_filter_workspace_bytes(n, h, w, 2, 2, precision='medium')


def test_blocked_conv_precision_argument():
    from ml_super_resolution_amd.blocked import BlockedConv
    for p in ('highest', 'high'):
        assert BlockedConv(128, 128, precision=p).precision == p
    c = BlockedConv(128, 256, act='relu')
    assert c.precision == 'highest' and c.runs_at(16) == 'highest'
    c.set_precision('high')
    assert c.runs_at(16) == 'high'
    with pytest.raises(ValueError):
        c.set_precision('medium')
    # the layers that stay exact at 'high'
    assert BlockedConv(3, 64, act='relu', precision='high').runs_at(32) == 'highest'
    assert BlockedConv(32, 32, act='lrelu', precision='high').runs_at(32) == 'highest'
    assert BlockedConv(64, 64, stride=2, act='lrelu', precision='high').runs_at(32) == 'highest'
    assert BlockedConv(64, 64, act='relu', precision='high').runs_at(32) == 'high'


def test_enet_model_rejects_a_bad_precision():
    from ml_super_resolution_amd.enet import model_enet
    with pytest.raises(ValueError):
        model_enet.EnetModel('pat', {}, device='cpu', precision='medium')
