"""Host-side checks of precision 1 (bf16x3, include/srx.h srx_precision): the capability query, the workspace query and
argument validation, without a GPU."""
import ctypes

import pytest

from ml_super_resolution_amd import _lib


def _desc(N=256, H=41, W=41, Cin=64, Cout=64, K=3, stride=1, pad=0, act=1, post=0, precision=1, r=0):
    return _lib.ConvDesc(N, H, W, Cin, Cout, K, K, stride, pad, act, post, precision, r)


def _query(d, op):
    L = _lib.lib()
    return L.srx_conv2d_precision_supported(ctypes.byref(d), op), L.srx_last_error().decode()


@pytest.mark.parametrize('op', [_lib.OP_FWD, _lib.OP_BWD_DATA, _lib.OP_BWD_FILTER])
@pytest.mark.parametrize('nhw', [(256, 41, 41), (1, 1, 1), (1, 720, 1280), (3, 5, 200)])
def test_vdsr_body_layer_is_supported(op, nhw):
    for act in (_lib.ACT_NONE, _lib.ACT_RELU):
        assert _query(_desc(*nhw, act=act), op)[0] == 1


@pytest.mark.parametrize('op', [_lib.OP_FWD, _lib.OP_BWD_DATA, _lib.OP_BWD_FILTER])
@pytest.mark.parametrize('kw', [dict(K=9, Cin=3), dict(Cout=32), dict(stride=2), dict(post=_lib.ACT_RELU), dict(r=3),
                                dict(act=_lib.ACT_TANH), dict(pad=_lib.PAD_VALID), dict(Cin=3), dict(Cout=3)])
def test_outside_the_set_is_refused_with_a_reason(op, kw):
    ok, msg = _query(_desc(**kw), op)
    assert ok == 0
    assert msg       # (the reason: 'precision 1 (bf16x3): ...', or what makes the descriptor invalid)


def test_precision_zero_always_supported():
    for kw in (dict(K=9, Cin=3), dict(Cout=32), dict(stride=2), dict(act=_lib.ACT_TANH)):
        assert _query(_desc(precision=0, **kw), _lib.OP_FWD)[0] == 1


def test_workspace_bytes_at_precision_one():
    L = _lib.lib()
    d = _desc()
    ws = L.srx_conv2d_workspace_bytes(ctypes.byref(d), _lib.OP_BWD_FILTER)
    assert ws > 0 and ws % 16 == 0
    # one partial filter per workgroup, at most two workgroups per CU of the largest device
    per = (9 * 64 * 64 + 64) * 4
    assert ws % per == 0 and 1 <= ws // per <= 512
    assert L.srx_conv2d_workspace_bytes(ctypes.byref(d), _lib.OP_FWD) > 0
    assert L.srx_conv2d_workspace_bytes(ctypes.byref(_desc(Cout=32)), _lib.OP_BWD_FILTER) == 0
    assert 'precision 1' in L.srx_last_error().decode()


def test_bad_precision_values_are_bad_arguments():
    L = _lib.lib()
    for p in (2, -1, 7):
        d = _desc(precision=p)
        assert L.srx_conv2d_precision_supported(ctypes.byref(d), _lib.OP_FWD) == 0
        assert L.srx_conv2d_workspace_bytes(ctypes.byref(d), _lib.OP_BWD_FILTER) == 0
        rc = L.srx_conv2d_fwd(ctypes.byref(d), None, None, None, None, None, None, 0, None)
        assert rc == -1 and b'precision' in L.srx_last_error()


def test_unsupported_layer_refused_before_any_launch():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)       # (host memory: the call must fail on the descriptor, before a launch)
    d = _desc(Cout=32)
    assert L.srx_conv2d_fwd(ctypes.byref(d), p, p, None, None, p, None, 0, None) == -2
    assert 'precision 1' in L.srx_last_error().decode()
    assert L.srx_conv2d_bwd_data(ctypes.byref(d), p, p, None, 0, p, None, 0, None) == -2
    n = ctypes.c_int(0)
    assert L.srx_conv2d_bwd_filter_partials(ctypes.byref(d), p, p, p, 1 << 20, ctypes.byref(n), None) == -2


def test_python_names():
    from ml_super_resolution_amd import ops
    assert ops.precision_code('highest') == 0 and ops.precision_code('high') == 1 and ops.precision_code(1) == 1
    with pytest.raises(ValueError):
        ops.precision_code('medium')
    assert ops.precision_supported((8, 41, 41, 64), (3, 3, 64, 64), _lib.OP_FWD, act='relu') == (True, '')
    ok, why = ops.precision_supported((8, 41, 41, 3), (3, 3, 3, 64), _lib.OP_BWD_FILTER)
    assert not ok and 'channels' in why
