"""Host-side checks of the chained body layers (srx_conv_chain_supported / srx_set_chain): which layers a chain takes.
No device call: without a GPU the library plans for 256 compute units."""
import ctypes

from ml_super_resolution_amd import _lib


def _q(L, n, h, w, op=_lib.OP_FWD, act=_lib.ACT_RELU, in_act=_lib.ACT_RELU, cin=64, cout=64, k=3, stride=1, pad=_lib.PAD_SAME,
       precision=0):
    d = _lib.ConvDesc(n, h, w, cin, cout, k, k, stride, pad, act, 0, precision, 0)
    return L.srx_conv_chain_supported(ctypes.byref(d), op, in_act)


def test_chain_eligibility_without_gpu():
    L = _lib.lib()
    try:
        assert L.srx_set_chain(1) in (0, 1)
        assert _q(L, 256, 41, 41) == 1
        assert _q(L, 512, 41, 41) == 1
        assert _q(L, 256, 41, 41, op=_lib.OP_BWD_DATA) == 1
        assert _q(L, 256, 41, 41, op=_lib.OP_BWD_DATA, in_act=_lib.ACT_NONE) == 1
        assert _q(L, 16, 41, 41) == 0 and b'multiple' in L.srx_last_error()      # a workgroup would split an image
        assert _q(L, 300, 41, 41) == 0
        assert _q(L, 4, 128, 128) == 0                                            # column strips
        assert _q(L, 256, 41, 41, precision=1) == 0                               # bf16x3
        assert _q(L, 256, 41, 41, cout=32) == 0
        assert _q(L, 256, 41, 41, k=5) == 0
        assert _q(L, 256, 41, 41, pad=_lib.PAD_VALID) == 0
        assert _q(L, 256, 41, 41, act=_lib.ACT_TANH) == 0
        assert _q(L, 256, 41, 41, op=_lib.OP_BWD_FILTER) == 0
        assert L.srx_set_chain(0) == 1
        assert _q(L, 256, 41, 41) == 0 and b'switched off' in L.srx_last_error()
        old = L.srx_set_conv_path(0)
        L.srx_set_chain(1)
        try:
            assert _q(L, 256, 41, 41) == 0                                        # conv path 0
        finally:
            L.srx_set_conv_path(old)
    finally:
        L.srx_set_chain(-1)


def test_chain_refuses_bad_layer_counts_without_gpu():
    L = _lib.lib()
    d = _lib.ConvDesc(256, 41, 41, 64, 64, 3, 3, 1, _lib.PAD_SAME, _lib.ACT_RELU, 0, 0, 0)
    arr = (ctypes.c_void_p * 33)()
    assert L.srx_conv_chain(ctypes.byref(d), _lib.OP_FWD, 0, 0, arr, arr, None, None, arr, None) == -1   # SRX_ERR_BAD_ARG
    assert L.srx_conv_chain(ctypes.byref(d), _lib.OP_FWD, 0, 33, arr, arr, None, None, arr, None) == -1   # SRX_ERR_BAD_ARG
    assert L.srx_conv_chain(ctypes.byref(d), _lib.OP_FWD, 0, 2, arr, arr, None, None, arr, None) != 0   # null tensors
