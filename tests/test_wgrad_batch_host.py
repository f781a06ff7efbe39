"""Host-side checks of the batched body filter gradients (srx_conv2d_bwd_filter_batch_plan / _workspace_bytes /
srx_set_wgrad_batch): which batches the library takes and how it splits them.  No device call: without a GPU the library
plans for 256 compute units."""
import ctypes

import pytest

from ml_super_resolution_amd import _lib

PART_STRIDE = 9 * 64 * 64 + 64


def _desc(n, h=41, w=41, cin=64, cout=64, k=3, stride=1, pad=_lib.PAD_SAME, precision=0):
    return _lib.ConvDesc(n, h, w, cin, cout, k, k, stride, pad, _lib.ACT_NONE, 0, precision, 0)


def _plan(L, d, layers):
    wpl, grid = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.srx_conv2d_bwd_filter_batch_plan(ctypes.byref(d), layers, ctypes.byref(wpl), ctypes.byref(grid))
    return rc, wpl.value, grid.value


@pytest.fixture
def L():
    lib = _lib.lib()
    lib.srx_set_wgrad_batch(1)
    yield lib
    lib.srx_set_wgrad_batch(-1)


@pytest.mark.parametrize('n', [1, 2, 7, 64, 256, 300])
@pytest.mark.parametrize('layers', [2, 3, 18, 32])
def test_plan_gives_every_workgroup_rows_and_fits_the_grid(L, n, layers):
    d = _desc(n)
    rc, wpl, grid = _plan(L, d, layers)
    assert rc == 0
    assert 1 <= wpl <= n * 41                     # no workgroup without a row
    assert wpl * layers <= grid <= 256
    assert wpl == min(grid // layers, n * 41)
    assert L.srx_conv2d_bwd_filter_batch_workspace_bytes(ctypes.byref(d), layers) == layers * wpl * PART_STRIDE * 4
    # the even split u0 = sub U / wpl: every range holds at least one row
    rows = n * 41
    assert all((s + 1) * rows // wpl > s * rows // wpl for s in range(wpl))


def test_the_benchmark_shape(L):
    assert _plan(L, _desc(256), 18) == (0, 14, 256)


@pytest.mark.parametrize('d,layers,reason', [
    (_desc(7), 1, b'layers'), (_desc(7), 33, b'layers'), (_desc(7, w=40), 18, b'W 40'), (_desc(7, precision=1), 18, b'precision 1'),
    (_desc(7, cout=32), 18, b'64->64'), (_desc(7, k=5), 18, b'64->64'), (_desc(7, pad=_lib.PAD_VALID), 18, b'SAME'),
    (_desc(7, stride=2), 18, b'stride-1'), (_desc(4, h=128, w=128), 18, b'W 128'),
])
def test_ineligible_batches_plan_zero_workgroups(L, d, layers, reason):
    rc, wpl, grid = _plan(L, d, layers)
    assert rc == -2 and wpl == 0 and grid == 0                    # SRX_ERR_UNSUPPORTED
    assert reason in L.srx_last_error()
    assert L.srx_conv2d_bwd_filter_batch_workspace_bytes(ctypes.byref(d), layers) == 0


def test_other_row_heights_are_eligible(L):
    # (the per-layer kernel takes any number of 41-pixel rows)
    assert _plan(L, _desc(3, h=17), 18)[1] == 14


def test_switch_round_trips_and_does_not_follow_the_other_switches(L):
    d = _desc(256)
    assert L.srx_set_wgrad_batch(0) == 1
    assert _plan(L, d, 18)[1] == 0 and b'switched off' in L.srx_last_error()
    assert L.srx_set_wgrad_batch(1) == 0
    assert L.srx_set_wgrad_batch(1) == 1
    old_chain, old_path = L.srx_set_chain(0), L.srx_set_conv_path(0)
    try:
        assert _plan(L, d, 18) == (0, 14, 256)
    finally:
        L.srx_set_chain(-1)
        L.srx_set_conv_path(old_path)
    # where the per-layer call would not run wgrad_rows_full_kernel, neither does the batch
    L.srx_set_wgrad_path(1)
    try:
        assert _plan(L, d, 18)[1] == 0
    finally:
        L.srx_set_wgrad_path(-1)
