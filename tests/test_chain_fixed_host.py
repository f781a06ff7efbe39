"""Host-side checks of the fixed-geometry chain switch (srx_set_chain_fixed / SRX_CHAIN_FIXED): it round-trips, and it does
not change which layers a chain takes -- only which kernel instance runs them.  No device call."""
import ctypes

from ml_super_resolution_amd import _lib, ops


def _q(L, n, h, w, op=_lib.OP_FWD, act=_lib.ACT_RELU, in_act=_lib.ACT_RELU, cin=64, cout=64, k=3, stride=1, pad=_lib.PAD_SAME,
       precision=0):
    d = _lib.ConvDesc(n, h, w, cin, cout, k, k, stride, pad, act, 0, precision, 0)
    return L.srx_conv_chain_supported(ctypes.byref(d), op, in_act)


# the queries of test_chain_host.py
QUERIES = [
    dict(n=256, h=41, w=41), dict(n=512, h=41, w=41), dict(n=256, h=41, w=41, op=_lib.OP_BWD_DATA),
    dict(n=256, h=41, w=41, op=_lib.OP_BWD_DATA, in_act=_lib.ACT_NONE), dict(n=16, h=41, w=41), dict(n=300, h=41, w=41),
    dict(n=4, h=128, w=128), dict(n=256, h=41, w=41, precision=1), dict(n=256, h=41, w=41, cout=32), dict(n=256, h=41, w=41, k=5),
    dict(n=256, h=41, w=41, pad=_lib.PAD_VALID), dict(n=256, h=41, w=41, act=_lib.ACT_TANH),
    dict(n=256, h=41, w=41, op=_lib.OP_BWD_FILTER), dict(n=256, h=33, w=33), dict(n=256, h=41, w=40),
]


def test_switch_round_trips_and_returns_the_previous_value():
    L = _lib.lib()
    default = L.srx_set_chain_fixed(-1)
    try:
        assert default in (0, 1)
        assert L.srx_set_chain_fixed(0) == default       # (unset: the environment's default is reported)
        assert L.srx_set_chain_fixed(1) == 0
        assert L.srx_set_chain_fixed(7) == 1             # any positive value: on
        assert L.srx_set_chain_fixed(0) == 1
        assert L.srx_set_chain_fixed(-1) == 0
        assert L.srx_set_chain_fixed(-5) == default      # back at the default
        assert ops.set_chain_fixed(1) == default
        assert ops.set_chain_fixed(-1) == 1
    finally:
        L.srx_set_chain_fixed(-1)


def test_switch_does_not_change_chain_eligibility():
    L = _lib.lib()
    old_chain = L.srx_set_chain(1)
    try:
        answers = []
        for on in (0, 1):
            L.srx_set_chain_fixed(on)
            answers.append([_q(L, **q) for q in QUERIES])
        assert answers[0] == answers[1]
        assert answers[0][:4] == [1, 1, 1, 1] and 0 in answers[0]
    finally:
        L.srx_set_chain_fixed(-1)
        L.srx_set_chain(old_chain if old_chain in (0, 1) else -1)
        L.srx_set_chain(-1)
