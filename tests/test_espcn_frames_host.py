"""Host-side checks of the bytes-in, bytes-out ESPCN path (no GPU): the NumPy restatement of encode_unit_u8 against the
expression of the route that existed, the plan of a frame-sequence run (espcn/frames.py: frame_schedule), and what
srx_espcn_forward_u8 refuses before it would launch."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import espcn_frames_ref as R


def test_restated_encode_equals_the_host_route_on_the_crafted_set():
    y = R.crafted_set()
    assert y.dtype == np.float32 and not np.isnan(y).any()
    got = R.encode_unit_u8(y)
    np.testing.assert_array_equal(got, R.host_route_bytes(y))
    np.testing.assert_array_equal(got, R.encode_unit_u8_by_float64(y))
    # the set holds what it promises: every byte value, each boundary from both sides, the clamp on both sides
    assert sorted(set(got.tolist())) == list(range(256))
    for k in range(1, 256):
        first = y[np.flatnonzero(got == k)].min()
        assert R.encode_unit_u8(np.nextafter(first, np.float32(-np.inf))) == k - 1
        for s in range(1, 4):                       # its neighbours up to 3 ulps on either side are in the set
            up = down = first
            for _ in range(s):
                up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
            assert (y == up).any() and (y == down).any(), k
    for v, b in ((0.0, 128), (-0.0, 128), (np.inf, 255), (-np.inf, 0), (1.5, 255), (-1.5, 0), (1e30, 255), (-1e30, 0), (1.0, 255), (-1.0, 0)):
        assert (y == np.float32(v)).any() and R.encode_unit_u8(np.float32(v)) == b, v
    assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()


def test_lut_is_the_host_routes_decode():
    img = np.arange(256, dtype=np.uint8)
    want = (img / 127.5 - 1.0).astype(np.float32)
    np.testing.assert_array_equal(R.lut_ref(), want)
    assert (img / 127.5).dtype == np.float64
    from ml_super_resolution_amd import ops
    np.testing.assert_array_equal(ops.unit_lut('cpu').numpy(), want)


@pytest.mark.parametrize('n,batch,depth', list(itertools.product((0, 1, 2, 7, 8), (1, 3), (1, 2, 3))))
def test_frame_schedule(n, batch, depth):
    from ml_super_resolution_amd.espcn.frames import frame_schedule
    steps = frame_schedule(n, batch, depth)
    assert all(op in ('upload', 'compute', 'download', 'yield') and 0 <= slot < depth for op, slot, _, _ in steps)
    batches = [(f, min(batch, n - f)) for f in range(0, n, batch)]
    at = {}
    for i, (op, slot, first, count) in enumerate(steps):
        assert (op, first) not in at, 'listed twice'
        assert (first, count) in batches and slot == batches.index((first, count)) % depth
        at[op, first] = i
    # every frame is uploaded, computed, downloaded and yielded exactly once, in that order
    assert len(steps) == 4 * len(batches)
    for first, _ in batches:
        assert at['upload', first] < at['compute', first] < at['download', first] < at['yield', first]
    # each kind of step, the yields among them, runs in input order
    for op in ('upload', 'compute', 'download', 'yield'):
        assert [f for o, _, f, _ in steps if o == op] == [f for f, _ in batches]
    for k, (first, _) in enumerate(batches):
        if k >= depth:
            # the slot is not uploaded into before its previous occupant has been yielded, and so not between that
            # occupant's compute and its yield
            prev = batches[k - depth][0]
            assert at['upload', first] > at['yield', prev] > at['compute', prev]
        if depth >= 2 and k + 1 < len(batches):
            assert at['upload', batches[k + 1][0]] < at['download', first]
        if depth >= 3 and k + 1 < len(batches):
            # the host waits for batch k's download (its yield) after batch k + 1's compute was enqueued
            assert at['compute', batches[k + 1][0]] < at['yield', first]


def test_frame_schedule_refuses_bad_arguments_and_reads_counts_lazily():
    from ml_super_resolution_amd.espcn.frames import frame_schedule, iter_schedule
    for args in ((-1, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError):
            frame_schedule(*args)
    taken = []

    def counts():
        for c in (2, 2, 1):
            taken.append(c)
            yield c

    seen = []
    for step in iter_schedule(counts(), 3):
        # a batch's size is asked for when its upload is listed, not before: a runner can feed it from a stream of frames
        assert len(taken) == sum(1 for s in seen + [step] if s[0] == 'upload')
        seen.append(step)
    assert seen == frame_schedule(5, 2, 3)


def test_espcn_forward_u8_refusals_without_gpu():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below is refused before a launch
    def call(lr=p, lut=p, hr=p, w1=p, b1=p, N=1, H=8, W=8, r=3):
        return L.srx_espcn_forward_u8(lr, lut, w1, b1, p, p, p, p, hr, N, H, W, r, None)
    for kw in ({'lr': None}, {'lut': None}, {'hr': None}, {'w1': None}):
        assert call(**kw) == -1 and b'null' in L.srx_last_error(), kw
    for r in (1, 5):
        assert call(r=r) != 0 and b'scaling factor %d' % r in L.srx_last_error()
    assert call(N=0) == -1 and b'dimension' in L.srx_last_error()
    assert call(b1=ctypes.c_void_p(4100)) != 0 and b'aligned' in L.srx_last_error()
    # N H W 3 r^2 >= 2^31: 2^16 x 2^11 x 2^0 x 27 = 1.6875 x 2^31
    assert call(N=1, H=1 << 16, W=1 << 11) != 0 and b'32-bit' in L.srx_last_error()
    # the two streaming passes refuse null pointers too
    assert L.srx_u8_lut_float(None, p, p, 16, None) == -1 and L.srx_u8_lut_float(p, None, p, 16, None) == -1
    assert L.srx_unit_u8(None, p, 16, None) == -1 and L.srx_unit_u8(p, None, 16, None) == -1
    assert L.srx_unit_u8(ctypes.c_void_p(4098), p, 16, None) != 0 and b'aligned' in L.srx_last_error()
    assert L.srx_unit_u8(p, p, 0, None) == 0 and L.srx_u8_lut_float(p, p, p, 0, None) == 0
