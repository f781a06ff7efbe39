"""NumPy restatements for the bytes-in, bytes-out ESPCN path (csrc/u8_encode.h: encode_unit_u8; ops.unit_lut) and the
crafted fp32 set its encoder is checked on.  Shared by tests/test_espcn_frames_host.py and tests/test_gpu_espcn_frames.py."""
import functools

import numpy as np

F = np.float32


def lut_ref():
    """The host route's decode of every byte (espcn/espcn/experiment_test.py:160): float64 arithmetic, one cast."""
    return (np.arange(256, dtype=np.uint8) / 127.5 - 1.0).astype(np.float32)


def encode_unit_u8(y):
    """encode_unit_u8 step by step in float32: `* 0.5`, `+ 0.5`, clamp to [0, 1], `* 255`, `+ 0.5`, truncation."""
    t = np.asarray(y, dtype=np.float32) * F(0.5)
    t = t + F(0.5)
    t = np.minimum(np.maximum(t, F(0.0)), F(1.0))
    t = t * F(255.0)
    t = t + F(0.5)
    assert t.dtype == np.float32
    return t.astype(np.uint8)


def encode_unit_u8_by_float64(y):
    """The same five steps, each evaluated in float64 and rounded to float32 once: a float64 product or sum of two float32
    values of these magnitudes is exact, so the cast is the one correct rounding of the step -- no float32 arithmetic of
    NumPy's is trusted here."""
    with np.errstate(over='ignore'):
        t = (np.asarray(y, dtype=np.float32).astype(np.float64) * 0.5).astype(np.float32)
        t = (t.astype(np.float64) + 0.5).astype(np.float32)
        t = np.clip(t, F(0.0), F(1.0))
        t = (t.astype(np.float64) * 255.0).astype(np.float32)
        t = (t.astype(np.float64) + 0.5).astype(np.float32)
    return np.floor(t.astype(np.float64)).astype(np.uint8)


def host_route_bytes(y):
    """What the route that existed makes of network outputs y: experiment_test.py:76 -- ops.affine(sr, 0.5, 0.5) (multiply
    and add rounded separately, in float32) and clamp_(0, 1) -- then :85 verbatim."""
    sr = np.asarray(y, dtype=np.float32) * F(0.5)
    sr = np.clip(sr + F(0.5), 0.0, 1.0)
    return (sr * 255.0 + 0.5).astype(np.uint8)


def _steps(x, n):
    """x, then n floats upward and n floats downward of it, one ulp apart."""
    out, up, down = [x], x, x
    for _ in range(n):
        up = np.nextafter(up, F(np.inf))
        down = np.nextafter(down, F(-np.inf))
        out += [up, down]
    return out


def _key(x):
    """float32 -> an int that orders as the floats do (-0 and +0 share 0)."""
    i = int(np.array(x, dtype=np.float32).view(np.int32))
    return i if i >= 0 else -(i & 0x7fffffff)


def _float(key):
    return np.array(key if key >= 0 else (-key) | 0x80000000, dtype=np.uint32).view(np.float32)[()]


@functools.lru_cache(maxsize=None)
def _crafted():
    vals = []
    for k in range(256):
        # the byte changes to k near y = (2 k - 1) / 255 - 1; find the first float that encodes to k exactly
        if k == 0:
            vals += _steps(F(-1.0), 3)
            continue
        # (by bisection over the floats in order: near y = 0, byte 128, the boundary lies millions of ulps of y from there)
        lo, hi = _key(F(-2.0)), _key(F(2.0))
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if encode_unit_u8(_float(mid)) >= k:
                hi = mid
            else:
                lo = mid
        y = _float(hi)
        assert encode_unit_u8(y) == k and encode_unit_u8(np.nextafter(y, F(-np.inf))) == k - 1, k
        vals += _steps(y, 3)
    vals += _steps(F(1.0), 3)
    vals += [F(0.0), F(-0.0), F(np.inf), F(-np.inf), F(1.5), F(-1.5), F(2.0), F(-2.0), F(255.0), F(-255.0), F(1e30), F(-1e30),
             F(3.4e38), F(-3.4e38), F(1e-45), F(-1e-45), F(1e-38), F(-1e-38), F(0.999999), F(-0.999999)]
    a = np.array(vals, dtype=np.float32)
    a.setflags(write=False)
    return a


def crafted_set():
    """For every byte k the first float that encodes to k with its +-3-ulp neighbours (k = 0: -1 and its neighbours), +-0,
    +-inf, subnormals and values beyond [-1, 1].  No NaN: the host route's astype of one is undefined.  Read-only."""
    return _crafted()


def crafted_values(n, start=0):
    """n values of the crafted set from position start on, wrapping round."""
    s = crafted_set()
    return np.take(s, np.arange(start, start + n), mode='wrap')
