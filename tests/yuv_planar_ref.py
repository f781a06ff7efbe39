"""NumPy restatement of the planar YUV arithmetic at 8, 10 and 12 bits and 4:4:4, 4:2:2 and 4:2:0 sampling
(csrc/espcn_yuv_formats.hip, include/srx.h), crafted floats per depth and Y4M streams built in memory.  Shared by
tests/test_espcn_yuv_formats_host.py and tests/test_gpu_espcn_yuv_formats.py.  Everything is int64 here: no accumulator can wrap.
Frames are uint8 arrays of frame_bytes bytes at every depth; samples above 8 bits are two bytes, little-endian."""
import functools
import math

import numpy as np

from tests import yuv420_ref as Y
from tests.espcn_frames_ref import _float, _key, _steps

F = np.float32
NAMES, MATRICES, COMBOS = Y.NAMES, Y.MATRICES, Y.COMBOS
DEPTHS = (8, 10, 12)
# name -> (depth, sub_x, sub_y)
FORMATS = {'yuv%sp%s' % (s, suffix): (depth, sx, sy) for s, sx, sy in (('420', 1, 1), ('422', 1, 0), ('444', 0, 0))
           for suffix, depth in (('', 8), ('10le', 10), ('12le', 12))}
SAMPLINGS = ((0, 0), (1, 0), (1, 1))
Y4M_TAGS = {'yuv420p': 'C420jpeg', 'yuv422p': 'C422', 'yuv444p': 'C444', 'yuv420p10le': 'C420p10', 'yuv422p10le': 'C422p10',
            'yuv444p10le': 'C444p10', 'yuv420p12le': 'C420p12', 'yuv422p12le': 'C422p12', 'yuv444p12le': 'C444p12'}
# the issue's pins, bt709 limited at depth 10
PINS_709_10 = dict(yoff=64, cy=19133, crv=29459, cgu=3504, cgv=8757, cbu=34711, kry=2983, kgy=10034, kby=1013,
                   kru=-1644, kgu=-5531, kbu=7175, krv=7175, kgv=-6517, kbv=-658)
# (R, G, B) codes -> (Y, U, V), bt709 limited at depth 10
KNOWN_709_10 = [((1023, 0, 0), (250, 409, 960)), ((0, 1023, 0), (691, 167, 105)), ((0, 0, 1023), (127, 960, 471))]


def coeffs(matrix, full_range, depth):
    """{name: int}: floor(v * 16384 + 0.5) of the real values in double, from (Kr, Kb), the range and the depth."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    step, top = float(1 << (depth - 8)), float((1 << depth) - 1)
    ys, cs = (1.0, 1.0) if full_range else (219.0 * step / top, 224.0 * step / top)
    real = dict(cy=1.0 / ys, crv=2.0 * (1.0 - kr) / cs, cgu=2.0 * (1.0 - kb) * kb / kg / cs, cgv=2.0 * (1.0 - kr) * kr / kg / cs,
                cbu=2.0 * (1.0 - kb) / cs, kry=kr * ys, kgy=kg * ys, kby=kb * ys,
                kru=-kr / (2.0 * (1.0 - kb)) * cs, kgu=-kg / (2.0 * (1.0 - kb)) * cs, kbu=0.5 * cs,
                krv=0.5 * cs, kgv=-kg / (2.0 * (1.0 - kr)) * cs, kbv=-kb / (2.0 * (1.0 - kr)) * cs)
    out = {k: int(math.floor(v * 16384.0 + 0.5)) for k, v in real.items()}
    out['yoff'] = 0 if full_range else 16 << (depth - 8)
    return out


of_struct = Y.of_struct


def geometry(h, w, fmt):
    """(depth, sub_x, sub_y, bytes per sample, CH, CW) of a format name at h x w."""
    depth, sx, sy = FORMATS[fmt]
    return depth, sx, sy, 1 if depth == 8 else 2, (h + sy) >> sy, (w + sx) >> sx


def frame_samples(h, w, fmt):
    _, _, _, _, ch, cw = geometry(h, w, fmt)
    return h * w + 2 * ch * cw


def frame_bytes(h, w, fmt):
    return geometry(h, w, fmt)[3] * frame_samples(h, w, fmt)


def to_samples(frames, h, w, fmt):
    """[N, frame_bytes] uint8 -> [N, frame_samples] int64 sample values as stored (not yet limited to max)."""
    frames = np.ascontiguousarray(np.asarray(frames, dtype=np.uint8)).reshape(-1, frame_bytes(h, w, fmt))
    if geometry(h, w, fmt)[3] == 1:
        return frames.astype(np.int64)
    return frames.view('<u2').astype(np.int64)


def to_bytes(samples, fmt):
    """[N, frame_samples] sample values -> [N, frame_bytes] uint8."""
    samples = np.asarray(samples)
    if FORMATS[fmt][0] == 8:
        return samples.astype(np.uint8)
    return np.ascontiguousarray(samples.astype('<u2')).view(np.uint8).reshape(samples.shape[0], -1)


def split(samples, h, w, fmt):
    """[N, frame_samples] -> Y [N,H,W], U, V [N,CH,CW] (views)."""
    _, _, _, _, ch, cw = geometry(h, w, fmt)
    n = samples.shape[0]
    return (samples[:, :h * w].reshape(n, h, w), samples[:, h * w:h * w + ch * cw].reshape(n, ch, cw),
            samples[:, h * w + ch * cw:].reshape(n, ch, cw))


def decode(frames, h, w, fmt, c):
    """[N, frame_bytes] uint8 -> RGB codes [N,H,W,3] int64: a sample above max is read as max; pixel (y, x) takes the chroma
    sample (y >> sub_y, x >> sub_x)."""
    depth, sx, sy = FORMATS[fmt]
    top, mid = (1 << depth) - 1, 1 << (depth - 1)
    y, u, v = split(np.minimum(to_samples(frames, h, w, fmt), top), h, w, fmt)
    rows, cols = np.arange(h) >> sy, np.arange(w) >> sx
    cc = y - c['yoff']
    d = u[:, rows][:, :, cols] - mid
    e = v[:, rows][:, :, cols] - mid
    half = 1 << 13
    r = np.clip((c['cy'] * cc + c['crv'] * e + half) >> 14, 0, top)
    g = np.clip((c['cy'] * cc - c['cgu'] * d - c['cgv'] * e + half) >> 14, 0, top)
    b = np.clip((c['cy'] * cc + c['cbu'] * d + half) >> 14, 0, top)
    return np.stack([r, g, b], axis=-1)


def encode(rgb, fmt, c):
    """RGB codes [N,H,W,3] -> [N, frame_bytes] uint8: luma per pixel; chroma from the sums over the block of
    (1 << sub_y) x (1 << sub_x) pixels with the edge replicated, one rounding for the average and the matrix."""
    depth, sx, sy = FORMATS[fmt]
    top, mid = (1 << depth) - 1, 1 << (depth - 1)
    rgb = np.asarray(rgb).astype(np.int64)
    n, h, w, _ = rgb.shape
    ch, cw = (h + sy) >> sy, (w + sx) >> sx
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = np.clip(c['yoff'] + ((c['kry'] * r + c['kgy'] * g + c['kby'] * b + (1 << 13)) >> 14), 0, top)
    s = np.zeros((n, ch, cw, 3), dtype=np.int64)
    for a in range(1 << sy):
        rows = np.minimum((np.arange(ch) << sy) + a, h - 1)
        for bb in range(1 << sx):
            cols = np.minimum((np.arange(cw) << sx) + bb, w - 1)
            s += rgb[:, rows][:, :, cols]
    shift = 14 + sx + sy
    u = np.clip(mid + ((c['kru'] * s[..., 0] + c['kgu'] * s[..., 1] + c['kbu'] * s[..., 2] + (1 << (shift - 1))) >> shift), 0, top)
    v = np.clip(mid + ((c['krv'] * s[..., 0] + c['kgv'] * s[..., 1] + c['kbv'] * s[..., 2] + (1 << (shift - 1))) >> shift), 0, top)
    return to_bytes(np.concatenate([y.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], axis=1), fmt)


def accumulator_bound(c, depth, sx, sy):
    """The largest magnitude any accumulator of the two kernels can take with these coefficients: samples and codes in
    [0, max], sums over the chroma block, the rounding constants included."""
    top, mid = (1 << depth) - 1, 1 << (depth - 1)
    block = (1 << sx) * (1 << sy)
    luma = max(abs(c['cy'] * (top - c['yoff'])), abs(c['cy'] * c['yoff']))
    dmax = max(mid, top - mid)
    dec = luma + max(abs(c['crv']), abs(c['cbu']), abs(c['cgu']) + abs(c['cgv'])) * dmax + (1 << 13)
    enc_y = (abs(c['kry']) + abs(c['kgy']) + abs(c['kby'])) * top + (1 << 13)
    enc_c = max(sum(abs(c[n]) for n in k) for k in (('kru', 'kgu', 'kbu'), ('krv', 'kgv', 'kbv'))) * top * block + (1 << (13 + sx + sy))
    return max(dec, enc_y, enc_c)


# ---- the float encode ---------------------------------------------------------------------------------------------------------
def lut_ref(depth):
    """The host route's decode of every code at the depth: float64 arithmetic, one cast (depth 8: `/ 127.5 - 1.0`)."""
    return (np.arange(1 << depth) / (((1 << depth) - 1) / 2.0) - 1.0).astype(np.float32)


def encode_unit_bits(y, top):
    """encode_unit_bits step by step in float32: `* 0.5`, `+ 0.5`, clamp to [0, 1] (a NaN becomes 0, as fmaxf drops it),
    `* max`, `+ 0.5`, truncation."""
    with np.errstate(over='ignore', invalid='ignore'):
        t = np.asarray(y, dtype=np.float32) * F(0.5)
        t = t + F(0.5)
        t = np.fmin(np.fmax(t, F(0.0)), F(1.0))
        t = t * F(top)
        t = t + F(0.5)
    assert t.dtype == np.float32
    return t.astype(np.int64)


@functools.lru_cache(maxsize=None)
def crafted_set(depth):
    """For every code k of the depth the first float that encodes to k with its +-3-ulp neighbours (k = 0: -1 and its
    neighbours) -- at depth 12 a stride of 37 through the codes plus both ends, to keep the set small -- then +-0, +-inf, NaN,
    subnormals and values beyond [-1, 1].  Read-only."""
    top = (1 << depth) - 1
    codes = range(top + 1) if depth < 12 else sorted(set(range(0, top + 1, 37)) | {1, 2, top - 1, top})
    vals = []
    for k in codes:
        if k == 0:
            vals += _steps(F(-1.0), 3)
            continue
        lo, hi = _key(F(-2.0)), _key(F(2.0))                              # bisection over the floats in order
        while hi - lo > 1:
            m = (lo + hi) // 2
            if encode_unit_bits(_float(m), top) >= k:
                hi = m
            else:
                lo = m
        y = _float(hi)
        assert encode_unit_bits(y, top) == k and encode_unit_bits(np.nextafter(y, F(-np.inf)), top) == k - 1, k
        vals += _steps(y, 3)
    vals += _steps(F(1.0), 3)
    vals += [F(0.0), F(-0.0), F(np.inf), F(-np.inf), F(np.nan), F(1.5), F(-1.5), F(2.0), F(-2.0), F(4095.0), F(-4095.0), F(1e30), F(-1e30),
             F(3.4e38), F(-3.4e38), F(1e-45), F(-1e-45), F(1e-38), F(-1e-38), F(0.999999), F(-0.999999)]
    a = np.array(vals, dtype=np.float32)
    a.setflags(write=False)
    return a


def crafted_values(depth, n, start=0):
    """n values of the depth's crafted set from position start on, wrapping round."""
    return np.take(crafted_set(depth), np.arange(start, start + n), mode='wrap')


# ---- frames -------------------------------------------------------------------------------------------------------------------
def special_samples(fmt, full_range=False):
    """0, yoff - 1, yoff, mid, 235 s, 240 s and max (s = 2^(depth - 8)); in a 16-bit container also 0xFFFF and max + 1."""
    depth = FORMATS[fmt][0]
    s, top = 1 << (depth - 8), (1 << depth) - 1
    yoff = 16 * s
    vals = [0, yoff - 1, yoff, 1 << (depth - 1), 235 * s, 240 * s, top]
    if depth > 8:
        vals += [0xFFFF, top + 1]
    return np.array(vals, dtype=np.int64)


def plane_bytes(n, h, w, fmt, seed=0):
    """[n, frame_bytes] uint8: random legal samples with the special ones in every plane that has room for them (smaller planes
    take the first few, rotated by frame and plane, so that over the n frames every plane position meets several)."""
    depth = FORMATS[fmt][0]
    rng = np.random.default_rng(seed * 7919 + h * 131 + w + depth)
    samples = rng.integers(0, 1 << depth, (n, frame_samples(h, w, fmt)), dtype=np.int64)
    special = special_samples(fmt)
    for k in range(n):
        for p, plane in enumerate(split(samples[k:k + 1], h, w, fmt)):
            flat = plane.reshape(-1)                                     # (a view: the planes are contiguous pieces of a row)
            m = min(flat.size, special.size)
            at = rng.permutation(flat.size)[:m]
            flat[at] = np.roll(special, k + 2 * p)[:m]
    return to_bytes(samples, fmt)


def y4m_stream(frames, h, w, fmt, tags=None, frame_params=''):
    """The bytes of a Y4M stream of the format, with its colour tag unless `tags` gives the header tags, and frames
    [N, frame_bytes]."""
    return Y.y4m_stream(frames, h, w, tags=('F30:1', 'Ip', 'A1:1', Y4M_TAGS[fmt]) if tags is None else tags, frame_params=frame_params)
