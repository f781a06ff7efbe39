"""NumPy restatement of the planar YUV 4:2:0 arithmetic (csrc/espcn_yuv.hip, include/srx.h) and Y4M streams built in memory.
Shared by tests/test_espcn_yuv_host.py and tests/test_gpu_espcn_yuv.py.  Everything is int64 here: no accumulator can wrap."""
import math

import numpy as np

NAMES = ('yoff', 'cy', 'crv', 'cgu', 'cgv', 'cbu', 'kry', 'kgy', 'kby', 'kru', 'kgu', 'kbu', 'krv', 'kgv', 'kbv')
MATRICES = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}
COMBOS = [(m, f) for m in ('bt601', 'bt709') for f in (False, True)]
# the issue's pins, bt601 limited
PINS = dict(yoff=16, cy=19077, crv=26149, cgu=6419, cgv=13320, cbu=33050, kry=4207, kgy=8260, kby=1604,
            kru=-2428, kgu=-4768, kbu=7196, krv=7196, kgv=-6026, kbv=-1170)
# (R, G, B) -> (Y, U, V), bt601 limited
KNOWN = [((255, 0, 0), (81, 90, 240)), ((0, 255, 0), (145, 54, 34)), ((0, 0, 255), (41, 240, 110)),
         ((255, 255, 255), (235, 128, 128)), ((0, 0, 0), (16, 128, 128))]


def coeffs(matrix, full_range):
    """{name: int}: floor(v * 16384 + 0.5) of the real values in double, from (Kr, Kb) and the range."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    real = dict(cy=1.0 / ys, crv=2.0 * (1.0 - kr) / cs, cgu=2.0 * (1.0 - kb) * kb / kg / cs, cgv=2.0 * (1.0 - kr) * kr / kg / cs,
                cbu=2.0 * (1.0 - kb) / cs, kry=kr * ys, kgy=kg * ys, kby=kb * ys,
                kru=-kr / (2.0 * (1.0 - kb)) * cs, kgu=-kg / (2.0 * (1.0 - kb)) * cs, kbu=0.5 * cs,
                krv=0.5 * cs, kgv=-kg / (2.0 * (1.0 - kr)) * cs, kbv=-kb / (2.0 * (1.0 - kr)) * cs)
    out = {k: int(math.floor(v * 16384.0 + 0.5)) for k, v in real.items()}
    out['yoff'] = 0 if full_range else 16
    return out


def of_struct(c):
    """{name: int} of a _lib.Yuv420Coeffs."""
    return {k: int(getattr(c, k)) for k in NAMES}


def frame_bytes(h, w):
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def split(frames, h, w):
    """[N, frame_bytes] -> Y [N,H,W], U, V [N,CH,CW] (views)."""
    frames = np.asarray(frames).reshape(-1, frame_bytes(h, w))
    ch, cw = (h + 1) // 2, (w + 1) // 2
    n = frames.shape[0]
    return (frames[:, :h * w].reshape(n, h, w), frames[:, h * w:h * w + ch * cw].reshape(n, ch, cw),
            frames[:, h * w + ch * cw:].reshape(n, ch, cw))


def clip8(v):
    return np.clip(v, 0, 255)


def decode(frames, h, w, c):
    """[N, frame_bytes] uint8 -> RGB bytes [N,H,W,3]: pixel (y, x) takes the chroma sample (y >> 1, x >> 1)."""
    y, u, v = split(frames, h, w)
    rows, cols = np.arange(h) >> 1, np.arange(w) >> 1
    cc = y.astype(np.int64) - c['yoff']
    d = u.astype(np.int64)[:, rows][:, :, cols] - 128
    e = v.astype(np.int64)[:, rows][:, :, cols] - 128
    half = 1 << 13
    r = clip8((c['cy'] * cc + c['crv'] * e + half) >> 14)
    g = clip8((c['cy'] * cc - c['cgu'] * d - c['cgv'] * e + half) >> 14)
    b = clip8((c['cy'] * cc + c['cbu'] * d + half) >> 14)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def encode(rgb, c):
    """RGB bytes [N,H,W,3] -> [N, frame_bytes] uint8: luma per pixel; chroma from the sums over the 2 x 2 block with the
    edge replicated, one rounding for the average and the matrix."""
    rgb = np.asarray(rgb).astype(np.int64)
    n, h, w, _ = rgb.shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = clip8(c['yoff'] + ((c['kry'] * r + c['kgy'] * g + c['kby'] * b + (1 << 13)) >> 14))
    s = np.zeros((n, ch, cw, 3), dtype=np.int64)
    for a in (0, 1):
        rows = np.minimum(2 * np.arange(ch) + a, h - 1)
        for bb in (0, 1):
            cols = np.minimum(2 * np.arange(cw) + bb, w - 1)
            s += rgb[:, rows][:, :, cols]
    u = clip8(128 + ((c['kru'] * s[..., 0] + c['kgu'] * s[..., 1] + c['kbu'] * s[..., 2] + (1 << 15)) >> 16))
    v = clip8(128 + ((c['krv'] * s[..., 0] + c['kgv'] * s[..., 1] + c['kbv'] * s[..., 2] + (1 << 15)) >> 16))
    return np.concatenate([y.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], axis=1).astype(np.uint8)


SPECIAL = np.array([0, 16, 128, 235, 240, 255], dtype=np.uint8)


def plane_bytes(n, h, w, seed=0):
    """[n, frame_bytes] uint8, random, with 0, 16, 128, 235, 240 and 255 in every plane that has room for them (smaller planes
    take the first few, rotated by frame and plane, so that over the n frames every plane position meets several)."""
    rng = np.random.default_rng(seed * 7919 + h * 131 + w)
    frames = rng.integers(0, 256, (n, frame_bytes(h, w)), dtype=np.uint8)
    for k in range(n):
        for p, plane in enumerate(split(frames[k:k + 1], h, w)):
            flat = plane.reshape(-1)
            m = min(flat.size, SPECIAL.size)
            at = rng.permutation(flat.size)[:m]
            flat[at] = np.roll(SPECIAL, k + 2 * p)[:m]
    return frames


def y4m_stream(frames, h, w, tags=('F30:1', 'Ip', 'A1:1', 'C420jpeg'), frame_params=''):
    """The bytes of a Y4M stream with the given header tags and frames ([N, frame_bytes])."""
    head = ' '.join(['YUV4MPEG2', 'W%d' % w, 'H%d' % h] + list(tags)).encode() + b'\n'
    body = b''.join(b'FRAME' + frame_params.encode() + b'\n' + np.asarray(f, dtype=np.uint8).tobytes() for f in frames)
    return head + body
