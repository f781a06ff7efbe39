"""Host-side checks of the planar YUV formats beyond 8-bit 4:2:0 (no GPU): srx_yuv_coeffs against srx_yuv420_coeffs, the pinned
integers and the restatement's formulas, the accumulator bound, the restatement's known answers, round trip and code identity,
srx_yuv_frame_bytes, the refusals of the entry points, the Y4M reader and writer with the wide set of colour tags, route_plan
and the arguments of FrameResolver(layout='yuv')."""
import ctypes
import io
import itertools

import numpy as np
import pytest

from tests import yuv420_ref as Y
from tests import yuv_planar_ref as P


# ---- coefficients -------------------------------------------------------------------------------------------------------------
def test_coeffs_at_depth_8_are_the_420_coeffs_and_the_pins_hold():
    from ml_super_resolution_amd import _lib, ops
    for matrix, full in P.COMBOS:
        a, b = ops.yuv_coeffs(matrix, full, 8), ops.yuv420_coeffs(matrix, full)
        for name, _ in _lib.Yuv420Coeffs._fields_:
            assert getattr(a, name) == getattr(b, name), (matrix, full, name)
    c = ops.yuv_coeffs('bt709', False, 10)
    assert P.of_struct(c) == P.PINS_709_10 and c.reserved == 0
    for matrix, full in P.COMBOS:
        for depth in P.DEPTHS:
            assert P.of_struct(ops.yuv_coeffs(matrix, full, depth)) == P.coeffs(matrix, full, depth), (matrix, full, depth)
    with pytest.raises(ValueError, match='bt2020'):
        ops.yuv_coeffs('bt2020')
    with pytest.raises(ValueError, match='depth must be 8, 10 or 12'):
        ops.yuv_coeffs('bt601', False, 9)
    L = _lib.lib()
    assert L.srx_yuv_coeffs(0, 0, 10, None) == -1 and b'null' in L.srx_last_error()
    assert L.srx_yuv_coeffs(2, 0, 10, ctypes.byref(_lib.Yuv420Coeffs())) == -1 and b'matrix 2' in L.srx_last_error()
    for depth in (0, 9, 14, 16):
        assert L.srx_yuv_coeffs(0, 0, depth, ctypes.byref(_lib.Yuv420Coeffs())) == -1 and b'depth %d' % depth in L.srx_last_error()


@pytest.mark.parametrize('matrix,full', P.COMBOS)
@pytest.mark.parametrize('depth', P.DEPTHS)
def test_accumulators_stay_below_2_to_the_28(matrix, full, depth):
    """int32 is safe with room to spare: the worst case of every sum of both kernels, from the library's own coefficients."""
    from ml_super_resolution_amd import ops
    c = P.of_struct(ops.yuv_coeffs(matrix, full, depth))
    for sx, sy in P.SAMPLINGS:
        assert P.accumulator_bound(c, depth, sx, sy) < 1 << 28, (sx, sy)
    # and the corner inputs themselves, evaluated: every plane at 0 and max, every code at 0 and max, 2 x 2 sums
    top, mid = (1 << depth) - 1, 1 << (depth - 1)
    worst = 0
    for yv, uv, vv in itertools.product((0, top), repeat=3):
        cc, d, e = c['cy'] * (yv - c['yoff']), uv - mid, vv - mid
        worst = max(worst, *(abs(v + (1 << 13)) for v in (cc + c['crv'] * e, cc - c['cgu'] * d - c['cgv'] * e, cc + c['cbu'] * d)))
    for r, g, b in itertools.product((0, 4 * top), repeat=3):
        worst = max(worst, abs(c['kru'] * r + c['kgu'] * g + c['kbu'] * b + (1 << 15)), abs(c['krv'] * r + c['kgv'] * g + c['kbv'] * b + (1 << 15)))
    assert worst < 1 << 28
    if (matrix, full, depth) == ('bt709', False, 12):
        assert worst == 144620164                                        # the largest of all twelve combinations: the decode


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', sorted(P.FORMATS))
def test_known_answers(fmt):
    from ml_super_resolution_amd import ops
    depth, sx, sy = P.FORMATS[fmt]
    s, top, mid = 1 << (depth - 8), (1 << depth) - 1, 1 << (depth - 1)
    bh, bw = 1 << sy, 1 << sx

    def one_block(rgb, c):
        frames = P.encode(np.tile(np.array(rgb, dtype=np.int64), (1, bh, bw, 1)), fmt, c)
        return P.to_samples(frames, bh, bw, fmt)[0].tolist()

    for matrix in ('bt601', 'bt709'):
        limited, full = (P.of_struct(ops.yuv_coeffs(matrix, f, depth)) for f in (False, True))      # the library's integers
        assert one_block((top, top, top), limited) == [235 * s] * (bh * bw) + [mid, mid]
        assert one_block((0, 0, 0), limited) == [16 * s] * (bh * bw) + [mid, mid]
        assert one_block((top, top, top), full) == [top] * (bh * bw) + [mid, mid]
        assert one_block((0, 0, 0), full) == [0] * (bh * bw) + [mid, mid]
    if depth == 10:
        c = P.of_struct(ops.yuv_coeffs('bt709', False, 10))
        for rgb, yuv in P.KNOWN_709_10:
            assert one_block(rgb, c) == [yuv[0]] * (bh * bw) + [yuv[1], yuv[2]], rgb
    if depth == 8:
        c = P.of_struct(ops.yuv_coeffs('bt601', False, 8))
        for rgb, yuv in Y.KNOWN:
            assert one_block(rgb, c) == [yuv[0]] * (bh * bw) + [yuv[1], yuv[2]], rgb
    # odd sizes: the edge is replicated, white and black come back exactly
    c = P.coeffs('bt601', False, depth)
    for v in (0, top):
        block = np.full((1, 3, 5, 3), v, dtype=np.int64)
        frames = P.encode(block, fmt, c)
        assert frames.shape == (1, P.frame_bytes(3, 5, fmt)) and frames.dtype == np.uint8
        np.testing.assert_array_equal(P.decode(frames, 3, 5, fmt, c), block)


def test_the_restatement_at_yuv420p_is_the_420_restatement():
    frames = Y.plane_bytes(3, 5, 7, seed=3)
    rgb = np.random.default_rng(5).integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    for matrix, full in P.COMBOS:
        assert P.coeffs(matrix, full, 8) == Y.coeffs(matrix, full)
        np.testing.assert_array_equal(P.decode(frames, 5, 7, 'yuv420p', P.coeffs(matrix, full, 8)), Y.decode(frames, 5, 7, Y.coeffs(matrix, full)))
        np.testing.assert_array_equal(P.encode(rgb, 'yuv420p', P.coeffs(matrix, full, 8)), Y.encode(rgb, Y.coeffs(matrix, full)))


@pytest.mark.parametrize('matrix,full', P.COMBOS)
@pytest.mark.parametrize('depth', P.DEPTHS)
def test_constant_colour_round_trip_within_two(matrix, full, depth):
    c = P.coeffs(matrix, full, depth)
    top = (1 << depth) - 1
    colours = np.random.default_rng(11 + depth).integers(0, top + 1, (20000, 1, 1, 3), dtype=np.int64)
    colours[:8, 0, 0] = [[r, g, b] for r in (0, top) for g in (0, top) for b in (0, top)]
    fmt = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le'}[depth]
    blocks = np.tile(colours, (1, 2, 2, 1))
    back = P.decode(P.encode(blocks, fmt, c), 2, 2, fmt, c)
    assert np.abs(back - blocks).max() <= (1 if full else 2)


@pytest.mark.parametrize('depth', P.DEPTHS)
def test_every_code_of_the_table_encodes_to_itself(depth):
    from ml_super_resolution_amd import ops
    top = (1 << depth) - 1
    table = ops.unit_lut('cpu', depth).numpy()
    assert table.shape == (top + 1,) and table.dtype == np.float32 and table.tobytes() == P.lut_ref(depth).tobytes()
    np.testing.assert_array_equal(P.encode_unit_bits(table, top), np.arange(top + 1))
    if depth == 8:
        from tests import espcn_frames_ref as R
        assert ops.unit_lut('cpu').numpy().tobytes() == R.lut_ref().tobytes()
        s = P.crafted_set(8)
        np.testing.assert_array_equal(P.encode_unit_bits(s[~np.isnan(s)], 255), R.encode_unit_u8(s[~np.isnan(s)]))
    with pytest.raises(ValueError, match='depth must be'):
        ops.unit_lut('cpu', 16)


def test_crafted_sets_meet_every_code_and_the_odd_values():
    for depth in P.DEPTHS:
        s, top = P.crafted_set(depth), (1 << depth) - 1
        codes = set(P.encode_unit_bits(s, top).tolist())
        # (the neighbours below the first float of a code encode to the code before it)
        assert {0, 1, top - 1, top} <= codes and set(range(0, top + 1, 1 if depth < 12 else 37)) <= codes
        assert np.isnan(s).any() and np.isinf(s).any() and not s.flags.writeable
        assert P.encode_unit_bits(np.array([np.nan, -np.inf, np.inf, -0.0], dtype=np.float32), top).tolist() == [0, 0, top, top // 2 + 1]
    assert P.crafted_set(12).size < 1000


# ---- frame sizes ----------------------------------------------------------------------------------------------------------------
def test_frame_bytes_of_all_nine_formats():
    from ml_super_resolution_amd import _lib, ops
    assert sorted(_lib.PIXEL_FORMATS) == sorted(P.FORMATS) and len(_lib.PIXEL_FORMATS) == 9
    assert _lib.PIXEL_FORMATS == P.FORMATS and ctypes.sizeof(_lib.YuvFormat) == 16
    for fmt in P.FORMATS:
        for h, w in ((1, 1), (3, 5), (4, 6), (135, 240)):
            assert ops.yuv_frame_bytes(h, w, fmt) == P.frame_bytes(h, w, fmt), (fmt, h, w)
    for h, w in ((1, 1), (3, 5), (4, 6), (135, 240)):
        assert ops.yuv_frame_bytes(h, w, 'yuv420p') == ops.yuv420_frame_bytes(h, w)
    assert ops.yuv_frame_bytes(4, 6, 'yuv444p') == ops.yuv_frame_bytes(4, 6, 'yuv420p10le') == 72
    with pytest.raises(ValueError, match='pixel_format must be one of .*yuv444p12le.*nv12'):
        ops.yuv_frame_bytes(4, 6, 'nv12')
    with pytest.raises(ValueError, match='yuv422p frames of 0 x 6: non-positive'):
        ops.yuv_frame_bytes(0, 6, 'yuv422p')
    L = _lib.lib()

    def size(depth=8, sx=1, sy=1, reserved=0, h=4, w=6):
        return L.srx_yuv_frame_bytes(ctypes.byref(_lib.YuvFormat(depth, sx, sy, reserved)), h, w)

    assert size() == 36 and size(12, 0, 0) == 144
    assert L.srx_yuv_frame_bytes(None, 4, 6) == 0 and b'null' in L.srx_last_error()
    for kw, message in (({'depth': 9}, b'depth 9'), ({'depth': 16}, b'depth 16'), ({'sx': 0, 'sy': 1}, b'subsampling (0, 1)'),
                        ({'sx': 2, 'sy': 0}, b'subsampling (2, 0)'), ({'reserved': 1}, b'reserved'), ({'h': 0}, b'dimension'), ({'w': -3}, b'dimension')):
        assert size(**kw) == 0 and message in L.srx_last_error(), kw
    # the largest sizes an int can name: the count fits 64 bits at 8-bit 4:2:0 and does not at 16-bit 4:4:4
    big = (1 << 31) - 1
    assert size(8, 1, 1, h=big, w=big) == big * big + 2 * (1 << 30) * (1 << 30)
    assert size(12, 0, 0, h=big, w=big) == 0 and b'does not fit' in L.srx_last_error()


# ---- the entry points' refusals -------------------------------------------------------------------------------------------------
def test_entry_points_refuse_without_gpu():
    from ml_super_resolution_amd import _lib, ops
    L = _lib.lib()
    p = ctypes.c_void_p(4096)                        # never dereferenced: every call below is refused before a launch
    c = ctypes.byref(ops.yuv_coeffs('bt601', False, 10))
    f10 = ctypes.byref(_lib.YuvFormat(10, 1, 0, 0))

    def dec(yuv=p, N=1, H=4, W=4, f=f10, c=c, lut=p, out=p):
        return L.srx_yuv_lut_float(yuv, N, H, W, f, c, lut, out, None)

    def enc(x=p, N=1, H=4, W=4, f=f10, c=c, yuv=p):
        return L.srx_unit_yuv(x, N, H, W, f, c, yuv, None)

    for kw in ({'yuv': None}, {'lut': None}, {'out': None}, {'c': None}, {'f': None}):
        assert dec(**kw) == -1 and b'null' in L.srx_last_error(), kw
    for kw in ({'x': None}, {'yuv': None}, {'c': None}, {'f': None}):
        assert enc(**kw) == -1 and b'null' in L.srx_last_error(), kw
    for call, who in ((dec, b'yuv_lut_float'), (enc, b'unit_yuv')):
        for kw in ({'N': 0}, {'H': 0}, {'W': -1}):
            assert call(**kw) == -1 and b'dimension' in L.srx_last_error(), kw
        for fmt, message in (((9, 1, 1, 0), b'depth 9 '), ((14, 0, 0, 0), b'depth 14 '), ((16, 1, 0, 0), b'depth 16 '), ((0, 1, 1, 0), b'depth 0 '),
                             ((8, 0, 1, 0), b'subsampling (0, 1)'), ((10, 2, 2, 0), b'subsampling (2, 2)'), ((10, -1, 0, 0), b'subsampling (-1, 0)'),
                             ((12, 1, 1, 7), b"the format's reserved field must be 0, got 7")):
            assert call(f=ctypes.byref(_lib.YuvFormat(*fmt))) == -1 and who + b': ' + message in L.srx_last_error() + b' ', fmt
        # N H W 3 >= 2^31: 2^15 x 2^15 x 1 x 3, and a product that would wrap 64 bits if taken at once -- in every format
        for fmt in P.FORMATS.values():
            f = ctypes.byref(_lib.YuvFormat(*fmt))
            assert call(f=f, N=1, H=1 << 15, W=1 << 15) != 0 and who + b': frames beyond 32-bit' in L.srx_last_error()
            assert call(f=f, N=(1 << 31) - 1, H=(1 << 31) - 1, W=(1 << 31) - 1) != 0 and b'32-bit' in L.srx_last_error()
        # a 16-bit plane at an odd address; an 8-bit one may start anywhere (that call would launch, so it is not made here)
        for depth in (10, 12):
            f = ctypes.byref(_lib.YuvFormat(depth, 0, 0, 0))
            assert call(f=f, yuv=ctypes.c_void_p(4097)) != 0 and who + b': yuv must be 2-byte aligned at depth %d' % depth in L.srx_last_error()
    assert dec(out=ctypes.c_void_p(4098)) != 0 and b'yuv_lut_float: out must be 4-byte aligned' in L.srx_last_error()
    assert enc(x=ctypes.c_void_p(4098)) != 0 and b'unit_yuv: x must be 4-byte aligned' in L.srx_last_error()
    # (8, 1, 1) is checked here before it is handed over
    f8 = ctypes.byref(_lib.YuvFormat(8, 1, 1, 0))
    assert dec(f=f8, out=ctypes.c_void_p(4098)) != 0 and b'yuv_lut_float: out' in L.srx_last_error()
    assert enc(f=f8, x=ctypes.c_void_p(4098)) != 0 and b'unit_yuv: x' in L.srx_last_error()


# ---- Y4M ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt,tag,size', [('yuv422p', 'C422', 33), ('yuv444p', 'C444', 45), ('yuv420p10le', 'C420p10', 54), ('yuv444p12le', 'C444p12', 90)])
def test_y4m_round_trip_at_an_odd_size(fmt, tag, size):
    from ml_super_resolution_amd.espcn import y4m
    frames = P.plane_bytes(3, 3, 5, fmt, seed=1)                         # 5 wide, 3 high
    tags = ['F25:1', 'Ip', 'A1:1', tag]
    header = y4m.Header(5, 3, tags, formats=y4m.PLANAR_FORMATS)
    assert header.frame_bytes == size == P.frame_bytes(3, 5, fmt) and header.pixel_format == fmt and header.full_range is None
    sink = io.BytesIO()
    writer = y4m.Y4MWriter(sink, header)
    for f in frames:
        writer.write(f)
    assert writer.frames == 3
    assert sink.getvalue() == P.y4m_stream(frames, 3, 5, fmt, tags=tags)
    src = io.BytesIO(sink.getvalue())
    back = y4m.read_header(src, formats=y4m.PLANAR_FORMATS)
    assert (back.width, back.height, back.tags, back.pixel_format) == (5, 3, tags, fmt)
    got = list(y4m.read_frames(src, back))
    assert len(got) == 3 and all(g.dtype == np.uint8 and g.shape == (size,) for g in got)
    np.testing.assert_array_equal(np.stack(got), frames)
    with pytest.raises(ValueError, match='frame 3 .*%d bytes' % size):
        writer.write(np.zeros((size - 1,), dtype=np.uint8))
    # a short last frame is refused by index, size and format
    src = io.BytesIO(sink.getvalue()[:-4])
    back = y4m.read_header(src, formats=y4m.PLANAR_FORMATS)
    with pytest.raises(ValueError, match=r'frame 2 is short: %d of %d bytes \(5 x 3, %s\)' % (size - 4, size, fmt)):
        list(y4m.read_frames(src, back))


def test_y4m_reads_into_the_callers_ring_and_scales_with_its_tags():
    from ml_super_resolution_amd.espcn import y4m
    fmt = 'yuv422p10le'
    frames = P.plane_bytes(5, 4, 6, fmt, seed=2)
    src = io.BytesIO(P.y4m_stream(frames, 4, 6, fmt))
    header = y4m.read_header(src, formats=y4m.PLANAR_FORMATS)
    assert header.pixel_format == fmt and header.frame_bytes == 96
    ring = [np.zeros((header.frame_bytes,), dtype=np.uint8) for _ in range(2)]
    for k, got in enumerate(y4m.read_frames(src, header, buffers=itertools.cycle(ring))):
        assert got is ring[k % 2]
        np.testing.assert_array_equal(got, frames[k])
    assert k == 4
    tags = ('F30000:1001', 'Ip', 'A128:117', 'C444p10', 'XCOLORRANGE=FULL')
    header = y4m.read_header(io.BytesIO(Y.y4m_stream([], 135, 240, tags=tags)), formats=y4m.PLANAR_FORMATS)
    assert header.full_range is True and header.pixel_format == 'yuv444p10le' and header.frame_bytes == 135 * 240 * 6
    out = header.scaled(3)
    assert (out.width, out.height, out.pixel_format) == (720, 405, 'yuv444p10le') and out.tags == list(tags)
    assert out.formats is y4m.PLANAR_FORMATS and out.frame_bytes == 405 * 720 * 6
    assert out.line() == b'YUV4MPEG2 W720 H405 ' + ' '.join(tags).encode() + b'\n'
    # the 8-bit 4:2:0 tags, and none, under the wide set
    for tags in (('C420jpeg',), ('C420mpeg2',), ('C420paldv',), ('C420',), ()):
        header = y4m.read_header(io.BytesIO(Y.y4m_stream([], 3, 5, tags=tags)), formats=y4m.PLANAR_FORMATS)
        assert header.pixel_format == 'yuv420p' and header.frame_bytes == 27
    assert sorted(set(y4m.PLANAR_FORMATS.values())) == sorted(P.FORMATS)
    assert all(y4m.PLANAR_FORMATS[tag] == fmt for fmt, tag in P.Y4M_TAGS.items())


@pytest.mark.parametrize('tag,message', [('C422', 'colour tag C422: only 4:2:0 is taken'), ('C444', 'colour tag C444: only 4:2:0 is taken'),
                                         ('C420p10', 'colour tag C420p10: a bit depth of 10, only 8-bit samples are taken'),
                                         ('C422p12', 'colour tag C422p12: a bit depth of 12, only 8-bit samples are taken')])
def test_y4m_default_set_still_refuses(tag, message):
    from ml_super_resolution_amd.espcn import y4m
    stream = Y.y4m_stream([], 4, 4, tags=('F25:1', tag))
    with pytest.raises(ValueError, match=message):
        y4m.read_header(io.BytesIO(stream))
    with pytest.raises(ValueError, match=message):
        y4m.Header(4, 4, ['F25:1', tag])
    assert y4m.read_header(io.BytesIO(stream), formats=y4m.PLANAR_FORMATS).pixel_format == y4m.PLANAR_FORMATS[tag]
    assert y4m.read_header(io.BytesIO(Y.y4m_stream([], 4, 4))).pixel_format == 'yuv420p'


@pytest.mark.parametrize('tag,message', [('Cmono', 'colour tag Cmono: only planar'), ('Cmono16', 'colour tag Cmono16: only planar'),
                                         ('C411', 'colour tag C411: only planar'), ('C440', 'colour tag C440: only planar'),
                                         ('C444alpha', 'colour tag C444alpha: only planar'), ('C420p9', 'colour tag C420p9: a bit depth of 9'),
                                         ('C422p14', 'colour tag C422p14: a bit depth of 14'), ('C444p16', 'colour tag C444p16: a bit depth of 16'),
                                         ('It', 'interlace tag It'), ('Ib', 'interlace tag Ib'), ('Im', 'interlace tag Im')])
def test_y4m_wide_set_refuses_by_tag(tag, message):
    from ml_super_resolution_amd.espcn import y4m
    with pytest.raises(ValueError, match=message):
        y4m.read_header(io.BytesIO(Y.y4m_stream([], 4, 4, tags=('F25:1', tag))), formats=y4m.PLANAR_FORMATS)


# ---- route_plan and FrameResolver -------------------------------------------------------------------------------------------------
def test_route_plan_keys_by_format_and_leaves_the_old_routes():
    from ml_super_resolution_amd.espcn.model_espcn import RoutePlan, route_plan
    lr, t1, t2, hr = (2, 4, 6, 3), (2, 4, 6, 64), (2, 4, 6, 32), (2, 12, 18, 3)
    # what the three routes returned before 'yuv' existed, written out
    assert route_plan('float', 2, 4, 6, 3) == RoutePlan(lr, (t1, t2), hr, 'float32', (('sr', 0), ('sr', 1)), ('sr', 2))
    assert route_plan('u8', 2, 4, 6, 3) == RoutePlan(('u8',) + lr, (lr, t1, t2, hr), hr, 'uint8', (('sr8', 0), ('sr', 0), ('sr', 1), ('sr', 2)), 'sr5')
    assert route_plan('yuv420', 2, 4, 6, 3, True, 'bt709', True) == RoutePlan(
        ('yuv420', 2, 4, 6, 'bt709', True, True), (lr, None, None, hr), (2, Y.frame_bytes(12, 18)), 'uint8',
        (('sry', 0), ('sr', 0), ('sr', 1), ('sry', 1)), 'sry')
    plans = {fmt: route_plan('yuv', 2, 4, 6, 3, False, 'bt601', False, fmt) for fmt in P.FORMATS}
    assert len({p.key for p in plans.values()}) == 9
    for fmt, p in plans.items():
        assert fmt in p.key and p.floats == (lr, t1, t2, hr) and p.out_shape == (2, P.frame_bytes(12, 18, fmt)) and p.out_dtype == 'uint8'
    # 4 x 6 frames of yuv444p and yuv420p10le are both 72 bytes, at r = 1 times anything: the key tells them apart
    a, b = route_plan('yuv', 1, 4, 6, 2, True, 'bt601', False, 'yuv444p'), route_plan('yuv', 1, 4, 6, 2, True, 'bt601', False, 'yuv420p10le')
    assert a.out_shape == b.out_shape and a.key != b.key and a.floats == ((1, 4, 6, 3), None, None, (1, 8, 12, 3))
    assert plans['yuv420p'].key != route_plan('yuv420', 2, 4, 6, 3).key
    assert route_plan('yuv', 2, 4, 6, 3, False, 'bt709', False, 'yuv422p').key != plans['yuv422p'].key
    with pytest.raises(ValueError, match='route must be'):
        route_plan('nv12', 1, 4, 6, 2)
    with pytest.raises(ValueError, match='pixel_format must be one of'):
        route_plan('yuv', 1, 4, 6, 2, False, 'bt601', False, 'nv12')


class _Model(object):
    scaling_factor = 3


def test_frame_resolver_arguments_without_gpu():
    from ml_super_resolution_amd.espcn import frames
    # refused before anything is allocated
    for kw, message in (({'layout': 'nv12'}, "layout must be 'rgb' or 'yuv420'"), ({'layout': 'yuv'}, "pixel_format goes with layout='yuv'"),
                        ({'layout': 'yuv420', 'pixel_format': 'yuv420p'}, "pixel_format goes with layout='yuv'"),
                        ({'layout': 'rgb', 'pixel_format': 'yuv444p'}, "pixel_format goes with layout='yuv'"),
                        ({'pixel_format': 'yuv444p'}, "pixel_format goes with layout='yuv'"),
                        ({'layout': 'yuv', 'pixel_format': 'nv12'}, 'pixel_format must be one of'),
                        ({'layout': 'yuv', 'pixel_format': 'yuv422p', 'matrix': 'bt2020'}, 'matrix must be'),
                        ({'layout': 'yuv', 'pixel_format': 'yuv422p', 'batch': 0}, 'batch and depth'),
                        ({'layout': 'yuv', 'pixel_format': 'yuv422p', 'depth': 0}, 'batch and depth')):
        with pytest.raises(ValueError, match=message):
            frames.FrameResolver(_Model(), 6, 10, **kw)
    with pytest.raises(ValueError, match='height and width'):
        frames.FrameResolver(_Model(), 0, 10, layout='yuv', pixel_format='yuv420p10le')
