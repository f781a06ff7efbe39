"""CPU-side checks of SRCNN's whole-image pair source: srx_srcnn_eval_footprint (the per-axis reach of a tile, shared by the
host check and the kernel's pixel loops) against a brute-force enumeration of every pixel's taps, srx_srcnn_eval_table_check
(pure host code: the only bound between a table and the kernel's reads and writes), srx_srcnn_eval_tiles, the argument
checks of srx_srcnn_eval_pairs that come before any launch, the record builder, DeviceEvalSet's refusals and the new flags.
The GPU tests are in tests/test_gpu_srcnn_eval.py."""
import ctypes
import functools

import numpy as np
import pytest

from tests import eval_tables

BAD_ARG = -1          # SRX_ERR_BAD_ARG
T = 32                # SRX_SRCNN_EVAL_TILE
SHAPES = ((13, 14), (23, 70), (33, 32), (64, 97), (65, 31), (100, 47), (130, 129))      # decoded (height, width)
F, BORDER = 3, 6
f32 = np.float32


def literal_table(shapes, border=BORDER):
    """The records of every shape over ONE arena that holds each once, with plain Python sums: (records, arena_bytes,
    (out_floats, crop_floats), tiles)."""
    from ml_super_resolution_amd import ops
    rows, at, out, crop, tiles, out_end, crop_end = [], 0, 0, 0, 0, 0, 0
    for h, w in shapes:
        rows.append((at, w, h, out, crop, tiles, 0))
        at += 3 * h * w
        out_end, crop_end = out + 3 * h * w, crop + 3 * (h - 2 * border) * (w - 2 * border)
        out, crop = (out_end + 3) // 4 * 4, (crop_end + 3) // 4 * 4
        tiles += len(range(0, h, T)) * len(range(0, w, T))
    return np.array(rows, ops.SRCNN_EVAL_IMAGE_DTYPE), at, (out_end, crop_end), tiles


def run_check(rec, arena_bytes, floats, n=None, f=F, border=BORDER):
    return eval_tables.run_check('srx_srcnn_eval_table_check', rec, f, border, arena_bytes, floats[0], floats[1], n=n)


# ---- the footprint ----------------------------------------------------------------------------------------------------
def _taps(o, n_in, n_out):
    """The four clamped tap indices of outputs `o` (int array) of a resize from n_in to n_out pixels, in float32: the
    expression of tap_positions in tests/test_gpu_srcnn_pairs.py (scale = n_in / n_out, lower = floor(o * scale))."""
    scale = f32(n_in) / f32(n_out)
    lower = np.floor(o.astype(f32) * scale).astype(np.int64)
    return np.clip(lower[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)


def _brute_force(side, f, tile):
    """Every output pixel of the tile through both passes: (lo, source) index sets' (min, max)."""
    L = side // f
    o = np.arange(tile * T, min(tile * T + T, side))
    lo = np.unique(_taps(o, L, side))
    src = np.unique(_taps(lo, side, L))
    return (lo.min(), lo.max()), (src.min(), src.max())


@pytest.mark.parametrize('f', (2, 3, 4, 8))
def test_footprint_against_brute_force(f):
    """Sides 5 .. 130 and 243, 256, 1000, every tile: the function's two ranges ARE the enumerated ones (the ends of a run
    bracket its taps exactly, since floor(o * scale) does not decrease)."""
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int * 4)()
    seen = 0
    for side in list(range(5, 131)) + [243, 256, 1000]:
        tiles = -(-side // T)
        if side // f < 1:
            assert L.srx_srcnn_eval_footprint(side, f, 0, out) == BAD_ARG and b'no low-resolution pixel' in L.srx_last_error()
            continue
        for tile in range(tiles):
            assert L.srx_srcnn_eval_footprint(side, f, tile, out) == 0, L.srx_last_error()
            got = list(out)
            (lo0, lo1), (s0, s1) = _brute_force(side, f, tile)
            assert got == [lo0, lo1, s0, s1], (side, f, tile, got)
            assert 0 <= got[0] <= got[1] < side // f and 0 <= got[2] <= got[3] < side
            seen += 1
        assert L.srx_srcnn_eval_footprint(side, f, tiles, out) == BAD_ARG and L.srx_srcnn_eval_footprint(side, f, -1, out) == BAD_ARG
    assert seen > 300


def test_footprint_refusals():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int * 4)()
    for args, piece in (((64, 2, 0, None), b'null out'), ((0, 2, 0, out), b'side 0'), ((64, 1, 0, out), b'f 1 outside 2..8'),
                        ((64, 9, 0, out), b'f 9 outside 2..8'), ((3, 4, 0, out), b'no low-resolution pixel'), ((64, 2, 2, out), b'tile 2')):
        assert L.srx_srcnn_eval_footprint(*args) == BAD_ARG, args
        assert b'srcnn_eval_footprint' in L.srx_last_error() and piece in L.srx_last_error(), L.srx_last_error()


# ---- the check --------------------------------------------------------------------------------------------------------
def test_the_sizes_reach_every_branch():
    """What the seven sizes are for, at T = 32 and border 6: 13 is one pixel inside the margin and below a tile; sides of T,
    T - 1, T + 1, 2 T, 2 T + 1; ragged last tiles on both axes; sides that are multiples of 3 and sides that are not, on
    each axis; records whose floats are no multiple of 4, in sd and in the crops."""
    assert T == 32
    heights, widths = {h for h, _ in SHAPES}, {w for _, w in SHAPES}
    assert {T - 1, T, T + 1, 2 * T, 2 * T + 1} <= heights | widths and min(heights | widths) == 2 * BORDER + 1
    assert any(h % T for h in heights) and any(w % T for w in widths)
    for sides in (heights, widths):
        assert any(s % F == 0 for s in sides) and any(s % F for s in sides)
    assert any((3 * h * w) % 4 for h, w in SHAPES) and any((3 * (h - 12) * (w - 12)) % 4 for h, w in SHAPES)


def test_check_accepts_the_records_of_ops():
    """The last image ends on the arena's last byte; the records of ops.srcnn_eval_records are the literal sums."""
    from ml_super_resolution_amd import ops
    rec, arena_bytes, floats, tiles = literal_table(SHAPES)
    got = ops.srcnn_eval_records(rec['height'], rec['width'], rec['offset'], F, BORDER)
    assert got.dtype == ops.SRCNN_EVAL_IMAGE_DTYPE and got.dtype.itemsize == 40 and np.array_equal(got, rec)
    assert (rec['out_offset'] % 4 == 0).all() and (rec['crop_offset'] % 4 == 0).all()
    assert ((rec['out_offset'][1:] - rec['out_offset'][:-1]) != 3 * rec['height'][:-1] * rec['width'][:-1]).any()
    for f in (2, 3, 4, 8):
        rc, msg = run_check(rec, arena_bytes, floats, f=f)
        assert rc == 0, msg
    rc, msg = run_check(rec[:1], arena_bytes, (3 * 13 * 14, 3 * 1 * 2))
    assert rc == 0, msg
    for border in (0, 1):
        other, ab, fl, _ = literal_table(SHAPES + ((14, 13), (2, 3)) if border == 0 else SHAPES, border)
        assert run_check(other, ab, fl, f=2, border=border)[0] == 0
        assert np.array_equal(ops.srcnn_eval_records(other['height'], other['width'], other['offset'], 2, border), other)
    wide, ab, fl, _ = literal_table(((40, 1100), (1000, 17)), 0)             # the ends of the factor range on long sides
    for f in (2, 8):
        assert run_check(wide, ab, fl, f=f, border=0)[0] == 0


_edited = functools.partial(eval_tables._edited, lambda: literal_table(SHAPES))


# (name, (records, arena_bytes, floats), keyword arguments, the entry named, a piece of the message)
def _bad_cases():
    rec, ab, fl, _ = literal_table(SHAPES)
    last = len(rec) - 1
    return [
        ('width 0', _edited('width', 2, 0), {}, 2, 'each side must be in 1..'),
        ('negative height', _edited('height', 4, -3), {}, 4, 'each side must be in 1..'),
        ('a side inside the border', _edited('height', 1, 12), {}, 1, 'nothing inside a border of 6'),
        ('an image one byte past the arena', (rec, ab - 1, fl), {}, last, 'leaves the arena'),
        ('an offset one byte too far', _edited('offset', last, rec['offset'][last] + 1), {}, last, 'leaves the arena'),
        ('an offset that wraps', _edited('offset', 1, 2 ** 64 - 1), {}, 1, 'leaves the arena'),
        ('reserved set', _edited('reserved', 3, 1), {}, 3, 'reserved 1 is not 0'),
        ('out_offset one above', _edited('out_offset', 3, rec['out_offset'][3] + 1), {}, 3, 'out_offset'),
        ('out_offset unpadded', _edited('out_offset', 1, 3 * 13 * 14), {}, 1, 'out_offset 546 is not 548'),
        ('out_offset of the first entry', _edited('out_offset', 0, 4), {}, 0, 'out_offset 4 is not 0'),
        ('crop_offset one above', _edited('crop_offset', 2, rec['crop_offset'][2] + 1), {}, 2, 'crop_offset'),
        ('crop_offset unpadded', _edited('crop_offset', 1, 3 * 1 * 2), {}, 1, 'crop_offset 6 is not 8'),
        ('first_tile one above', _edited('first_tile', 2, rec['first_tile'][2] + 1), {}, 2, 'first_tile'),
        ('first_tile one below', _edited('first_tile', last, rec['first_tile'][last] - 1), {}, last, 'first_tile'),
        ('out_floats one short', (rec, ab, (fl[0] - 1, fl[1])), {}, last, "from out_offset %d on are more than the output's" % rec['out_offset'][last]),
        ('crop_floats one short', (rec, ab, (fl[0], fl[1] - 1)), {}, last, "from crop_offset %d on are more than the output's" % rec['crop_offset'][last]),
    ]


BAD = _bad_cases()
# the whole message of every case above, as the build before the walks shared their running sums printed it
MESSAGES = {
    'width 0':
        'srcnn_eval_table_check: entry 2: image of 0 x 33 pixels: each side must be in 1..1073741824',
    'negative height':
        'srcnn_eval_table_check: entry 4: image of 31 x -3 pixels: each side must be in 1..1073741824',
    'a side inside the border':
        'srcnn_eval_table_check: entry 1: image of 70 x 12 pixels has no low-resolution pixel at f 3 or nothing inside a border of 6',
    'an image one byte past the arena':
        'srcnn_eval_table_check: entry 6: image of 50310 bytes at offset 47313 leaves the arena of 97622 bytes',
    'an offset one byte too far':
        'srcnn_eval_table_check: entry 6: image of 50310 bytes at offset 47314 leaves the arena of 97623 bytes',
    'an offset that wraps':
        'srcnn_eval_table_check: entry 1: image of 4830 bytes at offset 18446744073709551615 leaves the arena of 97623 bytes',
    'reserved set':
        'srcnn_eval_table_check: entry 3: reserved 1 is not 0',
    'out_offset one above':
        'srcnn_eval_table_check: entry 3: out_offset 8549 is not 8548, the floats of the entries before it padded to 4',
    'out_offset unpadded':
        'srcnn_eval_table_check: entry 1: out_offset 546 is not 548, the floats of the entries before it padded to 4',
    'out_offset of the first entry':
        'srcnn_eval_table_check: entry 0: out_offset 4 is not 0, the floats of the entries before it padded to 4',
    'crop_offset one above':
        'srcnn_eval_table_check: entry 2: crop_offset 1925 is not 1924, the floats of the entries before it padded to 4',
    'crop_offset unpadded':
        'srcnn_eval_table_check: entry 1: crop_offset 6 is not 8, the floats of the entries before it padded to 4',
    'first_tile one above':
        'srcnn_eval_table_check: entry 2: first_tile 5 is not the 4 tiles of the entries before it',
    'first_tile one below':
        'srcnn_eval_table_check: entry 6: first_tile 24 is not the 25 tiles of the entries before it',
    'out_floats one short':
        "srcnn_eval_table_check: entry 6: 50310 floats from out_offset 47320 on are more than the output's 97629",
    'crop_floats one short':
        "srcnn_eval_table_check: entry 6: 41418 floats from crop_offset 28708 on are more than the output's 70125",
}


@pytest.mark.parametrize('name,args,kwargs,entry,piece', BAD, ids=[b[0] for b in BAD])
def test_check_refuses_and_names_the_entry(name, args, kwargs, entry, piece):
    rc, msg = run_check(*args, **kwargs)
    assert rc == BAD_ARG, (name, msg)
    assert 'srcnn_eval_table_check: entry %d:' % entry in msg and piece in msg, (name, msg)
    assert msg == MESSAGES[name]


def test_check_refuses_a_side_without_a_low_resolution_pixel():
    """(5, 40) at f = 8: 5 // 8 = 0 rows; and at f = 4 it passes."""
    rec, ab, fl, _ = literal_table(((20, 20), (5, 40)), 0)
    assert run_check(rec, ab, fl, f=4, border=0)[0] == 0
    rc, msg = run_check(rec, ab, fl, f=8, border=0)
    assert rc == BAD_ARG and msg == ('srcnn_eval_table_check: entry 1: image of 40 x 5 pixels has no low-resolution pixel at f 8 or nothing inside a '
                                     'border of 0'), msg
    rec, ab, fl, _ = literal_table(((20, 20), (40, 12)), 6)                 # 12 <= 2 * 6
    rc, msg = run_check(rec, ab, fl)
    assert rc == BAD_ARG and msg == ('srcnn_eval_table_check: entry 1: image of 12 x 40 pixels has no low-resolution pixel at f 3 or nothing inside a '
                                     'border of 6'), msg


def test_check_refuses_table_wide_faults():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    rec, arena_bytes, floats, _ = literal_table(SHAPES)
    assert L.srx_srcnn_eval_table_check(None, 1, F, BORDER, arena_bytes, floats[0], floats[1]) == BAD_ARG
    assert L.srx_last_error() == b'srcnn_eval_table_check: null table'
    for n in (0, -1):
        rc, msg = run_check(rec, arena_bytes, floats, n=n)
        assert rc == BAD_ARG and msg == 'srcnn_eval_table_check: n %d below 1' % n, msg
    for f in (1, 0, -2, 9):
        rc, msg = run_check(rec, arena_bytes, floats, f=f)
        assert rc == BAD_ARG and msg == 'srcnn_eval_table_check: f %d outside 2..8' % f, msg
    rc, msg = run_check(rec, arena_bytes, floats, border=-1)
    assert rc == BAD_ARG and msg == 'srcnn_eval_table_check: border -1 is negative', msg
    for grown in ((floats[0] + 1, floats[1]), (floats[0], floats[1] + 1)):   # totals below the outputs' sizes
        rc, msg = run_check(rec, arena_bytes, grown)
        assert floats == (97630, 70126)
        assert rc == BAD_ARG and msg == ("srcnn_eval_table_check: the table's 7 entries end at float 97630 of sd and 70126 of bq and hd, not at "
                                         'out_floats %d and crop_floats %d' % grown), msg


def test_check_refuses_more_tiles_than_a_grid_index_holds():
    """Records of 32768 x 32768 tiles (2^30) each: one passes, two reach 2^31.  The records share their bytes (only outputs
    must not overlap) and the arena is a number: the check reads no image byte."""
    from ml_super_resolution_amd import _lib, ops
    side = T * 32768
    rec = ops.srcnn_eval_records([side] * 3, [side] * 3, [0] * 3, F, BORDER)
    per, crop = 3 * side * side, 3 * (side - 12) * (side - 12)
    assert run_check(rec[:1], per, (per, crop))[0] == 0
    rc, msg = run_check(rec[:2], per, (2 * per, int(rec['crop_offset'][1]) + crop))
    assert rc == BAD_ARG and msg == 'srcnn_eval_table_check: entry 1: 2147483648 tiles up to this entry, above 2147483647', msg
    L = _lib.lib()
    assert L.srx_srcnn_eval_tiles(ctypes.c_void_p(rec.ctypes.data), 1) == 2 ** 30
    assert L.srx_srcnn_eval_tiles(ctypes.c_void_p(rec.ctypes.data), 2) == 0 and b'tiles' in L.srx_last_error()


def test_check_refuses_a_footprint_beyond_the_lds_layout():
    """Past 2^24 pixels a side fp32 no longer holds every pixel index and a tile's ranges widen; at 2^29 x 2^29 and f = 3 a
    tile would need more than the kernel's 40 KiB, and the record is refused for that (before its tiles are counted).
    Every tile row and tile column is walked: one size past the limit is refused for its size."""
    from ml_super_resolution_amd import ops
    side = 2 ** 29
    rec = ops.srcnn_eval_records([side], [side], [0], 3, 0)
    rc, msg = run_check(rec, 3 * side * side, (3 * side * side, 3 * side * side), border=0)
    assert rc == BAD_ARG and msg == ("srcnn_eval_table_check: entry 0: a tile's footprint (68 x 68 source pixels, 20 x 20 low-resolution pixels: 47024 "
                                     'bytes) is beyond the LDS layout of 40960 bytes'), msg
    rec = ops.srcnn_eval_records([side * 2 + 1], [32], [0], 3, 0)
    rc, msg = run_check(rec, 2 ** 62, (2 ** 40, 2 ** 40), border=0)
    assert rc == BAD_ARG and msg == 'srcnn_eval_table_check: entry 0: image of 32 x 1073741825 pixels: each side must be in 1..1073741824', msg


# ---- tile counts ------------------------------------------------------------------------------------------------------
def test_tiles_equal_the_sum():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    shapes = SHAPES + ((T, 2 * T), (T + 1, T), (3 * T, T - 1), (1, 1), (512, 768))
    rec, _, _, tiles = literal_table(shapes, 0)
    want = int((np.ceil(rec['height'] / T) * np.ceil(rec['width'] / T)).sum())
    assert want == tiles
    assert L.srx_srcnn_eval_tiles(ctypes.c_void_p(rec.ctypes.data), len(rec)) == want
    for k in range(len(rec)):                                               # first_tile is the count of the entries before
        got = L.srx_srcnn_eval_tiles(ctypes.c_void_p(rec.ctypes.data), k + 1)
        assert got == (rec['first_tile'][k + 1] if k + 1 < len(rec) else want)
    p = ctypes.c_void_p(rec.ctypes.data)
    bad = rec.copy()
    bad['width'][1] = 0
    for args, piece in (((None, 1), b'null table'), ((p, 0), b'n 0'), ((ctypes.c_void_p(bad.ctypes.data), 3), b'entry 1:')):
        assert L.srx_srcnn_eval_tiles(*args) == 0
        assert b'srcnn_eval_tiles' in L.srx_last_error() and piece in L.srx_last_error(), L.srx_last_error()


def test_eval_pairs_refuses_before_any_launch():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    # never dereferenced: every case below is refused before any launch (this test runs without a GPU)
    a, t, sd, bq, hd = (ctypes.c_void_p(v) for v in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))
    cases = [(None, t, 4, 3, 6, sd, bq, hd), (a, None, 4, 3, 6, sd, bq, hd), (a, t, 4, 3, 6, None, bq, hd), (a, t, 4, 3, 6, sd, None, hd),
             (a, t, 4, 3, 6, sd, bq, None), (a, t, 0, 3, 6, sd, bq, hd), (a, t, -3, 3, 6, sd, bq, hd), (a, t, 4, 1, 6, sd, bq, hd),
             (a, t, 4, 9, 6, sd, bq, hd), (a, t, 4, 3, -1, sd, bq, hd), (a, t, 4, 3, 6, sd, sd, hd), (a, t, 4, 3, 6, sd, bq, sd),
             (a, t, 4, 3, 6, sd, bq, bq)]
    for args in cases:
        assert L.srx_srcnn_eval_pairs(*args, None) == BAD_ARG, args
        assert b'srcnn_eval_pairs' in L.srx_last_error(), args


# ---- the wrappers and the set's metadata ----------------------------------------------------------------------------------
def test_ops_table_raises_with_the_c_message_before_any_upload():
    import torch
    from ml_super_resolution_amd import _lib, ops
    rec, arena_bytes, floats, _ = literal_table(SHAPES)
    arena = torch.zeros(arena_bytes, dtype=torch.uint8)
    tab = ops.srcnn_eval_table(rec, F, BORDER, arena)
    assert len(tab) == len(rec) and (tab.f, tab.border, tab.arena_bytes, tab.out_floats, tab.crop_floats) == (F, BORDER, arena_bytes) + floats
    assert tuple(tab.words.shape) == (len(rec), 10)
    assert np.array_equal(tab.words.numpy().view(ops.SRCNN_EVAL_IMAGE_DTYPE).reshape(-1), rec)
    bad = rec.copy()
    bad['first_tile'][3] += 1
    with pytest.raises(_lib.SrxError, match=r'entry 3: first_tile'):
        ops.srcnn_eval_table(bad, F, BORDER, arena)
    with pytest.raises(_lib.SrxError, match=r'entry 6: image of \d+ bytes at offset \d+ leaves the arena'):
        ops.srcnn_eval_table(rec, F, BORDER, arena[:-1])
    with pytest.raises(_lib.SrxError, match=r'n 0'):
        ops.srcnn_eval_table(rec[:0], F, BORDER, arena)
    with pytest.raises(_lib.SrxError, match=r'crop_offset'):
        ops.srcnn_eval_table(rec, F, 5, arena)                               # a table built for another border
    with pytest.raises(ValueError):
        ops.srcnn_eval_table(rec.view(np.int32).reshape(-1, 10), F, BORDER, arena)
    with pytest.raises(ValueError, match='uint8'):
        ops.srcnn_eval_table(rec, F, BORDER, arena.to(torch.int8))


def test_eval_records_pack_the_images():
    from ml_super_resolution_amd.srcnn import srcnn
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    (arena, offsets, widths, heights), rec = srcnn.eval_records(images, F, BORDER)
    lit, arena_bytes, floats, _ = literal_table(SHAPES)
    assert np.array_equal(rec, lit) and arena.size == arena_bytes == sum(im.size for im in images)
    for k, im in enumerate(images):
        np.testing.assert_array_equal(arena[int(offsets[k]):int(offsets[k]) + im.size].reshape(im.shape), im)
    assert run_check(rec, arena_bytes, floats)[0] == 0


def test_device_eval_set_refuses_by_name_before_any_gpu_work():
    from ml_super_resolution_amd.srcnn import srcnn
    ok = np.zeros((23, 40, 3), np.uint8)
    with pytest.raises(ValueError, match='image small.png of 22 x 40 pixels is too small to score'):
        srcnn.DeviceEvalSet([ok, np.zeros((22, 40, 3), np.uint8)], 3, 6, 'cpu', names=['ok.png', 'small.png'])
    with pytest.raises(ValueError, match='image 0 of 40 x 22 '):
        srcnn.DeviceEvalSet([np.zeros((40, 22, 3), np.uint8)], 3, 6, 'cpu')
    with pytest.raises(ValueError, match='image 1 must be uint8'):
        srcnn.DeviceEvalSet([ok, np.zeros((40, 40), np.uint8)], 3, 6, 'cpu')
    with pytest.raises(ValueError, match='image f.png must be uint8'):
        srcnn.DeviceEvalSet([np.zeros((40, 40, 3), np.float32)], 3, 6, 'cpu', names=['f.png'])
    with pytest.raises(ValueError, match='no image'):
        srcnn.DeviceEvalSet([], 3, 6, 'cpu')
    with pytest.raises(ValueError, match='names'):
        srcnn.DeviceEvalSet([ok], 3, 6, 'cpu', names=['a', 'b'])


def test_new_flags_default_to_the_old_behaviour(tmp_path):
    from ml_super_resolution_amd.srcnn import evaluate, srcnn
    f = srcnn._flags().parse_args([])
    assert f.valid_images_path is None and f.valid_every == 0
    assert srcnn.FLAGS.valid_images_path is None and srcnn.FLAGS.valid_every == 0
    f = srcnn._flags().parse_args(['--valid-images-path', 'd', '--valid-every', '7'])
    assert (f.valid_images_path, f.valid_every) == ('d', 7)
    with pytest.raises(ValueError, match='--valid-images-path'):             # refused before a model or a file is touched
        srcnn.train(srcnn._flags().parse_args(['--train', '--valid-every', '2']), device='cpu', max_steps=0)
    e = evaluate.parse_flags(['--ckpt-dir-path', 'c', '--hd-dir-path', 'h'])
    assert (e.pairs, e.upscaling_factor, e.target_dir_path) == ('host', 3, None)
    assert set(srcnn.VALID_TAGS) == {'valid_psnr', 'valid_ssim', 'valid_psnr_bq', 'valid_ssim_bq'}
