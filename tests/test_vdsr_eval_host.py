"""CPU-side checks of VDSR's whole-image pair source: srx_vdsr_eval_footprint (the per-axis reach of a tile, shared by the
host check and the kernel's pixel loops) against a brute-force enumeration of every pixel's taps, srx_vdsr_eval_table_check
(pure host code: the only bound between a table and the kernel's reads and writes), srx_vdsr_eval_tiles, the argument
checks of srx_vdsr_eval_pairs that come before any launch, the record builder, DeviceEvalSet's refusals and the new flags.
The GPU tests are in tests/test_gpu_vdsr_eval.py."""
import ctypes
import functools

import numpy as np
import pytest

from tests import eval_tables

BAD_ARG = -1          # SRX_ERR_BAD_ARG
T = 32                # SRX_VDSR_EVAL_TILE
SHAPES = ((5, 7), (11, 11), (23, 31), (33, 64), (50, 47), (97, 130), (128, 32))      # decoded (height, width)
FACTORS = (1.5, 2, 2.5, 3, 4)
f32 = np.float32


def literal_table(shapes, factors):
    """The records of every (factor, shape) with int(side / s) >= 1, factor-major over ONE arena that holds each shape once,
    with plain Python sums: (records, arena_bytes, out_floats, tiles)."""
    from ml_super_resolution_amd import ops
    offsets, at = [], 0
    for h, w in shapes:
        offsets.append(at)
        at += 3 * h * w
    rows, floats, tiles, end = [], 0, 0, 0
    for s in factors:
        for (h, w), off in zip(shapes, offsets):
            if int(h / s) < 1 or int(w / s) < 1:
                continue
            rows.append((off, w, h, floats, tiles, s))
            end = floats + 3 * h * w
            floats = (end + 3) // 4 * 4
            tiles += len(range(0, h, T)) * len(range(0, w, T))
    return np.array(rows, ops.VDSR_EVAL_IMAGE_DTYPE), at, end, tiles


run_check = functools.partial(eval_tables.run_check, 'srx_vdsr_eval_table_check')      # (rec, arena_bytes, out_floats, n=None)


# ---- the footprint ----------------------------------------------------------------------------------------------------
def _taps(o, scale, n):
    """resize_bilinear_kernel's two taps of outputs `o` (int array) from n inputs, in float32 with every operation rounded
    (numpy has no fma)."""
    f = (o.astype(f32) + f32(0.5)) * scale - f32(0.5)
    f = np.minimum(np.maximum(f, f32(0)), f32(n - 1))
    i0 = f.astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1)


def _brute_force(side, s, tile):
    """Every output pixel of the tile through both resizes and the blur halo: (lo, blurred, source) index sets' (min, max)."""
    L = int(side / s)
    sigma = f32(0.5) * (f32(s) - f32(1))
    R = int(f32(4) * sigma + f32(0.5))
    o = np.arange(tile * T, min(tile * T + T, side))
    lo = np.unique(np.concatenate(_taps(o, f32(L) / f32(side), L)))
    bl = np.unique(np.concatenate(_taps(lo, f32(side) / f32(L), side)))
    src = np.clip(bl[:, None] + np.arange(-R, R + 1)[None, :], 0, side - 1)
    return (lo.min(), lo.max()), (bl.min(), bl.max()), (src.min(), src.max())


@pytest.mark.parametrize('s', (1.25, 1.5, 2, 2.5, 3, 4, 8))
def test_footprint_against_brute_force(s):
    """Sides 1 .. 200, every tile: the function's three ranges contain the enumerated ones and exceed them by at most one
    index per side."""
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int * 6)()
    seen = 0
    for side in range(1, 201):
        tiles = -(-side // T)
        if int(side / s) < 1:
            assert L.srx_vdsr_eval_footprint(side, s, 0, out) == BAD_ARG and b'no low-resolution pixel' in L.srx_last_error()
            continue
        for tile in range(tiles):
            assert L.srx_vdsr_eval_footprint(side, s, tile, out) == 0, L.srx_last_error()
            got = list(out)
            for (lo, hi), (g_lo, g_hi) in zip(_brute_force(side, s, tile), (got[0:2], got[2:4], got[4:6])):
                assert g_lo <= lo and hi <= g_hi, (side, s, tile, got)
                assert lo - g_lo <= 1 and g_hi - hi <= 1, (side, s, tile, got)
            assert 0 <= got[0] and got[1] < int(side / s) and 0 <= got[4] <= got[2] and got[3] <= got[5] < side
            seen += 1
        assert L.srx_vdsr_eval_footprint(side, s, tiles, out) == BAD_ARG and L.srx_vdsr_eval_footprint(side, s, -1, out) == BAD_ARG
    assert seen > 600


def test_footprint_refusals():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int * 6)()
    for args, piece in (((64, 2.0, 0, None), b'null out'), ((0, 2.0, 0, out), b'side 0'), ((64, 1.0, 0, out), b'(1, 8]'),
                        ((64, 8.5, 0, out), b'(1, 8]'), ((64, float('nan'), 0, out), b'(1, 8]'), ((64, float('inf'), 0, out), b'(1, 8]'),
                        ((3, 4.0, 0, out), b'no low-resolution pixel'), ((64, 2.0, 2, out), b'tile 2')):
        assert L.srx_vdsr_eval_footprint(*args) == BAD_ARG, args
        assert b'vdsr_eval_footprint' in L.srx_last_error() and piece in L.srx_last_error(), L.srx_last_error()


# ---- the check --------------------------------------------------------------------------------------------------------
def test_the_sizes_reach_every_branch():
    """What the seven sizes are for, at T = 32: (5, 7) at s = 4 is smaller than the blur's window (radius 6) and its
    low-resolution image is 1 x 1; (11, 11) is the smallest image that can be scored; sides of exactly T and 2 T and one past
    a tile edge (33); a 4 x 5 grid of tiles with interior tiles whose reach is real image on all sides (97 x 130); a record
    whose floats are no multiple of 4, so the next one's start is padded; and pairs the factors drop (int(side / s) < 1)."""
    assert T == 32
    assert (int(5 / 4), int(7 / 4)) == (1, 1) and 5 < 2 * 6 + 1
    sides = {v for hw in SHAPES for v in hw}
    assert {11, T, 2 * T, T + 1} <= sides and {97, 130} <= sides
    assert -(-97 // T) == 4 and -(-130 // T) == 5
    assert any((3 * h * w) % 4 for h, w in SHAPES)
    assert int(5 / 8) < 1                                                   # s = 8 drops (5, 7)
    rec, _, _, _ = literal_table(SHAPES, FACTORS)
    assert len(rec) == len(SHAPES) * len(FACTORS)                           # none dropped at the GPU tests' factors


def test_check_accepts_the_records_of_ops():
    """The last image ends on the arena's last byte; the records of ops.vdsr_eval_records are the literal sums."""
    from ml_super_resolution_amd import ops
    rec, arena_bytes, floats, tiles = literal_table(SHAPES, FACTORS)
    got = ops.vdsr_eval_records(rec['height'], rec['width'], rec['offset'], rec['scaling_factor'])
    assert got.dtype == ops.VDSR_EVAL_IMAGE_DTYPE and np.array_equal(got, rec)
    assert (rec['out_offset'] % 4 == 0).all() and ((rec['out_offset'][1:] - rec['out_offset'][:-1]) != 3 * rec['height'][:-1] * rec['width'][:-1]).any()
    rc, msg = run_check(rec, arena_bytes, floats)
    assert rc == 0, msg
    rc, msg = run_check(rec[:1], arena_bytes, 3 * 5 * 7)
    assert rc == 0, msg
    one, ab, fl, _ = literal_table(((2, 2),), (2,))                         # the smallest record: one low-resolution pixel
    assert run_check(one, ab, fl)[0] == 0
    wide, ab, fl, _ = literal_table(((40, 300),), (8, 1.25, 1.001))         # the ends of the factor range
    assert run_check(wide, ab, fl)[0] == 0


_edited = functools.partial(eval_tables._edited, lambda: literal_table(SHAPES, FACTORS))


# (name, (records, arena_bytes, out_floats), the entry named, a piece of the message)
def _bad_cases():
    rec, ab, fl, _ = literal_table(SHAPES, FACTORS)
    last = len(rec) - 1
    return [
        ('width 0', _edited('width', 2, 0), 2, 'at least 1'),
        ('negative height', _edited('height', 4, -3), 4, 'at least 1'),
        ('s = 1', _edited('scaling_factor', 3, 1.0), 3, 'scaling_factor 1 is not'),
        ('s below 1', _edited('scaling_factor', 3, 0.5), 3, 'scaling_factor 0.5 is not'),
        ('s above 8', _edited('scaling_factor', 9, 8.5), 9, 'scaling_factor 8.5 is not'),
        ('s nan', _edited('scaling_factor', 1, np.nan), 1, 'is not a finite value'),
        ('s inf', _edited('scaling_factor', 1, np.inf), 1, 'is not a finite value'),
        ('no low-resolution row', _edited('scaling_factor', 0, 6.0), 0, 'no low-resolution pixel'),          # int(5 / 6) = 0
        ('no low-resolution column', _edited('scaling_factor', 7, 8.0), 7, 'no low-resolution pixel'),       # (5, 7) at 8
        ('an image one byte past the arena', (rec, ab - 1, fl), 6, 'leaves the arena'),
        ('an offset one byte too far', _edited('offset', 6, rec['offset'][6] + 1), 6, 'leaves the arena'),
        ('an offset that wraps', _edited('offset', 1, 2 ** 64 - 1), 1, 'leaves the arena'),
        ('out_offset one above', _edited('out_offset', 3, rec['out_offset'][3] + 1), 3, 'out_offset'),
        ('out_offset unpadded', _edited('out_offset', 1, 3 * 5 * 7), 1, 'out_offset 105 is not 108'),
        ('out_offset of the first entry', _edited('out_offset', 0, 4), 0, 'out_offset'),
        ('first_tile one above', _edited('first_tile', 2, rec['first_tile'][2] + 1), 2, 'first_tile'),
        ('first_tile one below', _edited('first_tile', last, rec['first_tile'][last] - 1), last, 'first_tile'),
        ('out_floats one short', (rec, ab, fl - 1), last, 'more than out_floats'),
    ]


BAD = _bad_cases()
# the whole message of every case above, as the build before the checks were shared printed it
MESSAGES = {
    'width 0':
        'vdsr_eval_table_check: entry 2: image of 0 x 23 pixels: each side must be at least 1',
    'negative height':
        'vdsr_eval_table_check: entry 4: image of 47 x -3 pixels: each side must be at least 1',
    's = 1':
        'vdsr_eval_table_check: entry 3: scaling_factor 1 is not a finite value in (1, 8]',
    's below 1':
        'vdsr_eval_table_check: entry 3: scaling_factor 0.5 is not a finite value in (1, 8]',
    's above 8':
        'vdsr_eval_table_check: entry 9: scaling_factor 8.5 is not a finite value in (1, 8]',
    's nan':
        'vdsr_eval_table_check: entry 1: scaling_factor nan is not a finite value in (1, 8]',
    's inf':
        'vdsr_eval_table_check: entry 1: scaling_factor inf is not a finite value in (1, 8]',
    'no low-resolution row':
        'vdsr_eval_table_check: entry 0: image of 7 x 5 pixels has no low-resolution pixel at scaling_factor 6',
    'no low-resolution column':
        'vdsr_eval_table_check: entry 7: image of 7 x 5 pixels has no low-resolution pixel at scaling_factor 8',
    'an image one byte past the arena':
        'vdsr_eval_table_check: entry 6: image of 12288 bytes at offset 53823 leaves the arena of 66110 bytes',
    'an offset one byte too far':
        'vdsr_eval_table_check: entry 6: image of 12288 bytes at offset 53824 leaves the arena of 66111 bytes',
    'an offset that wraps':
        'vdsr_eval_table_check: entry 1: image of 363 bytes at offset 18446744073709551615 leaves the arena of 66111 bytes',
    'out_offset one above':
        'vdsr_eval_table_check: entry 3: out_offset 2613 is not 2612, the floats of the entries before it padded to 4',
    'out_offset unpadded':
        'vdsr_eval_table_check: entry 1: out_offset 105 is not 108, the floats of the entries before it padded to 4',
    'out_offset of the first entry':
        'vdsr_eval_table_check: entry 0: out_offset 4 is not 0, the floats of the entries before it padded to 4',
    'first_tile one above':
        'vdsr_eval_table_check: entry 2: first_tile 3 is not the 2 tiles of the entries before it',
    'first_tile one below':
        'vdsr_eval_table_check: entry 34: first_tile 170 is not the 171 tiles of the entries before it',
    'out_floats one short':
        'vdsr_eval_table_check: entry 34: 12288 floats from 318312 on are more than out_floats 330599',
}


@pytest.mark.parametrize('name,args,entry,piece', BAD, ids=[b[0] for b in BAD])
def test_check_refuses_and_names_the_entry(name, args, entry, piece):
    rc, msg = run_check(*args)
    assert rc == BAD_ARG, (name, msg)
    assert 'vdsr_eval_table_check: entry %d:' % entry in msg and piece in msg, (name, msg)
    assert msg == MESSAGES[name]


def test_check_refuses_table_wide_faults():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    rec, arena_bytes, floats, _ = literal_table(SHAPES, FACTORS)
    assert L.srx_vdsr_eval_table_check(None, 1, arena_bytes, floats) == BAD_ARG and b'null table' in L.srx_last_error()
    assert L.srx_last_error() == b'vdsr_eval_table_check: null table'
    for n, whole in ((0, 'vdsr_eval_table_check: n 0 below 1'), (-1, 'vdsr_eval_table_check: n -1 below 1')):
        rc, msg = run_check(rec, arena_bytes, floats, n=n)
        assert rc == BAD_ARG and 'n %d' % n in msg, msg
        assert msg == whole
    rc, msg = run_check(rec, arena_bytes, floats + 1)                       # a total below out_floats
    assert rc == BAD_ARG and 'end at float %d, not at out_floats %d' % (floats, floats + 1) in msg, msg
    assert msg == "vdsr_eval_table_check: the table's 35 entries end at float 330600, not at out_floats 330601"


def test_check_refuses_more_tiles_than_a_grid_index_holds():
    """Records of 32768 x 32768 tiles (2^30) each: one passes, two reach 2^31.  The records share their bytes (only outputs
    must not overlap) and the arena is a number: the check reads no image byte."""
    from ml_super_resolution_amd import _lib, ops
    side = T * 32768
    rec = ops.vdsr_eval_records([side] * 3, [side] * 3, [0] * 3, [2.0] * 3)
    per = 3 * side * side
    assert run_check(rec[:1], per, per)[0] == 0
    rc, msg = run_check(rec[:2], per, 2 * per)
    assert rc == BAD_ARG and 'entry 1:' in msg and 'tiles' in msg and '2147483647' in msg, msg
    L = _lib.lib()
    assert L.srx_vdsr_eval_tiles(ctypes.c_void_p(rec.ctypes.data), 1) == 2 ** 30
    assert L.srx_vdsr_eval_tiles(ctypes.c_void_p(rec.ctypes.data), 2) == 0 and b'tiles' in L.srx_last_error()


def test_check_refuses_a_footprint_beyond_the_lds_layout():
    """Past 2^24 pixels a side fp32 no longer holds every pixel centre and a tile's ranges widen; at 2^27 x 2^27 and s = 1.25
    a tile would need more than the kernel's 40 KiB, and the record is refused for that (before its tiles are counted)."""
    from ml_super_resolution_amd import ops
    side = 2 ** 27
    rec = ops.vdsr_eval_records([side], [side], [0], [1.25])
    rc, msg = run_check(rec, 3 * side * side, 3 * side * side)
    assert rc == BAD_ARG and 'entry 0:' in msg and 'beyond the LDS layout of 40960 bytes' in msg, msg


# ---- tile counts ------------------------------------------------------------------------------------------------------
def test_tiles_equal_the_sum():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    shapes = SHAPES + ((T, 2 * T), (T + 1, T), (3 * T, T - 1), (1, 1), (512, 768))
    rec, _, _, tiles = literal_table(shapes, (2,))
    rec = rec[[k for k in range(len(rec))]]
    want = int((np.ceil(rec['height'] / T) * np.ceil(rec['width'] / T)).sum())
    assert want == tiles
    assert L.srx_vdsr_eval_tiles(ctypes.c_void_p(rec.ctypes.data), len(rec)) == want
    for k in range(len(rec)):                                               # first_tile is the count of the entries before
        got = L.srx_vdsr_eval_tiles(ctypes.c_void_p(rec.ctypes.data), k + 1)
        assert got == (rec['first_tile'][k + 1] if k + 1 < len(rec) else want)
    p = ctypes.c_void_p(rec.ctypes.data)
    bad = rec.copy()
    bad['width'][1] = 0
    for args, piece in (((None, 1), b'null table'), ((p, 0), b'n 0'), ((ctypes.c_void_p(bad.ctypes.data), 3), b'entry 1:')):
        assert L.srx_vdsr_eval_tiles(*args) == 0
        assert b'vdsr_eval_tiles' in L.srx_last_error() and piece in L.srx_last_error(), L.srx_last_error()


def test_eval_pairs_refuses_before_any_launch():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    # never dereferenced: every case below is refused before any launch (this test runs without a GPU)
    a, t, sd, hd = (ctypes.c_void_p(v) for v in (0x10000, 0x20000, 0x30000, 0x40000))
    cases = [(None, t, 4, sd, hd), (a, None, 4, sd, hd), (a, t, 4, None, hd), (a, t, 4, sd, None), (a, t, 0, sd, hd), (a, t, -3, sd, hd),
             (a, t, 4, sd, sd)]
    for args in cases:
        assert L.srx_vdsr_eval_pairs(*args, None) == BAD_ARG, args
        assert b'vdsr_eval_pairs' in L.srx_last_error(), args


# ---- the wrappers and the set's metadata ----------------------------------------------------------------------------------
def test_ops_table_raises_with_the_c_message_before_any_upload():
    import torch
    from ml_super_resolution_amd import _lib, ops
    rec, arena_bytes, floats, _ = literal_table(SHAPES, FACTORS)
    arena = torch.zeros(arena_bytes, dtype=torch.uint8)
    tab = ops.vdsr_eval_table(rec, arena)
    assert len(tab) == len(rec) and (tab.arena_bytes, tab.out_floats) == (arena_bytes, floats) and tuple(tab.words.shape) == (len(rec), 8)
    assert np.array_equal(tab.words.numpy().view(ops.VDSR_EVAL_IMAGE_DTYPE).reshape(-1), rec)
    bad = rec.copy()
    bad['first_tile'][3] += 1
    with pytest.raises(_lib.SrxError, match=r'entry 3: first_tile'):
        ops.vdsr_eval_table(bad, arena)
    with pytest.raises(_lib.SrxError, match=r'entry 6: image of \d+ bytes at offset \d+ leaves the arena'):
        ops.vdsr_eval_table(rec, arena[:-1])
    with pytest.raises(_lib.SrxError, match=r'n 0'):
        ops.vdsr_eval_table(rec[:0], arena)
    with pytest.raises(ValueError):
        ops.vdsr_eval_table(rec.view(np.int32).reshape(-1, 8), arena)


def test_eval_records_hold_each_image_once_and_every_factor():
    from ml_super_resolution_amd.vdsr import dataset
    rng = np.random.default_rng(3)
    shapes = tuple(s for s in SHAPES if min(s) >= 11)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]
    (arena, offsets, widths, heights), rec = dataset.eval_records(images, (2, 3, 4))
    lit, arena_bytes, floats, _ = literal_table(shapes, (2, 3, 4))
    assert np.array_equal(rec, lit) and arena.size == arena_bytes == sum(im.size for im in images)
    for k, im in enumerate(images):
        np.testing.assert_array_equal(arena[int(offsets[k]):int(offsets[k]) + im.size].reshape(im.shape), im)
    assert run_check(rec, arena_bytes, floats)[0] == 0


def test_device_eval_set_refuses_by_name_before_any_gpu_work():
    from ml_super_resolution_amd.vdsr import dataset
    ok = np.zeros((11, 40, 3), np.uint8)
    with pytest.raises(ValueError, match='image small.png of 10 x 40 pixels is too small to score'):
        dataset.DeviceEvalSet([ok, np.zeros((10, 40, 3), np.uint8)], [2], 'cpu', names=['ok.png', 'small.png'])
    with pytest.raises(ValueError, match='image 0 of 40 x 3 '):
        dataset.DeviceEvalSet([np.zeros((40, 3, 3), np.uint8)], [2], 'cpu')
    with pytest.raises(ValueError, match='uint8'):
        dataset.DeviceEvalSet([np.zeros((40, 40), np.uint8)], [2], 'cpu')
    with pytest.raises(ValueError, match='no image'):
        dataset.DeviceEvalSet([], [2], 'cpu')
    with pytest.raises(ValueError, match='names'):
        dataset.DeviceEvalSet([ok], [2], 'cpu', names=['a', 'b'])
    for factors in ([], [1.0], [2, 9]):
        with pytest.raises(ValueError, match='scaling factors'):
            dataset.DeviceEvalSet([ok], factors, 'cpu')


def test_new_flags_default_to_the_old_behaviour():
    from ml_super_resolution_amd.vdsr import experiment_train
    f = experiment_train.parse_flags([])
    assert f.valid_data_path is None and f.valid_every == 0 and f.valid_scaling_factors == '2_3_4'
    f = experiment_train.parse_flags(['--valid_data_path', 'd', '--valid_every', '7', '--valid_scaling_factors', '2_3'])
    assert (f.valid_data_path, f.valid_every, f.valid_scaling_factors) == ('d', 7, '2_3')
