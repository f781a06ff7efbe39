"""CPU-side checks of ESPCN's whole-image pair source: srx_espcn_eval_table_check (pure host code: the only bound between a
table and the kernel's reads and writes), srx_espcn_eval_tiles, the argument checks of srx_espcn_eval_pairs that come before
any launch, the record builder and the trimming of espcn/dataset.py, and the new flags.  The GPU tests are in
tests/test_gpu_espcn_eval.py."""
import ctypes
import functools

import numpy as np
import pytest

from tests import eval_tables

BAD_ARG = -1          # SRX_ERR_BAD_ARG
T = 16                # SRX_ESPCN_EVAL_TILE
SHAPES = ((9, 9), (23, 31), (40, 37), (64, 52), (120, 75), (131, 135))      # decoded (height, width)


def literal_table(shapes, r):
    """The records of `shapes` trimmed to multiples of r and packed back to back, with plain Python sums: (records,
    arena_bytes, lr_floats, tiles)."""
    from ml_super_resolution_amd import ops
    rec = np.zeros(len(shapes), ops.EVAL_IMAGE_DTYPE)
    at = floats = tiles = 0
    for k, (h, w) in enumerate(shapes):
        h, w = h - h % r, w - w % r
        rec[k] = (at, w, h, floats, tiles, 0)
        at += 3 * h * w
        floats += 3 * (h // r) * (w // r)
        tiles += len(range(0, h // r, T)) * len(range(0, w // r, T))
    return rec, at, floats, tiles


def run_check(rec, r, arena_bytes, lr_floats, n=None):
    return eval_tables.run_check('srx_espcn_eval_table_check', rec, r, arena_bytes, lr_floats, n=n)


# ---- the check --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', (2, 3, 4))
def test_check_accepts_a_packed_table(r):
    """The last image ends on the arena's last byte; 9 x 9 at r = 4 is an image of 2 x 2 lr pixels."""
    rec, arena_bytes, floats, _ = literal_table(SHAPES, r)
    rc, msg = run_check(rec, r, arena_bytes, floats)
    assert rc == 0, msg
    rc, msg = run_check(rec[:1], r, arena_bytes, 3 * (9 // r) ** 2)
    assert rc == 0, msg
    one = literal_table(((r, r),), r)                               # the smallest image: one lr pixel
    assert run_check(one[0], r, one[1], 3)[0] == 0


_edited = functools.partial(eval_tables._edited, lambda: literal_table(SHAPES, 3))


# (name, r, (records, arena_bytes, lr_floats), the entry named, a piece of the message)
def _bad_cases():
    rec3, bytes3, floats3, _ = literal_table(SHAPES, 3)
    cases = [
        ('width not a multiple of r', 3, _edited('width', 2, 37), 2, 'multiple of r 3'),
        ('height not a multiple of r', 3, _edited('height', 4, 119), 4, 'multiple of r 3'),
        ('width below r', 3, _edited('width', 1, 0), 1, 'multiple of r 3'),
        ('negative height', 3, _edited('height', 1, -3), 1, 'multiple of r 3'),
        ('lr_offset one above', 3, _edited('lr_offset', 3, rec3['lr_offset'][3] + 1), 3, 'lr_offset'),
        ('lr_offset one below', 3, _edited('lr_offset', 5, rec3['lr_offset'][5] - 1), 5, 'lr_offset'),
        ('lr_offset of the first entry', 3, _edited('lr_offset', 0, 1), 0, 'lr_offset'),
        ('first_tile one above', 3, _edited('first_tile', 2, rec3['first_tile'][2] + 1), 2, 'first_tile'),
        ('first_tile one below', 3, _edited('first_tile', 5, rec3['first_tile'][5] - 1), 5, 'first_tile'),
        ('an image one byte past the arena', 3, (rec3, bytes3 - 1, floats3), 5, 'leaves the arena'),
        ('an offset one byte too far', 3, _edited('offset', 5, rec3['offset'][5] + 1), 5, 'leaves the arena'),
        ('an offset that wraps', 3, _edited('offset', 1, 2 ** 64 - 1), 1, 'leaves the arena'),
        ('reserved 1', 3, _edited('reserved', 4, 1), 4, 'reserved 1'),
        ('lr_floats one short', 3, (rec3, bytes3, floats3 - 1), 5, 'more than lr_floats'),
    ]
    return cases


BAD = _bad_cases()
# the whole message of every case above, as the build before the checks were shared printed it
MESSAGES = {
    'width not a multiple of r':
        'espcn_eval_table_check: entry 2: image of 37 x 39 pixels: each side must be a multiple of r 3, at least r',
    'height not a multiple of r':
        'espcn_eval_table_check: entry 4: image of 75 x 119 pixels: each side must be a multiple of r 3, at least r',
    'width below r':
        'espcn_eval_table_check: entry 1: image of 0 x 21 pixels: each side must be a multiple of r 3, at least r',
    'negative height':
        'espcn_eval_table_check: entry 1: image of 30 x -3 pixels: each side must be a multiple of r 3, at least r',
    'lr_offset one above':
        'espcn_eval_table_check: entry 3: lr_offset 706 is not the 705 lr floats of the entries before it',
    'lr_offset one below':
        'espcn_eval_table_check: entry 5: lr_offset 4775 is not the 4776 lr floats of the entries before it',
    'lr_offset of the first entry':
        'espcn_eval_table_check: entry 0: lr_offset 1 is not the 0 lr floats of the entries before it',
    'first_tile one above':
        'espcn_eval_table_check: entry 2: first_tile 3 is not the 2 tiles of the entries before it',
    'first_tile one below':
        'espcn_eval_table_check: entry 5: first_tile 12 is not the 13 tiles of the entries before it',
    'an image one byte past the arena':
        'espcn_eval_table_check: entry 5: image of 52245 bytes at offset 42984 leaves the arena of 95228 bytes',
    'an offset one byte too far':
        'espcn_eval_table_check: entry 5: image of 52245 bytes at offset 42985 leaves the arena of 95229 bytes',
    'an offset that wraps':
        'espcn_eval_table_check: entry 1: image of 1890 bytes at offset 18446744073709551615 leaves the arena of 95229 bytes',
    'reserved 1':
        'espcn_eval_table_check: entry 4: reserved 1 is not 0',
    'lr_floats one short':
        'espcn_eval_table_check: entry 5: 5805 lr floats after 4776 before it are more than lr_floats 10580',
}


@pytest.mark.parametrize('name,r,args,entry,piece', BAD, ids=[b[0] for b in BAD])
def test_check_refuses_and_names_the_entry(name, r, args, entry, piece):
    rc, msg = run_check(args[0], r, args[1], args[2])
    assert rc == BAD_ARG, (name, msg)
    assert 'espcn_eval_table_check: entry %d:' % entry in msg and piece in msg, (name, msg)
    assert msg == MESSAGES[name]


def test_check_refuses_table_wide_faults():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    rec, arena_bytes, floats, _ = literal_table(SHAPES, 3)
    assert L.srx_espcn_eval_table_check(None, 1, 3, arena_bytes, floats) == BAD_ARG and b'null table' in L.srx_last_error()
    assert L.srx_last_error() == b'espcn_eval_table_check: null table'
    for n, whole in ((0, 'espcn_eval_table_check: n 0 below 1'), (-1, 'espcn_eval_table_check: n -1 below 1')):
        rc, msg = run_check(rec, 3, arena_bytes, floats, n=n)
        assert rc == BAD_ARG and 'n %d' % n in msg, msg
        assert msg == whole
    for r, whole in ((1, 'espcn_eval_table_check: r 1 outside 2..4'), (0, 'espcn_eval_table_check: r 0 outside 2..4'),
                     (-2, 'espcn_eval_table_check: r -2 outside 2..4'), (5, 'espcn_eval_table_check: r 5 outside 2..4')):
        rc, msg = run_check(rec, r, arena_bytes, floats)
        assert rc == BAD_ARG and 'r %d outside 2..4' % r in msg, msg
        assert msg == whole
    rc, msg = run_check(rec, 3, arena_bytes, floats + 1)                    # a total below lr_floats
    assert rc == BAD_ARG and 'hold %d lr floats, not lr_floats %d' % (floats, floats + 1) in msg, msg
    assert msg == "espcn_eval_table_check: the table's 6 entries hold 10581 lr floats, not lr_floats 10582"
    # a table for r = 3 is not one for r = 2: the running sums differ from the second entry on
    rc, msg = run_check(rec, 2, arena_bytes, floats)
    assert rc == BAD_ARG and 'entry' in msg, msg
    assert msg == 'espcn_eval_table_check: entry 0: image of 9 x 9 pixels: each side must be a multiple of r 2, at least r'


def test_check_refuses_more_tiles_than_a_grid_index_holds():
    """Entries of 32768 x 32768 tiles (2^30) each: one passes, two reach 2^31.  The entries share their bytes (only outputs
    must not overlap) and the arena is a number: the check reads no image byte."""
    from ml_super_resolution_amd import ops
    r = 2
    w, h = 2 * T * 32768, 2 * T * 32768                                 # 2^30 tiles per entry
    per_floats, per_bytes = 3 * (h // r) * (w // r), 3 * h * w
    rec = np.zeros(3, ops.EVAL_IMAGE_DTYPE)
    for k in range(3):
        rec[k] = (0, w, h, k * per_floats, (k * 2 ** 30) % 2 ** 32, 0)
    assert run_check(rec[:1], r, per_bytes, per_floats)[0] == 0
    rc, msg = run_check(rec[:2], r, per_bytes, 2 * per_floats)
    assert rc == BAD_ARG and 'entry 1:' in msg and 'tiles' in msg and '2147483647' in msg, msg
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    assert L.srx_espcn_eval_tiles(ctypes.c_void_p(rec.ctypes.data), 1, r) == 2 ** 30
    assert L.srx_espcn_eval_tiles(ctypes.c_void_p(rec.ctypes.data), 2, r) == 0 and b'tiles' in L.srx_last_error()


# ---- tile counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', (2, 3, 4))
def test_tiles_against_a_numpy_count(r):
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    shapes = SHAPES + ((16 * r, 32 * r), (16 * r + 1, 17 * r), (33 * r, 15 * r), (r, r), (512, 768))
    rec, _, _, tiles = literal_table(shapes, r)
    hp, wp = rec['height'] // r, rec['width'] // r
    want = int((np.ceil(hp / T) * np.ceil(wp / T)).sum())
    assert want == tiles
    assert L.srx_espcn_eval_tiles(ctypes.c_void_p(rec.ctypes.data), len(rec), r) == want
    for k in range(len(rec)):                                               # first_tile is the count of the entries before
        got = L.srx_espcn_eval_tiles(ctypes.c_void_p(rec.ctypes.data), k + 1, r)
        assert got == (rec['first_tile'][k + 1] if k + 1 < len(rec) else want)


def test_tiles_refusals():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    rec = literal_table(SHAPES, 3)[0]
    p = ctypes.c_void_p(rec.ctypes.data)
    for args, piece in (((None, 1, 3), b'null table'), ((p, 0, 3), b'n 0'), ((p, 6, 5), b'r 5'), ((p, 6, 2), b'entry 0:')):
        assert L.srx_espcn_eval_tiles(*args) == 0
        assert b'espcn_eval_tiles' in L.srx_last_error() and piece in L.srx_last_error(), L.srx_last_error()


def test_eval_pairs_refuses_before_any_launch():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    # never dereferenced: every case below is refused before any launch (this test runs without a GPU)
    a, t, lr, lab = (ctypes.c_void_p(v) for v in (0x10000, 0x20000, 0x30000, 0x40000))
    cases = [(None, t, 4, 3, lr, lab), (a, None, 4, 3, lr, lab), (a, t, 4, 3, None, lab), (a, t, 4, 3, lr, None),
             (a, t, 0, 3, lr, lab), (a, t, -3, 3, lr, lab), (a, t, 4, 1, lr, lab), (a, t, 4, 5, lr, lab), (a, t, 4, 3, lr, lr)]
    for args in cases:
        assert L.srx_espcn_eval_pairs(*args, None) == BAD_ARG, args
        assert b'espcn_eval_pairs' in L.srx_last_error(), args


# ---- the record builder and the set's metadata ----------------------------------------------------------------------------
@pytest.mark.parametrize('r', (2, 3, 4))
def test_records_equal_the_literal_sums(r):
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.espcn import dataset
    rng = np.random.default_rng(3)
    shapes = tuple(s for s in SHAPES if s[0] // r >= 11)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]
    trimmed, names = dataset.trimmed_eval_images(images, r)
    assert names == [str(k) for k in range(len(images))]
    for im, tr in zip(images, trimmed):
        h, w = im.shape[0] - im.shape[0] % r, im.shape[1] - im.shape[1] % r
        assert tr.shape == (h, w, 3) and np.array_equal(tr, im[:h, :w])
    (arena, offsets, widths, heights), rec = dataset.eval_records(trimmed, r)
    lit, arena_bytes, floats, _ = literal_table(shapes, r)
    assert rec.dtype == ops.EVAL_IMAGE_DTYPE and np.array_equal(rec, lit)
    assert arena.size == arena_bytes
    for k, tr in enumerate(trimmed):
        np.testing.assert_array_equal(arena[int(offsets[k]):int(offsets[k]) + tr.size].reshape(tr.shape), tr)
    assert run_check(rec, r, arena_bytes, floats)[0] == 0


def test_ops_table_raises_with_the_c_message_before_any_upload():
    import torch
    from ml_super_resolution_amd import _lib, ops
    rec, arena_bytes, floats, _ = literal_table(SHAPES, 3)
    arena = torch.zeros(arena_bytes, dtype=torch.uint8)
    tab = ops.espcn_eval_table(rec, 3, arena)
    assert len(tab) == 6 and (tab.r, tab.arena_bytes, tab.lr_floats) == (3, arena_bytes, floats) and tuple(tab.words.shape) == (6, 8)
    assert np.array_equal(tab.words.numpy().view(ops.EVAL_IMAGE_DTYPE).reshape(-1), rec)
    bad = rec.copy()
    bad['first_tile'][3] += 1
    with pytest.raises(_lib.SrxError, match=r'entry 3: first_tile'):
        ops.espcn_eval_table(bad, 3, arena)
    with pytest.raises(_lib.SrxError, match=r'entry 5: image of \d+ bytes at offset \d+ leaves the arena'):
        ops.espcn_eval_table(rec, 3, arena[:-1])
    with pytest.raises(_lib.SrxError, match=r'r 5'):
        ops.espcn_eval_table(rec, 5, arena)
    with pytest.raises(_lib.SrxError, match=r'n 0'):
        ops.espcn_eval_table(rec[:0], 3, arena)
    with pytest.raises(ValueError):
        ops.espcn_eval_table(rec.view(np.int32).reshape(-1, 8), 3, arena)


def test_images_too_small_to_score_are_refused_by_name():
    from ml_super_resolution_amd.espcn import dataset
    ok = np.zeros((33, 6, 3), np.uint8)                                 # r = 3: h' = 11, w' r^2 = 18
    assert [t.shape for t in dataset.trimmed_eval_images([ok], 3)[0]] == [(33, 6, 3)]
    with pytest.raises(ValueError, match='image small.png of 32 x 40'):
        dataset.trimmed_eval_images([ok, np.zeros((32, 40, 3), np.uint8)], 3, names=['ok.png', 'small.png'])      # h' = 10
    with pytest.raises(ValueError, match='image 0 of 40 x 3 '):
        dataset.trimmed_eval_images([np.zeros((40, 3, 3), np.uint8)], 2)                                         # w' r^2 = 4
    with pytest.raises(ValueError):
        dataset.trimmed_eval_images([np.zeros((40, 40), np.uint8)], 2)
    with pytest.raises(ValueError):
        dataset.trimmed_eval_images([], 2)
    with pytest.raises(ValueError):
        dataset.trimmed_eval_images([ok], 3, names=['a', 'b'])


def test_new_flags_default_to_the_old_behaviour():
    from ml_super_resolution_amd.espcn import experiment_scores, experiment_train
    f = experiment_train.parse_flags([])
    assert f.valid_data_path is None and f.valid_every == 0
    f = experiment_train.parse_flags(['--valid_data_path', 'd', '--valid_every', '7'])
    assert (f.valid_data_path, f.valid_every) == ('d', 7)
    base = ['--ckpt_path', 'c', '--data_path', 'd']
    assert experiment_scores.parse_flags(base).pairs == 'host'
    assert experiment_scores.parse_flags(base + ['--pairs', 'device']).pairs == 'device'
    with pytest.raises(SystemExit):
        experiment_scores.parse_flags(base + ['--pairs', 'gpu'])
