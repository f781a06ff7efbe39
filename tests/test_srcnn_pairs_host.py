"""CPU-side checks of SRCNN's device batch sampler: srx_srcnn_patch_table_check (pure host code: the only thing between a
table and the kernel's reads), the argument checks of srx_srcnn_patch_pairs that come before any launch, the band and LDS
functions the launcher and the kernel share, srcnn/srcnn.py (DeviceImageSet, the random stream of patch_table) and the
--patch-source flag.  The GPU tests are in tests/test_gpu_srcnn_pairs.py."""
import ctypes
import os

import numpy as np
import pytest

from tests.patch_tables import bad_geometry_rows, entry_for, offsets_of, table_of

BAD_ARG = -1          # SRX_ERR_BAD_ARG
SHAPES = ((23, 31), (50, 47), (260, 300))        # (height, width) of the arena's images


OFFS, TOTAL = offsets_of(SHAPES)
entry = entry_for(SHAPES, 3.0)


def run_check(table, S, f, border, arena_bytes, B=None):
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    table = np.ascontiguousarray(table)
    rc = L.srx_srcnn_patch_table_check(ctypes.c_void_p(table.ctypes.data), len(table) if B is None else B, S, f, border, arena_bytes)
    return rc, L.srx_last_error().decode()


# ---- the record ---------------------------------------------------------------------------------------------------------
def test_record_layout_and_factor():
    from ml_super_resolution_amd import _lib, ops
    assert ops.PATCH_SRC_DTYPE.itemsize == ctypes.sizeof(_lib.PatchSrc) == 32
    for name, _ in _lib.PatchSrc._fields_:
        assert ops.PATCH_SRC_DTYPE.fields[name][1] == getattr(_lib.PatchSrc, name).offset, name
    words = ops.srcnn_patch_table_check(table_of([entry(1, 3, 4, 1, 3.0)]), 13, 3, 6, TOTAL)
    assert words.shape == (1, 8) and words.dtype == np.int32
    assert list(words[0, :7]) == [OFFS[1], 0, 47, 50, 3, 4, 1] and words[0, 7:].view(np.float32)[0] == 3.0
    # scaling_factor says what the table was built for: the same table is refused for another f
    for f in (2, 4):
        with pytest.raises(_lib.SrxError, match=r"entry 0: scaling factor 3 is not the table's f %d" % f):
            ops.srcnn_patch_table_check(table_of([entry(1, 3, 4, 1, 3.0)]), 13, f, 0, TOTAL)


# ---- the check --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', (2, 5, 13, 14, 243, 256))
def test_check_accepts_a_valid_table(S):
    """Both corners of every image that holds a crop, both flips; the far corner has x + S == width, y + S == height, and
    the last image ends on the arena's last byte.  Every f of 2..4 the size admits, and both limits of the border."""
    from ml_super_resolution_amd import _lib
    ran = 0
    for f in (2, 3, 4):
        if S // f < 1:
            assert run_check(table_of([entry(2, 0, 0, 0, float(f))]), S, f, 0, TOTAL)[0] == BAD_ARG
            continue
        entries = []
        for k, (h, w) in enumerate(SHAPES):
            if h >= S and w >= S:
                entries += [entry(k, 0, 0, fl, float(f)) for fl in (0, 1)] + [entry(k, w - S, h - S, 1, float(f))]
        assert entries and entries[-1][0] + 3 * SHAPES[-1][0] * SHAPES[-1][1] == TOTAL
        for border in (0, 1 if S > 2 else 0, (S - 1) // 2):
            assert 2 * border <= S - 1
            rc, msg = run_check(table_of(entries), S, f, border, TOTAL)
            assert rc == 0, msg
        assert 2 * ((S - 1) // 2) in (S - 1, S - 2)
        assert _lib.lib().srx_srcnn_pairs_band(S, f) >= 1
        ran += 1
    assert ran >= 1


def test_check_accepts_the_border_limits():
    t = table_of([entry(1, 0, 0)])
    assert run_check(t, 13, 3, 0, TOTAL)[0] == 0
    assert run_check(t, 13, 3, 6, TOTAL)[0] == 0          # 2 * border = S - 1
    assert run_check(t, 14, 3, 6, TOTAL)[0] == 0          # 2 * border = S - 2
    for S, border in ((13, 7), (14, 7), (13, -1), (13, 2 ** 30), (13, 2 ** 31 - 1)):
        rc, msg = run_check(t, S, 3, border, TOTAL)
        assert rc == BAD_ARG and 'border %d' % border in msg, msg


H1, W1 = SHAPES[1]
# (name, the bad entry, arena_bytes) at S = 20, f = 3, border = 6: each differs from a valid entry in ONE respect
BAD = bad_geometry_rows(SHAPES, 20, 3.0) + [
    ('y + S overflows int32', entry(1, 0, 2 ** 31 - 1), TOTAL),
    ('offset + size wraps to a small sum', (2 ** 64 - 3 * W1 * H1, W1, H1, 0, 0, 0, 3.0), TOTAL),
    ('zero height', (OFFS[1], W1, 0, 0, 0, 0, 3.0), TOTAL),
    ('negative width', (OFFS[1], -W1, H1, 0, 0, 0, 3.0), TOTAL),
    ('negative height', (OFFS[1], W1, -H1, 0, 0, 0, 3.0), TOTAL),
    ('flip 2', entry(1, 0, 0, 2), TOTAL),
    ('flip -1', entry(1, 0, 0, -1), TOTAL),
    ('factor 2', entry(1, 0, 0, 0, 2.0), TOTAL),
    ('factor 3.5', entry(1, 0, 0, 0, 3.5), TOTAL),
    ('factor NaN', entry(1, 0, 0, 0, np.nan), TOTAL),
]


# the whole message of the cases above that end at the arena bound (%d: the entry), as the build before the bound was
# shared with the whole-image tables printed it
ARENA_MESSAGES = {
    'image ends one byte past the arena':
        'srcnn_patch_table_check: entry %d: image of 234000 bytes at offset 9189 leaves the arena of 243188 bytes',
    'offset one byte too far':
        'srcnn_patch_table_check: entry %d: image of 234000 bytes at offset 9190 leaves the arena of 243189 bytes',
    'offset + size wraps around 2^64':
        'srcnn_patch_table_check: entry %d: image of 7050 bytes at offset 18446744073709551615 leaves the arena of 243189 bytes',
    'width * height * 3 far above the arena':
        'srcnn_patch_table_check: entry %d: image of 13835058042397261827 bytes at offset 2139 leaves the arena of 243189 bytes',
    'offset + size wraps to a small sum':
        'srcnn_patch_table_check: entry %d: image of 7050 bytes at offset 18446744073709544566 leaves the arena of 243189 bytes',
}
assert set(ARENA_MESSAGES) <= {b[0] for b in BAD}


@pytest.mark.parametrize('name,bad,arena_bytes', BAD, ids=[b[0] for b in BAD])
def test_check_refuses_one_bad_entry_and_names_it(name, bad, arena_bytes):
    good = entry(1, 1, 2, 1)
    assert run_check(table_of([good, good, good]), 20, 3, 6, TOTAL)[0] == 0
    for position in (0, 2):
        entries = [good, good, good]
        entries[position] = bad
        rc, msg = run_check(table_of(entries), 20, 3, 6, arena_bytes)
        assert rc == BAD_ARG, (name, msg)
        assert 'srcnn_patch_table_check' in msg and 'entry %d:' % position in msg, (name, msg)
        assert name not in ARENA_MESSAGES or msg == ARENA_MESSAGES[name] % position


def test_check_refuses_bad_table_B_S_f_and_border():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    good = table_of([entry(1, 0, 0)])
    assert L.srx_srcnn_patch_table_check(None, 1, 20, 3, 6, TOTAL) == BAD_ARG and b'null table' in L.srx_last_error()
    for B in (0, -1):
        rc, msg = run_check(good, 20, 3, 6, TOTAL, B=B)
        assert rc == BAD_ARG and 'B %d' % B in msg, msg
    for S in (1, 0, -5, 257, 2 ** 30):
        rc, msg = run_check(good, S, 3, 0, TOTAL)
        assert rc == BAD_ARG and 'S %d' % S in msg, msg
    for f in (1, 0, -3, 21, 2 ** 30):           # f < 2, or 20 // f < 1
        rc, msg = run_check(good, 20, f, 6, TOTAL)
        assert rc == BAD_ARG and 'f %d' % f in msg, msg
    assert run_check(table_of([entry(1, 0, 0, 0, 20.0)]), 20, 20, 6, TOTAL)[0] == 0          # 20 // 20 = 1
    for border in (-1, 10, 11, 2 ** 30):
        rc, msg = run_check(good, 20, 3, border, TOTAL)
        assert rc == BAD_ARG and 'border %d' % border in msg, msg


def test_patch_pairs_refuses_before_any_launch():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    # never dereferenced: every case below is refused before any launch (this test runs without a GPU)
    a, t, sd, hd = (ctypes.c_void_p(v) for v in (0x10000, 0x20000, 0x40000, 0x60000))
    cases = [(None, t, 4, 20, 3, 6, sd, hd), (a, None, 4, 20, 3, 6, sd, hd), (a, t, 4, 20, 3, 6, None, hd), (a, t, 4, 20, 3, 6, sd, None),
             (a, t, 0, 20, 3, 6, sd, hd), (a, t, -3, 20, 3, 6, sd, hd),
             (a, t, 4, 1, 3, 0, sd, hd), (a, t, 4, 0, 3, 0, sd, hd), (a, t, 4, 257, 3, 6, sd, hd), (a, t, 4, -20, 3, 6, sd, hd),
             (a, t, 4, 20, 1, 6, sd, hd), (a, t, 4, 20, 0, 6, sd, hd), (a, t, 4, 20, 21, 6, sd, hd), (a, t, 4, 20, -3, 6, sd, hd),
             (a, t, 4, 20, 3, -1, sd, hd), (a, t, 4, 20, 3, 10, sd, hd), (a, t, 4, 20, 3, 2 ** 30, sd, hd),
             (a, t, 4, 20, 3, 6, sd, sd)]
    for args in cases:
        assert L.srx_srcnn_patch_pairs(*args, None) == BAD_ARG, args
        assert b'srcnn_patch_pairs' in L.srx_last_error(), args


def test_ops_check_raises_with_the_c_message():
    from ml_super_resolution_amd import _lib, ops
    words = ops.srcnn_patch_table_check(table_of([entry(1, 0, 0), entry(1, 1, 9, 1)]), 20, 3, 6, TOTAL)
    assert words.dtype == np.int32 and words.shape == (2, 8)
    with pytest.raises(_lib.SrxError, match=r'entry 1: flip 3 is not 0 or 1'):
        ops.srcnn_patch_table_check(table_of([entry(1, 0, 0), entry(1, 0, 0, 3)]), 20, 3, 6, TOTAL)
    with pytest.raises(_lib.SrxError, match=r'entry 0: crop of 20 at x 40 y 0 leaves its 47 x 50 image'):
        ops.srcnn_patch_table_check(table_of([entry(1, 40, 0)]), 20, 3, 6, TOTAL)
    with pytest.raises(_lib.SrxError, match=r'B 0'):
        ops.srcnn_patch_table_check(table_of([]), 20, 3, 6, TOTAL)


# ---- the bands and the LDS formula ------------------------------------------------------------------------------------
def test_bands_cover_the_rows_and_lds_stays_within_the_cu():
    """For every admitted (S, f): the bands [k band, min(S, (k + 1) band)) cover [0, S) exactly once (1 <= band <= S is all
    that takes), the lo rows any band reaches (the first tap of its first row to the last tap of its last row, in the
    kernel's fp32 arithmetic) fit the rows the LDS formula allots, and the allocation stays within 160 KiB.  At the
    default shape a batch of 64 is at least 256 workgroups."""
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    worst = 0
    for S in range(2, 257):
        for f in range(2, S + 1):
            s = S // f
            band, lds = L.srx_srcnn_pairs_band(S, f), L.srx_srcnn_pairs_lds_bytes(S, f)
            assert 1 <= band <= S, (S, f, band)
            assert 0 < lds <= 160 * 1024, (S, f, lds)
            worst = max(worst, lds)
            starts = np.arange(0, S, band)
            ends = np.minimum(starts + band, S)
            assert starts[0] == 0 and ends[-1] == S and (starts[1:] == ends[:-1]).all() and (ends > starts).all()
            # layout of srcnn_pairs_lds: 1024 + 32 (s + S) + roundup16(12 n s) + 12 n S
            scale = np.float32(s) / np.float32(S)
            first = np.clip(np.floor(starts.astype(np.float32) * scale).astype(np.int64) - 1, 0, s - 1)
            last = np.clip(np.floor((ends - 1).astype(np.float32) * scale).astype(np.int64) + 2, 0, s - 1)
            n = int((last - first + 1).max())
            assert 1024 + 32 * (s + S) + ((12 * n * s + 15) & ~15) + 12 * n * S <= lds, (S, f, n, lds)
    assert worst <= 160 * 1024
    assert 64 * (-(-243 // L.srx_srcnn_pairs_band(243, 3))) >= 256
    for S, f in ((1, 2), (257, 2), (20, 1), (20, 21), (0, 0)):
        assert L.srx_srcnn_pairs_band(S, f) == -1 and L.srx_srcnn_pairs_lds_bytes(S, f) == -1


# ---- DeviceImageSet, the random stream, the flag ------------------------------------------------------------------------
def _write_jpgs(directory, shapes, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for i, (h, w) in enumerate(shapes):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(str(directory), '%d.jpg' % i), quality=90)


def _flags(argv):
    from ml_super_resolution_amd.srcnn import srcnn
    return srcnn._flags().parse_args(argv)


def test_image_set_packs_and_refuses_a_small_image():
    from ml_super_resolution_amd.srcnn import srcnn
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((20, 31), (25, 20))]
    s = srcnn.DeviceImageSet(images, 20, 'cpu')
    assert len(s) == 2 and s.crop_size == 20 and s.nbytes == 3 * (20 * 31 + 25 * 20) == s.arena.numel()
    assert s.offsets.tolist() == [0, 3 * 20 * 31] and s.widths.tolist() == [31, 20] and s.heights.tolist() == [20, 25]
    np.testing.assert_array_equal(s.arena.numpy()[:1860].reshape(20, 31, 3), images[0])
    np.testing.assert_array_equal(s.arena.numpy()[1860:].reshape(25, 20, 3), images[1])
    for shape in ((19, 31), (31, 19)):
        with pytest.raises(SystemExit, match='image smaller than the 20-pixel crop'):
            srcnn.DeviceImageSet(images + [np.zeros(shape + (3,), np.uint8)], 20, 'cpu')
    with pytest.raises(ValueError):
        srcnn.DeviceImageSet([np.zeros((20, 20, 3), np.float32)], 20, 'cpu')


def test_tables_follow_dataset_reader(tmp_path):
    """Three batches of 4 from 5 images, so both batch boundaries fall inside the image cycle (images 4, 0, 1, 2 and
    3, 4, 0, 1).  The crops rebuilt on the host from the tables are dataset_reader's batches, element for element: the same
    images in the same order, the same corners, the same flips."""
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.srcnn import srcnn
    shapes = ((40, 52), (33, 33), (60, 35), (34, 47), (51, 50))
    _write_jpgs(tmp_path, shapes, 7)
    flags = _flags(['--train', '--training-images-path', str(tmp_path), '--batch-size', '4', '--upscaling-factor', '3'])
    flags.crop_image_size = 33
    reader = srcnn.dataset_reader(flags, seed=11)
    images = srcnn.decode_training_images(flags)
    assert [im.shape[:2] for im in images] == list(shapes)
    image_set = srcnn.DeviceImageSet(images, 33, 'cpu')
    rng, state = np.random.default_rng(11), {}
    arena = image_set.arena.numpy()
    order, flips = [], set()
    for _ in range(3):
        want = next(reader)
        table = srcnn.patch_table(image_set, flags, rng, state)
        assert len(table) == 4 and (table['scaling_factor'] == 3.0).all()
        ops.srcnn_patch_table_check(table, 33, 3, 6, image_set.nbytes)
        got = []
        for t in table:
            k = image_set.offsets.tolist().index(int(t['offset']))
            order.append(k)
            h, w = shapes[k]
            assert (t['width'], t['height']) == (w, h)
            im = arena[int(t['offset']):int(t['offset']) + 3 * h * w].reshape(h, w, 3)
            crop = im[t['y']:t['y'] + 33, t['x']:t['x'] + 33]
            flips.add(int(t['flip']))
            got.append((crop[:, ::-1] if t['flip'] else crop).astype(np.float32) / np.float32(127.5) - np.float32(1.0))
        np.testing.assert_array_equal(np.stack(got), want)
    assert order == [k % 5 for k in range(12)] and state['k'] == 12 and flips == {0, 1}


def test_patch_source_flag():
    assert _flags([]).patch_source == 'host'
    assert _flags(['--patch-source', 'host']).patch_source == 'host'
    assert _flags(['--patch-source', 'device']).patch_source == 'device'
    for argv in (['--patch-source', 'gpu'], ['--patch-source']):
        with pytest.raises(SystemExit):
            _flags(argv)
