"""CPU-side checks of EnhanceNet's device batch sampler: srx_enet_patch_table_check (pure host code: the only thing between
a table and the kernel's reads), the argument checks of srx_enet_patch_pairs that come before any launch, the coefficient
block of srx_enet_pairs_tables, enet/datasets.py (the packing of DeviceImageSet, the random stream of
device_image_batches) and the --patch_source flag.  The GPU tests are in tests/test_gpu_enet_pairs.py."""
import ctypes
import os

import numpy as np
import pytest

from tests.patch_tables import bad_geometry_rows, entry_for, offsets_of, table_of

BAD_ARG = -1          # SRX_ERR_BAD_ARG
SHAPES = ((23, 31), (60, 52), (128, 130))        # (height, width) of the arena's images


OFFS, TOTAL = offsets_of(SHAPES)
entry = entry_for(SHAPES, 4.0)


def run_check(table, S, arena_bytes, B=None):
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    table = np.ascontiguousarray(table)
    rc = L.srx_enet_patch_table_check(ctypes.c_void_p(table.ctypes.data), len(table) if B is None else B, S, arena_bytes)
    return rc, L.srx_last_error().decode()


# ---- the check --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', (4, 8, 20, 128))
def test_check_accepts_a_valid_table(S):
    """Both corners of every image that holds a crop, every flip; the far corner has x + S == width, y + S == height, and
    the last image ends on the arena's last byte."""
    entries = []
    for k, (h, w) in enumerate(SHAPES):
        if h >= S and w >= S:
            entries += [entry(k, 0, 0, f) for f in range(4)] + [entry(k, w - S, h - S, 3)]
    assert entries and entries[-1][0] + 3 * SHAPES[-1][0] * SHAPES[-1][1] == TOTAL
    rc, msg = run_check(table_of(entries), S, TOTAL)
    assert rc == 0, msg


H1, W1 = SHAPES[1]
H2, W2 = SHAPES[2]
# (name, the bad entry, arena_bytes) at S = 20: each differs from a valid entry in ONE respect
BAD = bad_geometry_rows(SHAPES, 20, 4.0) + [
    ('offset + size wraps to a small sum', (2 ** 64 - 3 * W1 * H1, W1, H1, 0, 0, 0, 4.0), TOTAL),
    ('flip 4', entry(1, 0, 0, 4), TOTAL),
    ('flip -1', entry(1, 0, 0, -1), TOTAL),
    ('factor 3', entry(1, 0, 0, 0, 3.0), TOTAL),
    ('factor 4.5', entry(1, 0, 0, 0, 4.5), TOTAL),
    ('factor NaN', entry(1, 0, 0, 0, np.nan), TOTAL),
]


# the whole message of the cases above that end at the arena bound (%d: the entry), as the build before the bound was
# shared with the whole-image tables printed it
ARENA_MESSAGES = {
    'image ends one byte past the arena':
        'enet_patch_table_check: entry %d: image of 49920 bytes at offset 11499 leaves the arena of 61418 bytes',
    'offset one byte too far':
        'enet_patch_table_check: entry %d: image of 49920 bytes at offset 11500 leaves the arena of 61419 bytes',
    'offset + size wraps around 2^64':
        'enet_patch_table_check: entry %d: image of 9360 bytes at offset 18446744073709551615 leaves the arena of 61419 bytes',
    'width * height * 3 far above the arena':
        'enet_patch_table_check: entry %d: image of 13835058042397261827 bytes at offset 2139 leaves the arena of 61419 bytes',
    'offset + size wraps to a small sum':
        'enet_patch_table_check: entry %d: image of 9360 bytes at offset 18446744073709542256 leaves the arena of 61419 bytes',
}
assert set(ARENA_MESSAGES) <= {b[0] for b in BAD}


@pytest.mark.parametrize('name,bad,arena_bytes', BAD, ids=[b[0] for b in BAD])
def test_check_refuses_one_bad_entry_and_names_it(name, bad, arena_bytes):
    good = entry(1, 1, 2, 3)
    assert run_check(table_of([good, good, good]), 20, TOTAL)[0] == 0
    for position in (0, 2):
        entries = [good, good, good]
        entries[position] = bad
        rc, msg = run_check(table_of(entries), 20, arena_bytes)
        assert rc == BAD_ARG, (name, msg)
        assert 'enet_patch_table_check' in msg and 'entry %d:' % position in msg, (name, msg)
        assert name not in ARENA_MESSAGES or msg == ARENA_MESSAGES[name] % position


def test_check_at_both_arena_boundaries():
    """The last image ends exactly at arena_bytes: accepted.  One byte less of arena, or the image one byte further:
    refused.  The first image starts at offset 0."""
    last, first = table_of([entry(2, 2, 0, 1)]), table_of([entry(0, 0, 0)])
    assert OFFS[2] + 3 * W2 * H2 == TOTAL and OFFS[0] == 0
    assert run_check(last, 128, TOTAL)[0] == 0
    rc, msg = run_check(last, 128, TOTAL - 1)
    assert rc == BAD_ARG and 'entry 0:' in msg and 'leaves the arena' in msg, msg
    assert msg == 'enet_patch_table_check: entry 0: image of 49920 bytes at offset 11499 leaves the arena of 61418 bytes'
    assert run_check(first, 20, 3 * 23 * 31)[0] == 0                    # an arena of that image alone
    rc, msg = run_check(first, 20, 3 * 23 * 31 - 1)
    assert rc == BAD_ARG and 'entry 0:' in msg and 'leaves the arena' in msg, msg
    assert msg == 'enet_patch_table_check: entry 0: image of 2139 bytes at offset 0 leaves the arena of 2138 bytes'


def test_check_refuses_bad_table_B_and_S():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    good = table_of([entry(1, 0, 0)])
    assert L.srx_enet_patch_table_check(None, 1, 20, TOTAL) == BAD_ARG and b'null table' in L.srx_last_error()
    for B in (0, -1):
        rc, msg = run_check(good, 20, TOTAL, B=B)
        assert rc == BAD_ARG and 'B %d' % B in msg, msg
    for S in (0, -4, 2, 3, 6, 21, 130, 132, 2 ** 30):
        rc, msg = run_check(good, S, TOTAL)
        assert rc == BAD_ARG and 'S %d' % S in msg, msg


def test_patch_pairs_refuses_before_any_launch():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    # never dereferenced: every case below is refused before any launch (this test runs without a GPU)
    a, t, c, sd, bq, hd = (ctypes.c_void_p(v) for v in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000))
    cases = [(None, t, 4, 20, c, sd, bq, hd), (a, None, 4, 20, c, sd, bq, hd), (a, t, 4, 20, None, sd, bq, hd),
             (a, t, 4, 20, c, None, bq, hd), (a, t, 4, 20, c, sd, None, hd), (a, t, 4, 20, c, sd, bq, None),
             (a, t, 0, 20, c, sd, bq, hd), (a, t, -3, 20, c, sd, bq, hd),
             (a, t, 4, 0, c, sd, bq, hd), (a, t, 4, 2, c, sd, bq, hd), (a, t, 4, 22, c, sd, bq, hd), (a, t, 4, 132, c, sd, bq, hd),
             (a, t, 4, 20, c, sd, sd, hd), (a, t, 4, 20, c, sd, bq, bq), (a, t, 4, 20, c, hd, bq, hd)]
    for args in cases:
        assert L.srx_enet_patch_pairs(*args, None) == BAD_ARG, args
        assert b'enet_patch_pairs' in L.srx_last_error(), args


def test_ops_check_raises_with_the_c_message():
    from ml_super_resolution_amd import _lib, ops
    words = ops.enet_patch_table_check(table_of([entry(1, 0, 0), entry(1, 1, 9, 3)]), 20, TOTAL)
    assert words.dtype == np.int32 and words.shape == (2, 8)
    with pytest.raises(_lib.SrxError, match=r'entry 1: flip 7 outside 0..3'):
        ops.enet_patch_table_check(table_of([entry(1, 0, 0), entry(1, 0, 0, 7)]), 20, TOTAL)
    with pytest.raises(_lib.SrxError, match=r'entry 0: scaling factor 2 is not 4'):
        ops.enet_patch_table_check(table_of([entry(1, 0, 0, 0, 2.0)]), 20, TOTAL)
    with pytest.raises(_lib.SrxError, match=r'B 0'):
        ops.enet_patch_table_check(table_of([]), 20, TOTAL)


# ---- the coefficient block --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', (4, 8, 20, 128))
def test_coefficient_block_equals_the_oracle_and_the_existing_tables(S):
    from oracle import oracle as O
    from ml_super_resolution_amd import _lib, ops
    s = S // 4
    assert _lib.lib().srx_enet_pairs_table_words(S) == (2 + 9) * s + (2 + 5) * S
    block = ops.enet_pairs_tables(S)
    assert block.dtype == np.int32 and block.shape == ((2 + 9) * s + (2 + 5) * S,)
    parts = np.split(block, np.cumsum([2 * s, 9 * s, 2 * S]))
    got = ((parts[0].reshape(s, 2), parts[1].reshape(s, 9)), (parts[2].reshape(S, 2), parts[3].reshape(S, 5)))
    for (bounds, kk), (n_in, n_out, filt) in zip(got, ((S, s, 'bilinear'), (s, S, 'bicubic'))):
        ref_bounds, ref_kk = O.pil_resample_coeffs(n_in, n_out, filt)
        np.testing.assert_array_equal(bounds, ref_bounds)
        np.testing.assert_array_equal(kk, ref_kk)
        lib_bounds, lib_kk = ops.pil_resample_coeffs(n_in, n_out, filt)
        np.testing.assert_array_equal(bounds, lib_bounds)
        np.testing.assert_array_equal(kk, lib_kk)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all()     # what the kernel relies on


def test_coefficient_block_refusals():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    for S in (0, 2, 6, 132, -8):
        assert L.srx_enet_pairs_table_words(S) == -1 and ('S %d' % S).encode() in L.srx_last_error()
        buf = np.zeros(4096, np.int32)
        assert L.srx_enet_pairs_tables(S, ctypes.c_void_p(buf.ctypes.data)) == BAD_ARG and not buf.any()
    assert L.srx_enet_pairs_tables(8, None) == BAD_ARG and b'null block' in L.srx_last_error()


# ---- DeviceImageSet ---------------------------------------------------------------------------------------------------
def _write_pngs(directory, shapes, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    images = {}
    for i, (h, w) in enumerate(shapes):
        images['im%d.png' % i] = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        Image.fromarray(images['im%d.png' % i]).save(os.path.join(str(directory), 'im%d.png' % i))
    return images


def test_image_set_packs_the_reachable_region(tmp_path):
    from ml_super_resolution_amd.enet import datasets
    images = _write_pngs(tmp_path, ((300, 260), (255, 255)), 4)
    extra = np.random.default_rng(5).integers(0, 256, size=(256, 301, 3), dtype=np.uint8)
    paths = [str(tmp_path / 'im0.png'), str(tmp_path / 'im1.png')]
    s = datasets.DeviceImageSet(paths + [extra], 'cpu')
    assert len(s) == 3 and s.hd_size == 128
    assert s.widths.tolist() == [255, 255, 255] and s.heights.tolist() == [255, 255, 255]
    assert s.offsets.tolist() == [0, 195075, 390150] and s.nbytes == 3 * 195075 == s.arena.numel()
    assert s.index == {paths[0]: 0, paths[1]: 1}
    arena = s.arena.numpy()
    for k, im in enumerate((images['im0.png'], images['im1.png'], extra)):
        np.testing.assert_array_equal(arena[195075 * k:195075 * (k + 1)].reshape(255, 255, 3), im[:255, :255])
    # a smaller hd_size keeps a smaller region
    small = datasets.DeviceImageSet([extra], 'cpu', hd_size=20)
    np.testing.assert_array_equal(small.arena.numpy().reshape(39, 39, 3), extra[:39, :39])


@pytest.mark.parametrize('shape', ((254, 300), (300, 254)))
def test_image_set_refuses_a_small_image_and_names_it(tmp_path, shape):
    from ml_super_resolution_amd.enet import datasets
    _write_pngs(tmp_path, ((255, 255), shape), 6)
    with pytest.raises(ValueError, match=r'im1\.png is smaller than 255'):
        datasets.DeviceImageSet.from_directory(str(tmp_path), 'cpu')
    with pytest.raises(ValueError, match='image 0 is smaller than 255'):
        datasets.DeviceImageSet([np.zeros(shape + (3,), np.uint8)], 'cpu')
    with pytest.raises(ValueError):
        datasets.DeviceImageSet([np.zeros((255, 255, 3), np.float32)], 'cpu')


# ---- the random stream ------------------------------------------------------------------------------------------------
def reference_draws(dir_path, rng, batches, batch_size):
    """enet/enet/datasets.py:82-108 restated: the shuffled walk over the (sorted) directory and, per image, x then y."""
    names = sorted(os.listdir(dir_path))

    def image_paths():
        while True:
            rng.shuffle(names)
            for name in names:
                yield os.path.join(dir_path, name)
    gen = image_paths()
    out = []
    for _ in range(batches):
        batch = []
        for _ in range(batch_size):
            path = next(gen)
            x = rng.randint(128)
            y = rng.randint(128)
            batch.append((path, x, y))
        out.append(batch)
    return out


@pytest.fixture(scope='module')
def five_images(tmp_path_factory):
    d = tmp_path_factory.mktemp('enet_images')
    _write_pngs(d, ((255, 255), (260, 255), (255, 300), (256, 257), (270, 280)), 7)
    return str(d)


@pytest.mark.parametrize('flips', (False, True))
def test_tables_follow_the_reference_stream(five_images, flips):
    """Three batches of 4 from 5 images: the walk is reshuffled twice inside them.  No launch: the set lives on the CPU and
    only the tables are drawn; each passes the check."""
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.enet import datasets
    s = datasets.DeviceImageSet.from_directory(five_images, 'cpu')
    it = datasets.device_image_batches(s, 4, 4, 'cpu', rng=np.random.RandomState(77), flips=flips)
    ref = reference_draws(five_images, np.random.RandomState(77), 3, 4)
    seen_flips = set()
    for batch in ref:
        table = it.next_table()
        assert it.last_table is table and len(table) == 4
        ops.enet_patch_table_check(table, 128, s.nbytes)
        for got, (path, x, y) in zip(table, batch):
            k = s.index[path]
            assert (got['offset'], got['width'], got['height'], got['x'], got['y'], got['scaling_factor']) == \
                (s.offsets[k], 255, 255, x, y, 4.0)
            assert 0 <= got['flip'] <= 3 and (flips or got['flip'] == 0)
            seen_flips.add(int(got['flip']))
    assert len({p for b in ref for p, _, _ in b}) == 5
    assert not flips or len(seen_flips) > 1


def test_batches_refuse_another_factor_or_device(five_images):
    from ml_super_resolution_amd.enet import datasets
    s = datasets.DeviceImageSet.from_directory(five_images, 'cpu')
    with pytest.raises(ValueError):
        datasets.device_image_batches(s, 2, 4, 'cpu')
    with pytest.raises(ValueError):
        datasets.device_image_batches(s, 4, 4, 'cuda:0')


# ---- the flag -----------------------------------------------------------------------------------------------------------
def test_patch_source_flag(tmp_path, capsys):
    from ml_super_resolution_amd.enet import experiment_train
    assert experiment_train.parse_flags([]).patch_source == 'host'
    assert experiment_train.parse_flags(['--patch_source', 'host']).patch_source == 'host'
    assert experiment_train.parse_flags(['--patch_source', 'device', '--train_dir_path', str(tmp_path)]).patch_source == 'device'
    npz = tmp_path / 'pairs.npz'
    npz.write_bytes(b'')
    for argv in (['--patch_source', 'gpu'], ['--patch_source', 'device'], ['--patch_source', 'device', '--train_dir_path', str(npz)],
                 ['--patch_source', 'device', '--train_dir_path', str(tmp_path / 'missing')]):
        with pytest.raises(SystemExit) as info:
            experiment_train.parse_flags(argv)
        assert info.value.code == 2
    assert '--patch_source device needs a directory' in capsys.readouterr().err
