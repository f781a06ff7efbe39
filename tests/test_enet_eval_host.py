"""The host side of EnhanceNet's whole-image pairs (srx_enet_eval_*; enet/datasets.py: DeviceEvalSet): the coefficient blocks
and the tile footprints against the oracle's Pillow tables, what srx_enet_eval_table_check accepts and refuses, the trimming
and the new flags.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.eval_tables import run_check

SIDES = (12, 16, 68, 132, 260)
SHAPES = ((12, 12), (16, 68), (64, 64), (68, 132), (132, 76))           # trimmed (height, width)
CHECK = 'srx_enet_eval_table_check'


def lib():
    from ml_super_resolution_amd import _lib
    return _lib.lib()


def oracle_tables(side):
    """(down bounds, down kk, up bounds, up kk) of an axis of `side` pixels by the oracle."""
    return O.pil_resample_coeffs(side, side // 4, 'bilinear') + O.pil_resample_coeffs(side // 4, side, 'bicubic')


def test_the_tile_constant_matches_the_header():
    import os
    import re
    from ml_super_resolution_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'srx.h')).read()
    assert int(re.search(r'#define SRX_ENET_EVAL_TILE (\d+)', text).group(1)) == _lib.ENET_EVAL_TILE
    assert _lib.ENET_EVAL_TILE % 4 == 0


@pytest.mark.parametrize('side', SIDES)
def test_coefficient_blocks_against_the_oracle(side):
    from ml_super_resolution_amd import ops
    block = ops.enet_eval_coeffs(side)
    s = side // 4
    assert block.dtype == np.int32 and len(block) == lib().srx_enet_eval_coeff_words(side) == 1 + 39 * s
    assert block[0] == side
    db, dk, ub, uk = oracle_tables(side)
    assert dk.shape == (s, 9) and uk.shape == (side, 5)
    at = 1
    for want in (db, dk, ub, uk):
        np.testing.assert_array_equal(block[at:at + want.size].reshape(want.shape), want)
        at += want.size
    assert at == len(block)
    assert (np.count_nonzero(dk, axis=1) <= 8).all() and (np.count_nonzero(uk, axis=1) <= 4).all()


def test_coefficient_entries_refuse_bad_sides():
    L = lib()
    for side in (0, 3, 13, -4, (1 << 20) + 4):
        assert L.srx_enet_eval_coeff_words(side) == -1
        assert L.srx_enet_eval_coeffs(side, None) != 0 and 'enet_eval_coeffs' in L.srx_last_error().decode()
    assert L.srx_enet_eval_coeffs(16, None) != 0 and 'enet_eval_coeffs: null block' in L.srx_last_error().decode()
    assert L.srx_enet_eval_coeff_words(4) == 40


@pytest.mark.parametrize('side', SIDES)
def test_footprints_against_the_oracle_bounds(side):
    """Every tile of the side: the sd range is the union of the BICUBIC taps of its hd pixels, the hd range the union of the
    BILINEAR taps of those sd pixels, enumerated pixel by pixel from the oracle's bounds."""
    from ml_super_resolution_amd import _lib
    T, L = _lib.ENET_EVAL_TILE, lib()
    db, _, ub, _ = oracle_tables(side)
    out = (ctypes.c_int * 4)()
    for tile in range(-(-side // T)):
        assert L.srx_enet_eval_footprint(side, tile, out) == 0, L.srx_last_error().decode()
        sd = sorted({int(ub[o, 0]) + k for o in range(tile * T, min(tile * T + T, side)) for k in range(int(ub[o, 1]))})
        hd = sorted({int(db[j, 0]) + k for j in sd for k in range(int(db[j, 1]))})
        assert list(out) == [sd[0], sd[-1], hd[0], hd[-1]], (side, tile)
        assert sd == list(range(sd[0], sd[-1] + 1)) and hd == list(range(hd[0], hd[-1] + 1))      # no hole in either range
    for bad_side, bad_tile in ((8, 0), (14, 0), (side, -1), (side, -(-side // T))):
        assert L.srx_enet_eval_footprint(bad_side, bad_tile, out) != 0 and 'enet_eval_footprint' in L.srx_last_error().decode()
    assert L.srx_enet_eval_footprint(side, 0, None) != 0 and 'enet_eval_footprint: null out' in L.srx_last_error().decode()


def packed_table(shapes=SHAPES):
    """(records, arena_bytes, (out_floats, sd_floats), coefficient arena) of `shapes` packed back to back."""
    from ml_super_resolution_amd import ops
    rec = ops.enet_eval_records(shapes)
    arena_bytes = sum(3 * h * w for h, w in shapes)
    return rec, arena_bytes, ops._enet_eval_floats(rec), ops._enet_eval_coeff_arena(ops._enet_eval_sides(rec)).copy()


def check(rec, arena_bytes, floats, coeffs, n=None, coeff_words=None):
    return run_check(CHECK, rec, arena_bytes, floats[0], floats[1], ctypes.c_void_p(coeffs.ctypes.data),
                     len(coeffs) if coeff_words is None else coeff_words, n=n)


def test_check_accepts_the_records_of_enet_eval_records():
    from ml_super_resolution_amd import _lib
    rec, arena_bytes, floats, coeffs = packed_table()
    assert check(rec, arena_bytes, floats, coeffs)[0] == 0, check(rec, arena_bytes, floats, coeffs)[1]
    T = _lib.ENET_EVAL_TILE
    assert lib().srx_enet_eval_tiles(ctypes.c_void_p(rec.ctypes.data), len(rec)) == sum(-(-h // T) * -(-w // T) for h, w in SHAPES)
    # the running sums: every record starts at a multiple of 4 floats, and some padding exists
    assert (rec['out_offset'] % 4 == 0).all() and (rec['sd_offset'] % 4 == 0).all()
    assert list(rec['sd_offset'][:3]) == [0, 28, 28 + 3 * 4 * 17]                                # 27 floats of the 3 x 3 sd padded to 28
    assert floats == (int(rec['out_offset'][-1]) + 3 * 132 * 76, int(rec['sd_offset'][-1]) + 3 * 33 * 19)
    # one block per distinct side, in increasing order; a record with height != width names two
    sides = sorted({v for hw in SHAPES for v in hw})
    words = np.cumsum([0] + [1 + 39 * (s // 4) for s in sides])
    assert len(coeffs) == words[-1]
    for r, (h, w) in zip(rec, SHAPES):
        assert (r['height_coeffs'], r['width_coeffs']) == (words[sides.index(h)], words[sides.index(w)])
        assert coeffs[r['height_coeffs']] == h and coeffs[r['width_coeffs']] == w


P = 'enet_eval_table_check: '
MULTIPLE = ': each side must be a multiple of 4 in 12..1048576'
PADDED = ', the floats of the entries before it padded to 4'


def refused(message, rec, arena_bytes, floats, coeffs, **kw):
    """The check refuses, and its whole message is P + `message`: a literal, as the build before the walks shared their
    running sums printed it."""
    rc, text = check(rec, arena_bytes, floats, coeffs, **kw)
    assert rc != 0 and text == P + message, (rc, text)


def test_check_refuses_what_the_shared_helpers_refuse():
    rec, arena_bytes, floats, coeffs = packed_table()
    L = lib()
    assert L.srx_enet_eval_table_check(None, 1, arena_bytes, floats[0], floats[1], ctypes.c_void_p(coeffs.ctypes.data), len(coeffs)) != 0
    assert L.srx_last_error().decode() == 'enet_eval_table_check: null table'
    refused('n 0 below 1', rec, arena_bytes, floats, coeffs, n=0)
    assert L.srx_enet_eval_table_check(ctypes.c_void_p(rec.ctypes.data), len(rec), arena_bytes, floats[0], floats[1], None, len(coeffs)) != 0
    assert L.srx_last_error().decode() == 'enet_eval_table_check: null coefficient arena'
    assert L.srx_enet_eval_tiles(None, 1) == 0 and L.srx_last_error().decode() == 'enet_eval_tiles: null table'


def test_check_refuses_both_arena_boundaries_and_offsets_near_2_to_the_64():
    rec, arena_bytes, floats, coeffs = packed_table()
    assert arena_bytes == 73008
    refused('entry 4: image of 30096 bytes at offset 42912 leaves the arena of 73007 bytes', rec, arena_bytes - 1, floats, coeffs)      # the end, by one byte
    for k, offset, message in ((4, int(rec['offset'][4]) + 1, 'entry 4: image of 30096 bytes at offset 42913'),
                               (0, arena_bytes - 431, 'entry 0: image of 432 bytes at offset 72577'),
                               (2, 2 ** 64 - 1, 'entry 2: image of 12288 bytes at offset 18446744073709551615'),
                               (2, 2 ** 64 - 3 * 64 * 64, 'entry 2: image of 12288 bytes at offset 18446744073709539328'),
                               (1, 2 ** 63, 'entry 1: image of 3264 bytes at offset 9223372036854775808')):
        bad = rec.copy()
        bad['offset'][k] = offset
        refused(message + ' leaves the arena of 73008 bytes', bad, arena_bytes, floats, coeffs)
    bad = rec.copy()
    bad['offset'][0] = arena_bytes - 432                                                        # the last place that fits: accepted
    assert check(bad, arena_bytes, floats, coeffs)[0] == 0
    for field, start in (('out_offset', 15984), ('sd_offset', 1000)):
        for value in (2 ** 64 - 1, 2 ** 64 - 4, 2 ** 63):
            bad = rec.copy()
            bad[field][3] = value
            refused('entry 3: %s %d is not %d' % (field, value, start) + PADDED, bad, arena_bytes, floats, coeffs)


def test_check_refuses_bad_sides_running_sums_tiles_and_totals():
    rec, arena_bytes, floats, coeffs = packed_table()
    for field, k, value, message in (('width', 1, 8, 'entry 1: image of 8 x 16 pixels'), ('height', 0, 4, 'entry 0: image of 12 x 4 pixels'),
                                     ('width', 2, 66, 'entry 2: image of 66 x 64 pixels'), ('height', 3, 67, 'entry 3: image of 132 x 67 pixels'),
                                     ('width', 0, 0, 'entry 0: image of 0 x 12 pixels'), ('height', 2, -64, 'entry 2: image of 64 x -64 pixels'),
                                     ('width', 4, (1 << 20) + 4, 'entry 4: image of 1048580 x 132 pixels')):
        bad = rec.copy()
        bad[field][k] = value
        refused(message + MULTIPLE, bad, arena_bytes, floats, coeffs)
    for field, start in (('out_offset', 3696), ('sd_offset', 232)):
        assert int(rec[field][2]) == start
        for delta in (-4, 1, 4):
            bad = rec.copy()
            bad[field][2] = start + delta
            refused('entry 2: %s %d is not %d' % (field, start + delta, start) + PADDED, bad, arena_bytes, floats, coeffs)
    bad = rec.copy()
    bad['sd_offset'][1] = 27                                                                    # the unpadded sum: not 16-byte aligned
    refused('entry 1: sd_offset 27 is not 28' + PADDED, bad, arena_bytes, floats, coeffs)
    for k, value, message in ((0, 1, 'entry 0: first_tile 1 is not the 0 tiles'), (3, int(rec['first_tile'][3]) + 1, 'entry 3: first_tile 9 is not the 8 tiles'),
                              (4, int(rec['first_tile'][4]) - 1, 'entry 4: first_tile 22 is not the 23 tiles')):
        bad = rec.copy()
        bad['first_tile'][k] = value
        refused(message + ' of the entries before it', bad, arena_bytes, floats, coeffs)
    bad = rec.copy()
    bad['reserved'][1] = 1
    refused('entry 1: reserved 1 is not 0', bad, arena_bytes, floats, coeffs)
    assert floats == (73008, 4565)
    for f, totals in (((floats[0] + 1, floats[1]), 'out_floats 73009 and sd_floats 4565'), ((floats[0], floats[1] + 4), 'out_floats 73008 and sd_floats 4569')):
        refused("the table's 5 entries end at float 73008 of hd and 4565 of sd, not at " + totals, rec, arena_bytes, f, coeffs)
    for f, message in (((floats[0] - 1, floats[1]), "entry 4: 30096 floats from out_offset 42912 on are more than the output's 73007"),
                       ((floats[0], floats[1] - 1), "entry 4: 1881 floats from sd_offset 2684 on are more than the output's 4564")):
        refused(message, rec, arena_bytes, f, coeffs)


def test_check_refuses_a_coefficient_block_of_another_side_or_outside_the_arena():
    from ml_super_resolution_amd import ops
    rec, arena_bytes, floats, coeffs = packed_table()
    bad = rec.copy()
    bad['width_coeffs'][1] = rec['width_coeffs'][3]                                             # the block of 132 for a width of 68
    assert (int(rec['width_coeffs'][3]), int(rec['width_coeffs'][2]), len(coeffs)) == (2306, 275, 3594)
    refused('entry 1: the width block at word 2306 was built for a side of 132, not 68', bad, arena_bytes, floats, coeffs)
    bad = rec.copy()
    bad['height_coeffs'][2] = rec['height_coeffs'][0]                                           # the block of 12 for a height of 64
    refused('entry 2: the height block at word 0 was built for a side of 12, not 64', bad, arena_bytes, floats, coeffs)
    refused('entry 3: the width block of 1288 words at word 2306 leaves the coefficient arena of 3593 words',
            rec, arena_bytes, floats, coeffs, coeff_words=len(coeffs) - 1)
    for value in (len(coeffs), len(coeffs) + 1, 2 ** 32 - 1):
        bad = rec.copy()
        bad['height_coeffs'][4] = value
        refused('entry 4: the height block of 1288 words at word %d leaves the coefficient arena of 3594 words' % value, bad, arena_bytes, floats, coeffs)
    # a block with the right side in front and bounds that are not a resample's: a count of 0, a tap outside the input, a
    # first index that decreases
    at = int(rec['width_coeffs'][2]) + 1                                                        # the body of the block of 64
    for word, value in ((at + 1, 0), (at + 2 * 15, 60), (at + 2 * 5, 0), (at + 11 * 16 + 2 * 63 + 1, 6), (at + 11 * 16 + 2 * 63, 15)):
        broken = coeffs.copy()
        broken[word] = value
        refused('entry 2: the bounds of the width block at word 275 are not those of a resample of 64 pixels', rec, arena_bytes, floats, broken)
    assert np.array_equal(coeffs[at - 1:at - 1 + 1 + 39 * 16], ops.enet_eval_coeffs(64))


def test_check_refuses_a_footprint_beyond_the_lds_layout():
    """A block whose bounds are a resample's in shape but reach further than Pillow's: every sd pixel reading 9 hd pixels
    from 0 on would be sane; one whose windows all start at 0 and end at the image's end is not a footprint the layout
    holds."""
    from ml_super_resolution_amd import ops
    rec, arena_bytes, floats, coeffs = packed_table(((260, 260),))
    s = 65
    wide = coeffs.copy()
    up = 1 + 11 * s                                                                             # the BICUBIC bounds [260][2]
    wide[up:up + 2 * 260:2] = np.minimum(np.arange(260) // 4, s - 5)                            # sane, monotone, and 5 taps everywhere
    wide[up + 1:up + 2 * 260:2] = 5
    assert check(rec, arena_bytes, floats, wide)[0] == 0                                        # still inside the layout
    down = 1
    wide[down:down + 2 * s:2] = np.minimum(np.arange(s) * 3, 260 - 9)                           # windows that drift away from 4 j
    wide[down + 1:down + 2 * s:2] = 9
    refused("entry 0: a tile's footprint (42 x 42 hd pixels, 12 x 12 sd pixels: 0 bytes) leaves the image or is beyond the LDS layout of 40960 bytes",
            rec, arena_bytes, floats, wide)


def test_device_eval_set_trims_and_refuses_by_name():
    from ml_super_resolution_amd.enet import datasets
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((70, 131), (13, 15))]
    trimmed, names = datasets.trimmed_eval_images(images, ['a.png', 'b.png'])
    assert [t.shape for t in trimmed] == [(68, 128, 3), (12, 12, 3)] and names == ['a.png', 'b.png']
    assert np.array_equal(trimmed[0], images[0][:68, :128]) and np.array_equal(trimmed[1], images[1][:12, :12])      # the top-left pixel stays
    packed, records = datasets.eval_records(trimmed)
    assert list(records['height']) == [68, 12] and list(records['width']) == [128, 12]
    assert len(packed[0]) == 3 * (68 * 128 + 12 * 12) and list(records['offset']) == [0, 3 * 68 * 128]
    with pytest.raises(ValueError, match=r'image small\.png of 11 x 40 pixels trims to 8 x 40: too small to score'):
        datasets.DeviceEvalSet([images[0], np.zeros((11, 40, 3), np.uint8)], 'cpu', names=['ok.png', 'small.png'])
    with pytest.raises(ValueError, match='image 0 of 40 x 11 '):
        datasets.DeviceEvalSet([np.zeros((40, 11, 3), np.uint8)], 'cpu')
    with pytest.raises(ValueError, match='uint8'):
        datasets.DeviceEvalSet([np.zeros((40, 40), np.uint8)], 'cpu')
    with pytest.raises(ValueError, match='no image'):
        datasets.DeviceEvalSet([], 'cpu')
    with pytest.raises(ValueError, match='names'):
        datasets.DeviceEvalSet([images[0]], 'cpu', names=['a', 'b'])


def test_device_eval_set_names_the_file_of_a_directory(tmp_path):
    from PIL import Image
    from ml_super_resolution_amd.enet import datasets
    Image.fromarray(np.zeros((40, 40, 3), np.uint8)).save(str(tmp_path / 'fine.png'))
    Image.fromarray(np.zeros((11, 40, 3), np.uint8)).save(str(tmp_path / 'tiny.png'))
    with pytest.raises(ValueError, match=r'image tiny\.png of 11 x 40 pixels'):
        datasets.DeviceEvalSet(str(tmp_path), 'cpu')


def test_new_flags_default_to_the_old_behaviour():
    from ml_super_resolution_amd.enet import experiment_evaluate, experiment_train
    f = experiment_train.parse_flags([])
    assert f.valid_dir_path is None and f.valid_every == 0
    f = experiment_train.parse_flags(['--valid_dir_path', 'd', '--valid_every', '5'])
    assert (f.valid_dir_path, f.valid_every) == ('d', 5)
    f = experiment_evaluate.parse_flags(['--source_ckpt_path', 'c', '--hd_dir_path', 'd'])
    assert (f.pairs, f.precision, f.target_dir_path) == ('host', 'highest', None)
    f = experiment_evaluate.parse_flags(['--source_ckpt_path', 'c', '--hd_dir_path', 'd', '--pairs', 'device', '--precision', 'high',
                                         '--target_dir_path', 't'])
    assert (f.pairs, f.precision, f.target_dir_path) == ('device', 'high', 't')
    with pytest.raises(SystemExit):
        experiment_evaluate.parse_flags(['--source_ckpt_path', 'c', '--hd_dir_path', 'd', '--pairs', 'elsewhere'])


def test_the_trainer_refuses_validation_without_a_directory():
    """The usage error comes before any GPU work."""
    from ml_super_resolution_amd.enet import experiment_train
    with pytest.raises(ValueError, match='--valid_every 2 needs --valid_dir_path'):
        experiment_train.main(['--valid_every', '2', '--stop_training_at_k_step', '0'])


HIPCC = '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_a_host_only_build_refuses(tmp_path):
    """pairs_api.hip built --cuda-host-only and linked without srx_api.hip and without the kernel units
    (tests/enet_eval_host_driver.cpp): the launcher and the coefficient routines are weak references, and the entries that
    need them refuse by name, as the enet_pairs ones do."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'enet_eval_host_driver')
    cmd = [HIPCC, '-O1', '-std=c++17', '--cuda-host-only', '--offload-arch=gfx950', '-Wl,--as-needed', '-Wno-unused-result',
           os.path.join(root, 'ml_super_resolution_amd', 'csrc', 'pairs_api.hip'), '-x', 'hip',
           os.path.join(root, 'tests', 'enet_eval_host_driver.cpp'), '-o', exe]
    build = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode(errors='replace')[-4000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    lines = run.stdout.decode().splitlines()
    assert run.returncode == 0 and len(lines) == 5, lines
    assert lines[0] == 'coeff_words 157'
    for line, text in zip(lines[1:], ('enet_eval_coeffs: this build has no resample unit', 'enet_eval_coeffs: this build has no resample unit',
                                      'enet_eval_pairs: this build has no eval-pair kernel', 'enet_pairs_tables: this build has no resample unit')):
        code, message = line.split(' ', 2)[1:]
        assert int(code) == -2 and message == text, line           # SRX_ERR_UNSUPPORTED
