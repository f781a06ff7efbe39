"""CPU-side checks of the fused image scores (srx_image_scores): the exports and header constants, every refusal that
comes before a launch, the tile plan and the scratch formula, and scores_ref -- the numpy restatement of what one call
computes (clip, then the sub-pixel reshape, then Y, in float64, scored by oracle.psnr / oracle.ssim).  The GPU tests
(tests/test_gpu_image_scores.py) import scores_ref, the descriptor helper and the plan-derived edge shapes from here."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests.conftest import ROOT

BAD_ARG, UNSUPPORTED = -1, -2
Y_WEIGHTS = np.array([0.299, 0.587, 0.114])


def desc(shape, n_cand=1, space=0, unit_clip=0, max_val=1.0):
    from ml_super_resolution_amd import _lib
    N, H, W, C = shape
    return _lib.ScoresDesc(N, H, W, C, n_cand, space, unit_clip, max_val)


def plan(d):
    from ml_super_resolution_amd import _lib
    v = [ctypes.c_int(-1) for _ in range(4)]
    rc = _lib.lib().srx_image_scores_plan(ctypes.byref(d), *[ctypes.byref(x) for x in v])
    assert rc == 0, _lib.lib().srx_last_error()
    return tuple(x.value for x in v)


def effective(x, d):
    """The effective image of [N,H,W,C] under a descriptor, float64: clip, then the reshape, then Y."""
    x = np.asarray(x, np.float64)
    if d.unit_clip:
        x = np.clip(x * 0.5 + 0.5, 0.0, 1.0)
    if d.space == 1:
        n, h, w, c = x.shape
        x = (x.reshape(n, h, w * (c // 3), 3) * Y_WEIGHTS).sum(-1, keepdims=True)
    return x


def scores_ref(ref, cands, d):
    """[n_cand, N, 2] float64: (psnr, ssim) of every candidate against ref on the effective images."""
    a = effective(ref, d)
    return np.stack([np.stack([O.psnr(a, effective(b, d), d.max_val), O.ssim(a, effective(b, d), d.max_val)], -1)
                     for b in cands])


def noise_inputs(shape, n_cand, seed):
    """The issue's inputs: a uniform in (-1.1, 1.1), candidates a + 0.15 normal."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.1, 1.1, shape).astype(np.float32)
    return a, [(a + 0.15 * rng.standard_normal(shape)).astype(np.float32) for _ in range(n_cand)]


def edge_shapes():
    """(N,H,W,C) from the plan's own tile.  C = 1 (a window column is one float): every pair of H - 10 and W - 10 at 1,
    tile - 1, tile, tile + 1 and 2 tile + 1.  C = 3 (tap stride 3): (W - 10) * 3 at the multiples of 3 next below and
    above tile_w, at exactly 3 tile_w (whole tiles) and at 3 tile_w + 3, with H - 10 at tile_h and tile_h + 1."""
    tile_h, tile_w, _, _ = plan(desc((1, 11, 11, 1)))
    hs = [1, tile_h - 1, tile_h, tile_h + 1, 2 * tile_h + 1]
    ws = [1, tile_w - 1, tile_w, tile_w + 1, 2 * tile_w + 1]
    shapes = [(1, h + 10, w + 10, 1) for h in hs for w in ws]
    for k, w3 in enumerate((tile_w // 3, tile_w // 3 + 1, tile_w, tile_w + 1)):
        shapes.append((1, tile_h + k % 2 + 10, w3 + 10, 3))
    return shapes


def test_exports_and_header_constants():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'srx.h')).read()
    for name in ('srx_image_scores_scratch_bytes', 'srx_image_scores_plan', 'srx_image_scores_lds_bytes', 'srx_image_scores'):
        assert hasattr(L, name) and name in _lib.EXPORTS and name in header, name

    def const(name):
        return int(re.search(r'#define\s+%s\s+(\d+)' % name, header).group(1))
    assert const('SRX_SCORES_MAX_CAND') == _lib.SCORES_MAX_CAND == 4
    assert (const('SRX_SCORES_RGB'), const('SRX_SCORES_Y')) == (_lib.SCORES_RGB, _lib.SCORES_Y) == (0, 1)
    assert const('SRX_SCORES_MAX_TAP_STRIDE') == _lib.SCORES_MAX_TAP_STRIDE
    assert ctypes.sizeof(_lib.ScoresDesc) == 32


REFUSED = (
    # descriptor, words of the reason
    (dict(shape=(0, 20, 20, 3)), b'N 0 outside'),
    (dict(shape=(65536, 20, 20, 3)), b'N 65536 outside'),
    (dict(shape=(1, 20, 20, 0)), b'C 0 is below 1'),
    (dict(shape=(1, 20, 20, 3), n_cand=0), b'n_cand 0 outside'),
    (dict(shape=(1, 20, 20, 3), n_cand=5), b'n_cand 5 outside'),
    (dict(shape=(1, 20, 20, 3), space=2), b'space 2'),
    (dict(shape=(1, 20, 20, 3), space=-1), b'space -1'),
    (dict(shape=(1, 20, 20, 4), space=1), b'C % 3 == 0'),
    (dict(shape=(1, 20, 20, 3), unit_clip=2), b'unit_clip 2'),
    (dict(shape=(1, 20, 20, 3), unit_clip=-1), b'unit_clip -1'),
    (dict(shape=(1, 10, 20, 3)), b'at least 11'),
    (dict(shape=(1, 20, 10, 3)), b'at least 11'),
    (dict(shape=(1, 20, 3, 9), space=1), b'at least 11'),           # We = 3 * 9 / 3 = 9
    (dict(shape=(1, 20, 20, 3), max_val=float('nan')), b'max_val'),
    (dict(shape=(1, 20, 20, 3), max_val=float('inf')), b'max_val'),
    (dict(shape=(1, 20, 20, 3), max_val=0.0), b'max_val'),
    (dict(shape=(1, 20, 20, 3), max_val=-1.0), b'max_val'),
    (dict(shape=(1, 20, 20, 47)), b'above 46'),                     # the halo of 10 C columns leaves the LDS
    (dict(shape=(1, 20, 1 << 11, 3 << 20), space=1), b'overflow'),  # W * C = 3 * 2^31
    (dict(shape=(1, 0x7fffffff, 20, 3)), b'overflow'),              # H + a tile's overhang leaves int32
    (dict(shape=(1, 0x7fff0000, 1 << 30, 1)), b'overflow'),         # 2^27 x 2^23 tiles
)


@pytest.mark.parametrize('kw,reason', REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_descriptor_refusals_name_their_reason(kw, reason):
    """Refused by all three functions before any launch; the pointers are never dereferenced (no GPU here)."""
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    d = desc(**kw)
    ref, out, scratch = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
    cand = (ctypes.c_void_p * 4)(0x40000, 0x50000, 0x60000, 0x70000)
    rc = L.srx_image_scores(ctypes.byref(d), ref, cand, out, scratch, None)
    msg = L.srx_last_error()
    assert rc in (BAD_ARG, UNSUPPORTED) and b'image_scores:' in msg and reason in msg, (rc, msg)
    assert L.srx_image_scores_scratch_bytes(ctypes.byref(d)) == 0
    msg = L.srx_last_error()
    assert b'image_scores_scratch_bytes:' in msg and reason in msg, msg
    assert L.srx_image_scores_lds_bytes(ctypes.byref(d)) == 0
    msg = L.srx_last_error()
    assert b'image_scores_lds_bytes:' in msg and reason in msg, msg
    v = [ctypes.c_int(-1) for _ in range(4)]
    assert L.srx_image_scores_plan(ctypes.byref(d), *[ctypes.byref(x) for x in v]) == rc
    assert b'image_scores_plan:' in L.srx_last_error() and [x.value for x in v] == [-1] * 4


def test_null_pointers_are_refused():
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    d = desc((1, 20, 20, 3), n_cand=2)
    ref, out, scratch = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
    cand = (ctypes.c_void_p * 2)(0x40000, 0x50000)
    for args in ((None, ref, cand, out, scratch), (ctypes.byref(d), None, cand, out, scratch),
                 (ctypes.byref(d), ref, None, out, scratch), (ctypes.byref(d), ref, cand, None, scratch),
                 (ctypes.byref(d), ref, cand, out, None)):
        assert L.srx_image_scores(*args, None) == BAD_ARG
        assert b'image_scores: null pointer' in L.srx_last_error()
    hole = (ctypes.c_void_p * 2)(0x40000, None)
    assert L.srx_image_scores(ctypes.byref(d), ref, hole, out, scratch, None) == BAD_ARG
    assert b'null pointer (candidate 1)' in L.srx_last_error()
    assert L.srx_image_scores_scratch_bytes(None) == 0 and b'null descriptor' in L.srx_last_error()
    v = [ctypes.c_int(-1) for _ in range(4)]
    assert L.srx_image_scores_plan(None, *[ctypes.byref(x) for x in v]) == BAD_ARG
    assert L.srx_image_scores_plan(ctypes.byref(d), None, ctypes.byref(v[1]), ctypes.byref(v[2]), ctypes.byref(v[3])) == BAD_ARG


def _check_plan(d, win_rows, win_floats):
    from ml_super_resolution_amd import _lib
    tile_h, tile_w, tiles_y, tiles_x = plan(d)
    assert tile_h >= 1 and tile_w >= 1 and tiles_y >= 1 and tiles_x >= 1
    assert tiles_y * tile_h >= win_rows > (tiles_y - 1) * tile_h, (tile_h, tiles_y, win_rows)
    assert tiles_x * tile_w >= win_floats > (tiles_x - 1) * tile_w, (tile_w, tiles_x, win_floats)
    # the documented formula: two floats per (image, candidate, tile)
    assert _lib.lib().srx_image_scores_scratch_bytes(ctypes.byref(d)) == d.N * d.n_cand * tiles_y * tiles_x * 2 * 4
    # the documented LDS layout: 16 weights, two staged halo regions, three moment planes, 8 floats of block sums
    Ce = 1 if d.space == 1 else d.C
    lds = _lib.lib().srx_image_scores_lds_bytes(ctypes.byref(d))
    assert lds == 4 * (16 + 2 * (tile_h + 10) * (tile_w + 10 * Ce) + 3 * (tile_h + 10) * tile_w + 8) <= 160 * 1024


def test_plan_covers_the_window_grid_and_not_with_one_tile_fewer():
    tile_h, tile_w, _, _ = plan(desc((1, 11, 11, 1)))
    for dh in (1, tile_h - 1, tile_h, tile_h + 1, 2 * tile_h + 1):
        for dw in (1, tile_w - 1, tile_w, tile_w + 1, 2 * tile_w + 1):
            _check_plan(desc((3, dh + 10, dw + 10, 1), n_cand=2), dh, dw)
    # C = 3: (We - 10) * 3 at the multiples of 3 at or next above the same five values
    for target in (1, tile_w - 1, tile_w, tile_w + 1, 2 * tile_w + 1):
        dw = -(-target // 3) * 3
        _check_plan(desc((2, 30, dw // 3 + 10, 3), n_cand=4), 20, dw)
    _check_plan(desc((1, 1080, 1920, 3), n_cand=2), 1070, 1910 * 3)
    # Y: [H, W, 27] is scored as [H, 9 W, 1]
    _check_plan(desc((1, 170, 170, 27), space=1, unit_clip=1), 160, 170 * 9 - 10)
    _check_plan(desc((2, 23, 19, 12), n_cand=3, space=1), 13, 19 * 4 - 10)
    assert len(edge_shapes()) == 29


def test_scores_ref_reads_the_pixels_the_reference_reshape_reads():
    """On a label made by space_to_depth_numpy the Y space scores the image [h, w r^2, 3] that the reference's reshape
    produces (espcn/espcn/experiment_test.py:39-52): consecutive triples of a row of w * 3 r^2 floats."""
    from ml_super_resolution_amd.espcn.experiment_test import space_to_depth_numpy
    rng = np.random.default_rng(3)
    for r in (2, 3):
        hr = rng.uniform(-1, 1, (13 * r, 12 * r, 3))
        other = hr + 0.1 * rng.standard_normal(hr.shape)
        label, cand = space_to_depth_numpy(hr, r)[None], space_to_depth_numpy(other, r)[None]
        assert label.shape == (1, 13, 12, 3 * r * r)
        d = desc(label.shape, space=1, unit_clip=1)
        # the reference's steps, written out: clip, tf.reshape, rgb_to_yuv's first channel
        def ref_y(x):
            x = np.clip(x * 0.5 + 0.5, 0.0, 1.0)
            x = np.reshape(x, [1, 13, 12 * r * r, 3])
            return (x @ Y_WEIGHTS)[..., None]
        np.testing.assert_array_equal(effective(label, d).shape, (1, 13, 12 * r * r, 1))
        np.testing.assert_allclose(effective(label, d), ref_y(label), rtol=0, atol=1e-15)
        # pixel (y, x r^2 + k) of the reshaped image is sub-pixel k of label pixel (y, x): the hr pixel (y r + k // r, x r + k % r)
        img = np.reshape(label, [13, 12 * r * r, 3])
        for y, x, k in ((0, 0, 0), (5, 7, r * r - 1), (12, 11, r)):
            np.testing.assert_array_equal(img[y, x * r * r + k], hr[y * r + k // r, x * r + k % r])
        got = scores_ref(label, [cand], d)
        assert abs(got[0, 0, 0] - O.psnr(ref_y(label), ref_y(cand), 1.0)[0]) < 1e-12
        assert abs(got[0, 0, 1] - O.ssim(ref_y(label), ref_y(cand), 1.0)[0]) < 1e-12


def test_fixture_can_see_a_missing_clip():
    """a in (-1.1, 1.1) leaves [-1, 1]: scoring without the clip moves both numbers by far more than the GPU tests'
    tolerances (1e-4 on SSIM, 1e-5 relative on PSNR)."""
    a, cands = noise_inputs((2, 23, 19, 12), 1, seed=11)
    for space in (0, 1):
        clipped = scores_ref(a, cands, desc(a.shape, space=space, unit_clip=1))
        d = desc(a.shape, space=space, unit_clip=0)
        unclipped = scores_ref(a * 0.5 + 0.5, [cands[0] * 0.5 + 0.5], d)
        assert np.all(np.abs(clipped[..., 0] - unclipped[..., 0]) > 1e-2 * np.abs(clipped[..., 0])), (clipped, unclipped)
        assert np.all(np.abs(clipped[..., 1] - unclipped[..., 1]) > 1e-3), (clipped, unclipped)
