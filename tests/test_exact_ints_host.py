"""Host tests of tests/exact_ints.py: that the two references of the integer tests agree exactly, and that the equality check
can fail -- each way a filter gradient goes subtly wrong is rejected and located.  No GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_enet as E
from tests import exact_ints as X
from tests.test_gpu_ops import SHAPES


def _layer(seed, n, h, w, kh, kw, cin, cout, pad):
    rng = np.random.default_rng(seed)
    x = X.ints(rng, (n, h, w, cin), 'x')
    wt = X.ints(rng, (kh, kw, cin, cout), 'w')
    b = X.ints(rng, (cout,), 'b')
    oh, ow = (h, w) if pad == 'SAME' else (h - kh + 1, w - kw + 1)
    dpre = X.ints(rng, (n, oh, ow, cout), 'dpre')
    return x, wt, b, dpre


# (N, H, W, KH, KW, Cin, Cout, padding): SAME and VALID, a 1x1 image, a 1x1 filter, an even filter (TF pads it unevenly),
# a non-square filter
ORACLE_SHAPES = [(2, 9, 11, 3, 3, 8, 5, 'SAME'), (1, 12, 10, 5, 5, 3, 4, 'VALID'), (1, 1, 1, 3, 3, 64, 64, 'SAME'),
                 (2, 7, 6, 1, 1, 16, 8, 'SAME'), (1, 8, 9, 4, 4, 4, 4, 'SAME'), (3, 10, 13, 3, 5, 6, 7, 'VALID')]


@pytest.mark.parametrize('shape', ORACLE_SHAPES, ids=lambda s: '%dx%dx%d_k%dx%d_%d-%d_%s' % s)
def test_float64_oracle_and_c_restatement_agree_exactly_on_integers(shape):
    n, h, w, kh, kw, cin, cout, pad = shape
    x, wt, b, dpre = _layer(sum(shape[:7]), *shape)
    skip = X.ints(np.random.default_rng(1), dpre.shape, 'skip')
    assert X.magnitude_ratio(O.conv2d_fwd(np.abs(x), np.abs(wt), np.abs(b), pad) + np.abs(skip)) < 1
    for act in (None, 'relu'):
        assert np.array_equal(O.c_conv2d_fwd(x, wt, b, pad, act), O.conv2d_fwd(x, wt, b, pad, act))
        assert np.array_equal(O.c_conv2d_fwd(x, wt, b, pad, act, skip=skip, post_relu=True), O.conv2d_fwd(x, wt, b, pad, act, skip=skip, post_relu=True))
    assert np.array_equal(O.c_conv2d_bwd_data(dpre, wt, (h, w), pad), O.conv2d_bwd_data(dpre, wt, (h, w), pad))
    dw_c, db_c = O.c_conv2d_bwd_filter(x, dpre, (kh, kw), pad)
    dw, db = O.conv2d_bwd_filter(x, dpre, (kh, kw), pad)
    assert np.array_equal(dw_c, dw) and np.array_equal(db_c, db)
    # ... and the selecting wrappers of the GPU tests return the same, whichever side of their threshold
    old = X.C_ORACLE_ABOVE
    try:
        for X.C_ORACLE_ABOVE in (0.0, float('inf')):
            assert np.array_equal(X.ref_fwd(x, wt, b, pad, 'relu'), O.conv2d_fwd(x, wt, b, pad, 'relu'))
            assert np.array_equal(X.ref_bwd_data(dpre, wt, (h, w), pad), O.conv2d_bwd_data(dpre, wt, (h, w), pad))
            assert np.array_equal(X.ref_bwd_filter(x, dpre, (kh, kw), pad)[0], dw)
    finally:
        X.C_ORACLE_ABOVE = old


@pytest.mark.parametrize('hw', [(8, 12), (7, 9), (6, 5), (1, 1)], ids=lambda s: '%dx%d' % s)
def test_strided_oracle_agrees_with_the_sampled_c_restatement_on_integers(hw):
    """Stride 2 through oracle_enet: a 3x3 SAME layer at stride 2 is the stride-1 layer sampled at the odd positions of an
    even-sized axis and the even positions of an odd-sized one, and its filter gradient that of the zero-stuffed gradient."""
    h, w = hw
    x, wt, b, _ = _layer(h * 31 + w, 2, h, w, 3, 3, 8, 12, 'SAME')
    oy, ox = 1 - h % 2, 1 - w % 2
    ref = E.conv2d_same_fwd(x, wt, b, 2)
    assert ref.shape == (2, (h + 1) // 2, (w + 1) // 2, 12)
    assert np.array_equal(O.c_conv2d_fwd(x, wt, b, 'SAME')[:, oy::2, ox::2], ref)
    dpre = X.ints(np.random.default_rng(5), ref.shape, 'dpre')
    stuffed = np.zeros((2, h, w, 12), np.float32)
    stuffed[:, oy::2, ox::2] = dpre
    dx, dw, db = E.conv2d_same_bwd(x, wt, dpre, 2)
    dw_c, db_c = O.c_conv2d_bwd_filter(x, stuffed, (3, 3), 'SAME')
    assert np.array_equal(dw_c, dw) and np.array_equal(db_c, db)
    assert np.array_equal(O.c_conv2d_bwd_data(stuffed, wt, (h, w), 'SAME'), dx)


def _wgrad_case():
    x, _, _, dpre = _layer(77, 2, 9, 11, 3, 3, 8, 5, 'SAME')
    dw, _ = O.conv2d_bwd_filter(x, dpre, (3, 3), 'SAME')
    mag, _ = O.conv2d_bwd_filter(np.abs(x), np.abs(dpre), (3, 3), 'SAME')
    return x, dpre, dw, mag


def test_assert_exact_accepts_the_oracle_itself_and_minus_zero():
    x, dpre, dw, mag = _wgrad_case()
    ratio = X.assert_exact(dw.astype(np.float32), dw, mag, 'dw', 'hwio')
    assert 0 < ratio < 1e-3
    z = np.zeros((1, 2, 2, 3))
    X.assert_exact(-z.astype(np.float32), z, z + 1, 'zeros', 'nhwc')
    tally = {}
    X.assert_exact(dw, dw, mag + 0.5, 'dw', 'hwio', unit=0.5, tally=tally)
    assert tally == {'magnitude': X.magnitude_ratio(mag + 0.5, 0.5), 'checks': 1}


def test_assert_exact_rejects_one_element_off_by_one_and_names_it():
    x, dpre, dw, mag = _wgrad_case()
    bad = dw.copy()
    bad[1, 2, 3, 4] += 1
    with pytest.raises(AssertionError) as e:
        X.assert_exact(bad, dw, mag, 'dw', 'hwio')
    msg = str(e.value)
    assert '1 of %d elements differ' % dw.size in msg
    assert 'kh 1, kw 2, ci 3, co 4: got %r, want %r, difference 1.0' % (float(bad[1, 2, 3, 4]), float(dw[1, 2, 3, 4])) in msg
    assert 'all of them in: kh 1, kw 2, ci 3, co 4' in msg


def test_assert_exact_rejects_two_swapped_taps():
    x, dpre, dw, mag = _wgrad_case()
    bad = dw.copy()
    bad[0, 1], bad[1, 0] = dw[1, 0], dw[0, 1]
    assert not np.array_equal(dw[0, 1], dw[1, 0])
    with pytest.raises(AssertionError) as e:
        X.assert_exact(bad, dw, mag, 'dw', 'hwio')
    msg = str(e.value)
    assert 'kh 0, kw 1, ci 0' in msg                                # the first of them
    assert 'all of them in: no single row, column, tap or channel' in msg
    differing = int((bad != dw).sum())
    assert '%d of %d elements differ' % (differing, dw.size) in msg and differing > 40


def test_assert_exact_rejects_one_removed_contribution_and_names_the_tap():
    """One (pixel, tap) pair left out of the sum: what a filter-gradient walk that drops a row's last position does."""
    x, dpre, dw, mag = _wgrad_case()
    n, oh, ow, kh, kw = 1, 4, 10, 0, 0                            # the last output pixel of row 4 with input pixel (3, 9)
    contribution = np.outer(x[n, oh + kh - 1, ow + kw - 1].astype(np.float64), dpre[n, oh, ow].astype(np.float64))
    assert np.abs(contribution).max() >= 1
    bad = dw.copy()
    bad[kh, kw] -= contribution
    with pytest.raises(AssertionError) as e:
        X.assert_exact(bad, dw, mag, 'dw', 'hwio')
    msg = str(e.value)
    assert '%d of %d elements differ' % (int((contribution != 0).sum()), dw.size) in msg
    assert 'all of them in: kh 0, kw 0' in msg


def test_assert_exact_rejects_a_fake_position_leaking_a_one():
    """A pad slot or fake position that holds 1 instead of 0 in one input channel, paired with a real upstream gradient."""
    x, dpre, dw, mag = _wgrad_case()
    bad = dw.copy()
    bad[2, 1, 6, :] += 1.0 * dpre[0, 8, 3]                        # (the row below the image, seen by tap row 2)
    assert np.abs(dpre[0, 8, 3]).max() >= 1
    with pytest.raises(AssertionError) as e:
        X.assert_exact(bad, dw, mag, 'dw', 'hwio')
    assert 'all of them in: kh 2, kw 1, ci 6' in str(e.value)


def test_assert_exact_locates_a_wrong_row_of_an_activation_and_non_finite_values():
    x, wt, b, _ = _layer(3, 2, 9, 11, 3, 3, 8, 5, 'SAME')
    y = O.conv2d_fwd(x, wt, b, 'SAME', 'relu')
    mag = O.conv2d_fwd(np.abs(x), np.abs(wt), np.abs(b), 'SAME')
    bad = y.copy()
    bad[1, 8] = O.conv2d_fwd(x, wt, b, 'SAME', 'relu')[1, 7]      # the last row repeats the one above
    with pytest.raises(AssertionError) as e:
        X.assert_exact(bad, y, mag, 'y', 'nhwc')
    assert 'all of them in: image 1, row 8' in str(e.value)
    bad = y.copy()
    bad[0, 0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match=r'1 non-finite'):
        X.assert_exact(bad, y, mag, 'y', 'nhwc')


def test_assert_exact_refuses_to_compare_when_exactness_is_not_guaranteed():
    x, dpre, dw, mag = _wgrad_case()
    big = mag.copy()
    big[0, 0, 0, 0] = 2.0 ** 24
    with pytest.raises(AssertionError, match='cannot compare exactly.*use smaller operands'):
        X.assert_exact(dw, dw, big, 'dw', 'hwio')
    # half-integer terms halve the room
    with pytest.raises(AssertionError, match='cannot compare exactly'):
        X.assert_exact(dw, dw, np.full(dw.shape, 2.0 ** 23), 'dw', 'hwio', unit=0.5)
    with pytest.raises(AssertionError, match='not a multiple'):
        X.assert_exact(dw + 0.5, dw + 0.5, mag + 0.5, 'dw', 'hwio')
    # a magnitude that is not the reference's own operation on |operands|
    with pytest.raises(AssertionError, match='exceeds its magnitude'):
        X.assert_exact(dw, dw, np.zeros(dw.shape), 'dw', 'hwio')


def test_the_gap_the_integer_tests_close():
    """The "one contribution removed" error in `close`'s terms (max-norm error against 1e-3 of the tensor's largest value)
    on the random-float operands of tests/test_gpu_ops.test_conv_fwd_bwd_vs_oracle, at the SHAPES entries with the most
    terms per tap (n = N * OH * OW).  A measurement, printed and written down here, not a threshold.  The error of a
    removed pixel is its largest product |x[ci]| |dpre[co]|, as a multiple of `close`'s threshold 1e-3 * max|dw|:

        40x41x41 3x3 3 -> 64   n = 67,240   median pixel 3.1 x   largest pixel 7.5 x   (threshold 0.63)
        40x41x41 3x3 64 -> 3   n = 67,240   median pixel 2.3 x   largest pixel 8.0 x   (threshold 0.55)
        37x41x41 3x3 64 -> 64  n = 62,197   median pixel 4.2 x   largest pixel 8.9 x   (threshold 0.60)

    So at these shapes `close` sees a dropped pixel of ordinary size with a margin of 2 to 4, and misses what is smaller
    than a third of one: a pad slot or fake position leaking 0.1 (0.2 to 0.4 x), a pixel counted with a neighbour's small
    operand.  max|dw| grows like sqrt(n): at the recipe batch of tests/test_gpu_wgrad_strip.py (n = 1,048,576) the same
    dropped pixel is at 0.6 to 1.1 x, under the threshold.  On integers any of these changes a tap by at least 1, and the
    comparison is equality."""
    big = sorted((s for s in SHAPES if s[3] == 3), key=lambda s: -s[0] * s[1] * s[2])[:3]
    assert [s[:6] for s in big] == [(40, 41, 41, 3, 3, 64), (40, 41, 41, 3, 64, 3), (37, 41, 41, 3, 64, 64)]
    for (N, H, W, k, cin, cout, pad, _) in big:
        rng = np.random.default_rng(N + cin + cout)
        x = rng.uniform(-1, 1, (N, H, W, cin)).astype(np.float32)
        dpre = rng.normal(0, 1, (N, H, W, cout)).astype(np.float32)
        dw, _ = O.c_conv2d_bwd_filter(x, dpre, (k, k), pad)
        scale = float(np.abs(dw).max())
        px = np.abs(x).reshape(-1, cin).max(axis=1) * np.abs(dpre).reshape(-1, cout).max(axis=1)      # per pixel: its largest product
        print('%dx%dx%d %d->%d: one removed contribution is at most %.3f (median %.4f) of 1e-3 * max|dw| = %.3g'
              % (N, H, W, cin, cout, px.max() / (1e-3 * scale), np.median(px) / (1e-3 * scale), 1e-3 * scale))
        assert np.isfinite(scale) and scale > 0
