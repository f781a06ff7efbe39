"""Host tests of tests/exact_ints.py: that the two references of the integer tests agree exactly, and that the equality check
can fail -- each way a filter gradient goes subtly wrong is rejected and located; and of its operands with low parts (the
bf16x3 routes, tests/test_gpu_exact_bf16x3_parts.py): the generator's conditions, the two identities the GPU module rests on,
every row of its tables under the magnitude condition, and what its shapes reach in the tile planner.  No GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_enet as E
from tests import exact_ints as X
from tests import test_gpu_exact_bf16x3_parts as P
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


# ---- operands with low parts: the bf16x3 routes ---------------------------------------------------------------------------
def test_bf16_split_of_integers_is_exact_up_to_17_bits_and_no_further():
    """Every integer of up to 17 bits, not a sample: hi + lo == v with integer parts.  At 18 bits v - hi no longer fits bf16.
    wide_ints asserts the same of what it draws and refuses widths outside [MIN_WIDE_BITS, MAX_WIDE_BITS]."""
    v = np.arange(-(2 ** 17 - 1), 2 ** 17, dtype=np.float32)
    hi, lo = X.split_bf16(v)
    assert np.array_equal(hi + lo, v.astype(np.float64)) and np.array_equal(lo, np.round(lo))
    assert np.abs(lo).max() == 256 and not X.split_bf16(np.arange(-255, 256, dtype=np.float32))[1].any()
    v18 = np.arange(2 ** 17, 2 ** 18, dtype=np.float32)
    hi, lo = X.split_bf16(v18)
    assert not np.array_equal(hi + lo, v18.astype(np.float64))
    assert (X.MIN_WIDE_BITS, X.MAX_WIDE_BITS) == (11, 17)
    for bits in (10, 18):
        with pytest.raises(AssertionError, match='wide operands take'):
            X.wide_ints(np.random.default_rng(0), (8,), bits)


def test_wide_ints_have_low_parts_in_most_elements():
    """The share of lo != 0 by width, on 200,000 draws: at least half from 11 bits on (the GPU module's floor for a wide
    operand), a quarter at 9 bits.  A sparse draw reports the share among its nonzero elements."""
    rng = np.random.default_rng(11)
    want = {11: 0.69, 12: 0.81, 14: 0.94, 15: 0.97}
    for bits, share in want.items():
        v, got = X.wide_ints(rng, (200000,), bits)
        assert np.abs(v).max() <= 2 ** bits - 1 and v.dtype == np.float32
        assert abs(got - share) < 0.01 and got >= 0.5, (bits, got)
    nine = rng.integers(-511, 512, size=200000).astype(np.float32)
    assert abs(X.lo_share(nine) - 0.25) < 0.01
    v, got = X.wide_ints(rng, (200000,), 12, density=1.0 / 16)
    assert abs((v != 0).mean() - 1.0 / 16) < 0.005 and abs(got - 0.81) < 0.02
    assert X.lo_share(np.zeros(4, np.float32)) == 0.0


def _bilinear_ops(h, w):
    return {'fwd': lambda a, b: O.conv2d_fwd(a, b, None, 'SAME'),
            'dgrad': lambda a, b: O.conv2d_bwd_data(a, b, (h, w), 'SAME'),
            'wgrad': lambda a, b: O.conv2d_bwd_filter(a, b, (3, 3), 'SAME')[0]}


@pytest.mark.parametrize('shape,bits', [((2, 5, 7), 15), ((1, 9, 30), 15), ((1, 3, 4), 12)], ids=lambda v: str(v).replace(' ', ''))
def test_three_terms_are_the_product_itself_when_one_operand_is_narrow(shape, bits):
    """xh*w + xl*w == x*w in every operation and in both roles: the oracle of the parts equals the float64 oracle of the
    unsplit operands, and the magnitude over the parts is at least the one over |x| (|hi| + |lo| >= |x|)."""
    n, h, w = shape
    rng = np.random.default_rng(bits * 1000 + h)
    sa, sw = (n, h, w, 64), (3, 3, 64, 64)
    for name, op in _bilinear_ops(h, w).items():
        sb = sa if name == 'wgrad' else sw
        for wide in 'ab':
            a = X.wide_ints(rng, sa, bits)[0] if wide == 'a' else X.ints(rng, sa, 'x', 3)
            b = X.wide_ints(rng, sb, bits)[0] if wide == 'b' else X.ints(rng, sb, 'w')
            whole = op(a, b)
            assert np.array_equal(X.three_term(op, a, b), whole), (name, wide)
            mag, plain = X.split_magnitude(op, a, b), op(np.abs(a), np.abs(b))
            assert (mag >= plain).all() and (mag > plain).any() and mag.max() < 1.01 * plain.max()
            assert X.magnitude_ratio(mag) < 1


@pytest.mark.parametrize('shape,row', [c for c in P.LAYER_CASES if c[1].wide == 'ab'], ids=P._ids([c for c in P.LAYER_CASES if c[1].wide == 'ab']))
def test_both_wide_rows_pin_three_terms_not_four(shape, row):
    """Both operands wide: the reference of the GPU module's row is the three-term sum, exact under its magnitude (the
    Expected constructor), and differs from the full product -- the dropped lo*lo -- in a good share of the elements."""
    c = P.build(shape, 64, 64, row)
    assert row.bits >= X.MIN_WIDE_BITS and c.share >= 0.5
    op = _bilinear_ops(*shape[1:])[row.op]
    e = c.e['dw' if row.op == 'wgrad' else 'none']
    three = e.ref - (c.bias if row.op == 'fwd' else 0.0)
    full = op(c.a, c.b)
    al, bl = X.split_bf16(c.a)[1], X.split_bf16(c.b)[1]
    assert np.array_equal(full - three, op(al, bl))
    differ = float((full != three).mean())
    print('%s: magnitude / 2^24 = %.3f, three terms differ from the product in %.0f %% of the elements' % (c.tag, e.ratio, 100 * differ))
    assert differ > 0.25 and e.ratio < 1


def _table_groups():
    groups = [('layer %dx%dx%d' % s, [(s, 64, 64, r, True) for (s2, r) in P.LAYER_CASES if s2 == s]) for s in P.LAYER_SHAPES]
    groups += [('blocked %dx%d' % b, [(s, 64 * b[0], 64 * b[1], r, False) for (b2, s, r) in P.BLOCKED_CASES if b2 == b]) for b in P.BLOCKED]
    groups += [('BlockedConv', [(P.BLOCKED_CONV_SHAPE, c, c, r, False) for (c, r) in P.BLOCKED_CONV_CASES])]
    return groups


@pytest.mark.parametrize('name,rows', _table_groups(), ids=[g[0].replace(' ', '_') for g in _table_groups()])
def test_every_row_of_the_gpu_tables_can_be_compared_exactly(name, rows):
    """The tables of tests/test_gpu_exact_bf16x3_parts.py, imported: every row's operands satisfy the generator's conditions
    (>= 11 bits, an exact split, lo != 0 in at least half of a wide operand: asserted by build) and every reference passes
    the Expected constructor, which carries magnitude < 2^24 -- from the oracle alone.  A row that cannot be compared exactly
    fails here."""
    assert rows
    worst, least = 0.0, 1.0
    for shape, cin, cout, row, decay in rows:
        c = P.build(shape, cin, cout, row, decay=decay)
        assert row.bits >= X.MIN_WIDE_BITS and c.e
        worst, least = max([worst] + [e.ratio for e in c.e.values()]), min(least, c.share)
    print('%s: %d rows, largest magnitude / 2^24 = %.3f, smallest share of lo != 0 = %.2f' % (name, len(rows), worst, least))
    assert worst < 1 and least >= 0.5


def test_gpu_tables_hold_the_cases_they_are_meant_to():
    rows = lambda s: [r for (s2, r) in P.LAYER_CASES if s2 == s]
    for s in P.LAYER_SHAPES:
        have = {(r.op, r.wide) for r in rows(s)}
        assert {(op, wide) for op in ('fwd', 'dgrad', 'wgrad') for wide in 'ab'} <= have, s
        assert ({(op, 'ab') for op in ('fwd', 'dgrad', 'wgrad')} <= have) == (s in P.BOTH_WIDE_SHAPES)
    assert P.LAYER_SHAPES[:5] == [(1, 1, 1), (2, 5, 7), (3, 41, 41), (1, 9, 130), (600, 1, 2)]
    assert set(P.BLOCKED) == {(1, 2), (2, 2), (2, 4), (8, 8)} and P.BLOCKED[(8, 8)] == [(1, 1, 1), (2, 5, 7)]
    assert all(P.BLOCKED[b] == [(1, 1, 1), (2, 5, 7), (3, 16, 16), (1, 8, 130)] for b in ((1, 2), (2, 2), (2, 4)))
    fifteen = [c for c in P.LAYER_CASES + P.BLOCKED_CASES if c[-1].bits == 15]
    assert {c[-1].op for c in fifteen if len(c) == 2} == {'fwd', 'dgrad', 'wgrad'} and {c[-1].op for c in fifteen if len(c) == 3} == {'fwd', 'wgrad'}


def test_leaky_relu_restatement_is_one_float32_rounding():
    """float32(0.2) * v has at most 48 significant bits: float64 holds it exactly, so rounding it to float32 is the one
    rounding of the fp32 multiply; positive values and zero pass unchanged."""
    v = np.array([-7.0, -1.0, 0.0, 3.0, -16777215.0, 12345678.0, -4095.0 * 576])
    got = P.lrelu32(v)
    assert got.dtype == np.float32
    assert np.array_equal(got, np.where(v > 0, v, np.float64(np.float32(0.2)) * v).astype(np.float32))
    assert got[0] == np.float32(-1.4) and got[3] == 3.0 and got[2] == 0.0


def _bf16x3_plan(N, H, W, max_grid, wgrad):
    """csrc/srx_api.hip's bf16x3_plan, restated: TH, TW, tile counts and grid."""
    max_slots = 80 * 1024 // (288 if wgrad else 272)
    best, plan = 1e300, None
    for TW in (W, 16, 24, 32, 48, 64):
        if TW > W or TW < 1:
            continue
        RS = TW + 2
        fit = min(int((max_slots - 1 - 2 * RS) / (RS + TW)) if wgrad else max_slots // RS - 2, H)
        for th in range(fit, 0, -1):
            ntx, nty = -(-W // TW), -(-H // th)
            tiles, px = N * ntx * nty, th * TW
            slots, step = (th + 2) * RS + (1 + px if wgrad else 0), 32 if wgrad else 16
            per_tile = 20.0 * slots + 54.0 * ((px + step - 1) // step * step)
            grid = min(tiles, max_grid)
            cost = ((tiles + grid - 1) // grid) * per_tile + 1e-3 * tiles * per_tile / grid
            if cost < best:
                best, plan = cost, dict(TH=th, TW=TW, ntx=ntx, nty=nty, tiles=tiles, grid=grid)
    return plan


def test_what_the_layer_shapes_reach_in_the_tile_planner():
    """What the shape list of the GPU module says each shape is there for, on the restated planner with the MI355X's 256
    CUs (two workgroups per CU).  The planner takes one-row tiles while they number fewer than the workgroups -- which
    covers (2,5,7), (3,41,41) and (1,9,130): neither has a tile of more than one row -- so the list has two shapes whose
    tiles have two rows."""
    for wgrad in (False, True):
        step = 32 if wgrad else 16
        p = {s: _bf16x3_plan(*s, 512, wgrad) for s in P.LAYER_SHAPES}
        assert p[(1, 1, 1)]['tiles'] == 1
        assert (p[(2, 5, 7)]['TH'], p[(2, 5, 7)]['TW'], p[(2, 5, 7)]['tiles']) == (1, 7, 10)              # 7 pixels: a partial step
        assert (p[(3, 41, 41)]['TH'], p[(3, 41, 41)]['TW'], p[(3, 41, 41)]['ntx']) == (1, 16, 3)          # 16 + 16 + 9
        assert (p[(1, 9, 130)]['TH'], p[(1, 9, 130)]['TW'], p[(1, 9, 130)]['ntx']) == (1, 16, 9) and 130 % 16 == 2
        assert p[(600, 1, 2)]['tiles'] == 600 > p[(600, 1, 2)]['grid'] == 512                              # the loop wraps
        q = p[(57, 9, 17)]
        assert (q['TH'], q['TW'], q['nty']) == (2, 17, 5) and 9 % q['TH'] == 1                             # full rows; last tile 1 row
        assert q['TH'] * q['TW'] > step and (q['TH'] * q['TW']) % step != 0                                # 34: a full and a partial step
        q = p[(29, 9, 25)]
        assert (q['TH'], q['TW'], q['ntx'], q['nty']) == (2, 16, 2, 5) and 25 % 16 == 9 and 9 % 2 == 1     # ragged in both directions
