"""The bf16x3 routes (precision='high') EQUAL to the float64 oracle on integer operands that HAVE low parts.

tests/test_gpu_exact_ints.py holds these routes to equality on operands in [-3, 3]: exact in bf16, so every lo of the
split is zero, two of the three MFMAs of `mfma3` add zero, and nothing that decides equality passes through the second
store of `store_split4`, the `blo` / `wlo` operands, the deferred `split_tap` of the wide kernel's filter-slice reload,
the `+ 128` transposed reads of the filter gradient or the lo half of either LDS buffer.  Here one operand of every
product is an integer of 11 to 15 bits (tests/exact_ints.py: the split hi + lo is exact, both parts are integers) and
the other stays narrow: hi*w + lo*w = x*w, so the kernel must equal the oracle of the unsplit operands, and now an lo
that is dropped, misplaced or stale changes an integer.  With both operands wide (the second one sparse, to stay below
2^24) the dropped lo*lo is not zero and the kernel must equal the three-term sum `exact_ints.three_term`.

The tables below are data: tests/test_exact_ints_host.py imports them and builds every row's references on the host, so a
row whose magnitude reaches 2^24, or whose wide operand has a low part in fewer than half of its elements, fails there,
on a machine without a GPU.  Every output is NaN-filled before the call.

Leaky ReLU (the raw blocked entries take it as activation and as mask) has no dyadic slope, but the epilogue is one fp32
multiply (`act_apply4`: fmaxf(v, slope * v); `act_grad4`: m > 0 ? v : slope * v) of the exact integer v = sum + bias:
it is held bit for bit to the float32 restatement v > 0 ? v : float32(0.2) * v."""
import collections
import types
import zlib

import numpy as np
import pytest
import torch

from tests import exact_ints as X

pytestmark = pytest.mark.gpu

NAN = float('nan')
# what the whole module saw: comparisons, the largest magnitude / 2^24, the smallest share of lo != 0 among the wide
# operands, the 15-bit rows that held
TALLY = {'checks': 0, 'magnitude': 0.0, 'lo_share': 1.0, 'rows': 0, 'held15': 0}

# op: 'fwd' (operands a = x, b = w), 'dgrad' (a = dpre, b = w) or 'wgrad' (a = x, b = dpre).  wide: which operand is
# drawn from +-(2^bits - 1): 'a', 'b', or 'ab' (both; b is then sparse with `density`).  shrink divides the narrow
# operand's default range (exact_ints.RANGE).
Row = collections.namedtuple('Row', 'op wide bits shrink density')


def _row(op, wide, bits=12, shrink=1, density=1.0):
    return Row(op, wide, bits, shrink, density)


# ---- 1. the 64 -> 64 layer: srx_conv2d_fwd / _bwd_data / _bwd_filter at 'high' ---------------------------------------------
# The tiles are bf16x3_plan's (csrc/srx_api.hip).  It minimises the time of the busiest of 2 x CUs persistent workgroups, so
# while the one-row tiles of a call number fewer than that it takes one-row tiles, 16 columns wide where rows are longer:
# tests/test_exact_ints_host.py restates the planner and asserts, for 256 CUs, what each shape is said to reach here.
#   (1,1,1)    the smallest
#   (2,5,7)    rows of 7 pixels: a partial 16- and 32-pixel step
#   (3,41,41)  column tiles 16 + 16 + 9 of every row
#   (1,9,130)  column tiles, the last one 2 pixels wide
#   (600,1,2)  more tiles than workgroups: the persistent loop wraps
#   (57,9,17)  tiles of 2 full rows, the last row tile of an image 1 row: 34 pixels, so a full and a partial step of either size
#   (29,9,25)  tiles of 2 rows x 16 columns, the last column tile 9 wide and the last row tile 1 row: halo corners inside the image
LAYER_SHAPES = [(1, 1, 1), (2, 5, 7), (3, 41, 41), (1, 9, 130), (600, 1, 2), (57, 9, 17), (29, 9, 25)]
BOTH_WIDE_SHAPES = [(2, 5, 7), (3, 41, 41)]


def _layer_rows(shape):
    n, h, w = shape
    px = n * h * w
    # forward and data gradient: K = 576 products per element.  The filter gradient sums N*H*W products per element and
    # its bias gradient N*H*W values of dpre: both narrow operands shrink to [-1, 1] there, and beyond 41 x 41 x 3 pixels the
    # wide one takes 11 bits (the decay term's half-integers halve the room).
    wbits = 12 if px <= 3 * 41 * 41 else 11
    rows = [_row('fwd', 'a'), _row('fwd', 'b'), _row('dgrad', 'a'), _row('dgrad', 'b'),
            _row('wgrad', 'a', wbits, 3), _row('wgrad', 'b', wbits, 3)]
    if shape in BOTH_WIDE_SHAPES:
        # 11 bits each: a product is near 2^20 and at most 2^22, so an element may sum only a few of them: the sparse
        # operand keeps 1.5 (of K = 576) and 1.25 (of N*H*W) nonzero terms per element on average
        rows += [_row('fwd', 'ab', 11, 1, 1.0 / 384), _row('dgrad', 'ab', 11, 1, 1.0 / 384), _row('wgrad', 'ab', 11, 1, 1.25 / px)]
    # 15 bits where the magnitude leaves room (K = 576 with |w| <= 1; the filter gradient of 70 pixels)
    if shape in BOTH_WIDE_SHAPES or wbits == 11:
        rows += [_row('fwd', 'a', 15), _row('dgrad', 'a', 15)]
    if shape == (2, 5, 7):
        rows += [_row('wgrad', 'a', 15, 3)]
    return rows


LAYER_CASES = [(s, r) for s in LAYER_SHAPES for r in _layer_rows(s)]

# ---- 2. the raw blocked entries: srx_conv3x3_blocked_ex / _bwd_filter_ex at 'high' -----------------------------------------
# (cib, cob) -> shapes.  (1,2): more than one produced block; (2,2), (2,4): more than one staged block, so the filter-slice
# reload under the last sub-tile carries a wide w; (8,8): K = 4608.  (3,16,16): two tiles of at most 128 pixels per
# image; (1,8,130): column strips.
BLOCKED_SHAPES = [(1, 1, 1), (2, 5, 7), (3, 16, 16), (1, 8, 130)]
BLOCKED = {(1, 2): BLOCKED_SHAPES, (2, 2): BLOCKED_SHAPES, (2, 4): BLOCKED_SHAPES, (8, 8): [(1, 1, 1), (2, 5, 7)]}


def _blocked_rows(blocks, shape):
    cib, cob = blocks
    rows = []
    for op, k in (('fwd', 576 * cib), ('dgrad', 576 * cob)):
        bits, shrink = (11, 3) if k >= 4608 else (12, 3 if k >= 2304 else 1)
        rows += [_row(op, 'a', bits, shrink), _row(op, 'b', bits, shrink)]
    rows += [_row('wgrad', 'a', 12, 3), _row('wgrad', 'b', 12, 3)]
    if blocks == (1, 2) and shape == (2, 5, 7):
        rows += [_row('fwd', 'a', 15), _row('wgrad', 'a', 15, 3)]
    return rows


BLOCKED_CASES = [(b, s, r) for b, shapes in BLOCKED.items() for s in shapes for r in _blocked_rows(b, s)]

# ---- 3. BlockedConv(precision='high') at (2,7,9): the one-launch wide route and the single-block layer ------------------------
BLOCKED_CONV_SHAPE = (2, 7, 9)
BLOCKED_CONV_CASES = [(c, r) for c in (128, 64) for r in (_row('fwd', 'a'), _row('dgrad', 'a'), _row('wgrad', 'a', 12, 3))]


# ---- the references: NumPy / the C oracle only, so the host test builds them too -------------------------------------------
def _operands(rng, row, shape_a, kind_a, shape_b, kind_b):
    """(a, b, the smallest share of lo != 0 among the wide ones): the conditions on the inputs, from the inputs alone."""
    assert row.bits >= X.MIN_WIDE_BITS
    if row.wide == 'a':
        a, share = X.wide_ints(rng, shape_a, row.bits)
        b = X.ints(rng, shape_b, kind_b, row.shrink)
        assert not X.split_bf16(b)[1].any()
    elif row.wide == 'b':
        a = X.ints(rng, shape_a, kind_a, row.shrink)
        b, share = X.wide_ints(rng, shape_b, row.bits)
        assert not X.split_bf16(a)[1].any()
    else:
        a, s1 = X.wide_ints(rng, shape_a, row.bits)
        b, s2 = X.wide_ints(rng, shape_b, row.bits, row.density)
        share = min(s1, s2)
    assert share >= 0.5, 'only %.2f of a %d-bit operand has a low part' % (share, row.bits)
    return a, b, share


def build(shape, cin, cout, row, tally=None, decay=False):
    """The operands of one row and its references as exact_ints.Expected objects (each asserts its own magnitude condition).
    One operand narrow: the float64 oracle of the unsplit operands.  Both wide: the three-term oracle.  The magnitude is
    in both cases the oracle on the magnitudes of the parts."""
    n, h, w = shape
    tag = '%dx%dx%d %d->%d %s' % (n, h, w, cin, cout, '/'.join(str(v) for v in row))
    rng = np.random.default_rng(zlib.crc32(repr((shape, cin, cout, tuple(row))).encode()))
    xs, ys, ws = (n, h, w, cin), (n, h, w, cout), (3, 3, cin, cout)
    exp = lambda ref, mag, what, layout, unit=1.0: X.Expected(ref, mag, '%s: %s' % (tag, what), layout, unit, tally=tally)
    ref = lambda op, a, b: X.three_term(op, a, b) if row.wide == 'ab' else op(a, b)
    c = types.SimpleNamespace(row=row, tag=tag)
    if row.op == 'fwd':
        f = lambda a, b: X.ref_fwd(a, b, None, 'SAME')
        c.a, c.b, c.share = _operands(rng, row, xs, 'x', ws, 'w')
        c.bias = X.ints(rng, (cout,), 'b')
        pre, mag = ref(f, c.a, c.b) + c.bias, X.split_magnitude(f, c.a, c.b) + np.abs(c.bias)
        c.e = {'none': exp(pre, mag, 'forward', 'nhwc'), 'relu': exp(np.maximum(pre, 0), mag, 'forward, ReLU', 'nhwc')}
    elif row.op == 'dgrad':
        g = lambda a, b: X.ref_bwd_data(a, b, (h, w), 'SAME')
        c.a, c.b, c.share = _operands(rng, row, ys, 'dpre', ws, 'w')
        c.mask = X.ints(rng, xs, 'mask')
        dx, mag = ref(g, c.a, c.b), X.split_magnitude(g, c.a, c.b)
        c.e = {'none': exp(dx, mag, 'data gradient', 'nhwc'), 'relu': exp(dx * (c.mask > 0), mag, 'ReLU-masked data gradient', 'nhwc')}
    else:
        assert row.op == 'wgrad'
        k = lambda a, b: X.ref_bwd_filter(a, b, (3, 3), 'SAME')[0]
        c.a, c.b, c.share = _operands(rng, row, xs, 'x', ys, 'dpre')
        dw, mag = ref(k, c.a, c.b), X.split_magnitude(k, c.a, c.b)
        # the bias gradient is a plain fp32 sum of the unsplit dpre: its magnitude is the sum of |dpre|
        d2 = c.b.astype(np.float64).reshape(-1, cout)
        c.e = {'dw': exp(dw, mag, 'filter gradient', 'hwio'), 'db': exp(d2.sum(axis=0), np.abs(d2).sum(axis=0), 'bias gradient', 'c')}
        # (the decay term's half-integers halve the room: the both-wide rows, whose products are near 2^20, run without it)
        if decay and row.wide != 'ab':
            c.w = X.ints(rng, ws, 'w')
            c.e['dwd'] = exp(dw + 0.5 * c.w, mag + 0.5 * np.abs(c.w), 'filter gradient + 0.5 w', 'hwio', unit=0.5)
    return c


def lrelu32(v):
    """v > 0 ? v : float32(0.2) * v on the exact integers v, in float32: one rounding, as the kernels' epilogue."""
    v = np.asarray(v, np.float64).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), np.round(v.astype(np.float64)))
    return np.where(v > 0, v, np.float32(0.2) * v).astype(np.float32)


# ---- the device side -----------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def nan_like(shape):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device='cuda')


def to_nhwc(b):
    cb, n, h, w, c = b.shape
    return b.transpose(1, 2, 3, 0, 4).reshape(n, h, w, cb * c)


def to_blocked(a, cb):
    n, h, w, c = a.shape
    return np.ascontiguousarray(a.reshape(n, h, w, cb, c // cb).transpose(3, 0, 1, 2, 4))


def w_blocked(k, cib, cob):
    return np.ascontiguousarray(k.reshape(3, 3, cib, 64, cob, 64).transpose(2, 4, 0, 1, 3, 5))


def check(e, got, what=None):
    e.check(got, what, tally=TALLY)


def check_bits(e_int, got, ref32, what):
    """got == ref32 bit for bit (by value), for a result that is no integer: e_int is the Expected of the integers it was
    made from, whose magnitude condition has been asserted."""
    TALLY['checks'] += 1
    got = np.asarray(got, np.float32)
    if not np.array_equal(got, ref32):
        raise AssertionError('%s, %s: not equal to the float32 restatement\n%s'
                             % (e_int.what, what, X.describe_mismatch(got.astype(np.float64), ref32.astype(np.float64), e_int.layout)))


def held(c):
    """A row passed all its checks: the module's figures."""
    TALLY['rows'] += 1
    TALLY['lo_share'] = min(TALLY['lo_share'], c.share)
    if c.row.bits == 15:
        TALLY['held15'] += 1


def _ids(cases):
    out = []
    for c in cases:
        parts = []
        for v in c:
            if isinstance(v, Row):
                parts.append('%s_%s_%db' % (v.op, v.wide, v.bits))
            elif isinstance(v, tuple):
                parts.append('x'.join(str(i) for i in v))
            else:
                parts.append(str(v))
        out.append('-'.join(parts))
    return out


@pytest.fixture(scope='module')
def ops():
    from ml_super_resolution_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.mark.parametrize('shape,row', LAYER_CASES, ids=_ids(LAYER_CASES))
def test_layer_equals_the_oracle_on_operands_with_low_parts(shape, row, ops):
    from ml_super_resolution_amd import _lib
    c = build(shape, 64, 64, row, TALLY, decay=True)
    xs, ws = shape + (64,), (3, 3, 64, 64)
    op = {'fwd': _lib.OP_FWD, 'dgrad': _lib.OP_BWD_DATA, 'wgrad': _lib.OP_BWD_FILTER}[row.op]
    assert ops.precision_supported(xs, ws, op, act='relu' if row.op == 'fwd' else None, precision='high')[0]
    a, b = dev(c.a), dev(c.b)
    if row.op == 'fwd':
        bias = dev(c.bias)
        check(c.e['none'], ops.conv2d_fwd(a, b, bias, 'same', None, out=nan_like(xs), precision='high'))
        check(c.e['relu'], ops.conv2d_fwd(a, b, bias, 'same', 'relu', out=nan_like(xs), precision='high'))
    elif row.op == 'dgrad':
        check(c.e['none'], ops.conv2d_bwd_data(a, b, xs, 'same', out=nan_like(xs), precision='high'))
        check(c.e['relu'], ops.conv2d_bwd_data(a, b, xs, 'same', x_in=dev(c.mask), in_act='relu', out=nan_like(xs), precision='high'))
    else:
        g, gb = ops.conv2d_bwd_filter(a, b, ws, 'same', dw=nan_like(ws), dbias=nan_like((64,)), precision='high')
        check(c.e['dw'], g)
        check(c.e['db'], gb)
        if 'dwd' in c.e:
            g, gb = ops.conv2d_bwd_filter(a, b, ws, 'same', w_for_decay=dev(c.w), wd_scale=0.5, dw=nan_like(ws), dbias=nan_like((64,)),
                                          precision='high')
            check(c.e['dwd'], g)
            check(c.e['db'], gb, 'with the decay term')
    held(c)


@pytest.mark.parametrize('blocks,shape,row', BLOCKED_CASES, ids=_ids(BLOCKED_CASES))
def test_raw_blocked_entries_equal_the_oracle_on_operands_with_low_parts(blocks, shape, row, ops):
    """Compared in NHWC / HWIO, so a miss names the image's pixel and the layer's channel."""
    from ml_super_resolution_amd import blocked
    (cib, cob), (n, h, w) = blocks, shape
    c = build(shape, 64 * cib, 64 * cob, row, TALLY)
    nhwc = lambda t: to_nhwc(t.cpu().numpy())
    if row.op == 'fwd':
        xb, wb, bias, out = dev(to_blocked(c.a, cib)), dev(w_blocked(c.b, cib, cob)), dev(c.bias), (cob, n, h, w, 64)
        check(c.e['none'], nhwc(ops.conv3x3_blocked(xb, wb, bias, None, out=nan_like(out), precision='high')))
        check(c.e['relu'], nhwc(ops.conv3x3_blocked(xb, wb, bias, 'relu', out=nan_like(out), precision='high')))
        check_bits(c.e['none'], nhwc(ops.conv3x3_blocked(xb, wb, bias, 'lrelu', out=nan_like(out), precision='high')),
                   lrelu32(c.e['none'].ref), 'leaky ReLU')
    elif row.op == 'dgrad':
        db, wb, mb, out = dev(to_blocked(c.a, cob)), dev(w_blocked(c.b, cib, cob)), dev(to_blocked(c.mask, cib)), (cib, n, h, w, 64)
        run = lambda **kw: nhwc(ops.conv3x3_blocked(db, wb, None, None, transpose=True, out=nan_like(out), precision='high', **kw))
        check(c.e['none'], run())
        check(c.e['relu'], run(mask=mb, mask_act='relu'))
        dx32 = c.e['none'].ref.astype(np.float32)
        check_bits(c.e['none'], run(mask=mb, mask_act='lrelu'), np.where(c.mask > 0, dx32, np.float32(0.2) * dx32), 'leaky-ReLU mask')
    else:
        g, gb = nan_like((cib, cob, 3, 3, 64, 64)), nan_like((64 * cob,))
        ops.conv3x3_blocked_bwd_filter(dev(to_blocked(c.a, cib)), dev(to_blocked(c.b, cob)), g, gb, precision='high')
        check(c.e['dw'], blocked.blocked_to_hwio(g).cpu().numpy())
        check(c.e['db'], gb)
    held(c)


@pytest.mark.parametrize('channels,row', BLOCKED_CONV_CASES, ids=_ids(BLOCKED_CONV_CASES))
def test_blocked_conv_at_high_equals_the_oracle_on_operands_with_low_parts(channels, row, ops):
    """BlockedConv(precision='high'): 128 -> 128 runs the one-launch wide route, 64 -> 64 is one block pair and goes to
    srx_conv2d_* at precision 1; `used` must say that the pass ran at 'high'."""
    from ml_super_resolution_amd import blocked
    n, h, w = BLOCKED_CONV_SHAPE
    c = build(BLOCKED_CONV_SHAPE, channels, channels, row, TALLY)
    ks = blocked.BlockedConv.kernel_shape(channels, channels)
    layer = blocked.BlockedConv(channels, channels, 1, 'relu', torch.empty(ks, device='cuda'), torch.empty(channels, device='cuda'),
                                nan_like(ks), nan_like((channels,)), precision='high')
    blocks = lambda a: blocked.to_blocks(dev(a))
    if row.op == 'fwd':
        layer.set_kernel_hwio(c.b, c.bias)
        check(c.e['relu'], blocked.to_nhwc(layer.forward(blocks(c.a))).contiguous())
        assert layer.used == {'fwd': 'high'}
    elif row.op == 'dgrad':
        layer.set_kernel_hwio(c.b)
        check(c.e['relu'], blocked.to_nhwc(layer.dgrad(blocks(c.a), mask=blocks(c.mask), mask_act='relu')).contiguous())
        assert layer.used == {'dgrad': 'high'}
    else:
        layer.wgrad(blocks(c.a), blocks(c.b))
        check(c.e['dw'], layer.kernel_hwio(layer.dw).contiguous())
        check(c.e['db'], layer.db)
        assert layer.used == {'wgrad': 'high'}
    held(c)


# ---- the module's figures -------------------------------------------------------------------------------------------------
def test_figures_of_the_low_part_tests():
    """Runs last: the figures of the rows that ran before this one IN THIS PROCESS (they mean what they say when the whole
    module runs in file order; each row's own assertions do not depend on the tally)."""
    print('bf16x3 low-part tests: %d rows, %d comparisons; largest magnitude / 2^24 = %.4f; smallest share of lo != 0 = %.3f; '
          '15-bit rows that held: %d' % (TALLY['rows'], TALLY['checks'], TALLY['magnitude'], TALLY['lo_share'], TALLY['held15']))
    assert TALLY['magnitude'] < 1.0
    assert TALLY['lo_share'] >= 0.5
