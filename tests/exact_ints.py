"""Equality on small-integer operands: the tool of the tests that hold a convolution route to the float64 oracle EXACTLY.

With integer operands every product and every partial sum of a convolution is an integer.  While the sum of the products'
MAGNITUDES stays below 2^24, every partial sum in every order is an integer below 2^24, which float32 holds exactly: the
result does not depend on the summation order, on fused multiply-adds, or on how many partial filters a reduction adds.  A
kernel that indexes, covers and reduces correctly must then EQUAL the float64 oracle, element by element; one dropped,
doubled, misplaced or leaked contribution changes an integer by at least 1.  (On a bf16x3 route small integers are exact
in bf16: the low parts of the split are zero and only the hi*hi product carries value.  The low parts are held to the same
equality by tests/test_gpu_exact_bf16x3_parts.py, on integers wide enough to have them: `split_bf16`, `wide_ints`,
`three_term` and `split_magnitude` below.)

The condition is checked on the inputs, from the reference alone: `magnitude` is the same oracle operation on the
operands' magnitudes (plus |bias|, |skip|, |accumulator|).  Where a result has a half-integer term (the fused weight decay
0.5 * w), `unit` = 0.5: every value is a multiple of `unit`, and the condition is magnitude / unit < 2^24.

Activations: none and ReLU only (tanh and leaky ReLU multiply by constants that are not dyadic)."""
import numpy as np

LIMIT = 2.0 ** 24

# the default operand ranges, |value| <= RANGE[kind]; masks hold zeros and negatives
RANGE = {'x': 3, 'w': 1, 'b': 3, 'dpre': 3, 'skip': 3, 'dx_acc': 3, 'mask': 2}

LAYOUTS = {
    'nhwc': ('image', 'row', 'column', 'channel'),
    'hwio': ('kh', 'kw', 'ci', 'co'),
    'c': ('channel',),
}


def int_operands(rng, shape, lo=-3, hi=3):
    """A float32 array of integers drawn uniformly from [lo, hi] (both ends included)."""
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def ints(rng, shape, kind, shrink=1):
    """int_operands with the default range of an operand kind ('x', 'w', 'b', 'dpre', 'skip', 'dx_acc', 'mask'); `shrink`
    divides the range (a shape whose magnitude would reach 2^24 takes smaller operands, never a looser comparison)."""
    r = max(RANGE[kind] // shrink, 1)
    return int_operands(rng, shape, -r, r)


# ---- operands with low parts: what a bf16x3 route (csrc/bf16x3.h) makes of integers wider than bf16's 8 bits ---------------
# A bf16x3 kernel splits every operand a = hi + lo (hi = bf16_rne(a), lo = bf16_rne(a - hi)) and computes each product as
# hi*hi + hi*lo + lo*hi.  For an integer of up to 17 bits the split is exact and both parts are integers, so
# every term and every partial sum is an integer again and the magnitude condition decides as before -- with the magnitude
# taken over the parts, since |hi| + |lo| >= |a|.  If one operand of the products is narrow (its lo is 0) the three terms
# are the product itself: the kernel must equal the float64 oracle of the UNSPLIT operands.  If both are wide the dropped
# lo*lo is not zero and the kernel must equal `three_term`, the arithmetic bf16x3.h documents.
MIN_WIDE_BITS = 11              # below, fewer than two thirds of the drawn values have a low part at all
MAX_WIDE_BITS = 17              # |a - hi| <= 256 still fits bf16; from 18 bits on hi + lo != a for some a


def split_bf16(a):
    """hi = bf16_rne(a), lo = bf16_rne(a - hi), as float64 arrays."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi.numpy().astype(np.float64), lo.numpy().astype(np.float64)


def lo_share(a):
    """The share of the NONZERO elements of `a` whose split has lo != 0 (a sparse operand's zeros say nothing about the
    lo path; for a dense draw this is the share of all elements but the few that drew 0)."""
    nz = np.asarray(a) != 0
    return float((split_bf16(a)[1][nz] != 0).mean()) if nz.any() else 0.0


def wide_ints(rng, shape, bits, density=1.0):
    """(v, share): float32 integers drawn uniformly from +-(2^bits - 1), a share `density` of them kept and the others
    zero; share = lo_share(v).  Asserts that the split is exact: hi + lo == v, both parts integers."""
    assert MIN_WIDE_BITS <= bits <= MAX_WIDE_BITS, 'wide operands take %d to %d bits, not %d' % (MIN_WIDE_BITS, MAX_WIDE_BITS, bits)
    r = 2 ** bits - 1
    v = rng.integers(-r, r + 1, size=shape).astype(np.float32)
    if density < 1.0:
        v = v * (rng.random(size=shape) < density)
    v = v.astype(np.float32)
    hi, lo = split_bf16(v)
    assert np.array_equal(hi + lo, v.astype(np.float64)), 'the bf16 split of %d-bit integers is not exact' % bits
    assert np.array_equal(hi, np.round(hi)) and np.array_equal(lo, np.round(lo))
    return v, lo_share(v)


def _parts(a):
    hi, lo = split_bf16(a)
    return hi, (lo if lo.any() else None)


def three_term(op, a, b):
    """op(ah, bh) + op(ah, bl) + op(al, bh) for a bilinear `op` (a float64 oracle without its bias): what a bf16x3
    kernel computes, exactly, while `split_magnitude` stays below 2^24.  A term whose low part is all zero is left out."""
    (ah, al), (bh, bl) = _parts(a), _parts(b)
    r = op(ah, bh)
    if bl is not None:
        r = r + op(ah, bl)
    if al is not None:
        r = r + op(al, bh)
    return r


def split_magnitude(op, a, b):
    """The magnitude of `three_term`: the same three terms on the magnitudes of the parts.  At least op(|a|, |b|) less
    the |lo| |lo| term; it is what bounds every partial sum the kernel can form."""
    (ah, al), (bh, bl) = _parts(a), _parts(b)
    ah, bh = np.abs(ah), np.abs(bh)
    r = op(ah, bh)
    if bl is not None:
        r = r + op(ah, np.abs(bl))
    if al is not None:
        r = r + op(np.abs(al), bh)
    return r


# ---- the reference: the float64 NumPy oracle, or its C restatement where NumPy would take seconds -------------------------
# (tests/test_exact_ints_host.py shows that the two agree exactly on integer operands: the C forward and data gradient
# accumulate in float32, which is exact under the same magnitude condition, and the C filter gradient in double)
C_ORACLE_ABOVE = 2.0e8          # multiply-adds of one oracle call


def ref_fwd(x, w, b=None, padding='SAME', act=None, skip=None, post_relu=False):
    from oracle import oracle as O
    n, h, wd, cin = x.shape
    if float(n * h * wd) * w.shape[0] * w.shape[1] * cin * w.shape[3] > C_ORACLE_ABOVE:
        return O.c_conv2d_fwd(x, w, b, padding, act, skip=skip, post_relu=post_relu).astype(np.float64)
    return O.conv2d_fwd(x, w, b, padding, act, skip=skip, post_relu=post_relu)


def ref_bwd_data(dpre, w, in_hw, padding='SAME'):
    from oracle import oracle as O
    n, oh, ow, cout = dpre.shape
    if float(n * oh * ow) * w.shape[0] * w.shape[1] * w.shape[2] * cout > C_ORACLE_ABOVE:
        return O.c_conv2d_bwd_data(dpre, w, in_hw, padding).astype(np.float64)
    return O.conv2d_bwd_data(dpre, w, in_hw, padding)


def ref_bwd_filter(x, dpre, ksize, padding='SAME'):
    from oracle import oracle as O
    n, oh, ow, cout = dpre.shape
    if float(n * oh * ow) * ksize[0] * ksize[1] * x.shape[3] * cout > C_ORACLE_ABOVE:
        dw, db = O.c_conv2d_bwd_filter(x, dpre, ksize, padding)
        return dw.astype(np.float64), db.astype(np.float64)
    return O.conv2d_bwd_filter(x, dpre, ksize, padding)


def _np64(a):
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


def magnitude_ratio(magnitude, unit=1.0):
    """max(magnitude) / unit / 2^24: below 1 where equality is guaranteed."""
    m = _np64(magnitude)
    return float(m.max() / unit / LIMIT) if m.size else 0.0


def _axes(layout, ndim):
    names = LAYOUTS[layout] if isinstance(layout, str) else tuple(layout)
    if len(names) != ndim:
        raise ValueError('layout %r names %d axes, the tensor has %d' % (layout, len(names), ndim))
    return names


def describe_mismatch(got, ref, layout, first=5):
    """The report of a miss: how many elements differ, the first few as decomposed indices with got / want / difference,
    and the axes on which all of them share one index (one row, one column, one tap, one channel)."""
    names = _axes(layout, ref.ndim)
    bad = ~(got == ref)                          # (NaN differs from everything)
    where = np.argwhere(bad)
    lines = ['%d of %d elements differ' % (len(where), ref.size)]
    for idx in where[:first]:
        t = tuple(int(i) for i in idx)
        lines.append('  %s: got %r, want %r, difference %r'
                     % (', '.join('%s %d' % (n, i) for n, i in zip(names, t)), float(got[t]), float(ref[t]), float(got[t] - ref[t])))
    confined = ['%s %d' % (names[a], int(where[0, a])) for a in range(ref.ndim)
                if ref.shape[a] > 1 and np.all(where[:, a] == where[0, a])]
    lines.append('  all of them in: %s' % (', '.join(confined) if confined else 'no single row, column, tap or channel'))
    return '\n'.join(lines)


class Expected(object):
    """A reference with its magnitude condition, checked once; `check(got)` compares any number of results with it.  A
    result that is a device tensor is first compared on the device (the reference is uploaded once, as float32, which
    holds it exactly); only a miss is brought back to be described."""

    def __init__(self, ref, magnitude, what, layout, unit=1.0, tally=None):
        self.ref = _np64(ref)
        self.what, self.layout, self._dev = what, layout, None
        _axes(layout, self.ref.ndim)
        mag = _np64(magnitude)
        assert mag.shape == self.ref.shape, '%s: magnitude has shape %s, the reference %s' % (what, mag.shape, self.ref.shape)
        assert np.isfinite(self.ref).all() and np.isfinite(mag).all(), '%s: the reference is not finite' % what
        self.ratio = magnitude_ratio(mag, unit)
        assert self.ratio < 1.0, ('%s: cannot compare exactly: the sum of the operands\' magnitudes reaches %.3g x 2^24 '
                                  '(it must stay below 2^24 for float32 to be exact in every order): use smaller operands for this shape'
                                  % (what, self.ratio))
        assert (np.abs(self.ref) <= mag).all(), '%s: |reference| exceeds its magnitude: not the same operation' % what
        assert np.array_equal(self.ref / unit, np.round(self.ref / unit)), '%s: the reference is not a multiple of %g' % (what, unit)
        if tally is not None:
            tally['magnitude'] = max(tally.get('magnitude', 0.0), self.ratio)
            tally['checks'] = tally.get('checks', 0)

    def check(self, got, what=None, tally=None):
        what = self.what if what is None else '%s, %s' % (self.what, what)
        if tally is not None:
            tally['checks'] = tally.get('checks', 0) + 1
        if hasattr(got, 'detach') and got.is_cuda:
            import torch
            assert tuple(got.shape) == self.ref.shape, '%s: shape %s, expected %s' % (what, tuple(got.shape), self.ref.shape)
            if self._dev is None or self._dev.device != got.device:
                self._dev = torch.from_numpy(self.ref.astype(np.float32)).to(got.device)
            if torch.equal(got, self._dev):       # (by value: -0.0 == 0.0, NaN equals nothing)
                return
        got = _np64(got)
        assert got.shape == self.ref.shape, '%s: shape %s, expected %s' % (what, got.shape, self.ref.shape)
        if np.array_equal(got, self.ref):
            return
        nonfinite = int((~np.isfinite(got)).sum())
        raise AssertionError('%s: not equal to the float64 oracle on integer operands%s\n%s'
                             % (what, ' (%d non-finite elements)' % nonfinite if nonfinite else '', describe_mismatch(got, self.ref, self.layout)))


def assert_exact(got, ref, magnitude, what, layout, unit=1.0, tally=None):
    """got == ref by value, after asserting from `magnitude` that equality is guaranteed (module docstring).  layout: 'nhwc'
    (activations), 'hwio' (filters), 'c' (bias vectors) or a tuple of axis names.  Returns max(magnitude) / unit / 2^24."""
    e = Expected(ref, magnitude, what, layout, unit, tally)
    e.check(got, tally=tally)
    return e.ratio
