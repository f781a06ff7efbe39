"""Equality on small-integer operands: the tool of the tests that hold a convolution route to the float64 oracle EXACTLY.

With integer operands every product and every partial sum of a convolution is an integer.  While the sum of the products'
MAGNITUDES stays below 2^24, every partial sum in every order is an integer below 2^24, which float32 holds exactly: the
result does not depend on the summation order, on fused multiply-adds, or on how many partial filters a reduction adds.  A
kernel that indexes, covers and reduces correctly must then EQUAL the float64 oracle, element by element; one dropped,
doubled, misplaced or leaked contribution changes an integer by at least 1.  (A bf16x3 route sees the same thing: small
integers are exact in bf16, so the middle and low parts of the split are zero.)

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
