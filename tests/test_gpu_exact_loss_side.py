"""The second MFMA family and the flat kernels EQUAL to float64 NumPy on small-integer operands (tests/exact_ints.py): every
route of srx_gemm at the rows of tests/test_gemm_routes_host.CASES (imported, not copied; the route is asserted again here,
with the device's pointers and the workspace ops.gemm passes), srx_texture_gram / _bwd and the three launches they replace,
srx_channel_normalize / _bwd, and the reductions and optimizer kernels of csrc/elementwise.hip at sizes on both sides of the
point where their fixed grids wrap around.

Why equality holds.  GEMM: integer operands, |A| @ |B| (+ |bias|, |C|) below 2^24, alpha dyadic.  Texture statistics and
normalize(): the features are channel pairs (v, 2 - v), v in {0, 1, 2}, times a per-pixel scale of 1 or 2, so the channel mean
IS the scale, a power of two, and with eps = 0 every division is exact: the normalised features are the integers (v, 2 - v),
the gram matrices integers (asserted with unit 1/4), t = sum dn x an integer below 2^24 and dx a multiple of 1 / (4 C).  The scale
differs between neighbouring pixels, so a divisor taken from the wrong pixel is off by a factor of two.  Reductions: sums of
integer squares below 2^24, scaled by powers of two.  Each condition is asserted from the reference's magnitudes before
anything is compared.  Every output is filled with NaN before a call that does not accumulate.

Not equality, by the bounds tests/test_gpu_ops.py and tests/test_gpu_enet_pat.py already state: Adam (a square root and a
division per element) and the log loss (logf)."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import oracle_enet as E
from tests import exact_ints as X
from tests.test_gemm_routes_host import CASES, case_id, operand_shapes
from tests.test_gpu_ops import close

pytestmark = pytest.mark.gpu

NAN = float('nan')
SENTINEL = 12345.0            # the guard bands around an output: finite, no value any of these operations produces
BAND = 1024
TALLY = {'magnitude': 0.0, 'checks': 0, 'routes': {}}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def nan_like(shape):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device='cuda')


def expected(ref, magnitude, what, layout, unit=1.0):
    return X.Expected(ref, magnitude, what, layout, unit, tally=TALLY)


def check(e, got, what=None):
    e.check(got, what, tally=TALLY)


@pytest.fixture(scope='module')
def ops():
    from ml_super_resolution_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


class Banded(object):
    """An output of `shape` inside a larger buffer, BAND sentinel floats before and after it."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * BAND,), SENTINEL, dtype=torch.float32, device='cuda')
        self.out = self.buf[BAND:BAND + n].view(tuple(shape))
        self.band = torch.full((BAND,), SENTINEL, dtype=torch.float32, device='cuda').view(torch.int32)

    def fill(self, value):
        if torch.is_tensor(value):
            self.out.copy_(value)
        else:
            self.out.fill_(value)
        return self.out

    def assert_bands_intact(self, what):
        n = self.out.numel()
        assert torch.equal(self.buf[:BAND].view(torch.int32), self.band), '%s: a store landed before the output' % what
        assert torch.equal(self.buf[BAND + n:].view(torch.int32), self.band), '%s: a store landed after the output' % what


# ---- GEMM -------------------------------------------------------------------------------------------------------------------
def _t(a, trans):
    return np.swapaxes(a, -1, -2) if trans else a


def _gemm_call(ops, c, A, B, out, bias=None, act=None, alpha=1.0, accumulate=False):
    """ops.gemm, or -- for the row that passes no workspace, which ops.gemm always does -- srx_gemm itself."""
    if c.ws:
        return ops.gemm(A, B, bias=bias, act=act, alpha=alpha, trans_a=c.trans_a, trans_b=c.trans_b, out=out, accumulate=accumulate)
    from ml_super_resolution_amd import _lib
    d, shape = ops._gemm_desc(tuple(A.shape), tuple(B.shape), act, alpha, c.trans_a, c.trans_b, accumulate)
    assert tuple(out.shape) == shape
    _lib.check(_lib.lib().srx_gemm(ctypes.byref(d), A.data_ptr(), B.data_ptr(), None if bias is None else bias.data_ptr(), out.data_ptr(),
                                   None, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'srx_gemm')
    return out


@pytest.mark.parametrize('c', CASES, ids=[case_id(c) for c in CASES])
def test_gemm_equals_float64_on_the_route_the_row_names(c, ops):
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    a_shape, b_shape = operand_shapes(c)
    A, B, bias = X.ints(rng, a_shape, 'x'), X.ints(rng, b_shape, 'w'), X.ints(rng, (c.N,), 'b')
    ref = _t(A, c.trans_a).astype(np.float64) @ _t(B, c.trans_b).astype(np.float64)
    mag = np.abs(_t(A, c.trans_a)).astype(np.float64) @ np.abs(_t(B, c.trans_b)).astype(np.float64)
    c0 = X.ints(rng, ref.shape, 'dx_acc')
    layout = ('batch', 'row', 'column') if c.batch else ('row', 'column')
    Ad, bd, c0d = dev(A), dev(bias), dev(c0)
    store = torch.empty(B.size + 4, dtype=torch.float32, device='cuda')          # B where the row puts it
    Bd = store[c.b_offset // 4:c.b_offset // 4 + B.size].view(b_shape)
    Bd.copy_(torch.from_numpy(B))
    assert Bd.data_ptr() % 16 == c.b_offset and Bd.is_contiguous()
    ws = 'gemm' if c.ws else None

    def route(bias_given, act):
        return ops.gemm_route(Ad, Bd, bias=bd if bias_given else None, act=act, trans_a=c.trans_a, trans_b=c.trans_b, workspace=ws)[0]

    assert route(c.bias, c.act) == c.route, c.why
    TALLY['routes'][case_id(c)] = c.route
    # the row's own call, then with a bias and with bias + ReLU where the route has an epilogue (the NT kernel has none: a
    # bias or an activation is what sends its shape to the tile kernel, which the table's fall-through rows cover)
    forms = [(c.bias, c.act)]
    if c.route != 'skinny_nt':
        forms += [f for f in ((True, None), (True, 'relu')) if f != (c.bias, c.act)]
    out = Banded(ref.shape)
    for bias_given, act in forms:
        assert route(bias_given, act) == c.route, 'bias %s, act %s' % (bias_given, act)
        kw = dict(bias=bd if bias_given else None, act=act)
        b64, bmag = (bias.astype(np.float64), np.abs(bias)) if bias_given else (0.0, 0.0)
        fin = (lambda v: np.maximum(v, 0)) if act == 'relu' else (lambda v: v)
        what = 'gemm%s%s' % (' + bias' if bias_given else '', ', ReLU' if act else '')
        for alpha in (1.0, 0.5, 2.0):
            e = expected(fin(alpha * ref + b64), alpha * mag + bmag, '%s, alpha %g' % (what, alpha), layout, unit=0.5)
            check(e, _gemm_call(ops, c, Ad, Bd, out.fill(NAN), alpha=alpha, **kw))
            if alpha == 1.0:        # deterministic: the same call again, bit for bit
                first = out.out.clone()
                assert torch.equal(_gemm_call(ops, c, Ad, Bd, out.fill(NAN), **kw), first), '%s: two runs differ' % what
        for alpha in (1.0, 0.5):
            e = expected(fin(alpha * ref + b64) + c0, alpha * mag + bmag + np.abs(c0), '%s, alpha %g, accumulating' % (what, alpha), layout, unit=0.5)
            check(e, _gemm_call(ops, c, Ad, Bd, out.fill(c0d), alpha=alpha, accumulate=True, **kw))
    out.assert_bands_intact(case_id(c))


# (route, batch, M, N, K): once per tile route, srx_gemm itself with operands ops.gemm never passes
STRIDED = [('tile', 1, 70, 33, 19), ('tile_splitk', 1, 17, 9, 520), ('tile_per_wave', 1025, 48, 48, 5)]


@pytest.mark.parametrize('route,batch,M,N,K', STRIDED, ids=[s[0] for s in STRIDED])
def test_gemm_with_strided_operands_and_a_column_window_of_c(route, batch, M, N, K, ops):
    """A is a window of a wider matrix, C a column window of a wider sentinel-filled one (c_row_stride > N, which the ABI
    allows): the result is exact and the columns outside the window keep their bits."""
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(K)
    lda, a0, ldc, c0 = K + 5, 3, N + 11, 4
    Aw, B = X.ints(rng, (batch, M, lda), 'x'), X.ints(rng, (batch, K, N), 'w')
    A = Aw[:, :, a0:a0 + K]
    ref, mag = A.astype(np.float64) @ B.astype(np.float64), np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    Ad, Bd = dev(Aw), dev(B)
    Cw = torch.full((batch, M, ldc), SENTINEL, dtype=torch.float32, device='cuda')
    Cw[:, :, c0:c0 + N] = NAN
    d = _lib.GemmDesc(M, N, K, batch, lda, 1, M * lda, N, 1, K * N, ldc, 1, M * ldc, 1.0, _lib.ACT_NONE, 0)
    need = L.srx_gemm_workspace_bytes(M, N, K, batch)
    ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device='cuda')
    args = (ctypes.byref(d), Ad.data_ptr() + 4 * a0, Bd.data_ptr(), None)
    assert ops.GEMM_ROUTES[L.srx_gemm_route_of(*(args + (ws.data_ptr(), need, None)))] == route
    _lib.check(L.srx_gemm(*(args + (Cw.data_ptr() + 4 * c0, ws.data_ptr(), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))),
               'srx_gemm')
    check(expected(ref, mag, 'gemm into a column window, ' + route, ('batch', 'row', 'column')), Cw[:, :, c0:c0 + N].contiguous())
    outside = torch.cat([Cw[:, :, :c0], Cw[:, :, c0 + N:]], dim=2)
    assert torch.equal(outside.contiguous().view(torch.int32), torch.full_like(outside, SENTINEL).view(torch.int32)), 'a store left the window'


# ---- texture statistics and normalize() ----------------------------------------------------------------------------------------
def _pair_features(rng, shape):
    """Features [..., C] of channel pairs (v, 2 - v), v in {0, 1, 2}, times a per-pixel scale in {1, 2}: the channel mean is
    the scale."""
    C = shape[-1]
    assert C % 2 == 0
    v = rng.integers(0, 3, size=shape[:-1] + (C // 2,))
    x = np.empty(shape, np.float64)
    x[..., 0::2], x[..., 1::2] = v, 2 - v
    scale = rng.integers(1, 3, size=shape[:-1] + (1,))
    x *= scale
    assert np.array_equal(x.mean(axis=-1, keepdims=True), scale)
    return x.astype(np.float32)


TEXTURE_CASES = [(64, 1, 16, 16), (64, 2, 32, 48), (128, 3, 16, 32), (256, 2, 32, 16)]


@pytest.mark.parametrize('c,n,h,w', TEXTURE_CASES)
def test_texture_statistics_equal_float64(c, n, h, w, ops):
    rng = np.random.default_rng(c * 1009 + h * 31 + w)
    x = _pair_features(rng, (n, h, w, c))
    x64 = x.astype(np.float64)
    m = x64.mean(axis=-1, keepdims=True)                                  # (eps = 0)
    pat = E.patches16(x64 / m).reshape(-1, 256, c)
    gram = np.einsum('pki,pkj->pij', pat, pat)
    e_gram = expected(gram, gram, 'gram matrices', ('patch', 'row', 'column'), unit=0.25)       # (nothing is negative: its own magnitude)
    tri = np.triu(rng.integers(-1, 2, size=gram.shape))
    dg = (tri + np.triu(tri, 1).transpose(0, 2, 1)).astype(np.float32)    # symmetric integers in [-1, 1]
    assert np.array_equal(dg, dg.transpose(0, 2, 1))
    to_image = lambda t: E.patches16_bwd(t.reshape(n, -1, 256, c), (n, h, w, c))
    dn = to_image(2.0 * np.einsum('pkj,pjc->pkc', pat, dg.astype(np.float64)))
    dn_mag = to_image(2.0 * np.einsum('pkj,pjc->pkc', pat, np.abs(dg).astype(np.float64)))
    t, t_mag = (dn * x64).sum(axis=-1, keepdims=True), (dn_mag * x64).sum(axis=-1, keepdims=True)
    assert t_mag.max() < X.LIMIT                                          # the inner sum t = sum dn x: integers below 2^24
    TALLY['magnitude'] = max(TALLY['magnitude'], float(t_mag.max() / X.LIMIT))
    e_dx = expected(dn / m - t / (c * m * m), dn_mag / m + t_mag / (c * m * m), 'd loss / d x', 'nhwc', unit=1.0 / (4 * c))

    xd, dgd = dev(x), dev(dg)
    check(e_gram, ops.texture_gram(xd, eps=0.0, out=nan_like(gram.shape)), 'one pass')
    check(e_dx, ops.texture_gram_bwd(xd, dgd, eps=0.0, alpha=2.0, out=nan_like(x.shape)), 'one pass')
    # the three launches it replaces, and back
    sp = ops.extract_patches16(ops.channel_normalize(xd, eps=0.0, out=nan_like(x.shape)), out=nan_like((n, (h // 16) * (w // 16), 256, c))).view(-1, 256, c)
    check(e_gram, ops.gemm(sp, sp, trans_a=True, out=nan_like(gram.shape)), 'three launches')
    dsp = ops.gemm(sp, dgd, alpha=2.0, out=nan_like(sp.shape))
    dimg = ops.extract_patches16_bwd(dsp.view(n, -1, 256, c), (n, h, w, c), out=nan_like(x.shape))
    check(e_dx, ops.channel_normalize_bwd(xd, dimg, eps=0.0, out=nan_like(x.shape)), 'three launches')


@pytest.mark.parametrize('pixels', [1, 5, 61])
@pytest.mark.parametrize('C', [2, 6, 8, 64, 100, 130, 512])
def test_channel_normalize_equals_float64(C, pixels, ops):
    """Four pixels per workgroup, one per wave: 1, 5 and 61 pixels leave slots of the last workgroup idle.  The backward
    divides by C m^2: exact where C is a power of two."""
    rng = np.random.default_rng(C * 100 + pixels)
    x = _pair_features(rng, (pixels, C))
    x64 = x.astype(np.float64)
    m = x64.mean(axis=-1, keepdims=True)
    xd = dev(x)
    check(expected(x64 / m, x64 / m, 'normalize', ('pixel', 'channel')), ops.channel_normalize(xd, eps=0.0, out=nan_like(x.shape)))
    if C & (C - 1):
        return
    dy = X.ints(rng, x.shape, 'dpre')
    t, t_mag = (dy * x64).sum(axis=-1, keepdims=True), (np.abs(dy) * x64).sum(axis=-1, keepdims=True)
    e = expected(dy / m - t / (C * m * m), np.abs(dy) / m + t_mag / (C * m * m), 'normalize, backward', ('pixel', 'channel'), unit=1.0 / (4 * C))
    check(e, ops.channel_normalize_bwd(xd, dev(dy), eps=0.0, out=nan_like(x.shape)))


# ---- flat reductions and optimizers ----------------------------------------------------------------------------------------------
# sq_partial_kernel wraps around its 1024 x 256 x 4 grid above 1,048,576 elements, the Adam kernels above 2,097,152,
# momentum_clip_kernel above 524,288: the two large sizes are past all three, with a float4 tail and a scalar tail
SMALL = [1, 3, 4, 5, 1023]
WRAP_1M, WRAP_2M = 1048576 + 1027, 2097152 + 4 * 256 + 3
SIZES = SMALL + [WRAP_1M, WRAP_2M]


def _scalar(value, magnitude, what, unit):
    return expected(np.array([value], np.float64), np.array([magnitude], np.float64), what, ('scalar',), unit)


@pytest.mark.parametrize('n', SIZES)
def test_mse_equals_float64(n, ops):
    rng = np.random.default_rng(n)
    span = 3 if 9 * n < X.LIMIT else 1                                   # |a - b| <= span: span^2 n stays below 2^24
    b = X.int_operands(rng, (n,), -3, 3)
    a = b + X.int_operands(rng, (n,), -span, span)
    inv = 2.0 ** -10
    d = a.astype(np.float64) - b
    s = float((d * d).sum())
    e_loss = _scalar(s * inv, s * inv, 'mse loss', inv)
    e_acc = _scalar(s * inv + 7.0, s * inv + 7.0, 'mse loss, accumulating', inv)
    e_d = expected(2.0 * d * inv, 2.0 * np.abs(d) * inv, 'mse gradient', ('element',), unit=inv)
    ad, bd = dev(a), dev(b)
    loss = nan_like((1,))
    check(e_d, ops.mse_fwd_bwd(ad, bd, loss, inv_numel=inv, dpred=nan_like((n,))))
    check(e_loss, loss)
    loss = nan_like((1,))
    assert ops.mse_fwd_bwd(ad, bd, loss, inv_numel=inv, want_grad=False) is None
    check(e_loss, loss, 'without the gradient')
    loss = torch.full((1,), 7.0, device='cuda')
    check(e_d, ops.mse_fwd_bwd(ad, bd, loss, inv_numel=inv, accumulate=True, dpred=nan_like((n,))), 'accumulating call')
    check(e_acc, loss)


@pytest.mark.parametrize('n', SIZES)
def test_l2_loss_with_and_without_a_mask_equals_float64(n, ops):
    """The masked form is what the training engines run on the parameter pool every step."""
    rng = np.random.default_rng(n + 1)
    w = X.ints(rng, (n,), 'x', shrink=1 if 9 * n < X.LIMIT else 3)
    mask = X.int_operands(rng, (n,), 0, 1)
    scale = 2.0 ** -3
    wd, md = dev(w), dev(mask)
    for m, md_, what in ((np.ones(n), None, 'l2 loss'), (mask.astype(np.float64), md, 'masked l2 loss')):
        v = 0.5 * scale * float((m * w.astype(np.float64) ** 2).sum())
        loss = nan_like((1,))
        ops.l2_loss(wd, scale, loss, accumulate=False, mask=md_)
        check(_scalar(v, v, what, 0.5 * scale), loss)
        loss = torch.full((1,), 5.0, device='cuda')
        ops.l2_loss(wd, scale, loss, accumulate=True, mask=md_)
        check(_scalar(v + 5.0, v + 5.0, what + ', accumulating', 0.5 * scale), loss)


@pytest.mark.parametrize('n', SIZES)
def test_momentum_clip_two_steps_equal_the_float32_restatement(n, ops):
    """Bit equality with a float32 NumPy restatement that rounds after every operation.  It is derivable whatever the compiler
    contracts: with integer weights and gradients, lr = 1/4, momentum = 1/2 and an integer cap every intermediate is a small
    multiple of 1/16, exact in float32, so a fused multiply-add rounds nothing differently -- the float64 evaluation, which
    the restatement is asserted to equal, says so."""
    rng = np.random.default_rng(n + 2)
    lr, mom, cap = np.float32(0.25), np.float32(0.5), np.float32(3.0)
    w, acc = X.int_operands(rng, (n,), -3, 3), X.int_operands(rng, (n,), -2, 2)
    wd, accd = dev(w), dev(acc)
    w64, acc64 = w.astype(np.float64), acc.astype(np.float64)
    for step in range(2):
        g = X.int_operands(rng, (n,), -5, 5)                             # (the cap clips the 4s and 5s)
        ops.momentum_clip_step(wd, dev(g), accd, lr=float(lr), momentum=float(mom), cap=float(cap))
        gi = np.minimum(np.maximum(g, -cap), cap)
        prod = mom * acc
        acc = prod + gi
        step_ = lr * acc
        w = w - step_
        assert w.dtype == np.float32 and acc.dtype == np.float32
        acc64 = 0.5 * acc64 + np.clip(g.astype(np.float64), -3.0, 3.0)
        w64 = w64 - 0.25 * acc64
        assert np.array_equal(w, w64) and np.array_equal(acc, acc64)
        TALLY['checks'] += 2
        assert torch.equal(accd, dev(acc)), 'step %d: accumulator' % step
        assert torch.equal(wd, dev(w)), 'step %d: weights' % step
    if n > 5:
        assert (np.abs(g) > 3).any()


def test_adam_above_the_point_where_its_grid_wraps(ops):
    """tests/test_gpu_ops.test_mse_l2_adam_momentum_psnr's comparison at 2,098,179 elements (the grid covers 2,097,152)."""
    n = WRAP_2M
    rng = np.random.default_rng(12)
    wv = rng.normal(size=n).astype(np.float32)
    wd_, md_, vd_ = dev(wv), dev(np.zeros(n)), dev(np.zeros(n))
    w64, m64, v64 = wv.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in (1, 2):
        g = (rng.normal(size=n) * 10.0 ** rng.integers(-8, 1, size=n)).astype(np.float32)
        ops.adam_tf_step(wd_, dev(g), md_, vd_, 5e-5, t)
        w64, m64, v64 = O.adam_tf(w64, g.astype(np.float64), m64, v64, 5e-5, t)
    assert np.abs(wd_.cpu().numpy() - w64).max() <= 1e-6
    close(md_, m64, 1e-5)


@pytest.mark.parametrize('rows,cols', [(1, 1), (37, 130), (5, 257), (1000, 3)])
def test_column_sums_equal_float64(rows, cols, ops):
    rng = np.random.default_rng(rows + cols)
    a = X.ints(rng, (rows, cols), 'x')
    check(expected(a.astype(np.float64).sum(axis=0), np.abs(a).astype(np.float64).sum(axis=0), 'column sums', ('column',)),
          ops.column_sums(dev(a), out=nan_like((cols,))))


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_log_loss_over_more_than_one_trip_of_its_loop(n, ops):
    """The bounds of tests/test_gpu_enet_pat.test_normalize_logloss_preprocess_addscaled_colsum.  They hold by derivation: beside
    logf and the float32 sum, the only error is the float32 rounding of p + eps and 1 - p + eps, 2^-24 relative, which log
    turns into an ABSOLUTE 2^-24 per element -- nothing next to the loss wherever other elements contribute.  So p = 0 and
    p = 1 exactly (where one label gives -log(1e-7) and the other log(1 + 1e-7), which float32 holds to 19 % only) stand
    among interior values, in every n that has room for them; n = 1 is one interior value."""
    rng = np.random.default_rng(n)
    p = rng.uniform(0.01, 0.99, (n, 1)).astype(np.float32)
    if n >= 255:
        p[[0, 100, 254, n - 1]] = np.array([[0.0], [1.0], [1.0], [0.0]], np.float32)
    for label in (0.0, 1.0):
        loss = nan_like((1,))
        dp = ops.log_loss(dev(p), label, loss)
        ref_l, ref_d = E.log_loss(label, p)
        print('log_loss n %d label %g: loss %.9g, reference %.9g' % (n, label, loss.item(), ref_l))
        assert abs(loss.item() - ref_l) < 1e-6 * abs(ref_l)
        close(dp, ref_d)


# ---- the module's figures ------------------------------------------------------------------------------------------------------
def test_the_figures_of_this_module():
    """Runs last: what the tests before it IN THIS PROCESS compared (vacuous under -k or workers that split the module)."""
    by_route = {}
    for route in TALLY['routes'].values():
        by_route[route] = by_route.get(route, 0) + 1
    print('exact loss-side tests: %d comparisons; largest magnitude / 2^24 = %.4f; GEMM rows per route: %s'
          % (TALLY['checks'], TALLY['magnitude'], ', '.join('%s %d' % kv for kv in sorted(by_route.items()))))
    assert TALLY['magnitude'] < 1.0
    if len(TALLY['routes']) == len(CASES):
        assert all(TALLY['routes'][case_id(c)] == c.route for c in CASES)
