"""One 720 x 1280 frame -- the size every whole-image number of DESIGN.md is quoted at -- against the oracle, layer
by layer, on the default routes.  The per-route tests stop at about 463 rows x 400 columns; what only a frame has (40 column
strips x 720 rows, the grid cap of 2 x 256 workgroups, workgroup ranges that cut strips mid-image, offsets near the 32-bit
guards) was until now covered by bit-identity with conv path 0 alone (tests/test_gpu_subpixel_fused.py), which shares
make_plan / geometry / fill_conv_args with the routes it vouches for.

The oracle runs on SLABS: `oracle_rows` cuts the input rows that output rows [r0, r1) read, adds the zero rows (and columns)
SAME padding implies by hand and runs the C oracle's VALID convolution on the slab -- exactly the rows the whole-image
oracle would give (tests/test_host_logic.py proves that on small shapes, without a GPU).  Every column is kept, so every
column strip is inside every sampled row.

Row sample of every layer (`sample_rows`): the first 16 and the last 16 output rows; one band of 48 rows starting at a row
that is not a multiple of 16 (at least two seams of the tallest tile, 16 rows, and several workgroup-range cuts inside it);
every 31st row (31 is coprime to every tile height).  That is 100 distinct rows in 23 bands: 13.9 % of 720 output rows,
14.0 % / 14.1 % of SRCNN's 712 / 708; every layer asserts that its share is at least 10 %.

Two oracles take the slabs: the float64 NumPy convolution is the reference of the derived bound, the C restatement (which
accumulates in float32 itself) that of `close`.  Each layer's oracle input is the GPU's own output of the layer before, copied to the host: a miss names one kernel and
errors do not compound.  Layers without activation or with ReLU are held to the derived per-element bound
(tests/test_gpu_ops.close_elementwise); a tanh layer runs twice on the same route: without its tanh under the derived bound,
with it under the suite's 1e-3 `close` (the device tanh's own error is not derivable).  Outputs are pre-filled with NaN.

Wall time on one MI355X host (16 threads for the oracles): 3.0 s for the three tests, 2 % of the 148 s `-m gpu` suite.  Largest
|err| / derived bound seen per layer (printed on every run): between 0.002 (SRCNN f3, VDSR's last layer) and 0.09 (SRCNN's 1x1)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.test_gpu_ops import close, close_elementwise, close_elementwise_bwd_data

pytestmark = pytest.mark.gpu

H, W = 720, 1280
MIN_SHARE = 0.10


# ---- the slab oracle (host only; proven in tests/test_host_logic.py) ------------------------------------------------------
def oracle_rows(x, w, b, padding, act, r0, r1, skip=None, oracle=None):
    """Rows [r0, r1) of O.c_conv2d_fwd(x, w, b, padding, act, skip=skip) computed from the input rows they read.  `oracle`:
    O.c_conv2d_fwd (the default: the C restatement, float32 accumulation, the reference of `close`) or O.conv2d_fwd (NumPy,
    float64: the reference of the derived bound)."""
    x = np.asarray(x, np.float32)
    n, h, wd, c = x.shape
    kh, kw = w.shape[:2]
    pad_t, pad_l, oh, ow = O.conv_geometry(h, wd, kh, kw, padding)
    assert 0 <= r0 < r1 <= oh, (r0, r1, oh)
    lo, hi = r0 - pad_t, r1 - pad_t + kh - 1             # input rows [lo, hi), some of them outside the image under SAME
    top, bottom = max(0, -lo), max(0, hi - h)
    right = ow + kw - 1 - pad_l - wd
    slab = np.pad(x[:, max(lo, 0):min(hi, h)], ((0, 0), (top, bottom), (pad_l, right), (0, 0)))
    assert slab.shape[1] == r1 - r0 + kh - 1 and slab.shape[2] == ow + kw - 1
    return (oracle or O.c_conv2d_fwd)(slab, w, b, 'VALID', act, skip=None if skip is None else skip[:, r0:r1])


def oracle_rows_bwd_data(dpre, w, in_hw, padding, r0, r1, oracle=None):
    """Rows [r0, r1) of O.c_conv2d_bwd_data(dpre, w, in_hw, padding): the mirror image -- the gradient rows that input rows
    [r0, r1) receive from, run through the VALID data gradient (whose result has KH - 1 more rows and KW - 1 more columns
    than its operand: the rows / columns beyond the image are the ones SAME padding would have dropped)."""
    dpre = np.asarray(dpre, np.float32)
    h, wd = in_hw
    kh, kw = w.shape[:2]
    pad_t, pad_l, oh, ow = O.conv_geometry(h, wd, kh, kw, padding)
    assert 0 <= r0 < r1 <= h and dpre.shape[1:3] == (oh, ow)
    a, b = max(0, r0 + pad_t - (kh - 1)), min(oh, r1 + pad_t)       # gradient rows [a, b)
    full = (oracle or O.c_conv2d_bwd_data)(dpre[:, a:b], w, (b - a + kh - 1, ow + kw - 1), 'VALID')
    return full[:, r0 + pad_t - a:r1 + pad_t - a, pad_l:pad_l + wd]


def sample_rows(oh):
    """The sorted output rows every layer is checked at (module docstring)."""
    start = oh // 2 + 5
    assert start % 16 != 0 and start + 48 <= oh - 16
    rows = set(range(16)) | set(range(oh - 16, oh)) | set(range(start, start + 48)) | set(range(0, oh, 31))
    return sorted(rows)


def bands(rows):
    """[(r0, r1)]: the runs of consecutive rows."""
    out = []
    for r in rows:
        if out and out[-1][1] == r:
            out[-1][1] = r + 1
        else:
            out.append([r, r + 1])
    return [tuple(b) for b in out]


# ---- GPU side -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ops():
    from ml_super_resolution_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _layer(rng, k, cin, cout):
    w = rng.normal(0, 1.0 / np.sqrt(k * k * cin), (k, k, cin, cout)).astype(np.float32)
    return w, rng.uniform(-0.1, 0.1, (cout,)).astype(np.float32)


def _take_rows(t, rows, r=1):
    """Rows of a device tensor [1, OH * r, ...] that belong to output rows `rows` (r: the sub-pixel factor), on the host."""
    idx = torch.as_tensor([r * q + d for q in rows for d in range(r)], device=t.device)
    return t.index_select(1, idx).cpu().numpy()


def check_forward_layer(ops, x, w, b, padding, act, what, skip=None, subpixel_r=0):
    """Runs one layer on the GPU on its default route into a NaN-filled output and checks the sampled rows; returns the
    layer's output (device tensor) for the next layer."""
    xh = x.cpu().numpy()
    kh, kw, _, cout = w.shape
    _, _, oh, ow = O.conv_geometry(xh.shape[1], xh.shape[2], kh, kw, padding)
    rows = sample_rows(oh)
    assert len(rows) >= MIN_SHARE * oh, (len(rows), oh)
    r = max(subpixel_r, 1)
    out_shape = (1, oh * r, ow * r, cout // (r * r))
    wd, bd = _dev(w), _dev(b)
    sd = None if skip is None else _dev(skip)

    def run(a):
        y = torch.full(out_shape, float('nan'), device='cuda')
        got = ops.conv2d_fwd(x, wd, bd, padding.lower(), a, skip=sd, out=y, subpixel_r=subpixel_r)
        assert got.data_ptr() == y.data_ptr()
        assert torch.isfinite(y).all(), '%s: an output element was not written (or is not finite)' % what
        return y

    def conv(x_, w_, b_, act_, skip_, oracle=O.conv2d_fwd):
        ref = np.concatenate([oracle_rows(x_, w_, b_, padding, act_, r0, r1, skip=skip_, oracle=oracle) for r0, r1 in bands(rows)], axis=1)
        return O.depth_to_space(ref, subpixel_r) if subpixel_r > 1 else ref
    row_index = [r * q + d for q in rows for d in range(r)]
    y = run(act)
    exact = y if act in (None, 'relu') else run(None)
    worst = close_elementwise(_take_rows(exact, rows, r), xh, w, b, padding, act if act in (None, 'relu') else None, skip, conv=conv,
                              what=what + (' (without its %s)' % act if exact is not y else ''), rows=row_index)
    print('%s: largest |err| / derived bound on %d of %d rows: %.4f' % (what, len(rows), oh, worst))
    if exact is not y:
        close(_take_rows(y, rows, r), conv(xh, w, b, act, skip, oracle=O.c_conv2d_fwd))
    return y


def test_espcn_720p_layers_vs_oracle_slabs(ops):
    """ESPCN r = 3 (espcn/espcn/model_espcn.py:117-134): f1 5x5 3 -> 64 tanh (conv_pack3_kernel), f2 3x3 64 -> 32 tanh (the
    two-chunk pipelined strips, 40 strips x 720 rows), f3 3x3 32 -> 27 through the sub-pixel store (the same strips with the
    map as epilogue): output rows 3 r0 .. 3 r1 of the [1, 2160, 3840, 3] image against depth_to_space of the oracle slab."""
    rng = np.random.default_rng(7201)
    x = _dev(rng.uniform(-1, 1, (1, H, W, 3)))
    w1, b1 = _layer(rng, 5, 3, 64)
    w2, b2 = _layer(rng, 3, 64, 32)
    w3, b3 = _layer(rng, 3, 32, 27)
    t1 = check_forward_layer(ops, x, w1, b1, 'SAME', 'tanh', 'ESPCN f1 5x5 3->64')
    t2 = check_forward_layer(ops, t1, w2, b2, 'SAME', 'tanh', 'ESPCN f2 3x3 64->32')
    hr = check_forward_layer(ops, t2, w3, b3, 'SAME', None, 'ESPCN f3 3x3 32->27 sub-pixel store', subpixel_r=3)
    assert hr.shape == (1, 3 * H, 3 * W, 3)


def test_srcnn_720p_layers_vs_oracle_slabs(ops):
    """SRCNN 9-1-5 VALID (srcnn/srcnn.py:100-130): f1 9x9 3 -> 64 ReLU (conv_pack3_kernel<9,9>), f2 1x1 64 -> 32 ReLU
    (conv_1x1_kernel), f3 5x5 32 -> 3 tanh (conv_kwrows_kernel, whose order of the kw partial sums differs from the other
    kernels': the derived bound holds for any order)."""
    rng = np.random.default_rng(7202)
    x = _dev(rng.uniform(-1, 1, (1, H, W, 3)))
    w1, b1 = _layer(rng, 9, 3, 64)
    w2, b2 = _layer(rng, 1, 64, 32)
    w3, b3 = _layer(rng, 5, 32, 3)
    t1 = check_forward_layer(ops, x, w1, b1, 'VALID', 'relu', 'SRCNN f1 9x9 3->64')
    t2 = check_forward_layer(ops, t1, w2, b2, 'VALID', 'relu', 'SRCNN f2 1x1 64->32')
    y = check_forward_layer(ops, t2, w3, b3, 'VALID', 'tanh', 'SRCNN f3 5x5 32->3')
    assert y.shape == (1, H - 12, W - 12, 3)


def test_vdsr_720p_body_layer_forward_dgrad_and_last_layer_vs_oracle_slabs(ops):
    """VDSR on a whole image (vdsr/vdsr/model_vdsr.py:62-104): one body layer 3x3 64 -> 64 SAME ReLU forward on the column
    strips of the pipelined kernel; its data gradient with the upstream ReLU mask fused (in_act='relu') against the oracle's
    data gradient on the mirrored slab times the mask; the last layer 64 -> 3 with the residual `skip` operand."""
    rng = np.random.default_rng(7203)
    x = np.maximum(rng.uniform(-1, 1, (1, H, W, 64)), 0).astype(np.float32)        # (a ReLU output, as a body layer reads)
    xd = _dev(x)
    w, b = _layer(rng, 3, 64, 64)
    t = check_forward_layer(ops, xd, w, b, 'SAME', 'relu', 'VDSR body 3x3 64->64 forward')
    # masked data gradient
    rows = sample_rows(H)
    assert len(rows) >= MIN_SHARE * H
    dpre = rng.normal(0, 1, (1, H, W, 64)).astype(np.float32)
    dx = torch.full((1, H, W, 64), float('nan'), device='cuda')
    got = ops.conv2d_bwd_data(_dev(dpre), _dev(w), (1, H, W, 64), 'same', x_in=xd, in_act='relu', out=dx)
    assert got.data_ptr() == dx.data_ptr() and torch.isfinite(dx).all()
    conv = lambda d_, w_: np.concatenate([oracle_rows_bwd_data(d_, w_, (H, W), 'SAME', r0, r1, oracle=O.conv2d_bwd_data)
                                          for r0, r1 in bands(rows)], axis=1)
    worst = close_elementwise_bwd_data(_take_rows(dx, rows), dpre, w, (H, W), 'SAME', mask=(x[:, rows] > 0), conv=conv,
                                       what='VDSR body 3x3 64->64 masked data gradient', rows=rows)
    print('VDSR body 3x3 64->64 masked data gradient: largest |err| / derived bound on %d of %d rows: %.4f' % (len(rows), H, worst))
    # the output layer: conv + bias + the network's input (3 channels)
    w3, b3 = _layer(rng, 3, 64, 3)
    sd = rng.uniform(-1, 1, (1, H, W, 3)).astype(np.float32)
    check_forward_layer(ops, t, w3, b3, 'SAME', None, 'VDSR last layer 3x3 64->3 + skip', skip=sd)
