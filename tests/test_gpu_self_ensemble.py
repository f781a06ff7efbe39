"""Geometric self-ensemble on the GPU: srx_dihedral_expand / srx_dihedral_merge against their numpy restatement
(tests/dihedral_ref.py), bit for bit; forward_ensemble of the three models against merge_ref of plain forward passes on
uploaded expand_ref batches; and the --self_ensemble flag of the five scripts."""
import os

import numpy as np
import pytest
import torch

from tests.dihedral_ref import expand_ref, merge_ref

pytestmark = pytest.mark.gpu

# 1 x 1; one row, one column; odd sizes on both sides of the 32-pixel tile and H != W; exactly one tile; more than one
# tile per axis with C = 4, 8 (a 16-byte pixel, the widest) and 3 (a 12-byte pixel: rows at any 4-byte alignment)
SHAPES = ((1, 1, 1, 3), (1, 1, 37, 3), (1, 37, 1, 3), (2, 31, 33, 3), (1, 32, 32, 1), (1, 33, 65, 4), (2, 64, 40, 8), (1, 70, 45, 3))
IDS = ['x'.join(map(str, s)) for s in SHAPES]


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    assert a.dtype == np.float32
    return a.view(np.int32)


def assert_same_bits(got, want, what=''):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), '%s: %d of %d floats differ' % (what, int((g != w).sum()), g.size)


def shifted(shape, fill=None):
    """A contiguous tensor of this shape that starts one float behind a 16-byte boundary."""
    n = int(np.prod(shape))
    buf = torch.empty(n + 4, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    t = buf[1:1 + n].view(shape)
    if fill is not None:
        t.copy_(torch.from_numpy(fill))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def group_shapes(shape):
    n, h, w, c = shape
    return (4 * n, h, w, c), (4 * n, w, h, c)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_expand_equals_reference(shape):
    from ml_super_resolution_amd import ops
    x = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    a, b = ops.dihedral_expand(torch.from_numpy(x).cuda())
    want_a, want_b = expand_ref(x)
    assert_same_bits(a, want_a, 'a')
    assert_same_bits(b, want_b, 'b')


def test_expand_at_four_byte_alignment():
    """x, a and b each one float behind a 16-byte boundary, C = 3: no access may assume more than 4-byte alignment."""
    from ml_super_resolution_amd import ops
    shape = (2, 31, 33, 3)
    x = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
    sa, sb = group_shapes(shape)
    out = (shifted(sa), shifted(sb))
    a, b = ops.dihedral_expand(shifted(shape, x), out=out)
    assert a.data_ptr() == out[0].data_ptr() and b.data_ptr() == out[1].data_ptr()
    want_a, want_b = expand_ref(x)
    assert_same_bits(a, want_a, 'a')
    assert_same_bits(b, want_b, 'b')


@pytest.mark.parametrize('shape', ((1, 70, 45, 3), (1, 33, 65, 4)), ids=('70x45x3', '33x65x4'))
def test_poisoned_lds_does_not_show(shape):
    """Every CU's LDS is filled with NaNs first (srx_debug_poison_lds): a read of LDS the kernel has not written shows."""
    from ml_super_resolution_amd import _lib, ops
    rng = np.random.default_rng(6)
    x = rng.standard_normal(shape).astype(np.float32)
    sa, sb = group_shapes(shape)
    ya, yb = rng.standard_normal(sa).astype(np.float32), rng.standard_normal(sb).astype(np.float32)
    xd, yad, ybd = (torch.from_numpy(v).cuda() for v in (x, ya, yb))
    _lib.check(_lib.lib().srx_debug_poison_lds(ops._stream()), 'srx_debug_poison_lds')
    a, b = ops.dihedral_expand(xd)
    _lib.check(_lib.lib().srx_debug_poison_lds(ops._stream()), 'srx_debug_poison_lds')
    m = ops.dihedral_merge(yad, ybd)
    want_a, want_b = expand_ref(x)
    assert_same_bits(a, want_a, 'a')
    assert_same_bits(b, want_b, 'b')
    assert_same_bits(m, merge_ref(ya, yb), 'merge')


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_merge_equals_reference(shape):
    """a and b independent random floats, not an expand output: eight equal values would hide a wrong inverse."""
    from ml_super_resolution_amd import ops
    rng = np.random.default_rng(100 + sum(shape))
    sa, sb = group_shapes(shape)
    a, b = rng.standard_normal(sa).astype(np.float32), rng.standard_normal(sb).astype(np.float32)
    got = ops.dihedral_merge(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert tuple(got.shape) == shape
    assert_same_bits(got, merge_ref(a, b))


def test_merge_add_order_is_pinned_by_large_magnitudes():
    """Each float is +-1e30 or of order 1: fp32 sums of these depend on the order of the adds (1e30 + 1 - 1e30 is 0 in
    one order and 1 in another).  Eight times 1e30 is far below the largest float: nothing overflows, no NaN."""
    from ml_super_resolution_amd import ops
    shape = (2, 31, 33, 3)
    rng = np.random.default_rng(7)
    sa, sb = group_shapes(shape)

    def values(s):
        small = rng.standard_normal(s).astype(np.float32)
        big = rng.choice(np.array([1e30, -1e30], np.float32), size=s)
        return np.where(rng.random(s) < 0.5, big, small).astype(np.float32)
    a, b = values(sa), values(sb)
    want = merge_ref(a, b)
    assert np.isfinite(want).all()
    # the fixture can see the order: the sum of the two groups' own sums (a tree, not a chain) has other bits somewhere
    tree = ((_group_sum(a, 0) + _group_sum(b, 4)) * np.float32(0.125)).astype(np.float32)
    assert not np.array_equal(tree.view(np.int32), want.view(np.int32))
    assert_same_bits(ops.dihedral_merge(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()), want)


def _group_sum(g, k0):
    """Sequential float32 sum of the four inverses of one group (k0 = 0: the A group, 4: the B group)."""
    from tests.dihedral_ref import T_inv
    n = g.shape[0] // 4
    acc = None
    for k in range(4):
        u = np.ascontiguousarray(T_inv(k0 + k, g[k * n:k * n + n]), dtype=np.float32)
        acc = u if acc is None else (acc + u).astype(np.float32)
    return acc


@pytest.mark.parametrize('shape', ((2, 31, 33, 3), (1, 70, 45, 3), (1, 24, 24, 3)), ids=('31x33', '70x45', '24x24'))
def test_round_trip_on_integers_is_exact(shape):
    from ml_super_resolution_amd import ops
    x = np.random.default_rng(8).integers(-(1 << 20), (1 << 20) + 1, size=shape).astype(np.float32)
    got = ops.dihedral_merge(*ops.dihedral_expand(torch.from_numpy(x).cuda()))
    assert_same_bits(got, x)


def test_out_buffers_are_honoured_and_fully_overwritten():
    from ml_super_resolution_amd import ops
    shape = (2, 31, 33, 3)
    rng = np.random.default_rng(9)
    sa, sb = group_shapes(shape)
    a = torch.full(sa, float('nan'), device='cuda')
    b = torch.full(sb, float('nan'), device='cuda')
    o = torch.full(shape, float('nan'), device='cuda')
    for _ in range(2):                                # the second call, with other data, leaves nothing of the first
        x = rng.standard_normal(shape).astype(np.float32)
        ra, rb = ops.dihedral_expand(torch.from_numpy(x).cuda(), out=(a, b))
        assert ra is a and rb is b
        want_a, want_b = expand_ref(x)
        assert_same_bits(a, want_a, 'a')
        assert_same_bits(b, want_b, 'b')
        ya, yb = rng.standard_normal(sa).astype(np.float32), rng.standard_normal(sb).astype(np.float32)
        assert ops.dihedral_merge(torch.from_numpy(ya).cuda(), torch.from_numpy(yb).cuda(), out=o) is o
        assert_same_bits(o, merge_ref(ya, yb), 'merge')
    with pytest.raises(ValueError):
        ops.dihedral_expand(torch.zeros(shape, device='cuda'), out=(a, a))          # b has the transposed shape
    with pytest.raises(ValueError):
        ops.dihedral_merge(a, a)
    with pytest.raises(ValueError):
        ops.dihedral_merge(a, b, out=torch.empty((1, 31, 33, 3), device='cuda'))


# ---- models ----------------------------------------------------------------------------------------------------------

def _vdsr():
    from ml_super_resolution_amd.vdsr import model_vdsr
    m = model_vdsr.VdsrModel(4, device='cuda', seed=11)
    return m, (lambda x: m.forward(x)), m.forward_ensemble, 1


def _srcnn():
    from ml_super_resolution_amd.srcnn import srcnn
    m = srcnn.SrcnnModel(srcnn._flags().parse_args([]), device='cuda', seed=12)
    for i, scale in enumerate((40.0, 80.0, 30.0)):       # weights of a size that gives an output worth comparing
        m.stack.kernel(i).mul_(scale)
    return m, (lambda x: m.forward(x)), m.forward_ensemble, 1


def _enet():
    from ml_super_resolution_amd.enet import model_enet
    g = model_enet.EnetGenerator(device='cuda', seed=13)
    for w in g.kernels:         # sigma 0.06: a gain near 1 per 3x3 64 -> 64 layer, a residual of a size worth comparing
        w.mul_(3.0)
    return g, (lambda sd, bq: g.forward(sd, bq)), g.forward_ensemble, 2


@pytest.mark.parametrize('make', (_vdsr, _srcnn, _enet), ids=('vdsr', 'srcnn', 'enet'))
@pytest.mark.parametrize('hw', ((24, 36), (24, 24)), ids=('24x36', '24x24'))
def test_forward_ensemble_equals_the_eight_plain_passes(make, hw):
    """forward_ensemble against merge_ref of plain forward on the uploaded expand_ref batches: the same bits in, the same
    shapes, hence the same kernel routes and the same bits out.  24 x 24 is the hazard: the A and B batches have one
    shape, and the models hand out the same buffer for both."""
    _, forward, forward_ensemble, n_inputs = make()
    rng = np.random.default_rng(hw[0] * hw[1])
    inputs = [rng.uniform(-1, 1, (1, hw[0] * s, hw[1] * s, 3)).astype(np.float32) for s in (1, 4)[:n_inputs]]
    groups = [expand_ref(x) for x in inputs]
    ya = forward(*[torch.from_numpy(g[0]).cuda() for g in groups]).cpu().numpy()
    yb = forward(*[torch.from_numpy(g[1]).cuda() for g in groups]).cpu().numpy()
    want = merge_ref(ya, yb)
    dev = [torch.from_numpy(x).cuda() for x in inputs]
    got = forward_ensemble(*dev)
    assert_same_bits(got, want)
    for x, d in zip(inputs, dev):
        assert_same_bits(d, x, 'an input was written')
    plain = forward(*dev).cpu().numpy()
    assert plain.shape == want.shape
    diff = np.abs(plain - want).max()
    print('max |ensemble - plain| = %.3g (max |plain| %.3g)' % (diff, np.abs(plain).max()))
    assert diff > 0, 'random weights are not symmetric: the ensemble must differ from one pass'


# ---- scripts ---------------------------------------------------------------------------------------------------------

PNG_SIZES = ((24, 36), (40, 24))       # (height, width)


@pytest.fixture(scope='module')
def png_dir(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp('self_ensemble_pngs')
    rng = np.random.default_rng(14)
    for k, (h, w) in enumerate(PNG_SIZES):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(str(d / ('im%d.png' % k)))
    return d


@pytest.fixture(scope='module')
def vdsr_ckpt(tmp_path_factory):
    from ml_super_resolution_amd.vdsr import model_vdsr
    path = str(tmp_path_factory.mktemp('self_ensemble_vdsr') / 'model.ckpt-0.pt')
    torch.save(model_vdsr.VdsrModel(4, device='cuda', seed=15).stack.state_dict(), path)
    return path


def _vdsr_model(ckpt):
    from ml_super_resolution_amd.vdsr import model_vdsr
    m = model_vdsr.VdsrModel(4, device='cuda')
    m.stack.load_checkpoint(ckpt)
    return m


def test_vdsr_evaluate_flag(png_dir, vdsr_ckpt):
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.vdsr import experiment_evaluate
    argv = ['--ckpt_path', vdsr_ckpt, '--hd_image_dir_path', str(png_dir), '--num_layers', '4', '--scaling_factor', '2']
    plain = experiment_evaluate.main(argv)
    got = experiment_evaluate.main(argv + ['--self_ensemble'])
    assert got['names'] == plain['names'] == ['im0.png', 'im1.png']
    assert got['sd_psnrs'] == plain['sd_psnrs'] and got['sd_ssims'] == plain['sd_ssims']
    m = _vdsr_model(vdsr_ckpt)
    for k, name in enumerate(got['names']):
        sd, hd = (torch.from_numpy(v).cuda() for v in experiment_evaluate.load_image(str(png_dir / name), 2))
        sr = m.forward_ensemble(sd)
        assert got['sr_psnrs'][k] == ops.psnr(hd, sr, 2.0).item(), k
        assert got['sr_ssims'][k] == ops.ssim(hd, sr, 2.0).item(), k
        assert got['sr_psnrs'][k] != plain['sr_psnrs'][k], k
        assert plain['sr_psnrs'][k] == ops.psnr(hd, m.forward(sd), 2.0).item(), k       # flag off: as before


def test_vdsr_resolve_flag(png_dir, vdsr_ckpt, tmp_path):
    from PIL import Image
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.vdsr import dataset, experiment_resolve
    src = str(png_dir / 'im0.png')
    argv = ['--ckpt_path', vdsr_ckpt, '--hd_image_path', src, '--num_layers', '4', '--scaling_factor', '2']
    experiment_resolve.main(argv + ['--sr_image_path', str(tmp_path / 'plain_sr.png')])
    experiment_resolve.main(argv + ['--sr_image_path', str(tmp_path / 'ens_sr.png'), '--self_ensemble'])
    m = _vdsr_model(vdsr_ckpt)
    hd = np.asarray(Image.open(src).convert('RGB')).astype(np.float32) / 255.0
    sd = torch.from_numpy((dataset.hd_image_to_sd_image(hd, 2.0) * 2.0 - 1.0)[None].astype(np.float32)).cuda()
    want = ops.saturate_u8(m.forward_ensemble(sd))[0].cpu().numpy()
    assert np.asarray(Image.open(str(tmp_path / 'ens_sr.png'))).tobytes() == want.tobytes()
    assert np.asarray(Image.open(str(tmp_path / 'plain_sr.png'))).tobytes() == ops.saturate_u8(m.forward(sd))[0].cpu().numpy().tobytes()


@pytest.fixture(scope='module')
def enet_prefix(tmp_path_factory):
    from ml_super_resolution_amd import tf_bundle
    from ml_super_resolution_amd.enet import model_enet
    prefix = str(tmp_path_factory.mktemp('self_ensemble_enet') / 'model.ckpt')
    g = model_enet.EnetGenerator(device='cuda', seed=16)
    for w in g.kernels:         # the initial weights (sigma 0.02) leave sr = bq to the last bit of a score: three times that
        w.mul_(3.0)             # gives every 3x3 64 -> 64 layer a gain near 1, and a residual that moves the scores
    tf_bundle.save_checkpoint(prefix, {name: t.cpu().numpy() for name, t in g.variables().items()})
    return prefix


def test_enet_evaluate_flag(png_dir, enet_prefix):
    """sr scores are those of ops.image_scores, as the script computes them, on the ensemble output; bq is untouched; both
    --pairs routes."""
    from ml_super_resolution_amd import image_arena, ops
    from ml_super_resolution_amd.enet import experiment_evaluate, experiment_resolve
    argv = ['--source_ckpt_path', enet_prefix, '--hd_dir_path', str(png_dir)]
    plain = experiment_evaluate.main(argv)
    got = experiment_evaluate.main(argv + ['--self_ensemble'])
    assert got == experiment_evaluate.main(argv + ['--self_ensemble', '--pairs', 'device'])
    assert got['names'] == plain['names'] == ['im0.png', 'im1.png']
    assert got['bq_psnrs'] == plain['bq_psnrs'] and got['bq_ssims'] == plain['bq_ssims']
    g = experiment_resolve.load_generator(enet_prefix, 'cuda')
    for k, name in enumerate(got['names']):
        sd, bq, hd = experiment_evaluate.host_pair(image_arena.decode_rgb(str(png_dir / name)), torch.device('cuda'), name)
        want = ops.image_scores(hd, [bq, g.forward_ensemble(sd, bq)], 1.0, space='rgb', unit_clip=True).cpu().numpy()
        assert (got['sr_psnrs'][k], got['sr_ssims'][k]) == (float(want[1, 0, 0]), float(want[1, 0, 1])), k
        assert got['sr_psnrs'][k] != plain['sr_psnrs'][k], k


def test_enet_resolve_flag(png_dir, enet_prefix, tmp_path):
    from PIL import Image
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.enet import experiment_resolve
    argv = ['--source_ckpt_path', enet_prefix, '--source_dir_path', str(png_dir)]
    experiment_resolve.main(argv + ['--target_dir_path', str(tmp_path / 'plain')])
    experiment_resolve.main(argv + ['--target_dir_path', str(tmp_path / 'ens'), '--self_ensemble'])
    g = experiment_resolve.load_generator(enet_prefix, 'cuda')
    for k in range(len(PNG_SIZES)):
        sd_u8 = torch.from_numpy(np.array(Image.open(str(png_dir / ('im%d.png' % k))).convert('RGB'))[None]).cuda()
        bq_u8 = ops.resize_pil_u8(sd_u8, sd_u8.shape[1] * 4, sd_u8.shape[2] * 4, 'bicubic')
        sd, bq = ops.u8_to_pm1(sd_u8), ops.u8_to_pm1(bq_u8)
        want = ops.saturate_u8(g.forward_ensemble(sd, bq))[0].cpu().numpy()
        assert np.asarray(Image.open(str(tmp_path / 'ens' / ('im%d_sr.png' % k)))).tobytes() == want.tobytes(), k
        plain = ops.saturate_u8(g.forward(sd, bq))[0].cpu().numpy()
        assert np.asarray(Image.open(str(tmp_path / 'plain' / ('im%d_sr.png' % k)))).tobytes() == plain.tobytes(), k
        for s in ('plain', 'ens'):
            assert np.asarray(Image.open(str(tmp_path / s / ('im%d_bq.png' % k)))).tobytes() == ops.saturate_u8(bq)[0].cpu().numpy().tobytes()


def test_srcnn_evaluate_flag(png_dir, tmp_path):
    from ml_super_resolution_amd import image_arena, ops
    from ml_super_resolution_amd.srcnn import evaluate, srcnn
    ckpt = tmp_path / 'ckpts'
    os.makedirs(str(ckpt))
    m = srcnn.SrcnnModel(srcnn._flags().parse_args(['--upscaling-factor', '3']), device='cuda', seed=17)
    for i, scale in enumerate((40.0, 80.0, 30.0)):
        m.stack.kernel(i).mul_(scale)
    m.stack.save_tf_checkpoint(str(ckpt / 'model.ckpt-0'), adam_betas=(0.5, 0.9))
    argv = ['--ckpt-dir-path', str(ckpt), '--hd-dir-path', str(png_dir)]
    plain = evaluate.main(argv)
    got = evaluate.main(argv + ['--self-ensemble'])
    assert got == evaluate.main(argv + ['--self-ensemble', '--pairs', 'device'])
    assert got['names'] == plain['names'] == ['im0.png', 'im1.png']
    assert got['bq_psnrs'] == plain['bq_psnrs'] and got['bq_ssims'] == plain['bq_ssims']
    model = evaluate.load_model(str(ckpt), 3, torch.device('cuda', torch.cuda.current_device()))
    for k, name in enumerate(got['names']):
        sd, bq, hd = evaluate.host_triple(model, image_arena.decode_rgb(str(png_dir / name)), 'cuda')
        want = ops.image_scores(hd, [bq, model.forward_ensemble(sd)], 2.0).cpu().numpy()
        assert (got['sr_psnrs'][k], got['sr_ssims'][k]) == (float(want[1, 0, 0]), float(want[1, 0, 1])), k
        assert got['sr_psnrs'][k] != plain['sr_psnrs'][k], k
