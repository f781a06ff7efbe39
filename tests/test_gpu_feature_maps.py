"""The feature-map figure on the GPU: srx_feature_mosaic_u8 against the numpy restatement of the reference's layout
(exact), its stores against guard bytes at both alignments of `out`, the reference's own figures (P8: two whole images
by hash, four corners of two more layers by value), VdsrModel.feature_maps and the script around it."""
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.golden.make_golden import vdsr_params
from tests.test_feature_mosaic_host import full_maps, mosaic_ref, p8_hashes, p8_load, p8_tiles
from tests.test_oracle_pins import p7_decode, p7_load

pytestmark = pytest.mark.gpu


def _tw():
    from ml_super_resolution_amd import ops
    return ops.FEATURE_MOSAIC_TW


def make_input(N, H, W, seed=0):
    """uniform(-1.5, 1.5) (both clamps are reached), with values that sit ON a byte boundary and the clamps' ends mixed in."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, (N, H, W, 64)).astype(np.float32)
    flat = x.reshape(-1)
    special = np.concatenate([np.float32([-1.0, 0.0, 1.0, 3.0, -3.0]),
                              ((np.arange(256, dtype=np.float32) - np.float32(127.5)) / np.float32(127.5)).astype(np.float32)])
    idx = rng.permutation(flat.size)[:min(flat.size // 2, 4 * special.size)]
    flat[idx] = special[np.arange(idx.size) % special.size]
    return x


def restate_u8(u8):
    """[N,H,W,64] uint8 -> [N,8H,8W] uint8: the layout alone."""
    return np.stack([mosaic_ref(u8[n]) for n in range(u8.shape[0])])


def restate(x):
    """[N,H,W,64] float32 -> [N,8H,8W] uint8 on the CPU: encoding and layout."""
    return restate_u8(O.saturate_u8(x))


def _shapes():
    tw = 128        # = ops.FEATURE_MOSAIC_TW, asserted in test_kernel_matches_restatement (collection must not need the library)
    return [(1, 1, 1), (1, 3, 5), (1, 2, 15), (1, 2, 16), (1, 2, 17), (2, 5, 33), (1, 7, 24),
            (1, 2, tw - 1), (1, 2, tw), (1, 2, tw + 1), (1, 3, 2 * tw + 3)]


@pytest.mark.parametrize('shape', _shapes(), ids=lambda s: '%dx%dx%d' % s)
def test_kernel_matches_restatement(shape):
    from ml_super_resolution_amd import ops
    assert _tw() == 128
    x = make_input(*shape, seed=sum(shape))
    got = ops.feature_mosaic_u8(torch.from_numpy(x).cuda())
    N, H, W = shape
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, 8 * H, 8 * W)
    np.testing.assert_array_equal(got.cpu().numpy(), restate(x))


@pytest.mark.parametrize('misalign', [0, 1])
@pytest.mark.parametrize('shape', [(1, 2, 16), (1, 3, 129)], ids=lambda s: '%dx%dx%d' % s)
def test_nothing_outside_out_is_written(shape, misalign):
    """out as a view into a buffer of 0xA5 with 64 guard bytes on each side, starting on a 16-byte boundary and one byte
    after it: the choice between the 16-byte store and the narrower ones has to look at the pointer, not at W alone."""
    from ml_super_resolution_amd import ops
    assert shape[2] in (16, _tw() + 1)
    x = make_input(*shape, seed=7)
    numel = x.size
    buf = torch.full((numel + 160,), 0xA5, dtype=torch.uint8, device='cuda')
    start = 64 + (-(buf.data_ptr() + 64)) % 16 + misalign
    view = buf[start:start + numel]
    assert view.data_ptr() % 16 == misalign and start >= 64 and buf.numel() - (start + numel) >= 64
    got = ops.feature_mosaic_u8(torch.from_numpy(x).cuda(), out=view)
    assert got is view
    host = buf.cpu().numpy()
    np.testing.assert_array_equal(host[start:start + numel], restate(x).reshape(-1))
    assert (host[:start] == 0xA5).all() and (host[start + numel:] == 0xA5).all()


def test_op_argument_checks():
    from ml_super_resolution_amd import ops
    with pytest.raises(ValueError):
        ops.feature_mosaic_u8(torch.zeros((1, 2, 2, 32), device='cuda'))
    with pytest.raises(ValueError):
        ops.feature_mosaic_u8(torch.zeros((1, 2, 2, 64), device='cuda'), out=torch.zeros(7, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.feature_mosaic_u8(torch.zeros((1, 2, 2, 64)))


@pytest.mark.parametrize('name', ['conv1', 'conv19'])
def test_reference_whole_figure(name):
    """Every byte of the reference's vdsr-fig2-conv.1.png / conv.19.png, at the figure's own shape [1,256,256,64]."""
    from ml_super_resolution_amd import ops
    x = torch.from_numpy(p7_decode(full_maps()[name]).astype(np.float32)[None]).cuda()
    got = ops.feature_mosaic_u8(x).cpu().numpy()
    assert got.shape == (1, 2048, 2048)
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == p8_hashes()['sha256'][name]


@pytest.mark.parametrize('n', [2, 10])
def test_reference_corner_crops(n):
    from ml_super_resolution_amd import ops
    z, p8 = p7_load(), p8_load()
    C = int(z['corner'])
    x = torch.from_numpy(p7_decode(z['conv%d' % n]).astype(np.float32)).cuda()       # the four corners as a batch [4,C,C,64]
    got = ops.feature_mosaic_u8(x).cpu().numpy()
    for k in range(4):
        np.testing.assert_array_equal(p8_tiles(got[k], C), p8['conv%d' % n][k])


def _within_a_level(got, want):
    """tests/test_gpu_vdsr.py's bound for fp32 device arithmetic against the float64 oracle: a value next to an integer
    may truncate to the neighbouring byte."""
    got, want = got.astype(np.int32), want.astype(np.int32)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1 and (got != want).mean() < 0.01, (np.abs(got - want).max(), (got != want).mean())


def _oracle_maps(sd, params):
    """{file stem: uint8 array} of the float64 oracle for a batch sd [N,H,W,3]."""
    n = len(params)
    ref = O.vdsr_forward(sd, params)
    want = {'sd_image': O.saturate_u8(sd), 'sr_image': O.saturate_u8(ref['sr_images']), 'conv.%d' % n: O.saturate_u8(ref['conv.%d' % n])}
    for i in range(1, n):
        want['conv.%d' % i] = want['relu.%d' % i] = restate(ref['conv.%d' % i].astype(np.float32))
    return want


FEATURE_MAPS_SEED = 31      # fp32 oracle against float64 oracle at this seed: 0 differing bytes in every output (checked on the CPU)


def test_model_feature_maps():
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.engine import ConvStack
    from ml_super_resolution_amd.vdsr import model_vdsr
    layers = 4
    params = vdsr_params(FEATURE_MAPS_SEED, layers)
    m = model_vdsr.VdsrModel(layers, device='cuda')
    m.stack.set_params(params)
    sd = np.random.default_rng(FEATURE_MAPS_SEED).uniform(-1, 1, (2, 9, 13, 3)).astype(np.float32)
    maps = m.feature_maps(torch.from_numpy(sd).cuda())
    assert list(maps) == ['sd_image', 'sr_image', 'conv.1:0', 'relu.1:0', 'conv.2:0', 'relu.2:0', 'conv.3:0', 'relu.3:0', 'conv.4:0']
    assert maps['conv.2:0'] is maps['relu.2:0']
    assert all(t.is_cuda and t.dtype == torch.uint8 for t in maps.values())
    taps = m.taps()
    for i in range(1, layers):
        assert tuple(maps['conv.%d:0' % i].shape) == (2, 72, 104)
        np.testing.assert_array_equal(maps['conv.%d:0' % i].cpu().numpy(), restate_u8(ops.saturate_u8(taps['conv.%d' % i]).cpu().numpy()))
    want = _oracle_maps(sd, params)
    for key, t in maps.items():
        _within_a_level(t.cpu().numpy(), want[key[:-2] if key.endswith(':0') else key])
    narrow = model_vdsr.VdsrModel(3, device='cuda')
    narrow.stack = ConvStack(model_vdsr.layer_specs(3, width=32), device='cuda', residual=True)     # a body of 32 maps: no 8 x 8 mosaic
    with pytest.raises(ValueError):
        narrow.feature_maps(torch.from_numpy(sd).cuda())


def test_experiment_feature_map_visualize_script(tmp_path):
    """vdsr/vdsr/experiment_feature_map_visualize.py: TF-format checkpoint and an image in, the reference's set of PNGs out."""
    from PIL import Image
    from ml_super_resolution_amd.vdsr import dataset, experiment_feature_map_visualize, model_vdsr
    layers = 5
    params = vdsr_params(77, layers)
    m = model_vdsr.VdsrModel(layers, device='cuda')
    m.stack.set_params(params)
    prefix = str(tmp_path / 'model.ckpt-10')
    m.stack.save_tf_checkpoint(prefix)
    img = np.random.default_rng(5).integers(0, 256, (23, 31, 3), dtype=np.uint8)
    src, out = str(tmp_path / 'in.png'), str(tmp_path / 'maps')
    Image.fromarray(img).save(src)
    experiment_feature_map_visualize.main(['--ckpt_path', prefix, '--hd_image_path', src, '--result_dir_path', out,
                                           '--num_layers', str(layers), '--scaling_factor', '2'])
    names = ['sd_image', 'sr_image'] + ['conv.%d' % i for i in range(1, 6)] + ['relu.%d' % i for i in range(1, 5)]
    assert sorted(os.listdir(out)) == sorted(n + '.png' for n in names)
    sd = dataset.hd_image_to_sd_image(img.astype(np.float32) / np.float32(255.0), 2)
    want = _oracle_maps((sd * 2.0 - 1.0)[None].astype(np.float32), params)
    got = {}
    for n in names:
        im = Image.open(os.path.join(out, n + '.png'))
        if n in ('sd_image', 'sr_image', 'conv.5'):
            assert im.mode == 'RGB' and im.size == (31, 23), (n, im.mode, im.size)
        else:
            assert im.mode == 'L' and im.size == (248, 184), (n, im.mode, im.size)
        got[n] = np.asarray(im)
        _within_a_level(got[n], want[n][0])
    for i in range(1, 5):
        np.testing.assert_array_equal(got['relu.%d' % i], got['conv.%d' % i])
