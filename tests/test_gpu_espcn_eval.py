"""ESPCN's evaluation pairs built on the device (srx_espcn_eval_pairs, espcn/dataset.py: DeviceEvalSet): six small images at
every r against the reference arithmetic (espcn/espcn/experiment_test.py:60-98: trim, float64 map, whole-image blur by the
oracle, decimation, label layout), against the patch kernel bit for bit, independence of the images, the wrappers'
refusals, experiment_scores --pairs device and experiment_train's validation flags.

Bounds: the label has none -- (float)(u8 / 127.5 - 1.0) from float64, bit for bit.  lr: 2e-5, the bound
tests/test_gpu_espcn_pairs.py derives for this very arithmetic on [-1, 1] data (twice the 1e-5 tests/test_gpu_ops.py allows
srx_gaussian_blur on [0, 1] data against the same oracle).  The tests print what they measure (pytest -s); the figures
of one MI355X are in DESIGN.md 3.21."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.eval_tables import _pngs

gpu = pytest.mark.gpu

TOL = 2e-5
T = 16                                     # SRX_ESPCN_EVAL_TILE: at another T, add sizes whose lr side is T, T + 1 and 2 T
SHAPES = ((9, 9), (23, 31), (40, 37), (64, 52), (120, 75), (131, 135))
FACTORS = (2, 3, 4)


def make_images():
    """Half random, half hard-edged (every byte 0 or 255)."""
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) if k % 2 == 0
            else (rng.integers(0, 2, size=(h, w, 3), dtype=np.uint8) * np.uint8(255)) for k, (h, w) in enumerate(SHAPES)]


def trimmed(img, r):
    return img[:img.shape[0] - img.shape[0] % r, :img.shape[1] - img.shape[1] % r]


def reference_lr(img, r):
    """lr of one image in float64: the oracle's blur of the TRIMMED image, decimated at offset r // 2."""
    hr = trimmed(img, r) / 127.5 - 1.0
    return O.gaussian_blur(hr[None], 0.5 * (r - 1.0))[0][r // 2::r, r // 2::r]


def build(images, r, out=None):
    """The raw route (no DeviceEvalSet: it refuses images too small to score): trim, pack, records, check, one launch.
    Returns (arena, table, pairs)."""
    from ml_super_resolution_amd import image_arena, ops
    from ml_super_resolution_amd.espcn import dataset
    packed, records = dataset.eval_records([trimmed(im, r) for im in images], r)
    arena = image_arena.ImageArena(packed, torch.device('cuda')).arena
    table = ops.espcn_eval_table(records, r, arena)
    return arena, table, ops.espcn_eval_pairs(arena, table, out=out)


@pytest.fixture(scope='module')
def images():
    return make_images()


_cache = {}


def case(images, r):
    """The six images' device pairs for r: computed once, never modified."""
    if r not in _cache:
        _cache[r] = build(images, r)
    return _cache[r]


def test_the_sizes_reach_every_branch():
    """What the six sizes are for, at T = 16: an image smaller than the radius on both sides (9 x 9 at r = 4 trims to 8 x 8,
    radius 6); trimming in one axis, both and none; an lr side of exactly T and 2 T, and one past a tile edge; interior
    tiles whose halo is real image on all sides (a 3 x 3 grid of tiles)."""
    assert T == 16
    lr_sides = {r: [(h // r, w // r) for h, w in SHAPES] for r in FACTORS}
    assert (2, 2) in lr_sides[4] and 8 < 2 * 6 + 1                 # 8 x 8 pixels under a window of 13: it passes both edges
    assert any(h % r and w % r for r in FACTORS for h, w in SHAPES) and any(bool(h % r) != bool(w % r) for r in FACTORS for h, w in SHAPES)
    assert any(h % r == 0 and w % r == 0 for r in FACTORS for h, w in SHAPES)
    sides = {s for r in FACTORS for hw in lr_sides[r] for s in hw}
    assert T in sides and 2 * T in sides and {T + 1, 2 * T + 1, 4 * T + 1} & sides
    assert any(h > 2 * T and w > 2 * T for hw in lr_sides.values() for h, w in hw)


@gpu
@pytest.mark.parametrize('r', FACTORS)
def test_pairs_against_the_reference_arithmetic(images, r):
    from ml_super_resolution_amd.espcn import experiment_test
    _, table, pairs = case(images, r)
    assert pairs.lr.dtype == pairs.label.dtype == torch.float32 and pairs.lr.dim() == pairs.label.dim() == 1
    assert pairs.lr.numel() == sum(3 * (h // r) * (w // r) for h, w in SHAPES) and pairs.label.numel() == pairs.lr.numel() * r * r
    worst = (0.0, None)
    for k, img in enumerate(images):
        lr, label = pairs.views(k)
        hp, wp = img.shape[0] // r, img.shape[1] // r
        assert tuple(lr.shape) == (1, hp, wp, 3) and tuple(label.shape) == (1, hp, wp, 3 * r * r)
        assert lr.data_ptr() == pairs.lr.data_ptr() + 4 * int(table.records['lr_offset'][k])            # a view, no copy
        assert label.data_ptr() == pairs.label.data_ptr() + 4 * r * r * int(table.records['lr_offset'][k])
        host_lr, host_label = experiment_test.prepare_image_pair(img, r)
        assert host_label.dtype == np.float32
        np.testing.assert_array_equal(label[0].cpu().numpy(), host_label)
        err = np.abs(lr[0].cpu().numpy().astype(np.float64) - reference_lr(img, r))
        at = np.unravel_index(err.argmax(), err.shape)
        if err.max() > worst[0]:
            worst = (err.max(), (k,) + tuple(int(v) for v in at))
        assert err.max() <= TOL, (r, k, at, err.max())
        assert np.abs(lr[0].cpu().numpy() - host_lr).max() <= TOL          # scipy's float64 blur, rounded to float32
    print('r %d: worst |lr - oracle| %.3g at (image, i, j, c) = %s' % (r, worst[0], worst[1]))


@pytest.mark.parametrize('r', FACTORS)
def test_a_clamp_at_another_edge_would_fail(images, r):
    """The blur must see the TRIMMED edge.  Two other blurs, by the oracle alone: one clamped at the untrimmed image's edge
    (blur first, trim then) and one clamped at a tile's own edge (the first tile's T r x T r pixels blurred alone).  Both
    lie from the reference by far more than the bound, so the test above tells them apart."""
    img = images[5]                                        # 131 x 135: every r trims it in at least one axis
    assert img.shape[0] % r or img.shape[1] % r
    want = reference_lr(img, r)
    hp, wp = want.shape[:2]
    untrimmed = O.gaussian_blur((img / 127.5 - 1.0)[None], 0.5 * (r - 1.0))[0][r // 2::r, r // 2::r][:hp, :wp]
    tile = O.gaussian_blur((img[:T * r, :T * r] / 127.5 - 1.0)[None], 0.5 * (r - 1.0))[0][r // 2::r, r // 2::r]
    d_untrimmed, d_tile = np.abs(untrimmed - want).max(), np.abs(tile - want[:T, :T]).max()
    print('r %d: a clamp at the untrimmed edge lies %.3g from the reference, one at the tile edge %.3g (bound %g)' % (r, d_untrimmed, d_tile, TOL))
    assert d_untrimmed > 1e-2 and d_tile > 1e-2


@gpu
def test_patches_are_cut_from_the_image_bit_for_bit(images):
    """120 x 75 at r = 3: both sides are multiples of 3, so the trimmed and the untrimmed edges coincide, and every
    unflipped training patch of DevicePatchSet(..., 3, 5) is a window of the image's pair, bit for bit."""
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.espcn import dataset
    img, r, p = images[4], 3, 5
    _, _, pairs = build([img], r)
    lr_image, label_image = (v[0] for v in pairs.views(0))
    s = dataset.DevicePatchSet([img], r, p, torch.device('cuda'))
    lr, label = ops.espcn_patch_pairs(s.arena, s.table, 0, len(s))
    seen = 0
    for k, rec in enumerate(s.records):
        if rec['flip'] != 0:
            continue
        i, j = int(rec['y']) // r, int(rec['x']) // r
        assert torch.equal(lr[k], lr_image[i:i + p, j:j + p]), (k, rec)
        assert torch.equal(label[k], label_image[i:i + p, j:j + p]), (k, rec)
        seen += 1
    assert seen == 4 * 7                                       # len(range(0, 75 - 15, 15)) x len(range(0, 120 - 15, 15))


@gpu
@pytest.mark.parametrize('poison', (False, True), ids=('plain', 'poisoned_lds'))
@pytest.mark.parametrize('r', FACTORS)
def test_images_are_independent_and_deterministic(images, monkeypatch, r, poison):
    """An image gives the same bits on a second run, alone, and at another table position -- also when every CU's LDS is
    filled with NaNs before each call (what SRX_POISON_LDS=1 makes the wrappers do)."""
    from ml_super_resolution_amd import ops
    arena, table, pairs0 = case(images, r)
    assert not torch.isnan(pairs0.lr).any() and not torch.isnan(pairs0.label).any()
    monkeypatch.setattr(ops, '_POISON_LDS', poison)
    again = ops.espcn_eval_pairs(arena, table)
    assert torch.equal(again.lr, pairs0.lr) and torch.equal(again.label, pairs0.label)
    order = [3, 5, 0, 4, 2, 1]
    moved = build([images[k] for k in order], r)[2]
    for pos, k in enumerate(order):
        for got, want in zip(moved.views(pos), pairs0.views(k)):
            assert torch.equal(got, want), (pos, k)
    for k in (0, 5):
        for got, want in zip(build([images[k]], r)[2].views(0), pairs0.views(k)):
            assert torch.equal(got, want), k


@gpu
@pytest.mark.parametrize('r', FACTORS)
def test_nothing_outside_the_outputs_is_written(images, r):
    """The raw wrapper on outputs that sit inside larger sentinel-filled buffers: the guard bands keep the sentinel, and
    every float between them is written with the bits of the plain run."""
    pairs0 = case(images, r)[2]
    n, guard, sentinel = pairs0.lr.numel(), 4096, 7.0
    big_lr = torch.full((n + 2 * guard,), sentinel, device='cuda')
    big_label = torch.full((n * r * r + 2 * guard,), sentinel, device='cuda')
    build(images, r, out=(big_lr[guard:guard + n], big_label[guard:guard + n * r * r]))
    for big, want in ((big_lr, pairs0.lr), (big_label, pairs0.label)):
        assert (big[:guard] == sentinel).all() and (big[-guard:] == sentinel).all()
        assert torch.equal(big[guard:-guard], want)
    assert not (pairs0.lr == sentinel).any() and not (pairs0.label == sentinel).any()


@gpu
def test_wrapper_refusals(images):
    from ml_super_resolution_amd import _lib, ops
    arena, table, _ = case(images, 3)
    with pytest.raises(ValueError):
        ops.espcn_eval_pairs(arena.cpu(), table)
    with pytest.raises(ValueError, match='built for this arena'):
        ops.espcn_eval_pairs(arena[:-1], table)                            # not the arena the table was checked for
    with pytest.raises(ValueError, match='built for this arena'):
        ops.espcn_eval_pairs(arena, table.records)
    with pytest.raises(ValueError):
        ops.espcn_eval_pairs(arena, table, out=(torch.empty(3, device='cuda'), torch.empty(27, device='cuda')))
    bad = table.records.copy()
    bad['lr_offset'][2] += 1
    before = torch.cuda.memory_allocated()
    with pytest.raises(_lib.SrxError, match='entry 2: lr_offset'):
        ops.espcn_eval_table(bad, 3, arena)
    assert torch.cuda.memory_allocated() == before                         # refused before any upload


@gpu
def test_experiment_scores_with_device_pairs(tmp_path, capsys):
    """Two small PNGs, one whose sizes are no multiples of r: the printed line shapes are those of --pairs host --scores
    fused, and the returned scores are the bits of the composition written here.  The distance to the host route is
    printed, not asserted: the lr bound above is the assertion."""
    from PIL import Image
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.espcn import experiment_scores, experiment_test, model_espcn
    d = tmp_path / 'imgs'
    _pngs(d, ((45, 39), (40, 53)), 4)
    (d / 'notes.txt').write_text('not an image')
    path = str(tmp_path / 'model.ckpt.npz')
    model_espcn.EspcnModel(3, device='cuda', seed=7).save(path)
    argv = ['--ckpt_path', path, '--data_path', str(d)]
    host = experiment_scores.evaluate_images(argv + ['--scores', 'fused'])
    lines_host = capsys.readouterr().out.splitlines()
    dev = experiment_scores.main(argv + ['--pairs', 'device'])
    lines_dev = capsys.readouterr().out.splitlines()
    assert [l.split(':')[0] for l in lines_dev] == [l.split(':')[0] for l in lines_host] == ['name', 'name', 'data', 'psnr', 'ssim']
    assert [len(l) for l in lines_dev] == [len(l) for l in lines_host]
    assert dev['names'] == host['names'] == ['im0.png', 'im1.png']
    # the composition, spelled out
    m = experiment_test.build_model(experiment_scores.parse_flags(argv))['_model']
    imgs = [np.asarray(Image.open(str(d / n)).convert('RGB')) for n in dev['names']]
    _, _, pairs = build(imgs, 3)
    assert pairs.views(1)[0].data_ptr() % 16 != 0          # 3 x 15 x 13 floats in: the convolutions want 16-byte alignment
    for k in range(2):
        lr, label = pairs.views(k)
        got = ops.image_scores(label, [m.forward(lr if lr.data_ptr() % 16 == 0 else lr.clone())], 1.0, space='y', unit_clip=True)[0, 0].cpu()
        assert (float(got[0]), float(got[1])) == (dev['psnrs'][k], dev['ssims'][k]), k
    dp = np.abs(np.array(dev['psnrs']) - np.array(host['psnrs'])).max()
    ds = np.abs(np.array(dev['ssims']) - np.array(host['ssims'])).max()
    print('|device - host| of the end-to-end scores: psnr %.3g dB, ssim %.3g' % (dp, ds))
    assert np.isfinite(dev['psnrs']).all() and np.isfinite(dev['ssims']).all()


@gpu
def test_train_script_validates_without_changing_training(tmp_path, capsys):
    from ml_super_resolution_amd import summary
    from ml_super_resolution_amd.espcn import experiment_scores, experiment_train
    valid = tmp_path / 'valid'
    _pngs(valid, ((45, 39), (40, 53)), 5)
    logs = {}
    for name, extra in (('plain', []), ('valid', ['--valid_data_path', str(valid), '--valid_every', '2'])):
        log = []
        torch.manual_seed(5)
        experiment_train.main(['--ckpt_path', str(tmp_path / ('ckpt_' + name)), '--logs_path', str(tmp_path / ('logs_' + name)),
                               '--batch_size', '8', '--lr_patch_size', '5', '--initial_learning_rate', '1e-3',
                               '--stop_training_at_k_step', '4'] + extra, log=log.append)
        logs[name] = log
    plain, val = logs['plain'], logs['valid']
    assert [rec['step'] for rec in plain] == [rec['step'] for rec in val] == [1, 2, 3, 4]
    assert [rec['loss'] for rec in plain] == [rec['loss'] for rec in val]                  # bit-equal: validation changes nothing
    assert all('valid_psnr' not in rec and 'valid_ssim' not in rec for rec in plain)
    for rec in val:
        if rec['step'] % 2 == 0:
            assert np.isfinite(rec['valid_psnr']) and np.isfinite(rec['valid_ssim']) and rec['valid_ssim'] <= 1.0
        else:
            assert 'valid_psnr' not in rec and 'valid_ssim' not in rec
    # step 4's values are those of the saved checkpoint scored from the command line
    capsys.readouterr()
    got = experiment_scores.main(['--ckpt_path', str(tmp_path / 'ckpt_valid' / 'model.ckpt-4'), '--data_path', str(valid),
                                  '--pairs', 'device'])
    assert val[3]['valid_psnr'] == float(torch.tensor(got['psnrs'], dtype=torch.float32).mean())
    assert val[3]['valid_ssim'] == float(torch.tensor(got['ssims'], dtype=torch.float32).mean())
    # the event file carries both tags at steps 2 and 4, and the plain run's carries neither
    def scalars(logdir):
        found = {}
        for path in summary.event_files(logdir):
            for ev in summary.read_events(path):
                for v in ev.get('values', []):
                    if v['tag'].startswith('valid_'):
                        found[(v['tag'], ev['step'])] = v['simple_value']
        return found
    found = scalars(str(tmp_path / 'logs_valid'))
    assert sorted(found) == [('valid_psnr', 2), ('valid_psnr', 4), ('valid_ssim', 2), ('valid_ssim', 4)]
    assert found[('valid_psnr', 4)] == val[3]['valid_psnr'] and found[('valid_ssim', 2)] == val[1]['valid_ssim']
    assert scalars(str(tmp_path / 'logs_plain')) == {}
