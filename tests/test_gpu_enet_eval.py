"""EnhanceNet's evaluation pairs built on the device (srx_enet_eval_pairs, enet/datasets.py: DeviceEvalSet): five trimmed
sizes in three kinds of content against the oracle's Pillow resample of the WHOLE image and against the per-image launches
that existed, independence of the records, what a launch leaves untouched, the wrappers' refusals, DeviceEvalSet.evaluate,
experiment_evaluate --pairs device, experiment_train's validation flags and the timing script.

Every comparison of pairs is exact: the degradation is integer arithmetic up to one table lookup, so there is no bound.
(12, 12): sd is 3 x 3 and every window is cut by an edge; 68 has a last tile of 4 pixels at either tile size; 132 has an
interior tile at either tile size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.eval_tables import _pngs
from tests.test_gpu_image_scores import PSNR_RTOL, SSIM_TOL

gpu = pytest.mark.gpu

SIZES = ((12, 12), (16, 68), (64, 64), (68, 132), (132, 76))           # trimmed (height, width)
KINDS = ('random', 'blocks', 'checker')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_image(kind, h, w, rng):
    if kind == 'random':
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[:h, :w]
    cell = (y // 8 + x // 8) if kind == 'blocks' else (y + x)          # 8 x 8 blocks of 0 and 255, or a one-pixel checkerboard
    return np.ascontiguousarray(np.repeat(((cell % 2) * 255).astype(np.uint8)[..., None], 3, axis=2))


def make_images():
    """Kind-major: image len(SIZES) * kind + size."""
    rng = np.random.default_rng(41)
    return [make_image(kind, h, w, rng) for kind in KINDS for h, w in SIZES]


def build(images, out=None):
    """The raw route: pack `images` once, one record each, check, one launch.  Returns (arena, table, pairs)."""
    from ml_super_resolution_amd import image_arena, ops
    from ml_super_resolution_amd.enet import datasets
    packed, records = datasets.eval_records(images)
    arena = image_arena.ImageArena(packed, torch.device('cuda')).arena
    table = ops.enet_eval_table(records, arena)
    return arena, table, ops.enet_eval_pairs(arena, table, out=out)


@pytest.fixture(scope='module')
def images():
    return make_images()


_cache = {}


def case(images):
    """All images' device pairs: computed once, never modified."""
    if 'case' not in _cache:
        _cache['case'] = build(images)
    return _cache['case']


def reference(images, k):
    """(sd, bq) bytes of image k by the oracle on the whole image.  Computed once per image."""
    if k not in _cache:
        h, w = images[k].shape[:2]
        sd = O.pil_resize_u8(images[k], h // 4, w // 4, 'bilinear')
        _cache[k] = (sd, O.pil_resize_u8(sd, h, w, 'bicubic'))
    return _cache[k]


def test_the_block_images_reach_both_sides_of_the_clip(images):
    """For the block images at (16, 68) and (64, 64) the oracle's bq holds both 0 and 255."""
    for size in (1, 2):
        bq = reference(images, len(SIZES) * KINDS.index('blocks') + size)[1]
        assert bq.min() == 0 and bq.max() == 255, SIZES[size]


@gpu
def test_pairs_equal_the_oracle(images):
    _, table, pairs = case(images)
    assert pairs.sd.numel() == table.sd_floats and pairs.bq.numel() == pairs.hd.numel() == table.out_floats
    for t in pairs:
        assert t.dtype == torch.float32 and t.dim() == 1 and t.data_ptr() % 16 == 0
    for k, im in enumerate(images):
        h, w = im.shape[:2]
        sd, bq, hd = pairs.views(k)
        assert tuple(sd.shape) == (1, h // 4, w // 4, 3) and tuple(bq.shape) == tuple(hd.shape) == (1, h, w, 3)
        assert sd.data_ptr() == pairs.sd.data_ptr() + 4 * int(table.records['sd_offset'][k])             # views, no copy
        assert hd.data_ptr() == pairs.hd.data_ptr() + 4 * int(table.records['out_offset'][k])
        assert bq.data_ptr() == pairs.bq.data_ptr() + 4 * int(table.records['out_offset'][k])
        assert sd.data_ptr() % 16 == 0 and bq.data_ptr() % 16 == 0 and hd.data_ptr() % 16 == 0
        want_sd, want_bq = reference(images, k)
        np.testing.assert_array_equal(hd[0].cpu().numpy(), O.u8_to_pm1(im), err_msg='hd of image %d' % k)
        np.testing.assert_array_equal(sd[0].cpu().numpy(), O.u8_to_pm1(want_sd), err_msg='sd of image %d' % k)
        np.testing.assert_array_equal(bq[0].cpu().numpy(), O.u8_to_pm1(want_bq), err_msg='bq of image %d' % k)
    assert any((3 * (h // 4) * (w // 4)) % 4 for h, w in SIZES)                                         # some gap exists in sd


@gpu
def test_pairs_equal_the_per_image_launches(images):
    from ml_super_resolution_amd.enet import datasets
    _, _, pairs = case(images)
    for k, im in enumerate(images):
        want = datasets.degrade_on_device(torch.from_numpy(im[None]).cuda())
        for name, got, ref in zip(('sd', 'bq', 'hd'), pairs.views(k), want):
            assert torch.equal(got, ref), (k, name)


@gpu
@pytest.mark.parametrize('poison', (False, True), ids=('plain', 'poisoned_lds'))
def test_records_are_independent_and_deterministic(images, monkeypatch, poison):
    """A record gives the same bits on a second run, alone, at another table position and twice in one table -- also when
    every CU's LDS is filled with NaNs before each call (what SRX_POISON_LDS=1 makes the wrappers do)."""
    from ml_super_resolution_amd import ops
    arena, table, pairs0 = case(images)
    for k in range(len(images)):
        for v in pairs0.views(k):
            assert not torch.isnan(v).any()
    monkeypatch.setattr(ops, '_POISON_LDS', poison)
    again = ops.enet_eval_pairs(arena, table)
    for k in range(len(images)):
        for got, want in zip(again.views(k), pairs0.views(k)):
            assert torch.equal(got, want), k
    order = np.random.default_rng(5).permutation(len(images))
    moved = build([images[k] for k in order])[2]
    for pos, k in enumerate(order):
        for got, want in zip(moved.views(pos), pairs0.views(int(k))):
            assert torch.equal(got, want), (pos, k)
    for k in (0, 3, len(images) - 1):                                       # alone: its image the only one in the arena
        for got, want in zip(build([images[k]])[2].views(0), pairs0.views(k)):
            assert torch.equal(got, want), k
    twice = build([images[8], images[1], images[8]])[2]                     # one image twice in a table
    for pos, k in enumerate((8, 1, 8)):
        for got, want in zip(twice.views(pos), pairs0.views(k)):
            assert torch.equal(got, want), (pos, k)


@gpu
def test_nothing_outside_the_outputs_is_written(images):
    """Outputs that sit inside larger buffers pre-filled with a NaN pattern: the guard bands past the totals and the padding
    floats between the records keep the pattern, and every other float has the bits of the plain run."""
    _, table, pairs0 = case(images)
    guard = 4096
    sizes = {'sd': table.sd_floats, 'bq': table.out_floats, 'hd': table.out_floats}
    # 0x7fc0dead: a quiet NaN with a payload, written as bits
    big = {name: torch.full((n + 2 * guard,), 0x7fc0dead, dtype=torch.int32, device='cuda').view(torch.float32) for name, n in sizes.items()}
    got = build(images, out=tuple(big[name][guard:guard + sizes[name]] for name in ('sd', 'bq', 'hd')))[2]
    written = {name: torch.zeros(n, dtype=torch.bool, device='cuda') for name, n in sizes.items()}
    for k, im in enumerate(images):
        h, w = im.shape[:2]
        at, sd_at = int(table.records['out_offset'][k]), int(table.records['sd_offset'][k])
        written['sd'][sd_at:sd_at + 3 * (h // 4) * (w // 4)] = True
        written['bq'][at:at + 3 * h * w] = True
        written['hd'][at:at + 3 * h * w] = True
        for a, b in zip(got.views(k), pairs0.views(k)):
            assert torch.equal(a, b), k
    assert 0 < int((~written['sd']).sum()) < 4 * len(images)                 # the gaps: fewer than 4 floats per record
    for name, buf in big.items():
        bits = buf.view(torch.int32)
        keep = torch.ones_like(bits, dtype=torch.bool)
        keep[guard:guard + sizes[name]] = ~written[name]
        assert (bits[keep] == 0x7fc0dead).all(), name
        assert not torch.isnan(buf[guard:guard + sizes[name]][written[name]]).any(), name


@gpu
def test_wrapper_refusals(images):
    from ml_super_resolution_amd import _lib, ops
    arena, table, _ = case(images)
    with pytest.raises(ValueError):
        ops.enet_eval_pairs(arena.cpu(), table)
    with pytest.raises(ValueError, match='built for this arena'):
        ops.enet_eval_pairs(arena[:-1], table)                             # not the arena the table was checked for
    with pytest.raises(ValueError, match='built for this arena'):
        ops.enet_eval_pairs(arena, table.records)
    with pytest.raises(ValueError):
        ops.enet_eval_pairs(arena, table, out=tuple(torch.empty(3, device='cuda') for _ in range(3)))
    for field, message in (('sd_offset', 'entry 2: sd_offset'), ('height_coeffs', 'entry 2: the height block')):
        bad = table.records.copy()
        bad[field][2] += 4
        before = torch.cuda.memory_allocated()
        with pytest.raises(_lib.SrxError, match=message):                  # one bad record: refused before any upload or launch
            ops.enet_eval_table(bad, arena)
        assert torch.cuda.memory_allocated() == before


def _generator(seed):
    from ml_super_resolution_amd.enet import model_enet
    return model_enet.EnetGenerator(device='cuda', seed=seed)


def _host_scores(generator, image):
    """What experiment_evaluate --pairs host does with one decoded image: [2 (bq, sr), 2 (psnr, ssim)] on the device."""
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.enet import datasets
    h, w = image.shape[0] - image.shape[0] % 4, image.shape[1] - image.shape[1] % 4
    sd, bq, hd = datasets.degrade_on_device(torch.from_numpy(np.ascontiguousarray(image[None, :h, :w])).cuda())
    return ops.image_scores(hd, [bq, generator.forward(sd, bq)], 1.0, space='rgb', unit_clip=True)[:, 0]


@gpu
def test_evaluate_equals_the_host_route_and_the_oracle(images):
    """Equal input bits give equal scores: evaluate == the scores of the per-image route, by torch.equal; and both lie
    within the bounds of tests/test_gpu_image_scores.py of oracle.psnr / oracle.ssim on the mapped, clipped images."""
    from ml_super_resolution_amd.enet import datasets
    chosen = [images[k] for k in (0, 1, 7, 13)]                            # (12, 12) and (16, 68) random, (64, 64) blocks, (68, 132) checker
    g = _generator(3)
    eval_set = datasets.DeviceEvalSet(chosen, 'cuda')
    got = eval_set.evaluate(g)
    assert tuple(got.shape) == (len(chosen), 2, 2) and got.is_cuda
    for k, im in enumerate(chosen):
        assert torch.equal(got[k], _host_scores(g, im)), k
    got = got.cpu().numpy().astype(np.float64)
    for k, im in enumerate(chosen):
        sd, bq, hd = eval_set.views[k]
        unit = [np.clip(t.cpu().numpy().astype(np.float64) / 2 + 0.5, 0, 1) for t in (hd, bq, g.forward(sd, bq))]
        for c in (0, 1):
            want_psnr, want_ssim = O.psnr(unit[0], unit[1 + c], 1.0)[0], O.ssim(unit[0], unit[1 + c], 1.0)[0]
            print('image %d cand %d: psnr %.6f (oracle %.6f), ssim %.6f (oracle %.6f)' % (k, c, got[k, c, 0], want_psnr, got[k, c, 1], want_ssim))
            assert abs(got[k, c, 0] - want_psnr) <= PSNR_RTOL * abs(want_psnr), (k, c)
            assert abs(got[k, c, 1] - want_ssim) <= SSIM_TOL, (k, c)


def _save_generator(prefix, seed):
    from ml_super_resolution_amd import tf_bundle
    g = _generator(seed)
    tf_bundle.save_checkpoint(prefix, {name: t.cpu().numpy() for name, t in g.variables().items()})


@gpu
def test_experiment_evaluate_device_equals_host(tmp_path, capsys):
    """Three small PNGs, two with sizes that need trimming, and a stray .txt: --pairs device returns the dict of --pairs host
    and writes the same PNG bytes."""
    from ml_super_resolution_amd.enet import experiment_evaluate
    d = tmp_path / 'imgs'
    _pngs(d, ((45, 39), (40, 52), (70, 131)), 4)
    (d / 'notes.txt').write_text('not an image')
    prefix = str(tmp_path / 'g' / 'model.ckpt')
    os.makedirs(os.path.dirname(prefix))
    _save_generator(prefix, 7)
    got = {}
    for pairs in ('host', 'device'):
        capsys.readouterr()
        got[pairs] = experiment_evaluate.main(['--source_ckpt_path', prefix, '--hd_dir_path', str(d), '--pairs', pairs,
                                               '--target_dir_path', str(tmp_path / pairs)])
        lines = capsys.readouterr().out.splitlines()
        assert [l.split(':')[0] for l in lines] == ['name'] * 3 + ['data', 'psnr (bq, sr)', 'ssim (bq, sr)']
    assert got['host'] == got['device']
    assert got['device']['names'] == ['im0.png', 'im1.png', 'im2.png']
    for key in ('bq_psnrs', 'bq_ssims', 'sr_psnrs', 'sr_ssims'):
        assert len(got['device'][key]) == 3 and np.isfinite(got['device'][key]).all()
    assert sorted(os.listdir(str(tmp_path / 'device'))) == sorted('im%d_%s.png' % (k, s) for k in range(3) for s in ('bq', 'sr'))
    for name in os.listdir(str(tmp_path / 'device')):
        assert (tmp_path / 'device' / name).read_bytes() == (tmp_path / 'host' / name).read_bytes(), name


@gpu
def test_train_script_validates_without_changing_training(tmp_path):
    from ml_super_resolution_amd import summary
    from ml_super_resolution_amd.enet import experiment_train
    valid = tmp_path / 'valid'
    _pngs(valid, ((45, 39), (40, 52)), 5)
    keys = ['valid_psnr', 'valid_ssim', 'valid_psnr_bq', 'valid_ssim_bq']
    logs = {}
    for name, extra in (('plain', []), ('valid', ['--valid_dir_path', str(valid), '--valid_every', '2'])):
        log = []
        torch.manual_seed(5)
        experiment_train.main(['--log_path', str(tmp_path / ('logs_' + name)), '--batch_size', '2', '--allow_random_vgg', 'true',
                               '--stop_training_at_k_step', '4'] + extra, log=log.append)
        logs[name] = log
    plain, val = logs['plain'], logs['valid']
    assert [(r['step'], r['trainer']) for r in plain] == [(r['step'], r['trainer']) for r in val]
    assert [r['step'] for r in val if r['trainer'] == 'g'] == [0, 1, 2, 3]
    for a, b in zip(plain, val):                                            # bit-equal: validation changes nothing
        assert {k: v for k, v in a.items() if not k.startswith('valid_')} == {k: v for k, v in b.items() if not k.startswith('valid_')}
    assert all(not any(k.startswith('valid_') for k in r) for r in plain)
    for r in val:
        if r['trainer'] == 'g' and r['step'] in (1, 3):
            assert sorted(k for k in r if k.startswith('valid_')) == sorted(keys)
            assert all(np.isfinite(r[k]) for k in keys) and all(r[k] <= 1.0 for k in keys if 'ssim' in k)
        else:
            assert not any(k.startswith('valid_') for k in r)

    def scalars(logdir):
        found = {}
        for path in summary.event_files(logdir):
            for ev in summary.read_events(path):
                for v in ev.get('values', []):
                    if v['tag'].startswith('valid_'):
                        found[(v['tag'], ev['step'])] = v['simple_value']
        return found
    found = scalars(str(tmp_path / 'logs_valid'))
    by_step = {r['step']: r for r in val if r['trainer'] == 'g'}
    assert sorted(found) == sorted((k, step) for k in keys for step in (1, 3))
    assert all(found[(k, step)] == by_step[step][k] for k in keys for step in (1, 3))
    assert scalars(str(tmp_path / 'logs_plain')) == {}
    with pytest.raises(ValueError, match='--valid_dir_path'):
        experiment_train.main(['--valid_every', '2', '--allow_random_vgg', 'true', '--stop_training_at_k_step', '0'])


@gpu
def test_timing_script_runs_on_tiny_sizes():
    got = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'time_enet_eval.py'), '--sizes', '24x32,40x36', '--windows', '2',
                          '--repeats', '1'], capture_output=True, text=True, timeout=300)
    assert got.returncode == 0, got.stdout + got.stderr
    from ml_super_resolution_amd import _lib
    rec = json.loads(got.stdout.strip().splitlines()[-1])
    T = _lib.ENET_EVAL_TILE
    assert rec['images'] == 2 and rec['tiles'] == sum(-(-h // T) * -(-w // T) for h, w in ((24, 32), (40, 36)))
    assert rec['pixels'] == 24 * 32 + 40 * 36
    for key in ('pairs_host_us', 'pairs_launches_us', 'pairs_device_us', 'pairs_device_GBps', 'evaluate_host_us', 'evaluate_device_us',
                'resident_DeviceEvalSet.evaluate_us'):
        assert rec[key] > 0, key
    assert rec['pairs_device_equal_launches'] is True
