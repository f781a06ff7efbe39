"""VDSR's evaluation pairs built on the device (srx_vdsr_eval_pairs, vdsr/dataset.py: DeviceEvalSet): seven small images at
five factors against the oracle's hd_to_sd of the WHOLE image, against the seven-launch route that existed, independence of
the records, the wrappers' refusals, experiment_evaluate / experiment_resolve --pairs device, experiment_train's validation
flags and the timing script.

Bounds: hd has none -- (float)u8 / 255 * 2 - 1, bit for bit.  sd: 2e-5 against the float64 oracle, the bound
tests/test_gpu_patch_pairs.py holds this arithmetic to at S = 128; every side here is <= 130 because the fp32 half-pixel
coordinate loses precision with the side (a no-fma fp32 emulation on a CPU gave 1.4e-5 on these images, 3.8e-5 at
300 x 420, s = 1.25).  4e-5 between the two device routes: each within 2e-5 of one oracle.  The tests print what they
measure (pytest -s); the figures of one MI355X are in DESIGN.md 3.22."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.eval_tables import _pngs

gpu = pytest.mark.gpu

TOL = 2e-5
T = 32                                     # SRX_VDSR_EVAL_TILE: at another T, add sides T, T + 1 and 2 T
SHAPES = ((5, 7), (11, 11), (23, 31), (33, 64), (50, 47), (97, 130), (128, 32))
FACTORS = (1.5, 2, 2.5, 3, 4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_images():
    """Half random, half hard-edged (every byte 0 or 255)."""
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) if k % 2 == 0
            else (rng.integers(0, 2, size=(h, w, 3), dtype=np.uint8) * np.uint8(255)) for k, (h, w) in enumerate(SHAPES)]


def pairs_of(images):
    """Every (image index, factor) with int(side / s) >= 1, factor-major."""
    return [(k, s) for s in FACTORS for k, im in enumerate(images) if int(im.shape[0] / s) >= 1 and int(im.shape[1] / s) >= 1]


def build(images, which, out=None):
    """The raw route (no DeviceEvalSet: it refuses images too small to score): pack `images` once, one record per
    (image index, factor) of `which`, check, one launch.  Returns (arena, table, pairs)."""
    from ml_super_resolution_amd import image_arena, ops
    packed = image_arena.pack(images)
    _, offsets, widths, heights = packed
    idx = np.array([k for k, _ in which])
    records = ops.vdsr_eval_records(heights[idx], widths[idx], offsets[idx], [s for _, s in which])
    arena = image_arena.ImageArena(packed, torch.device('cuda')).arena
    table = ops.vdsr_eval_table(records, arena)
    return arena, table, ops.vdsr_eval_pairs(arena, table, out=out)


@pytest.fixture(scope='module')
def images():
    return make_images()


_cache = {}


def case(images):
    """All records' device pairs: computed once, never modified."""
    if 'case' not in _cache:
        _cache['case'] = (pairs_of(images),) + build(images, pairs_of(images))
    return _cache['case']


def reference_sd(images, k, s):
    """sd of image k at s in float64, in [-1, 1]: the oracle on the whole image.  Computed once per (k, s)."""
    if (k, s) not in _cache:
        hd01 = images[k].astype(np.float32) / np.float32(255)
        _cache[(k, s)] = O.hd_to_sd(hd01[None], s)[0] * 2 - 1
    return _cache[(k, s)]


@gpu
def test_pairs_against_the_oracle(images):
    which, _, table, pairs = case(images)
    assert len(which) == len(SHAPES) * len(FACTORS)
    assert pairs.sd.dtype == pairs.hd.dtype == torch.float32 and pairs.sd.dim() == pairs.hd.dim() == 1
    assert pairs.sd.numel() == pairs.hd.numel() == table.out_floats
    assert pairs.sd.data_ptr() % 16 == 0 and pairs.hd.data_ptr() % 16 == 0
    worst = (0.0, None)
    for r, (k, s) in enumerate(which):
        sd, hd = pairs.views(r)
        h, w = SHAPES[k]
        at = int(table.records['out_offset'][r])
        assert tuple(sd.shape) == tuple(hd.shape) == (1, h, w, 3)
        assert sd.data_ptr() == pairs.sd.data_ptr() + 4 * at and hd.data_ptr() == pairs.hd.data_ptr() + 4 * at      # views, no copy
        assert sd.data_ptr() % 16 == 0 and hd.data_ptr() % 16 == 0
        np.testing.assert_array_equal(hd[0].cpu().numpy(), (images[k].astype(np.float32) / np.float32(255)) * np.float32(2) - np.float32(1))
        err = np.abs(sd[0].cpu().numpy().astype(np.float64) - reference_sd(images, k, s))
        pos = np.unravel_index(err.argmax(), err.shape)
        if err.max() > worst[0]:
            worst = (err.max(), (h, w, s) + tuple(int(v) for v in pos))
        assert err.max() <= TOL, (h, w, s, pos, err.max())
    print('worst |sd - oracle| %.3g at (H, W, s, i, j, c) = %s' % worst)
    assert any((int(a) + 3 * h * w) % 4 for a, (h, w) in zip(table.records['out_offset'], [SHAPES[k] for k, _ in which]))    # some gap exists


@pytest.mark.parametrize('s', FACTORS)
def test_a_clamp_at_another_edge_would_fail(images, s):
    """The blur and both resizes must see the IMAGE's edge.  Two other degradations, by the oracle alone: the first tile's
    T x T pixels degraded by themselves (borders at the tile's edge), and the image with its last row and column dropped
    (borders one pixel early).  Both lie from the reference by far more than the bound, so the test above tells them
    apart."""
    k = 5                                                   # 97 x 130, hard-edged
    want = reference_sd(images, k, s)
    hd01 = images[k].astype(np.float32) / np.float32(255)
    tile = O.hd_to_sd(hd01[None, :T, :T], s)[0] * 2 - 1
    dropped = O.hd_to_sd(hd01[None, :-1, :-1], s)[0] * 2 - 1
    d_tile, d_dropped = np.abs(tile - want[:T, :T]).max(), np.abs(dropped - want[:-1, :-1]).max()
    print('s %g: the tile degraded alone lies %.3g from the reference, the image less a row and a column %.3g (bound %g)' % (s, d_tile, d_dropped, TOL))
    assert d_tile > 1e-2 and d_dropped > 1e-2


@gpu
def test_against_the_existing_device_route(images):
    """sd within 4e-5 of affine(degrade_on_device(hd01, s), 2, -1), the seven-launch route on the same image; both within
    2e-5 of one oracle."""
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.vdsr import dataset
    which, _, _, pairs = case(images)
    worst = worst_old = 0.0
    for r, (k, s) in enumerate(which):
        hd01 = ops.u8_to_unit_float(torch.from_numpy(images[k][None]).cuda())
        old = ops.affine(dataset.degrade_on_device(hd01, s), 2.0, -1.0)
        sd, hd = pairs.views(r)
        assert torch.equal(hd, ops.affine(hd01, 2.0, -1.0))
        d = (sd - old).abs().max().item()
        d_old = np.abs(old[0].cpu().numpy().astype(np.float64) - reference_sd(images, k, s)).max()
        worst, worst_old = max(worst, d), max(worst_old, d_old)
        assert d <= 4e-5 and d_old <= TOL, (SHAPES[k], s, d, d_old)
    print('worst |sd - sd of the seven launches| %.3g; worst |seven launches - oracle| %.3g' % (worst, worst_old))


@gpu
@pytest.mark.parametrize('poison', (False, True), ids=('plain', 'poisoned_lds'))
def test_records_are_independent_and_deterministic(images, monkeypatch, poison):
    """A record gives the same bits on a second run, alone, at another table position, and beside the same image at another
    factor or in a table of its own -- also when every CU's LDS is filled with NaNs before each call (what SRX_POISON_LDS=1
    makes the wrappers do)."""
    from ml_super_resolution_amd import ops
    which, arena, table, pairs0 = case(images)
    for r in range(len(which)):
        for v in pairs0.views(r):
            assert not torch.isnan(v).any()
    monkeypatch.setattr(ops, '_POISON_LDS', poison)
    again = ops.vdsr_eval_pairs(arena, table)
    for r in range(len(which)):
        for got, want in zip(again.views(r), pairs0.views(r)):
            assert torch.equal(got, want), which[r]
    order = np.random.default_rng(5).permutation(len(which))
    moved = build(images, [which[r] for r in order])[2]
    for pos, r in enumerate(order):
        for got, want in zip(moved.views(pos), pairs0.views(int(r))):
            assert torch.equal(got, want), (pos, which[r])
    for r in (0, len(which) - 2):                                           # alone: its image the only one in the arena
        k, s = which[r]
        for got, want in zip(build([images[k]], [(0, s)])[2].views(0), pairs0.views(r)):
            assert torch.equal(got, want), which[r]
    both = build([images[5]], [(0, 2), (0, 4)])[2]                          # one image, two factors, one table
    for pos, s in enumerate((2, 4)):
        alone = build([images[5]], [(0, s)])[2]
        for got, want, ref in zip(both.views(pos), alone.views(0), pairs0.views(which.index((5, s)))):
            assert torch.equal(got, want) and torch.equal(got, ref), s


@gpu
def test_the_widest_staged_region(images):
    """s = 8, the largest factor: radius 14, so a tile stages 73 source pixels per axis, the most the layout sees (the rows
    the staging loop copies are at their longest).  97 x 130 pixels: two tiles and a ragged third on one axis, four and a
    ragged fifth on the other.  hd has the image's bits; sd lies within the file's bounds of the oracle and of the
    seven-launch route (each blur sums 29 taps of values in [0, 1]: below 2e-6 of rounding a pass, and the blurred image is
    smoother than at any smaller factor, so the fp32 coordinate costs less than there); and the record has the same bits
    alone as beside the same image at s = 2."""
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.vdsr import dataset
    k, s = 5, 8
    assert min(SHAPES[k]) >= 65
    alone = build([images[k]], [(0, s)])[2]
    sd, hd = alone.views(0)
    hd01 = ops.u8_to_unit_float(torch.from_numpy(images[k][None]).cuda())
    assert torch.equal(hd, ops.affine(hd01, 2.0, -1.0))
    old = ops.affine(dataset.degrade_on_device(hd01, s), 2.0, -1.0)
    d = (sd - old).abs().max().item()
    d_oracle = np.abs(sd[0].cpu().numpy().astype(np.float64) - reference_sd(images, k, s)).max()
    print('s 8: |sd - sd of the seven launches| %.3g, |sd - oracle| %.3g' % (d, d_oracle))
    assert d <= 4e-5 and d_oracle <= TOL, (d, d_oracle)
    both = build([images[k]], [(0, 2), (0, s)])[2]
    for got, want in zip(both.views(1), alone.views(0)):
        assert torch.equal(got, want)


@gpu
def test_nothing_outside_the_outputs_is_written(images):
    """The raw wrapper on outputs that sit inside larger sentinel-filled buffers: the guard bands and the padding gaps
    between the records keep the sentinel, and every other float has the bits of the plain run."""
    which, _, table, pairs0 = case(images)
    n, guard, sentinel = table.out_floats, 4096, 7.0
    big_sd = torch.full((n + 2 * guard,), sentinel, device='cuda')
    big_hd = torch.full((n + 2 * guard,), sentinel, device='cuda')
    got = build(images, which, out=(big_sd[guard:guard + n], big_hd[guard:guard + n]))[2]
    written = torch.zeros(n, dtype=torch.bool, device='cuda')
    for r, (k, _) in enumerate(which):
        at = int(table.records['out_offset'][r])
        written[at:at + 3 * SHAPES[k][0] * SHAPES[k][1]] = True
        for a, b in zip(got.views(r), pairs0.views(r)):
            assert torch.equal(a, b), which[r]
            assert not (b == sentinel).any()
    assert 0 < int((~written).sum()) < 4 * len(which)                       # the gaps: fewer than 4 floats per record
    for big in (big_sd, big_hd):
        assert (big[:guard] == sentinel).all() and (big[-guard:] == sentinel).all()
        assert (big[guard:-guard][~written] == sentinel).all()


@gpu
def test_wrapper_refusals(images):
    from ml_super_resolution_amd import _lib, ops
    _, arena, table, _ = case(images)
    with pytest.raises(ValueError):
        ops.vdsr_eval_pairs(arena.cpu(), table)
    with pytest.raises(ValueError, match='built for this arena'):
        ops.vdsr_eval_pairs(arena[:-1], table)                             # not the arena the table was checked for
    with pytest.raises(ValueError, match='built for this arena'):
        ops.vdsr_eval_pairs(arena, table.records)
    with pytest.raises(ValueError):
        ops.vdsr_eval_pairs(arena, table, out=(torch.empty(3, device='cuda'), torch.empty(3, device='cuda')))
    bad = table.records.copy()
    bad['out_offset'][2] += 4
    before = torch.cuda.memory_allocated()
    with pytest.raises(_lib.SrxError, match='entry 2: out_offset'):
        ops.vdsr_eval_table(bad, arena)
    assert torch.cuda.memory_allocated() == before                         # refused before any upload


def _checkpoint(path, num_layers, seed):
    from ml_super_resolution_amd.vdsr import model_vdsr
    torch.save(model_vdsr.VdsrModel(num_layers, device='cuda', seed=seed).stack.state_dict(), path)


@gpu
def test_experiment_evaluate_with_device_pairs(tmp_path, capsys):
    """Two small PNGs, one with odd sizes, and a stray .txt: the printed line shapes are those of --pairs host, and the
    returned scores are the bits of the composition written here.  The distance to the host route is printed, not asserted:
    the sd bound above is the assertion."""
    from PIL import Image
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.vdsr import dataset, experiment_evaluate, model_vdsr
    d = tmp_path / 'imgs'
    _pngs(d, ((45, 39), (40, 52)), 4)
    (d / 'notes.txt').write_text('not an image')
    ckpt = str(tmp_path / 'model.ckpt-0.pt')
    _checkpoint(ckpt, 4, 7)
    argv = ['--ckpt_path', ckpt, '--hd_image_dir_path', str(d), '--num_layers', '4', '--scaling_factor', '3']
    for scores in ('fused', 'separate'):
        capsys.readouterr()
        host = experiment_evaluate.main(argv + ['--scores', scores])
        lines_host = capsys.readouterr().out.splitlines()
        dev = experiment_evaluate.main(argv + ['--scores', scores, '--pairs', 'device'])
        lines_dev = capsys.readouterr().out.splitlines()
        assert [l.split(':')[0] for l in lines_dev] == [l.split(':')[0] for l in lines_host] == ['x3', 'time (s)     ', 'psnr (sd, sr)', 'ssim (sd, sr)']
        assert [len(l.split(',')) for l in lines_dev] == [len(l.split(',')) for l in lines_host]
        assert dev['names'] == host['names'] == ['im0.png', 'im1.png']
        # the composition, spelled out
        m = model_vdsr.VdsrModel(4, device='cuda')
        m.stack.load_checkpoint(ckpt)
        imgs = [np.asarray(Image.open(str(d / n)).convert('RGB')) for n in dev['names']]
        eval_set = dataset.DeviceEvalSet(imgs, [3], 'cuda', names=dev['names'])
        for k in range(2):
            sd, hd = eval_set.views[k]
            if scores == 'fused':
                got = ops.image_scores(hd, [sd, m.forward(sd)], 2.0).cpu().numpy().astype(np.float64)
                want = [[dev['sd_psnrs'][k], dev['sd_ssims'][k]], [dev['sr_psnrs'][k], dev['sr_ssims'][k]]]
                assert got[:, 0].tolist() == want, k
            else:
                sr = m.forward(sd)
                assert (ops.psnr(hd, sd, 2.0).item(), ops.psnr(hd, sr, 2.0).item()) == (dev['sd_psnrs'][k], dev['sr_psnrs'][k]), k
                assert (ops.ssim(hd, sd, 2.0).item(), ops.ssim(hd, sr, 2.0).item()) == (dev['sd_ssims'][k], dev['sr_ssims'][k]), k
        for key in ('sd_psnrs', 'sr_psnrs', 'sd_ssims', 'sr_ssims'):
            assert np.isfinite(dev[key]).all()
            with capsys.disabled():
                print('--scores %s: |device - host| of %s: %.3g' % (scores, key, np.abs(np.array(dev[key]) - np.array(host[key])).max()))


@gpu
def test_experiment_resolve_with_device_pairs(tmp_path, capsys):
    from PIL import Image
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.vdsr import dataset, experiment_resolve, model_vdsr
    d = tmp_path / 'imgs'
    _pngs(d, ((45, 39),), 6)
    ckpt = str(tmp_path / 'model.ckpt-0.pt')
    _checkpoint(ckpt, 4, 9)
    out = str(tmp_path / 'sr.png')
    experiment_resolve.main(['--ckpt_path', ckpt, '--hd_image_path', str(d / 'im0.png'), '--sr_image_path', out, '--num_layers', '4',
                             '--scaling_factor', '2.5', '--pairs', 'device'])
    line = capsys.readouterr().out.splitlines()[-1]
    assert line.startswith('psnr (sd, sr): ') and len(line.split(',')) == 3
    # the composition, spelled out
    m = model_vdsr.VdsrModel(4, device='cuda')
    m.stack.load_checkpoint(ckpt)
    img = np.asarray(Image.open(str(d / 'im0.png')).convert('RGB'))
    sd, hd = dataset.DeviceEvalSet([img], [2.5], 'cuda').views[0]
    want = tmp_path / 'want.png'
    Image.fromarray(ops.saturate_u8(m.forward(sd))[0].cpu().numpy()).save(str(want))
    assert open(out, 'rb').read() == want.read_bytes()
    host_out = str(tmp_path / 'sr_host.png')
    experiment_resolve.main(['--ckpt_path', ckpt, '--hd_image_path', str(d / 'im0.png'), '--sr_image_path', host_out, '--num_layers', '4',
                             '--scaling_factor', '2.5'])
    a, b = np.asarray(Image.open(out)).astype(int), np.asarray(Image.open(host_out)).astype(int)
    with capsys.disabled():
        print('--pairs device against host: %d of %d bytes differ, by at most %d' % ((a != b).sum(), a.size, np.abs(a - b).max()))


@gpu
def test_train_script_validates_without_changing_training(tmp_path, capsys):
    from ml_super_resolution_amd import summary
    from ml_super_resolution_amd.vdsr import experiment_evaluate, experiment_train
    valid = tmp_path / 'valid'
    _pngs(valid, ((45, 39), (40, 52)), 5)
    logs = {}
    for name, extra in (('plain', []), ('valid', ['--valid_data_path', str(valid), '--valid_every', '2', '--valid_scaling_factors', '2_3'])):
        log = []
        torch.manual_seed(5)
        experiment_train.main(['--ckpt_path', str(tmp_path / ('ckpt_' + name)), '--logs_path', str(tmp_path / ('logs_' + name)),
                               '--batch_size', '8', '--image_size', '11', '--num_layers', '4', '--stop_training_at_k_step', '4'] + extra,
                              log=log.append)
        logs[name] = log
    plain, val = logs['plain'], logs['valid']
    keys = ['valid_psnr', 'valid_ssim', 'valid_psnr_x2', 'valid_ssim_x2', 'valid_psnr_x3', 'valid_ssim_x3']
    assert [rec['step'] for rec in plain] == [rec['step'] for rec in val] == [1, 2, 3, 4]
    assert [rec['loss'] for rec in plain] == [rec['loss'] for rec in val]                  # bit-equal: validation changes nothing
    assert all(not any(k.startswith('valid_') for k in rec) for rec in plain)
    for rec in val:
        if rec['step'] % 2 == 0:
            assert sorted(k for k in rec if k.startswith('valid_')) == sorted(keys)
            assert all(np.isfinite(rec[k]) for k in keys) and all(rec[k] <= 1.0 for k in keys if 'ssim' in k)
        else:
            assert not any(k.startswith('valid_') for k in rec)
    # step 4's values are those of the saved checkpoint scored from the command line, factor by factor
    capsys.readouterr()
    scores = torch.empty((4, 2, 2), device='cuda')                          # the trainer's layout: [record, (sd, sr), (psnr, ssim)]
    for f, s in enumerate((2, 3)):
        got = experiment_evaluate.main(['--ckpt_path', str(tmp_path / 'ckpt_valid' / 'model.ckpt-4'), '--hd_image_dir_path', str(valid),
                                        '--num_layers', '4', '--scaling_factor', str(s), '--pairs', 'device', '--scores', 'fused'])
        for k in range(2):
            scores[2 * f + k, 1, 0], scores[2 * f + k, 1, 1] = got['sr_psnrs'][k], got['sr_ssims'][k]
    mean = scores[:, 1].mean(dim=0).cpu()
    assert (val[3]['valid_psnr'], val[3]['valid_ssim']) == (float(mean[0]), float(mean[1]))
    for f, s in enumerate((2, 3)):
        m = scores[2 * f:2 * f + 2, 1].mean(dim=0).cpu()
        assert (val[3]['valid_psnr_x%d' % s], val[3]['valid_ssim_x%d' % s]) == (float(m[0]), float(m[1])), s

    def scalars(logdir):
        found = {}
        for path in summary.event_files(logdir):
            for ev in summary.read_events(path):
                for v in ev.get('values', []):
                    if v['tag'].startswith('valid_'):
                        found[(v['tag'], ev['step'])] = v['simple_value']
        return found
    found = scalars(str(tmp_path / 'logs_valid'))
    assert sorted(found) == sorted((k, step) for k in keys for step in (2, 4))
    assert all(found[(k, step)] == val[step - 1][k] for k in keys for step in (2, 4))
    assert scalars(str(tmp_path / 'logs_plain')) == {}
    with pytest.raises(ValueError, match='--valid_data_path'):
        experiment_train.main(['--valid_every', '2', '--stop_training_at_k_step', '0'])


@gpu
def test_timing_script_runs_on_tiny_sizes():
    got = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'time_vdsr_eval.py'), '--sizes', '24x31,40x33', '--num_layers', '4',
                          '--windows', '2', '--repeats', '1'], capture_output=True, text=True, timeout=300)
    assert got.returncode == 0, got.stdout + got.stderr
    rec = json.loads(got.stdout.strip().splitlines()[-1])
    assert rec['records'] == 6 and rec['tiles'] == 3 * (1 + 4) and rec['pixels'] == 3 * (24 * 31 + 40 * 33)
    for key in ('pairs_host_us', 'pairs_launches_us', 'pairs_device_us', 'evaluate_host_us', 'evaluate_device_us',
                'resident_DeviceEvalSet.evaluate_us', 'pairs_device_GBps'):
        assert rec[key] > 0, key
    assert rec['sd_device_vs_launches'] <= 4e-5
