"""The TensorBoard summaries on the GPU: the panel encoder (srx_summary_panel_u8 / _range) byte for byte against the numpy
restatements of the reference's graphs (tests/summary_reference.py), and the four trainers with their logs flag -- tags,
steps, losses, the decoded panel against the restatement applied to that step's tensors, and parameters bit-identical
to the same run without the flag."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from ml_super_resolution_amd import ops, summary
from tests import summary_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _values(rng, shape):
    """[-1.6, 1.6] with exact -1 and 1, both infinities, and values whose x * 127.5 + 127.5 lies within one ulp of an
    integer (where a fused multiply-add, or a rounding instead of the truncation, shows)."""
    x = rng.uniform(-1.6, 1.6, shape).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    k = rng.integers(0, 256, n)
    near = ((k.astype(np.float64) - 127.5) / 127.5).astype(np.float32)
    side = rng.integers(0, 3, n)                                   # the float nearest k's preimage, its lower and its upper neighbour
    near = np.where(side == 0, near, np.nextafter(near, np.where(side == 1, np.float32(-4), np.float32(4))))
    pick = rng.random(n)
    flat[:] = np.where(pick < 0.3, near, flat)
    specials = np.array([-1.0, 1.0, np.inf, -np.inf, 0.0, -0.0], np.float32)
    where = rng.random(n) < 0.05
    flat[where] = specials[rng.integers(0, len(specials), int(where.sum()))]
    return x


# (source widths, N, H, r): smallest first -- all tail; source boundaries inside a dword; an odd row length over several
# workgroups with a ragged last one; EnhanceNet's rows; every r at p = 1 and 2; the reference's ESPCN patch
PANEL_CASES = [((1,), 1, 1, 1), ((1, 2, 3), 2, 3, 1), ((41, 41, 41), 3, 41, 1), ((128, 128, 128), 2, 128, 1),
               ((1, 1), 2, 1, 2), ((2, 2), 2, 2, 2), ((1, 1), 2, 1, 3), ((2, 2), 2, 2, 3), ((1, 1), 2, 1, 4), ((2, 2), 2, 2, 4),
               ((17, 17), 4, 17, 3)]


def _expected(sources, r):
    return R.saturate(R.plain_layout(sources) if r == 1 else R.label_layout(sources, r))


def test_label_layout_restatement_matches_the_index_formula():
    """The numpy restatement of ESPCN's concat / split / reshape graph puts channel (dy*r + dx)*3 + ch of source pixel
    (n, y, x) at row (n*H + y)*r + dy, column (W_before + x)*r + dx: the formula the kernel is written from."""
    rng = np.random.default_rng(0)
    for r in (2, 3, 4):
        n, p = 2, 3
        srcs = [rng.standard_normal((n, p, p, 3 * r * r)).astype(np.float32) for _ in range(2)]
        panel = R.label_layout(srcs, r)
        assert panel.shape == (n * p * r, 2 * p * r, 3)
        for s, src in enumerate(srcs):
            for (b, y, x, c), v in np.ndenumerate(src):
                dy, dx, ch = c // 3 // r, c // 3 % r, c % 3
                assert panel[(b * p + y) * r + dy, (s * p + x) * r + dx, ch] == v


@pytest.mark.parametrize('widths,N,H,r', PANEL_CASES)
def test_panel_matches_the_restatement_at_every_alignment(widths, N, H, r):
    rng = np.random.default_rng(sum(widths) * 131 + N * 17 + H + r)
    sources = [_values(rng, (N, H, w, 3 * r * r)) for w in widths]
    want = _expected(sources, r)
    assert want.shape == (N * H * r, sum(widths) * r, 3)
    dev = [torch.from_numpy(s).to(DEV) for s in sources]
    got = ops.summary_panel_u8(dev, r=r)
    assert got.shape == want.shape and got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    size = want.size
    for shift in (0, 1, 2, 3):
        buf = torch.full((size + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        view = buf[16 + shift:16 + shift + size]
        assert ops.summary_panel_u8(dev, r=r, out=view) is view
        host = buf.cpu().numpy()
        np.testing.assert_array_equal(host[16 + shift:16 + shift + size].reshape(want.shape), want)
        assert (host[:16 + shift] == 0xA5).all() and (host[16 + shift + size:] == 0xA5).all(), shift


def test_panel_reads_cropped_views_in_place():
    """A source may be a crop of a larger tensor (SRCNN's sd strip): row and image pitches, no copy."""
    rng = np.random.default_rng(5)
    full = torch.from_numpy(_values(rng, (3, 19, 23, 3))).to(DEV)
    a = torch.from_numpy(_values(rng, (3, 7, 9, 3))).to(DEV)
    crop = full[:, 6:13, 5:16]
    assert not crop.is_contiguous()
    got = ops.summary_panel_u8([a, crop, a])
    np.testing.assert_array_equal(got.cpu().numpy(), _expected([a.cpu().numpy(), crop.cpu().numpy(), a.cpu().numpy()], 1))
    rng_buf = ops.summary_panel_range([a, crop])
    got = ops.summary_panel_u8([a, crop], range=rng_buf)
    np.testing.assert_array_equal(got.cpu().numpy(), R.ranged(R.plain_layout([a.cpu().numpy(), crop.cpu().numpy()])))
    with pytest.raises(ValueError):
        ops.summary_panel_u8([full[:, :, ::2]])                   # rows not dense
    with pytest.raises(ValueError):
        ops.summary_panel_u8([a, full])                           # different H
    with pytest.raises(ValueError):
        ops.summary_panel_u8([a.cpu()])


def _ranged_cases():
    rng = np.random.default_rng(11)
    shape = (2, 5, 6, 3)
    pos = rng.uniform(0.0, 0.9, (3,) + shape).astype(np.float32)
    neg_big = rng.uniform(-1.0, 0.5, (3,) + shape).astype(np.float32)
    neg_big[0, 0, 0, 0, 0] = -1.25                                 # |min| > max
    pos_big = rng.uniform(-0.5, 1.0, (3,) + shape).astype(np.float32)
    pos_big[2, 1, 4, 5, 2] = 1.75                                  # max > |min|
    zero = np.zeros((3,) + shape, np.float32)
    bad = rng.uniform(-1.0, 1.0, (3,) + shape).astype(np.float32)
    bad[1, 1, 2, 3, 1] = np.inf                                    # one channel of one pixel: bad colour, outside the range
    bad[2, 0, 0, 0, 0] = -np.inf
    bad[0, 1, 4, 5, 2] = np.nan
    return {'positive': pos, 'negative_dominates': neg_big, 'positive_dominates': pos_big, 'zero': zero, 'non_finite': bad}


@pytest.mark.parametrize('name', ['positive', 'negative_dominates', 'positive_dominates', 'zero', 'non_finite'])
def test_ranged_encoding(name):
    hd, sd, sr = _ranged_cases()[name]
    want = R.srcnn_panel(hd, sd, sr)
    dev = [torch.from_numpy(t).to(DEV) for t in (hd, sd, sr)]
    rng_buf = ops.summary_panel_range(dev)
    got = ops.summary_panel_u8(dev, range=rng_buf).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    scale, offset = rng_buf[:2].cpu().numpy()
    finite = np.concatenate([t[np.isfinite(t)] for t in (hd, sd, sr)])
    if name == 'zero':
        assert scale == 0 and offset == 0 and (got == 0).all()
    elif finite.min() < 0:
        assert offset == 128 and scale == np.float32(127) / max(abs(finite.min()), abs(finite.max()))
    else:
        assert offset == 0 and scale == np.float32(255) / finite.max()
    if name == 'non_finite':
        assert (want.reshape(-1, 3) == (255, 0, 0)).all(axis=1).sum() >= 3


def test_panel_is_repeatable():
    rng = np.random.default_rng(2)
    dev = [torch.from_numpy(_values(rng, (3, 41, 41, 3))).to(DEV) for _ in range(3)]
    assert torch.equal(ops.summary_panel_u8(dev), ops.summary_panel_u8(dev))
    fin = [torch.nan_to_num(t, posinf=1.5, neginf=-1.5) for t in dev]
    a = ops.summary_panel_u8(fin, range=ops.summary_panel_range(fin))
    b = ops.summary_panel_u8(fin, range=ops.summary_panel_range(fin))
    assert torch.equal(a, b) and torch.equal(ops.summary_panel_range(fin)[:2], ops.summary_panel_range(fin)[:2])


def test_writer_takes_device_values_without_waiting(tmp_path):
    """Device scalars and a device panel: the value written is the one the tensor held when add_summary was called, even
    though the tensor is overwritten right after (the copy is ordered on the stream)."""
    loss = torch.zeros(1, device=DEV)
    panel = torch.zeros((4, 6, 3), dtype=torch.uint8, device=DEV)
    with summary.EventFileWriter(str(tmp_path)) as w:
        for k in range(20):
            loss.fill_(k + 0.5)
            panel.fill_(k)
            w.add_summary(k, [('loss', loss), ('p/image', panel)])
    got = R.decode_file(w.path)[1:]
    assert [e['values'][0]['simple_value'] for e in got] == [k + 0.5 for k in range(20)]
    for k, e in enumerate(got):
        assert (R.png_pixels(e['values'][1]['image']['encoded_image_string']) == k).all()


# ---- the trainers ----------------------------------------------------------------------------------------------------
def _events(logdir):
    (path,) = summary.event_files(str(logdir))
    events = list(summary.read_events(path))
    assert events == R.decode_file(path)
    assert events[0]['file_version'] == 'brain.Event:2'
    return events[1:]


def _f32_bits(v):
    return struct.pack('<f', v)


def _image(value):
    image = value['image']
    px = R.png_pixels(image['encoded_image_string'])
    assert (image['height'], image['width'], image['colorspace']) == (px.shape[0], px.shape[1], 3)
    return px


def test_vdsr_trainer_writes_the_reference_summaries(tmp_path):
    from ml_super_resolution_amd.vdsr import dataset, experiment_train
    common = ['--batch_size', '2', '--num_layers', '4', '--image_size', '13', '--initial_learning_rate', '1e-3',
              '--stop_training_at_k_step', '100', '--use_adam']
    logs = tmp_path / 'logs'
    log = []
    torch.manual_seed(5)
    m1 = experiment_train.main(common + ['--logs_path', str(logs)], log=log.append)
    torch.manual_seed(5)
    m0 = experiment_train.main(common)
    assert torch.equal(m1.stack.params, m0.stack.params) and torch.equal(m1.stack.opt_v, m0.stack.opt_v)
    events = _events(logs)
    assert [e['step'] for e in events] == list(range(1, 101))
    for e, rec in zip(events, log):
        tags = [v['tag'] for v in e['values']]
        assert tags == (['loss', 'sd_sr_hd/image/0', 'psnr'] if e['step'] == 100 else ['loss']), e['step']
        assert _f32_bits(e['values'][0]['simple_value']) == _f32_bits(rec['loss']) and rec['step'] == e['step']
    # the panel of step 100: that step's batch and the forward pass of that step (the run without the flag still holds it)
    batches = dataset.synthetic_batches(13, 2, torch.device(DEV), seed=104)
    for _ in range(100):
        sd, hd = next(batches)
    sr = m0.stack.acts[-1]
    np.testing.assert_array_equal(_image(events[-1]['values'][1]), R.vdsr_panel(sd.cpu().numpy(), sr.cpu().numpy(), hd.cpu().numpy()))
    assert _image(events[-1]['values'][1]).shape == (2 * 13, 3 * 13, 3)
    psnr = ops.psnr(sr, hd, 2.0).mean().item()
    assert _f32_bits(events[-1]['values'][2]['simple_value']) == _f32_bits(psnr)
    # train.jsonl is still written, with the same figures
    (line,) = open(str(logs / 'train.jsonl')).read().splitlines()
    rec = json.loads(line)
    assert rec['step'] == 100 and rec['psnr'] == psnr and rec['loss'] == log[-1]['loss']


def test_espcn_trainer_writes_the_reference_summaries(tmp_path):
    from ml_super_resolution_amd.espcn import experiment_train
    common = ['--batch_size', '4', '--scaling_factor', '3', '--lr_patch_size', '17', '--initial_learning_rate', '1e-3',
              '--stop_training_at_k_step', '3']
    logs = tmp_path / 'logs'
    log = []
    torch.manual_seed(77)
    m1 = experiment_train.main(common + ['--logs_path', str(logs)], log=log.append)
    torch.manual_seed(77)
    m0 = experiment_train.main(common)
    assert torch.equal(m1.stack.params, m0.stack.params) and torch.equal(m1.stack.opt_v, m0.stack.opt_v)
    events = _events(logs)
    assert events[0]['session_log'] == 1 and events[0]['step'] == 0
    assert [(e['step'], [v['tag'] for v in e['values']]) for e in events[1:]] == \
        [(1, ['loss']), (1, ['patches/image']), (2, ['loss']), (3, ['loss'])]
    for e, rec in zip([events[1]] + events[3:], log):
        assert _f32_bits(e['values'][0]['simple_value']) == _f32_bits(rec['loss'])
    # the panel of the first step: a one-step run from the same seed still holds that step's forward pass
    torch.manual_seed(77)
    one = experiment_train.main(common[:-1] + ['1'])
    lr_patch, hr_patch = next(experiment_train.synthetic_batches(4, 17, 3, torch.device(DEV)))
    target = ops.space_to_depth(hr_patch, 3)
    want = R.espcn_panel(one.stack.acts[-1].cpu().numpy(), target.cpu().numpy(), 3)
    assert want.shape == (4 * 17 * 3, 2 * 17 * 3, 3)
    np.testing.assert_array_equal(_image(events[2]['values'][0]), want)
    # the right half of the panel is the ground truth itself, pixel for pixel in image layout
    np.testing.assert_array_equal(want[:, 51:].reshape(4, 51, 51, 3), R.saturate(hr_patch.cpu().numpy()))


def test_srcnn_trainer_writes_the_reference_summaries(tmp_path):
    from PIL import Image
    from ml_super_resolution_amd.srcnn import srcnn
    rng = np.random.default_rng(1)
    img_dir = tmp_path / 'jpg'
    img_dir.mkdir()
    yy, xx = np.mgrid[0:70, 0:80]
    im = np.stack([127 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / 9.0) for c in range(3)], -1)
    Image.fromarray(np.clip(im + rng.normal(0, 5, im.shape), 0, 255).astype(np.uint8)).save(str(img_dir / '0.jpg'), quality=95)
    argv = ['--train', '--training-images-path', str(img_dir), '--ckpt-dir-path', str(tmp_path / 'ckpt'), '--batch-size', '2',
            '--crop-image-size', '57', '--logs-dir-path', str(tmp_path / 'logs')]
    flags = srcnn.sanity_check(srcnn._flags().parse_args(argv))
    log = []
    with summary.EventFileWriter(flags.logs_dir_path) as reporter:
        m1 = srcnn.train(flags, max_steps=2, seed=4, log=lambda s, l: log.append((s, l)), reporter=reporter)
    m0 = srcnn.train(flags, max_steps=2, seed=4)                     # no reporter: nothing is written
    assert torch.equal(m1.stack.params, m0.stack.params) and torch.equal(m1.stack.opt_v, m0.stack.opt_v)
    events = _events(tmp_path / 'logs')
    assert len(os.listdir(str(tmp_path / 'logs'))) == 1
    assert events[0]['session_log'] == 1 and events[0]['step'] == 0
    assert [(e['step'], [v['tag'] for v in e['values']]) for e in events[1:]] == [(1, ['loss', 'image/image/0']), (2, ['loss'])]
    for e, (step, loss) in zip(events[1:], log):
        assert e['step'] == step and _f32_bits(e['values'][0]['simple_value']) == _f32_bits(loss)
    # the panel of the first step from a one-step run's tensors
    one = srcnn.train(flags, max_steps=1, seed=4)
    hd_full = torch.from_numpy(next(srcnn.dataset_reader(flags, 4))).to(DEV)
    sd_full = one.degrade(hd_full)
    side = one.crop_side()
    crop = lambda t: t[:, side:t.shape[1] - side, side:t.shape[2] - side].cpu().numpy()
    want = R.srcnn_panel(crop(hd_full), crop(sd_full), one.stack.acts[-1].cpu().numpy())
    width = flags.crop_image_size - 2 * side
    assert want.shape == (2 * width, 3 * width, 3)
    np.testing.assert_array_equal(_image(events[1]['values'][1]), want)


def test_enet_trainer_writes_the_reference_summaries(tmp_path):
    from ml_super_resolution_amd.enet import experiment_train
    common = ['--model', 'pat', '--batch_size', '2', '--allow_random_vgg', 'true', '--stop_training_at_k_step']
    logs = tmp_path / 'logs'
    log = []
    torch.manual_seed(31)
    m1 = experiment_train.main(common + ['2', '--log_path', str(logs)], log=log.append)
    torch.manual_seed(31)
    m0 = experiment_train.main(common + ['2'])
    assert torch.equal(m1.generator.params, m0.generator.params)
    assert torch.equal(m1.discriminator.pool.params, m0.discriminator.pool.params)
    events = _events(logs)
    gen = ['generator_loss', 'perceptual_loss', 'texture_loss']
    assert [(e['step'], [v['tag'] for v in e['values']]) for e in events] == \
        [(0, ['discriminator_loss']), (0, gen), (0, ['bq_sr_hd/image/0']), (1, gen)]
    assert _f32_bits(events[0]['values'][0]['simple_value']) == _f32_bits(log[0]['a_loss'])
    for e, rec in ((events[1], log[1]), (events[3], log[2])):
        assert [_f32_bits(v['simple_value']) for v in e['values']] == [_f32_bits(rec[k]) for k in ('g_loss', 'p_loss', 't_loss')]
    # the panel of step 0 from a one-step run's tensors: the second batch (the first went to the discriminator)
    torch.manual_seed(31)
    one = experiment_train.main(common + ['1'])
    batches = experiment_train.synthetic_batches(2, torch.device(DEV), seed=0)
    next(batches)
    sd, bq, hd = next(batches)
    want = R.enet_panel(bq.cpu().numpy(), one.last_sr.cpu().numpy(), hd.cpu().numpy())
    assert want.shape == (2 * 128, 3 * 128, 3)
    np.testing.assert_array_equal(_image(events[2]['values'][0]), want)
