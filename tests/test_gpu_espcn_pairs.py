"""ESPCN training pairs sampled on the device (srx_espcn_patch_pairs, espcn/dataset.py: device_patch_batches): every patch of
six small images against a float64 restatement of the reference (espcn/espcn/dataset.py:94-156: whole-image blur by the
oracle, decimation, flips, label layout), against the existing route (ops.gaussian_blur + slicing), independence of the
entries, the wrappers' refusals, the two batch sources against each other and the training script's --patch_source.

Bounds: the label has none -- (float)(u8 / 127.5 - 1.0) from float64, bit for bit.  lr: 2e-5, twice the 1e-5
tests/test_gpu_ops.py allows srx_gaussian_blur on [0, 1] data against the same oracle, the range here being twice as wide."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

TOL = 2e-5
SHAPES = ((9, 9), (23, 31), (40, 37), (64, 52), (120, 75), (131, 135))
CASES = [(r, p) for r in (2, 3, 4) for p in (1, 2, 5, 17)] + [(4, 32)]


def make_images():
    """Half random, half hard-edged (every byte 0 or 255)."""
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) if k % 2 == 0
            else (rng.integers(0, 2, size=(h, w, 3), dtype=np.uint8) * np.uint8(255)) for k, (h, w) in enumerate(SHAPES)]


def reference_pairs(img, r, p):
    """All pairs of one image in float64, in the reference's order: x outermost, then y, the row flip (-1 first), the
    column flip (-1 first).  Returns (lr [n,p,p,3], label [n,p,p,3 r^2])."""
    P, off = r * p, r // 2
    h, w, _ = img.shape
    nx, ny = len(range(0, w - P, P)), len(range(0, h - P, P))
    hr = img / 127.5 - 1.0
    bl = O.gaussian_blur(hr[None], 0.5 * (r - 1.0))[0]
    dec = bl[off::r, off::r]                               # bl[y + off + r i, x + off + r j] = dec[y / r + i, x / r + j]

    def tiles(a, s):                                       # [ny s, nx s, 3] -> [nx, ny, 4 flips, s, s, 3]
        t = a[:ny * s, :nx * s].reshape(ny, s, nx, s, 3).transpose(2, 0, 1, 3, 4)
        return np.stack([t[:, :, ::u, ::v] for u in (-1, 1) for v in (-1, 1)], axis=2)

    lr = tiles(dec, p).reshape(-1, p, p, 3)
    hrp = tiles(hr, P).reshape(-1, P, P, 3)
    label = hrp.reshape(-1, p, r, p, r, 3).transpose(0, 1, 3, 2, 4, 5).reshape(-1, p, p, 3 * r * r)
    if len(hrp):                                           # the label layout is the oracle's spelling of the reference's
        for k in (0, len(hrp) - 1):
            assert np.array_equal(label[k], O.s2d_ref_spelling_dataset(hrp[k], p))
    return lr, label


@pytest.fixture(scope='module')
def images():
    return make_images()


_cache = {}


def case(images, r, p):
    """The set, its device result on all patches and its float64 reference for (r, p): computed once, never modified."""
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.espcn import dataset
    if (r, p) not in _cache:
        s = dataset.DevicePatchSet(images, r, p, torch.device('cuda'))
        lr, label = ops.espcn_patch_pairs(s.arena, s.table, 0, len(s))
        refs = [reference_pairs(im, r, p) for im in images]
        _cache[(r, p)] = (s, lr, label, np.concatenate([a for a, _ in refs]), np.concatenate([b for _, b in refs]))
    return _cache[(r, p)]


@pytest.mark.parametrize('r,p', CASES)
def test_pairs_against_the_oracle(images, r, p):
    """All patches of all images, all four flips.  p = 1; a radius above the image's margin on both sides at once (9 x 9 at
    r = 4); interior patches whose halo is real image (120 x 75 at p = 5); LDS above 64 KiB ((4, 32): 109.9 KiB)."""
    s, lr, label, ref_lr, ref_label = case(images, r, p)
    n = len(ref_lr)
    assert n == len(s) > 0 and n % 4 == 0
    assert tuple(lr.shape) == (n, p, p, 3) and tuple(label.shape) == (n, p, p, 3 * r * r)
    assert lr.dtype == label.dtype == torch.float32
    np.testing.assert_array_equal(label.cpu().numpy(), ref_label.astype(np.float32))
    err = np.abs(lr.cpu().numpy().astype(np.float64) - ref_lr).reshape(n, -1).max(axis=1)
    print('r %d p %d: %d patches, worst |lr - oracle| %.3g (patch %d)' % (r, p, n, err.max(), err.argmax()))
    assert err.max() <= TOL, (r, p, s.records[err.argmax()], err.max())


def test_a_patch_local_clamp_would_fail(images):
    """What separates this from blurring the crop alone: at an interior patch of the 120 x 75 image the whole-image blur and
    the patch-local blur differ by far more than the bound, so the oracle test above tells them apart."""
    hr = images[4] / 127.5 - 1.0
    whole = O.gaussian_blur(hr[None], 1.0)[0][15 + 1:30:3, 15 + 1:30:3]
    local = O.gaussian_blur(hr[None, 15:30, 15:30], 1.0)[0][1::3, 1::3]
    assert np.abs(whole - local).max() > 1e-2


def test_pairs_against_the_existing_route(images):
    """One whole image (120 x 75, r = 3, p = 5): ops.gaussian_blur of the [-1, 1] image, then slicing.  Each route is within
    2e-5 of the same oracle, so they are within 4e-5 of each other; the largest difference is printed."""
    from ml_super_resolution_amd import ops
    r, p, P = 3, 5, 15
    s, lr, _, ref_lr, _ = case(images, r, p)
    k = 4
    img = images[k]
    first = sum(len(reference_pairs(im, r, p)[0]) for im in images[:k])
    hr = torch.from_numpy((img / 127.5 - 1.0).astype(np.float32)[None]).cuda()
    bl = ops.gaussian_blur(hr, 0.5 * (r - 1.0))[0].cpu().numpy()
    dec = bl[1::r, 1::r]
    worst, n = 0.0, 0
    for x in range(0, 75 - P, P):
        for y in range(0, 120 - P, P):
            t = dec[y // r:y // r + p, x // r:x // r + p]
            for u in (-1, 1):
                for v in (-1, 1):
                    worst = max(worst, np.abs(lr[first + n].cpu().numpy() - t[::u, ::v]).max())
                    n += 1
    assert n == 4 * 4 * 7
    print('|new - existing route| on 120 x 75 at r 3 p 5: %.3g' % worst)
    assert worst <= 2 * TOL


@pytest.mark.parametrize('poison', (False, True), ids=('plain', 'poisoned_lds'))
@pytest.mark.parametrize('r,p', ((3, 17), (4, 32)))
def test_entries_are_independent_and_deterministic(images, monkeypatch, r, p, poison):
    """An entry gives the same bits alone, permuted, repeated and on a second run -- also when every CU's LDS is filled
    with NaNs before each call (what SRX_POISON_LDS=1 makes the wrappers do)."""
    from ml_super_resolution_amd import ops
    s, lr0, label0 = case(images, r, p)[:3]
    assert not torch.isnan(lr0).any() and not torch.isnan(label0).any()
    monkeypatch.setattr(ops, '_POISON_LDS', poison)
    n = len(s)
    for _ in range(2):
        lr, label = ops.espcn_patch_pairs(s.arena, s.table, 0, n)
        assert torch.equal(lr, lr0) and torch.equal(label, label0)
    idx = np.concatenate([np.random.default_rng(1).permutation(n), [0, 0, n - 1, 0]])          # permuted, then repeated
    tab = s.table.permuted(torch.from_numpy(idx).cuda())
    lr, label = ops.espcn_patch_pairs(s.arena, tab, 0, len(idx))
    assert torch.equal(lr, lr0[idx]) and torch.equal(label, label0[idx])
    for k in range(0, n, 3):
        lr, label = ops.espcn_patch_pairs(s.arena, s.table, k, 1)
        assert torch.equal(lr[0], lr0[k]) and torch.equal(label[0], label0[k]), k


def test_wrapper_refusals(images):
    from ml_super_resolution_amd import _lib, ops
    s = case(images, 3, 17)[0]
    n = len(s)
    for start, B in ((0, n + 1), (n, 1), (-1, 2), (3, 0), (n - 1, 2)):
        with pytest.raises(ValueError, match='outside the table'):
            ops.espcn_patch_pairs(s.arena, s.table, start, B)
    with pytest.raises(ValueError):
        ops.espcn_patch_pairs(s.arena.cpu(), s.table, 0, 1)
    with pytest.raises(ValueError):
        ops.espcn_patch_pairs(s.arena[:-1], s.table, 0, 1)                 # not the arena the table was checked for
    bad = s.records.copy()
    bad['x'][2] += 200
    before = torch.cuda.memory_allocated()
    with pytest.raises(_lib.SrxError, match='entry 2: patch of 51'):
        ops.espcn_patch_table(bad, 3, 17, s.arena)
    assert torch.cuda.memory_allocated() == before                         # refused before any upload


def test_sources_agree_across_an_epoch_boundary(images):
    """One seed: the device source and the host source yield the same patches in the same order -- labels equal, lr within
    the bound (the host's is float64 scipy) -- with the epoch boundary inside a batch (28 patches, batches of 8)."""
    from ml_super_resolution_amd.espcn import dataset
    dev = torch.device('cuda')
    s = case(images, 3, 17)[0]
    assert len(s) == 28
    a = dataset.device_patch_batches(s, 3, 17, 8, dev, seed=6)
    b = dataset.host_patch_batches(images, 3, 17, 8, dev, seed=6)
    seen = []
    for _ in range(8):                                                     # 64 draws: two epochs and the start of a third
        lr_a, lab_a = next(a)
        lr_b, lab_b = next(b)
        seen.append(a.last_indices)
        assert tuple(lr_a.shape) == (8, 17, 17, 3) and tuple(lab_a.shape) == (8, 17, 17, 27) and lr_a.is_cuda
        assert torch.equal(lab_a, lab_b)
        assert (lr_a - lr_b).abs().max().item() <= TOL
    seen = np.concatenate(seen)
    assert sorted(seen[:28]) == sorted(seen[28:56]) == list(range(28)) and not np.array_equal(seen[:28], seen[28:56])


def test_train_script_with_patch_sources(tmp_path):
    from PIL import Image
    from ml_super_resolution_amd.espcn import experiment_train
    rng = np.random.default_rng(8)
    data = tmp_path / 'images'
    data.mkdir()
    for i, (h, w) in enumerate(((40, 37), (15, 60), (33, 16), (50, 31))):              # 15 x 60 holds no 15 x 15 patch
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(str(data / ('im%d.png' % i)))
    first = {}
    for source in ('device', 'host'):
        ckpt = str(tmp_path / ('ckpt_' + source))
        log = []
        torch.manual_seed(5)
        experiment_train.main(['--data_path', str(data), '--ckpt_path', ckpt, '--batch_size', '8', '--lr_patch_size', '5',
                               '--initial_learning_rate', '1e-3', '--stop_training_at_k_step', '3', '--patch_source', source],
                              log=log.append)
        assert [rec['step'] for rec in log] == [1, 2, 3]
        assert all(np.isfinite(rec['loss']) for rec in log)
        assert 'model.ckpt-3.index' in os.listdir(ckpt)
        first[source] = log[0]['loss']
    print('first-step loss: device %.8g, host %.8g' % (first['device'], first['host']))
    assert abs(first['device'] - first['host']) <= 1e-5 * abs(first['host'])
