"""VDSR training pairs sampled on the device (srx_vdsr_patch_pairs, vdsr/dataset.py: device_image_batches): against the
float64 oracle of the reference's degradation (oracle.hd_to_sd), against the existing per-factor route
(degrade_on_device), independence of the entries, the generator and the training script's --patch_source device.

Tolerance: tests/test_gpu_ops.py allows 1e-5 on [0,1] for blur + resize + resize against the same oracle; the map
x * 2 - 1 doubles it: 2e-5.  hd has no tolerance: (u8 / 255) * 2 - 1 in fp32 is one division and exact doubling."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.patch_tables import entry_for, offsets_of, table_of

pytestmark = pytest.mark.gpu

SHAPES = ((23, 31), (50, 47), (128, 130))        # (height, width) of the arena's images
entry = entry_for(SHAPES, 2.0)
FACTORS = (1.5, 2.0, 2.5, 3.0, 4.0)
TOL = 2e-5


def make_images():
    rng = np.random.default_rng(20)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in SHAPES]


def oracle_table(S):
    """Both corners of every image that fits, both flips, every factor with int(S / s) >= 1."""
    entries = []
    for k, (h, w) in enumerate(SHAPES):
        if h < S or w < S:
            continue
        for x, y in ((0, 0), (w - S, h - S)):
            for flip in (0, 1):
                entries += [entry(k, x, y, flip, s) for s in FACTORS if int(S / s) >= 1]
    return table_of(entries)


def table_128():
    """B = 3 on the third image (128 x 130): factors 2, 3, 4, a flipped entry, the far corner (x = 2)."""
    return table_of([entry(2, 0, 0, 0, 2.0), entry(2, 2, 0, 1, 3.0), entry(2, 1, 0, 0, 4.0)])


def crops_of(images, table, S):
    """The uint8 crops a table describes, flipped where it says so: [B,S,S,3]."""
    offs, _ = offsets_of([im.shape[:2] for im in images])
    out = []
    for t in table:
        im = images[offs.index(int(t['offset']))]
        assert im.shape[:2] == (t['height'], t['width'])
        c = im[t['y']:t['y'] + S, t['x']:t['x'] + S]
        out.append(c[:, ::-1] if t['flip'] else c)
    return np.stack(out)


def expected(crops, factors):
    """(sd, hd) as the reference computes them: hd in fp32 exactly, sd from the float64 oracle per factor."""
    hd01 = crops.astype(np.float32) / np.float32(255)
    hd = hd01 * np.float32(2) - np.float32(1)
    sd = np.empty(hd01.shape, np.float64)
    for s in sorted(set(factors.tolist())):
        m = factors == s
        sd[m] = O.hd_to_sd(hd01[m], float(s)) * 2.0 - 1.0
    return sd, hd


@pytest.fixture(scope='module')
def arena():
    images = make_images()
    flat = np.concatenate([im.reshape(-1) for im in images])
    return images, torch.from_numpy(flat).cuda()


@pytest.fixture(scope='module')
def case41(arena):
    """One table at S = 41, its device result and its oracle: shared by the tests below, never modified."""
    from ml_super_resolution_amd import ops
    images, dev = arena
    table = oracle_table(41)
    sd, hd = ops.vdsr_patch_pairs(dev, table, 41)
    ref_sd, ref_hd = expected(crops_of(images, table, 41), table['scaling_factor'])
    return table, sd, hd, ref_sd, ref_hd


def _check(images, dev, table, S):
    from ml_super_resolution_amd import ops
    sd, hd = ops.vdsr_patch_pairs(dev, table, S)
    assert sd.shape == hd.shape == (len(table), S, S, 3) and sd.dtype == hd.dtype == torch.float32
    ref_sd, ref_hd = expected(crops_of(images, table, S), table['scaling_factor'])
    np.testing.assert_array_equal(hd.cpu().numpy(), ref_hd)
    err = np.abs(sd.cpu().numpy().astype(np.float64) - ref_sd).reshape(len(table), -1).max(axis=1)
    print('S %d: B %d, worst |sd - oracle| %.3g (entry %d)' % (S, len(table), err.max(), err.argmax()))
    assert err.max() <= TOL, (S, table[err.argmax()], err.max())


@pytest.mark.parametrize('S', (5, 17))
def test_pairs_against_the_oracle(arena, S):
    """S = 5: the blur radius of 6 (factor 4) exceeds the patch and the low-resolution image is 1 x 1."""
    images, dev = arena
    table = oracle_table(S)
    assert len(table) == {5: 60, 17: 60}[S]
    _check(images, dev, table, S)


def test_pairs_against_the_oracle_41(case41):
    table, sd, hd, ref_sd, ref_hd = case41
    assert len(table) == 40
    np.testing.assert_array_equal(hd.cpu().numpy(), ref_hd)
    err = np.abs(sd.cpu().numpy().astype(np.float64) - ref_sd).reshape(len(table), -1).max(axis=1)
    print('S 41: worst |sd - oracle| %.3g (entry %d)' % (err.max(), err.argmax()))
    assert err.max() <= TOL, (table[err.argmax()], err.max())


def test_pairs_against_the_oracle_128(arena):
    """The large-LDS route: 128.25 KiB per workgroup."""
    images, dev = arena
    _check(images, dev, table_128(), 128)


def test_pairs_against_the_existing_route(arena, case41):
    """sd within 4e-5 of affine(degrade_on_device(hd01, s), 2, -1): each is within 2e-5 of the same oracle (the existing
    route: tests/test_gpu_ops.py, and below).  No bit equality is asked: fma contraction may differ between kernels."""
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.vdsr import dataset
    images, _ = arena
    table, sd, hd, ref_sd, _ = case41
    crops = torch.from_numpy(np.ascontiguousarray(crops_of(images, table, 41))).cuda()
    hd01 = ops.u8_to_unit_float(crops)
    assert torch.equal(ops.affine(hd01, 2.0, -1.0), hd)
    for s in FACTORS:
        m = np.flatnonzero(table['scaling_factor'] == np.float32(s))
        old = ops.affine(dataset.degrade_on_device(hd01[m].contiguous(), s), 2.0, -1.0)
        d_new = (old - sd[m]).abs().max().item()
        d_old = np.abs(old.cpu().numpy().astype(np.float64) - ref_sd[m]).max()
        print('factor %g: |new - existing| %.3g, |existing - oracle| %.3g' % (s, d_new, d_old))
        assert d_old <= TOL and d_new <= 2 * TOL, (s, d_new, d_old)


@pytest.mark.parametrize('poison', (False, True), ids=('plain', 'poisoned_lds'))
@pytest.mark.parametrize('S', (41, 128))
def test_entries_are_independent_and_deterministic(arena, case41, monkeypatch, S, poison):
    """An entry gives the same bits alone, at any position of a permuted table and on a second run -- also when every
    CU's LDS is filled with NaNs before each call (what SRX_POISON_LDS=1 makes the wrappers do)."""
    from ml_super_resolution_amd import ops
    images, dev = arena
    if S == 41:
        table, sd0, hd0 = case41[0][::3], case41[1][::3], case41[2][::3]       # 14 entries, every factor and flip
    else:
        table = table_128()
        sd0, hd0 = ops.vdsr_patch_pairs(dev, table, S)
    assert not torch.isnan(sd0).any()
    monkeypatch.setattr(ops, '_POISON_LDS', poison)
    for _ in range(2):
        sd, hd = ops.vdsr_patch_pairs(dev, table, S)
        assert torch.equal(sd, sd0) and torch.equal(hd, hd0)
    perm = np.random.default_rng(1).permutation(len(table))
    sd, hd = ops.vdsr_patch_pairs(dev, table[perm], S)
    assert torch.equal(sd, sd0[perm]) and torch.equal(hd, hd0[perm])
    for k in range(0, len(table), 3 if S == 41 else 1):
        sd, hd = ops.vdsr_patch_pairs(dev, table[k:k + 1], S)
        assert torch.equal(sd[0], sd0[k]) and torch.equal(hd[0], hd0[k]), k


def test_wrapper_checks_before_it_launches(arena):
    from ml_super_resolution_amd import _lib, ops
    _, dev = arena
    with pytest.raises(_lib.SrxError, match='entry 1: crop of 17'):
        ops.vdsr_patch_pairs(dev, table_of([entry(0, 0, 0), entry(0, 15, 0)]), 17)          # 15 + 17 > 31
    with pytest.raises(_lib.SrxError, match='leaves the arena'):
        ops.vdsr_patch_pairs(dev[:-1], table_of([entry(2, 0, 0)]), 17)
    with pytest.raises(ValueError):
        ops.vdsr_patch_pairs(dev.cpu(), table_of([entry(0, 0, 0)]), 17)
    words = ops.patch_table_words(table_of([entry(1, 3, 2, 1, 3.0)]))                        # the int32 view is a table too
    a, b = ops.vdsr_patch_pairs(dev, words, 17), ops.vdsr_patch_pairs(dev, table_of([entry(1, 3, 2, 1, 3.0)]), 17)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_device_image_batches():
    from ml_super_resolution_amd.vdsr import dataset
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, size=(60 + 7 * i, 80 + 5 * i, 3), dtype=np.uint8) for i in range(5)]
    images.insert(2, rng.integers(0, 256, size=(20, 20, 3), dtype=np.uint8))           # too small: dropped
    gen = dataset.device_image_batches(images, [2.0, 3.0, 4.0], 41, 16, torch.device('cuda'), seed=1)
    kept = [im for im in images if im.shape[0] >= 41]
    for _ in range(2):
        sd, hd = next(gen)
        table = gen.last_table
        assert sd.shape == hd.shape == (16, 41, 41, 3) and sd.is_cuda and hd.is_cuda and sd.dtype == torch.float32
        assert hd.min() >= -1 and hd.max() <= 1 and sd.min() >= -1.0001 and sd.max() <= 1.0001
        assert len(table) == 16 and set(table['scaling_factor']) <= {2.0, 3.0, 4.0}
        ref_sd, ref_hd = expected(crops_of(kept, table, 41), table['scaling_factor'])
        np.testing.assert_array_equal(hd.cpu().numpy(), ref_hd)
        assert np.abs(sd.cpu().numpy().astype(np.float64) - ref_sd).max() <= TOL
    # a prepared set is taken as it is
    again = dataset.device_image_batches(gen.image_set, [2.0, 3.0, 4.0], 41, 16, torch.device('cuda'), seed=1)
    sd2, _ = next(again)
    assert again.image_set is gen.image_set and sd2.shape == (16, 41, 41, 3)


def test_train_script_with_device_patches(tmp_path):
    from PIL import Image
    from ml_super_resolution_amd.vdsr import experiment_train
    rng = np.random.default_rng(8)
    data = tmp_path / 'images'
    data.mkdir()
    for i, (h, w) in enumerate(((64, 70), (41, 90), (30, 30), (80, 55))):              # one too small
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(str(data / ('im%d.png' % i)))
    ckpt = str(tmp_path / 'ckpt')
    log = []
    torch.manual_seed(5)
    experiment_train.main(['--data_path', str(data), '--ckpt_path', ckpt, '--batch_size', '8', '--num_layers', '5',
                           '--initial_learning_rate', '1e-3', '--stop_training_at_k_step', '3', '--patch_source', 'device'],
                          log=log.append)
    assert [r['step'] for r in log] == [1, 2, 3]
    assert all(np.isfinite(r['loss']) for r in log)
    assert 'model.ckpt-3.index' in os.listdir(ckpt)
