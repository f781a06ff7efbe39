"""BASELINE configs[4]'s tile shape -- EnhanceNet-PAT on 512x512 HR tiles (128 -> 512) -- checked for CORRECTNESS, not only
timed.  Paths that only this size reaches: the discriminator's dense layer on 16*16*512 = 131,072 inputs (split-K GEMM;
enet/enet/model_enet.py:148-154 -- the dense layer fixes D's input size, so a 512-tile discriminator is
Discriminator(image_size=512)), its first layers on 512-wide column strips, VGG block 1 on 512-wide strips,
conv_wide_pipe_kernel on 256^2 / 128^2 maps, the texture statistics on 32 x 32 patches per image.
Reference: enet/enet/model_enet.py:118-162 (discriminator), :185-261 (losses), :264-350 (build_enet); model_vgg.py:65-99."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import oracle_enet as E
from tests.test_gpu_enet_pat import (_device_disc_state, _device_vgg_feats, _disc_params, _enet_setup, _np,
                                     _oracle_vgg_weights, to_nhwc_np)
from tests.test_gpu_ops import close, dev

pytestmark = pytest.mark.gpu

SIZE = 512


def test_discriminator_at_512(width=32, units=1024, n=2):
    """Forward, input gradient and every variable's gradient at 512 x 512, at the reference's widths (32 .. 512 channels,
    1024 dense units), two tiles: the stride-2 chain 512 -> 16, the dense layer on 16*16*512 = 131,072 inputs (the
    deterministic split-K GEMM with M = batch).  (Narrower discriminators are not a case: the filter-gradient kernels
    exist for the reference's layer shapes, and a 3 -> 8 channel first layer is refused with SRX_ERR_UNSUPPORTED.)"""
    from ml_super_resolution_amd.enet import model_enet
    rng = np.random.default_rng(70 + width)
    convs, dense = _disc_params(rng, width, SIZE, units)
    assert dense[0][0].shape[0] == 16 * 16 * 16 * width
    D = model_enet.Discriminator(device='cuda', width=width, image_size=SIZE, dense_units=units)
    D.set_params(convs, dense)
    x = rng.uniform(-1, 1, (n, SIZE, SIZE, 3)).astype(np.float32)
    p = D.forward(dev(x), keep=True)
    pref, saved = E.discriminator_forward(x, convs, dense, keep=True)
    close(p, pref)
    for i in (0, 1, 4, 9):
        close(to_nhwc_np(D._saved[0][i]), saved[0][i])
    del saved
    dp = rng.normal(size=pref.shape).astype(np.float32)
    dx = D.backward(dev(dp), want_dx=True, want_dw=True)
    dev_saved = ([to_nhwc_np(a).astype(np.float64) for a in D._saved[0]], _np(D._saved[1]).astype(np.float64),
                 _np(D._saved[2]).astype(np.float64))
    dx_ref, cg, dg = E.discriminator_backward(dev_saved, _np(p).astype(np.float64), dp, convs, dense)
    close(dx, dx_ref)
    grads = D.gradients()
    for i, (gk, gb) in enumerate(cg):
        scope = 'd_/conv2d' if i == 0 else 'd_/conv2d_%d' % i
        close(grads[scope + '/kernel'], gk)
        close(grads[scope + '/bias'], gb)
    for i, (gw, gb) in enumerate(dg):
        scope = 'd_/dense' if i == 0 else 'd_/dense_%d' % i
        close(grads[scope + '/kernel'], gw)
        close(grads[scope + '/bias'], gb)
    # deterministic: the same forward / backward again gives the same bits
    p2 = D.forward(dev(x), keep=True)
    dx2 = D.backward(dev(dp), want_dx=True, want_dw=True)
    assert torch.equal(p, p2) and torch.equal(dx, dx2)
    g2 = D.gradients()
    assert all(torch.equal(grads[k], g2[k]) for k in grads)


def test_vgg19_at_512():
    """VGG-19 at full width on one 512 x 512 tile: every tap the losses use and the deepest one, then the input gradient
    for gradients given on the perceptual + texture taps (block 1 runs on 512-wide column strips, blocks 2-3 on the
    pipelined wide kernel at 256^2 / 128^2)."""
    from ml_super_resolution_amd.enet import model_vgg
    w = model_vgg.random_vgg_weights(5, 64)
    net = model_vgg.Vgg19(w, device='cuda')
    rng = np.random.default_rng(8)
    img = rng.uniform(-1, 1, (1, SIZE, SIZE, 3)).astype(np.float32)
    feats = net.forward(dev(img), keep=True)
    ow = _oracle_vgg_weights(w)
    ref = E.vgg19_forward(img, ow)
    for name in ('block1_conv1', 'block1_conv2', 'block2_conv1', 'block2_pool', 'block3_conv1', 'block3_conv4', 'block4_conv1',
                 'block5_conv4', 'block5_pool'):
        close(net.tap(feats, name), ref[name])
    assert net.tap(feats, 'block5_pool').shape == (1, 16, 16, 512)
    taps = {}
    for name in ('block1_conv1', 'block2_conv1', 'block2_pool', 'block3_conv1', 'block5_pool'):
        taps[name] = (rng.normal(size=ref[name].shape) / ref[name].size).astype(np.float32)
    del ref
    got = net.backward({k: dev(v) for k, v in taps.items()})
    dev_feats = {'input': _np(net.tap(feats, 'input')).astype(np.float64)}
    for name in model_vgg.LAYER_NAMES:
        dev_feats[name] = _np(net.tap(feats, name)).astype(np.float64)
    close(got, E.vgg19_backward(dev_feats, ow, taps))


def test_generator_objective_at_512_against_the_oracle():
    """build_enet's generator objective on a 512-tile (model_enet.py:286-326) at the reference's widths: the five losses
    and d(g_losses)/d(sr_images), the oracle differentiating at the device's activations."""
    m, w, g_pairs, convs, dense, sd, bq, hd = _enet_setup('pat', 64, 32, SIZE, 1024, 1, seed=21)
    assert sd.shape == (1, 128, 128, 3)
    sr = m.generator.forward(dev(sd), dev(bq), keep=True)
    close(sr, O.enet_generator_forward(sd, bq, g_pairs))
    d_sr = m.generator_objective(sr, dev(hd), want_a_loss=True)
    ref_losses, dsr_ref = E.enet_losses_and_sr_gradient(_np(sr).astype(np.float64), hd, _oracle_vgg_weights(w), convs, dense, 'pat',
                                                        at_sr_feats=_device_vgg_feats(m.vgg),
                                                        at_fake=_device_disc_state(m.discriminator))
    for k, v in ref_losses.items():
        assert abs(m.losses[k].item() - v) <= 2e-4 * abs(v) + 1e-9, (k, m.losses[k].item(), v)
    close(d_sr, dsr_ref)


def test_trainers_at_512_batch_shard_invariance_and_determinism():
    """g_trainer / d_trainer on two 512-tiles: (1) every per-image quantity of the batch of two equals, bit for bit, the
    same image run alone (sr, D's outputs) and the gradient on sr_images is exactly half the single-image one (all
    losses are batch means; 1/2 is exact in binary) -- the property data parallelism over tiles rests on; (2) the same
    step from the same state gives the same bits; (3) the Adam updates move every variable group."""
    m, w, g_pairs, convs, dense, sd, bq, hd = _enet_setup('pat', 16, 32, SIZE, 64, 2, seed=31)
    sdd, bqd, hdd = dev(sd), dev(bq), dev(hd)
    sr = m.generator.forward(sdd, bqd, keep=True)
    d_sr = m.generator_objective(sr, hdd).clone()
    fake = m.discriminator.forward(sr).clone()
    for i in range(2):
        one = slice(i, i + 1)
        sr1 = m.generator.forward(sdd[one].contiguous(), bqd[one].contiguous(), keep=True)
        assert torch.equal(sr1[0], sr[i])
        assert torch.equal(m.discriminator.forward(sr1)[0], fake[i])
        d1 = m.generator_objective(sr1, hdd[one].contiguous())
        assert torch.equal(d1[0] * 0.5, d_sr[i]), float((d1[0] * 0.5 - d_sr[i]).abs().max())
    state = (m.generator.params.clone(), m.discriminator.pool.params.clone())
    runs = []
    for _ in range(2):
        m.generator.params.copy_(state[0]); m.discriminator.pool.params.copy_(state[1])
        for pool in (m.generator.pool, m.discriminator.pool):
            pool.opt_m = pool.opt_v = None
            pool.t = 0
        m.global_step = 0
        a = m.d_step(sdd, bqd, hdd).clone()
        losses = {k: v.clone() for k, v in m.g_step(sdd, bqd, hdd).items()}
        runs.append((a, losses, m.generator.params.clone(), m.discriminator.pool.params.clone(), m.generator.grads.clone(),
                     m.discriminator.pool.grads.clone()))
    (a0, l0, g0, d0, gg0, dg0), (a1, l1, g1, d1_, gg1, dg1) = runs
    assert torch.equal(a0, a1) and all(torch.equal(l0[k], l1[k]) for k in l0)
    assert torch.equal(g0, g1) and torch.equal(d0, d1_) and torch.equal(gg0, gg1) and torch.equal(dg0, dg1)
    assert not torch.equal(g0, state[0]) and not torch.equal(d0, state[1])
    assert all(torch.isfinite(v).all() for v in (g0, d0, gg0, dg0)) and m.global_step == 1
