"""ESPCN and SRCNN through the reference-shaped entry points, against golden vectors / the oracle."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.golden.make_golden import espcn_params, srcnn_params
from tests.test_gpu_ops import close, dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('r', [3, 4])
def test_espcn_test_model_and_d2s(r, golden_nets, tmp_path):
    from ml_super_resolution_amd import graph, ops
    from ml_super_resolution_amd.espcn import model_espcn, experiment_test
    g = golden_nets
    params = espcn_params(103 + r, r)
    # checkpoint with the reference's variable names; build_test_model infers the scale from f3/bias
    ck = {}
    for name, (k, b) in zip(('f1', 'f2', 'f3'), params):
        ck[name + '/kernel:0'] = k
        ck[name + '/bias:0'] = b
    path = str(tmp_path / 'model.ckpt.npz')
    np.savez(path, **ck)
    assert set(model_espcn.extract_weights(None, path)) == set(ck)
    model = model_espcn.build_test_model(None, path)
    assert model['scaling_factor'] == r
    assert set(k for k in model if not k.startswith('_')) == {'lr_sources', 'sr_results', 'scaling_factor'}
    with graph.Session() as session:
        sr = session.run(model['sr_results'], feed_dict={model['lr_sources']: g['espcn%d.lr' % r]})
    close(sr, g['espcn%d.y' % r])
    # depth-to-space of the GPU result is the same permutation as the oracle's
    hr = ops.depth_to_space(dev(sr), r).cpu().numpy()
    np.testing.assert_array_equal(hr, O.depth_to_space(sr, r))
    close(hr, g['espcn%d.d2s' % r])
    # reference host spelling (experiment_test.py:171-177) on image 0
    np.testing.assert_array_equal(hr[0], O.d2s_ref_spelling_test(sr[0], r))
    # label layout helper == space_to_depth op == reference spelling (dataset.py:140-156)
    lab = experiment_test.space_to_depth_numpy(hr[0], r)
    np.testing.assert_array_equal(lab, sr[0])
    np.testing.assert_array_equal(ops.space_to_depth(dev(hr), r).cpu().numpy(), sr)
    # whole-image path of experiment_test.py:159-181: uint8 image -> [-1,1] (float64 arithmetic, as numpy does for
    # uint8 / 127.5) -> net -> depth-to-space -> * 0.5 + 0.5 -> clip
    img = np.random.default_rng(r).integers(0, 256, (11, 9, 3), dtype=np.uint8)
    got = experiment_test.super_resolve_array(model, img)
    lr_ref = (img / 127.5 - 1.0).astype(np.float32)[None]
    y_ref = O.espcn_forward(lr_ref, params)
    y_ref = np.asarray(y_ref['sr_result'] if isinstance(y_ref, dict) else y_ref)
    want = np.clip(O.depth_to_space(y_ref, r)[0] * 0.5 + 0.5, 0.0, 1.0)
    assert got.shape == (11 * r, 9 * r, 3)
    close(got, want)


def test_espcn_train_step_vs_oracle():
    from ml_super_resolution_amd import graph
    from ml_super_resolution_amd.espcn import model_espcn
    r = 3
    lr_ph = graph.placeholder([None, None, None, 3])
    hr_ph = graph.placeholder([None, None, None, 3 * r * r])
    model = model_espcn.build_model(lr_ph, r, hr_ph)
    assert set(k for k in model if not k.startswith('_')) == {'lr_source', 'sr_result', 'hr_target', 'step', 'loss',
                                                               'optimizer', 'learning_rate'}
    params = espcn_params(200, r)
    m = model['_model']
    m.stack.set_params(params)
    rng = np.random.default_rng(21)
    lr = rng.uniform(-1, 1, (4, 17, 17, 3)).astype(np.float32)
    hr = rng.uniform(-1, 1, (4, 51, 51, 3)).astype(np.float32)
    target = O.space_to_depth(hr, r)
    with graph.Session() as session:
        out = session.run({'step': model['step'], 'loss': model['loss'], 'optimizer': model['optimizer']},
                          feed_dict={model['lr_source']: lr, model['hr_target']: target, model['learning_rate']: 0.01})
    # oracle: forward, MSE in sub-pixel space, backward through tanh/tanh/linear, TF-Adam
    (k1, b1), (k2, b2), (k3, b3) = [(k.astype(np.float64), b.astype(np.float64)) for k, b in params]
    t1 = O.conv2d_fwd(lr, k1, b1, 'SAME', 'tanh'); t2 = O.conv2d_fwd(t1, k2, b2, 'SAME', 'tanh')
    y = O.conv2d_fwd(t2, k3, b3, 'SAME', None)
    loss, dy = O.mse_fwd_bwd(y, target)
    assert out['step'] == 1 and abs(out['loss'] - loss) <= 1e-4 * loss
    dk3, db3 = O.conv2d_bwd_filter(t2, dy, (3, 3)); d2 = O.conv2d_bwd_data(dy, k3, (17, 17)) * (1 - t2 * t2)
    dk2, db2 = O.conv2d_bwd_filter(t1, d2, (3, 3)); d1 = O.conv2d_bwd_data(d2, k2, (17, 17)) * (1 - t1 * t1)
    dk1, db1 = O.conv2d_bwd_filter(lr, d1, (5, 5))
    st = m.stack
    for i, (dk, db) in enumerate(((dk1, db1), (dk2, db2), (dk3, db3))):
        close(st.kernel(i, st.grads), dk)
        close(st.bias(i, st.grads), db)
    close(st.kernel(0), O.adam_tf(k1, dk1, 0.0, 0.0, 0.01, 1)[0], 1e-4)


@pytest.mark.parametrize('n,h,w,r', [(64, 17, 17, 3), (5, 23, 40, 2), (3, 9, 9, 4), (70, 17, 17, 3)],
                         ids=['recipe_batch', 'r2_ragged', 'r4', 'more_tiles_than_cus'])
def test_espcn_train_forward_in_one_launch_equals_three_launches(n, h, w, r):
    """The forward pass of ESPCN's train step as ONE launch (srx_espcn_forward_keep: the layers chained through LDS, t1 / t2 / y
    written for backward; espcn/espcn/model_espcn.py:117-160) against the three per-layer launches: activations, loss,
    gradients and the weights after three Adam steps bit-identical; t1 against the oracle."""
    from ml_super_resolution_amd.espcn import model_espcn
    g = torch.Generator(device='cuda').manual_seed(n * 100 + h)
    x = torch.rand((n, h, w, 3), device='cuda', generator=g) * 2 - 1
    target = torch.rand((n, h, w, 3 * r * r), device='cuda', generator=g) * 2 - 1
    res = []
    for fused in (True, False):
        m = model_espcn.EspcnModel(r, device='cuda', seed=77)
        for i in range(3):
            m.stack.bias(i).copy_(torch.linspace(-0.1, 0.1, m.stack.bias(i).numel(), device='cuda'))
        m.use_single_launch_train = fused
        m.single_launch_train_max_pixels = 10 ** 9
        m.stack.use_step_graph = False
        y = m.stack.forward(x, keep=True)
        acts = [a.clone() for a in m.stack.acts]
        losses = [float(m.train_step(x, target, 1e-3)) for _ in range(3)]
        res.append((y.clone(), acts, losses, m.stack.grads.clone(), m.stack.params.clone()))
    (y1, a1, l1, g1, p1), (y0, a0, l0, g0, p0) = res
    assert torch.equal(y1, y0) and all(torch.equal(u, v) for u, v in zip(a1, a0))
    assert l1 == l0 and torch.equal(g1, g0) and torch.equal(p1, p0)
    if n * h * w <= 6000:
        m = model_espcn.EspcnModel(r, device='cuda', seed=77)
        k1 = m.stack.kernel(0).cpu().numpy()
        b1 = np.linspace(-0.1, 0.1, 64).astype(np.float32)
        close(a1[1], O.conv2d_fwd(x.cpu().numpy(), k1, b1, 'SAME', 'tanh'))


def test_srcnn_forward_and_train_vs_oracle(golden_nets):
    from ml_super_resolution_amd import graph
    from ml_super_resolution_amd.srcnn import srcnn
    g = golden_nets
    flags = srcnn._flags().parse_args(['--train', '--crop-image-size', '33'])
    srcnn.sanity_check(flags)
    assert (flags.crop_image_side, flags.crop_image_size) == (6, 33)
    model = srcnn.build_srcnn(flags=flags)
    assert set(k for k in model if not k.startswith('_')) == {'step', 'loss', 'trainer', 'hd_images', 'sd_images', 'sr_images'}
    m = model['_model']
    params = srcnn_params(107)
    m.stack.set_params(params)
    hd_full = np.random.default_rng(5).uniform(-1, 1, (1, 33, 33, 3)).astype(np.float32)
    feed = {model['_feed_sd_images']: g['srcnn.lo'], model['_feed_hd_images']: hd_full}
    with graph.Session() as session:
        out = session.run({'sr': model['sr_images'], 'loss': model['loss'], 'hd': model['hd_images']}, feed_dict=feed)
    assert out['sr'].shape == (1, 21, 21, 3) and out['hd'].shape == (1, 21, 21, 3)
    close(out['sr'], g['srcnn.y'])
    np.testing.assert_array_equal(out['hd'], hd_full[:, 6:27, 6:27])
    ref_loss, dsr = O.srcnn_loss_and_grad(O.srcnn_forward(g['srcnn.lo'], params), hd_full[:, 6:27, 6:27])
    assert abs(out['loss'] - ref_loss) <= 1e-4 * ref_loss
    # one Adam(1e-3, .5, .9) step; check the gradient of the last layer against the oracle
    with graph.Session() as session:
        o2 = session.run({'step': model['step'], 'trainer': model['trainer'], 'loss': model['loss']}, feed_dict=feed)
    assert o2['step'] == 1
    (k1, b1), (k2, b2), (k3, b3) = params
    t1 = O.conv2d_fwd(g['srcnn.lo'], k1, b1, 'VALID', 'relu'); t2 = O.conv2d_fwd(t1, k2, b2, 'VALID', 'relu')
    y = O.conv2d_fwd(t2, k3, b3, 'VALID', 'tanh')
    dpre3 = dsr * (1 - y * y)
    dk3, db3 = O.conv2d_bwd_filter(t2, dpre3, (5, 5), 'VALID')
    close(m.stack.kernel(2, m.stack.grads), dk3)
    close(m.stack.bias(2, m.stack.grads), db3)
    d2 = O.conv2d_bwd_data(dpre3, k3, t2.shape[1:3], 'VALID') * (t2 > 0)
    dk2, _ = O.conv2d_bwd_filter(t1, d2, (1, 1), 'VALID')
    close(m.stack.kernel(1, m.stack.grads), dk2)
    d1 = O.conv2d_bwd_data(d2, k2, t1.shape[1:3], 'VALID') * (t1 > 0)
    dk1, _ = O.conv2d_bwd_filter(g['srcnn.lo'], d1, (9, 9), 'VALID')
    close(m.stack.kernel(0, m.stack.grads), dk1)


def test_srcnn_config1_shape():
    """BASELINE configs[0]: SRCNN 9-1-5 on one 256x256 image -> crop 243 -> 231x231 (pin P4)."""
    from ml_super_resolution_amd.srcnn import srcnn
    flags = srcnn._flags().parse_args([])
    srcnn.sanity_check(flags)
    assert (flags.crop_image_side, flags.crop_image_size, flags.batch_size) == (6, 243, 1)
    m = srcnn.SrcnnModel(flags, seed=3)
    x = torch.rand((1, 243, 243, 3), device='cuda') * 2 - 1
    y = m.forward(x)
    assert tuple(y.shape) == (1, 231, 231, 3)
    params = [(m.stack.kernel(i).cpu().numpy(), m.stack.bias(i).cpu().numpy()) for i in range(3)]
    ref = O.c_conv2d_fwd(O.c_conv2d_fwd(O.c_conv2d_fwd(x.cpu().numpy(), *params[0], 'VALID', 'relu'), *params[1], 'VALID', 'relu'),
                         *params[2], 'VALID', 'tanh')
    close(y, ref)


def test_enet_generator_forward_vs_oracle():
    """EnhanceNet generator (model_enet.py:44-115): 3x3 / 1x1 convs, residual blocks with fused
    skip + ReLU, nearest-neighbour x2 upsampling twice, + bicubic image."""
    from ml_super_resolution_amd import graph
    from ml_super_resolution_amd.enet import model_enet
    sd_ph, bq_ph = graph.placeholder([None, None, None, 3]), graph.placeholder([None, None, None, 3])
    model = model_enet.build_enet(sd_ph, bq_ph, None)
    assert set(k for k in model if not k.startswith('_')) == {'sd_images', 'bq_images', 'sr_images'}
    g = model['_model']
    rng = np.random.default_rng(31)
    pairs = []
    for k, cin, cout in model_enet.generator_layers():
        pairs.append((rng.normal(0, 1.0 / np.sqrt(k * k * cin), (k, k, cin, cout)).astype(np.float32),
                      rng.uniform(-0.1, 0.1, cout).astype(np.float32)))
    g.set_params(pairs)
    assert len(g.variables()) == 2 * 25 and 'g_/conv2d_24/kernel' in g.variables()
    sd = rng.uniform(-1, 1, (1, 12, 10, 3)).astype(np.float32)
    bq = rng.uniform(-1, 1, (1, 48, 40, 3)).astype(np.float32)
    with graph.Session() as session:
        sr = session.run(model['sr_images'], feed_dict={sd_ph: sd, bq_ph: bq})
    # oracle
    t = O.c_conv2d_fwd(sd, *pairs[0], 'SAME', 'relu')
    i = 1
    for _ in range(10):
        x = O.c_conv2d_fwd(t, *pairs[i], 'SAME', 'relu')
        t = O.c_conv2d_fwd(x, *pairs[i + 1], 'SAME', None, skip=t, post_relu=True)
        i += 2
    for _ in range(2):
        t = np.repeat(np.repeat(t, 2, axis=1), 2, axis=2)     # resize_nearest_neighbor by an integer factor
        t = O.c_conv2d_fwd(t, *pairs[i], 'SAME', 'relu')
        i += 1
    t = O.c_conv2d_fwd(t, *pairs[i], 'SAME', 'relu')
    ref = O.c_conv2d_fwd(t, *pairs[i + 1], 'SAME', None, skip=bq)
    assert sr.shape == (1, 48, 40, 3)
    close(sr, ref)


def test_enet_generator_backward_and_adam_vs_oracle():
    """Generator backward for a given gradient on sr_images + the Adam(1e-4) update of the g_ variables
    (model_enet.py:331-337): residual blocks, 2x2 block sums of the two upsamplings, fused ReluGrad masks."""
    from ml_super_resolution_amd.enet import model_enet
    g = model_enet.EnetGenerator(device='cuda', seed=3)
    rng = np.random.default_rng(32)
    pairs = []
    for k, cin, cout in model_enet.generator_layers():
        pairs.append((rng.normal(0, 1.0 / np.sqrt(k * k * cin), (k, k, cin, cout)).astype(np.float32),
                      rng.uniform(-0.1, 0.1, cout).astype(np.float32)))
    g.set_params(pairs)
    sd = rng.uniform(-1, 1, (2, 9, 19, 3)).astype(np.float32)        # 4x: 36 x 76 (column strips at the last layers)
    bq = rng.uniform(-1, 1, (2, 36, 76, 3)).astype(np.float32)
    d_sr = rng.normal(0, 1, (2, 36, 76, 3)).astype(np.float32)
    with pytest.raises(RuntimeError):
        g.backward(dev(d_sr))
    sr = g.forward(dev(sd), dev(bq), keep=True)
    grads = g.backward(dev(d_sr))
    sr_ref, ins = O.enet_generator_forward(sd, bq, pairs, keep=True)
    close(sr, sr_ref)
    ref = O.enet_generator_backward(ins, d_sr, pairs)
    for i, ((dw, db), (rw, rb)) in enumerate(zip(grads, ref)):
        close(dw, rw)
        close(db, rb)
    # one Adam step (checked on the gradients the device produced: the first step's m / sqrt(v) amplifies the last
    # bits of a near-zero gradient, which is a property of Adam, not of the update kernel)
    dev_grads = [(dw.cpu().numpy().astype(np.float64), db.cpu().numpy().astype(np.float64)) for dw, db in grads]
    assert all(dw.data_ptr() == g.pool.view(2 * i, g.grads).data_ptr() and db.data_ptr() == g.pool.view(2 * i + 1, g.grads).data_ptr()
               for i, (dw, db) in enumerate(grads))                  # (backward wrote the buffer the optimizer reads)
    g.pool.adam_step(1e-4)
    assert g.pool.t == 1
    for i, ((k0, b0), (gw, gb)) in enumerate(zip(pairs, dev_grads)):
        wk, _, _ = O.adam_tf(k0.astype(np.float64), gw, np.zeros_like(gw), np.zeros_like(gw), 1e-4, 1)
        wb, _, _ = O.adam_tf(b0.astype(np.float64), gb, np.zeros_like(gb), np.zeros_like(gb), 1e-4, 1)
        np.testing.assert_allclose(g.kernels[i].cpu().numpy(), wk, rtol=0, atol=1e-6)
        np.testing.assert_allclose(g.biases[i].cpu().numpy(), wb, rtol=0, atol=1e-6)


def test_enet_experiment_resolve_script(tmp_path):
    """enet/enet/experiment_resolve.py: --extract_model keeps the g_ variables of a training checkpoint; the resolving
    mode writes <name>_bq.png (PIL bicubic x4, as scipy.misc.imresize) and <name>_sr.png (saturate_cast bytes)."""
    from PIL import Image
    from ml_super_resolution_amd import tf_bundle
    from ml_super_resolution_amd.enet import experiment_resolve, model_enet
    rng = np.random.default_rng(41)
    pairs, tensors = [], {}
    for i, (k, cin, cout) in enumerate(model_enet.generator_layers()):
        w = rng.normal(0, 1.0 / np.sqrt(k * k * cin), (k, k, cin, cout)).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, cout).astype(np.float32)
        pairs.append((w, b))
        scope = 'g_/conv2d' if i == 0 else 'g_/conv2d_%d' % i
        tensors[scope + '/kernel'], tensors[scope + '/bias'] = w, b
        tensors[scope + '/kernel/Adam'] = np.zeros_like(w)            # optimizer slots and the other networks'
    tensors['d_/conv2d/kernel'] = np.zeros((3, 3, 3, 32), np.float32)  # variables must not survive the extraction
    tensors['global_step'] = np.asarray(1234, np.int64)
    full = str(tmp_path / 'train' / 'model.ckpt-1234')
    tf_bundle.save_checkpoint(full, tensors)
    experiment_resolve.main(['--extract_model', 'true', '--source_ckpt_path', full,
                             '--target_ckpt_path', str(tmp_path / 'extracted')])
    kept = tf_bundle.load_checkpoint(str(tmp_path / 'extracted' / 'model.ckpt'))
    assert len(kept) == 50 and all(k.startswith('g_/') and k.split('/')[-1] in ('kernel', 'bias') for k in kept)
    src, dst = tmp_path / 'src', tmp_path / 'dst'
    src.mkdir()
    imgs = {'a': rng.integers(0, 256, (9, 14, 3), dtype=np.uint8), 'b': rng.integers(0, 256, (12, 10, 3), dtype=np.uint8)}
    for name, im in imgs.items():
        Image.fromarray(im).save(str(src / (name + '.png')))
    (src / 'notes.txt').write_text('not an image')
    # pin P5: a crop of the reference's assets/enet_eagle.png; its `_bq.png` must reproduce the reference's own
    # assets/enet_eagle_bq.png bytes (away from the crop border) through the DEVICE path u8 -> /127.5-1 -> saturate_u8
    import os
    p5 = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'pin_p5_eagle_crop.npz'))
    Image.fromarray(p5['source']).save(str(src / 'eagle.png'))
    experiment_resolve.main(['--source_ckpt_path', str(tmp_path / 'extracted' / 'model.ckpt'),
                             '--source_dir_path', str(src), '--target_dir_path', str(dst)])
    assert sorted(p.name for p in dst.iterdir()) == ['a_bq.png', 'a_sr.png', 'b_bq.png', 'b_sr.png', 'eagle_bq.png',
                                                      'eagle_sr.png']
    got_bq = np.asarray(Image.open(str(dst / 'eagle_bq.png')))
    m = 12
    np.testing.assert_array_equal(got_bq[m:-m, m:-m], p5['reference_bq'][m:-m, m:-m])
    # and the encoder alone, on the reference's bytes mapped to [-1, 1] as the reference feeds them: identity
    from ml_super_resolution_amd import ops as srx_ops
    ref_f = dev(p5['reference_bq'].astype(np.float32) / np.float32(127.5) - np.float32(1.0))
    np.testing.assert_array_equal(srx_ops.saturate_u8(ref_f).cpu().numpy(), p5['reference_bq'])
    for name, im in imgs.items():
        bq_u8 = np.asarray(Image.fromarray(im).resize((im.shape[1] * 4, im.shape[0] * 4), Image.BICUBIC))
        sd = im.astype(np.float32)[None] / np.float32(127.5) - np.float32(1.0)
        bq = bq_u8.astype(np.float32)[None] / np.float32(127.5) - np.float32(1.0)
        # the bicubic image goes through the same float round trip and truncating encode as in the reference
        np.testing.assert_array_equal(np.asarray(Image.open(str(dst / (name + '_bq.png')))), O.saturate_u8(bq)[0])
        sr_ref = O.enet_generator_forward(sd, bq, pairs)
        got = np.asarray(Image.open(str(dst / (name + '_sr.png')))).astype(np.int32)
        want = O.saturate_u8(sr_ref.astype(np.float32))[0].astype(np.int32)
        assert got.shape == want.shape == (im.shape[0] * 4, im.shape[1] * 4, 3)
        # fp32 on the device vs float64 in the oracle: a value next to an integer may truncate to the neighbouring byte
        assert np.abs(got - want).max() <= 1 and (got != want).mean() < 0.01


def test_tf_bicubic_resize_vs_oracle_and_reference_panels():
    """srx_resize_bicubic_tf (tf.image.resize_bicubic with TensorFlow 1.x semantics, srcnn/srcnn.py:89-93) against the
    oracle on up / down / non-integer scales, and against the reference's own hd | sd panels (pin P6)."""
    import os
    from ml_super_resolution_amd import ops
    rng = np.random.default_rng(8)
    for (n, h, w, c), (oh, ow) in (((2, 9, 12, 3), (27, 36)), ((1, 30, 21, 3), (10, 7)), ((2, 8, 8, 4), (13, 5)),
                                   ((1, 243, 243, 3), (81, 81)), ((1, 5, 7, 1), (5, 7))):
        x = rng.uniform(-1, 1, (n, h, w, c)).astype(np.float32)
        close(ops.resize_bicubic_tf(dev(x), oh, ow), O.resize_bicubic_tf(x, oh, ow))
    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'pin_p6_srcnn_panels.npz'))
    for j in (0, 1):
        hd, sd = z['hd%d' % j].astype(np.float32), z['sd%d' % j].astype(np.float64)
        up = ops.resize_bicubic_tf(ops.resize_bicubic_tf(dev(hd[None]), 77, 77), 231, 231)[0].cpu().numpy().astype(np.float64)
        d = np.clip(up, 0, 255)[15:-15, 15:-15] - sd[15:-15, 15:-15]
        assert 10 * np.log10(255.0 ** 2 / np.mean(d * d)) > 40.0


def test_srcnn_script_train_checkpoint_resume_and_panel(tmp_path):
    """srcnn/srcnn.py's script (:208-298): the dataset reader's crop, the on-device bicubic degradation, Adam(1e-3, .5,
    .9) steps, checkpoints in tf.train.Saver format under the graph's variable names, resume, and the hd | sd | sr panel."""
    from PIL import Image
    from ml_super_resolution_amd import tf_bundle
    from ml_super_resolution_amd.srcnn import srcnn
    rng = np.random.default_rng(1)
    img_dir = tmp_path / 'jpg'
    img_dir.mkdir()
    for i in range(2):
        yy, xx = np.mgrid[0:300, 0:320]
        im = np.stack([127 + 100 * np.sin(xx / (7.0 + i) + c) * np.cos(yy / 9.0) for c in range(3)], -1)
        Image.fromarray(np.clip(im + rng.normal(0, 5, im.shape), 0, 255).astype(np.uint8)).save(str(img_dir / ('%d.jpg' % i)), quality=95)
    ckpt = str(tmp_path / 'ckpt')
    argv = ['--train', '--training-images-path', str(img_dir), '--ckpt-dir-path', ckpt, '--batch-size', '2', '--save-every', '2']
    flags = srcnn.sanity_check(srcnn._flags().parse_args(argv))
    assert flags.crop_image_size == 243 and flags.crop_image_side == 6
    log = []
    torch.manual_seed(9)
    m = srcnn.train(flags, max_steps=3, seed=4, log=lambda s, l: log.append((s, l)))
    assert [s for s, _ in log] == [1, 2, 3] and all(np.isfinite(l) for _, l in log)
    saved = tf_bundle.load_checkpoint(tf_bundle.latest_checkpoint(ckpt))
    assert tf_bundle.latest_checkpoint(ckpt).endswith('model.ckpt-2') and int(saved['global_step']) == 2
    for key, shape in (('patch_extraction/weights', (9, 9, 3, 64)), ('non_linear_mapping/biases', (32,)),
                       ('reconstruction/weights', (5, 5, 32, 3)), ('reconstruction/weights/Adam_1', (5, 5, 32, 3))):
        assert saved[key].shape == shape, key
    np.testing.assert_allclose(saved['beta1_power'], 0.5 ** 3, rtol=1e-6)          # Adam(beta1 = .5), two steps
    np.testing.assert_allclose(saved['beta2_power'], 0.9 ** 3, rtol=1e-6)
    # resume: starts at step 2
    log2 = []
    srcnn.train(flags, max_steps=1, seed=4, log=lambda s, l: log2.append(s))
    assert log2 == [3]
    # inference: one crop of the source -> the 693 x 231 panel
    out = str(tmp_path / 'panel.jpg')
    fl = srcnn.sanity_check(srcnn._flags().parse_args(['--sr-source-path', str(img_dir / '0.jpg'), '--sr-target-path', out,
                                                       '--ckpt-dir-path', ckpt]))
    assert fl.batch_size == 1
    px = srcnn.super_resolution(fl, seed=2)
    assert px.shape == (231, 693, 3) and Image.open(out).size == (693, 231)
    # the sd strip of the panel is TensorFlow's bicubic of the hd strip's source crop: both strips differ, both are images
    assert np.abs(px[:, :231].astype(int) - px[:, 231:462].astype(int)).mean() > 0.5


@pytest.mark.parametrize('filt', ['bilinear', 'bicubic'])
def test_resize_pil_u8_on_the_device_is_byte_exact(filt):
    """ops.resize_pil_u8 (srx_pil_resample_coeffs on the host + two integer passes of srx_resample_u8) against the
    oracle's restatement of Pillow's resample -- the reference's scipy.misc.imresize -- byte for byte; and
    astype(float32) / 127.5 - 1."""
    from ml_super_resolution_amd import ops
    rng = np.random.default_rng(23)
    for n, h, w, oh, ow in ((3, 128, 128, 32, 32), (2, 32, 32, 128, 128), (1, 90, 51, 22, 12), (2, 40, 40, 57, 33), (1, 64, 64, 64, 16),
                            (1, 17, 23, 17, 92)):
        img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        got = ops.resize_pil_u8(torch.from_numpy(img).cuda(), oh, ow, filt)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, oh, ow, 3)
        np.testing.assert_array_equal(got.cpu().numpy(), O.pil_resize_u8(img, oh, ow, filt))
    x = torch.arange(256, dtype=torch.uint8).cuda()
    np.testing.assert_array_equal(ops.u8_to_pm1(x).cpu().numpy(), O.u8_to_pm1(np.arange(256, dtype=np.uint8)))


def test_enet_datasets_image_batches(tmp_path):
    """enet/enet/datasets.py:79-127 on the device: random 128x128 crops, 25 % bilinear down, 400 % bicubic up, / 127.5 - 1 --
    the same bytes as scipy.misc.imresize (= Pillow) on the host, with the reference's random-number calls in order."""
    from PIL import Image
    from ml_super_resolution_amd.enet import datasets
    rng = np.random.default_rng(29)
    images = {}
    for name in ('a.png', 'b.jpg', 'c.PNG'):
        images[name] = rng.integers(0, 256, (260, 300, 3), dtype=np.uint8)
        Image.fromarray(images[name]).save(str(tmp_path / name), quality=95)
    (tmp_path / 'readme.txt').write_text('not an image')
    it = datasets.image_batches(str(tmp_path), 4, batch_size=5, device='cuda', rng=np.random.RandomState(7))
    sd, bq, hd = next(it)
    assert tuple(sd.shape) == (5, 32, 32, 3) and tuple(bq.shape) == (5, 128, 128, 3) and tuple(hd.shape) == (5, 128, 128, 3)
    # the same walk on the host
    ref_rng = np.random.RandomState(7)
    names = sorted(n for n in os.listdir(str(tmp_path)) if datasets.is_image_name(n))

    def walk():
        while True:
            ref_rng.shuffle(names)
            for n in names:
                yield n
    order = walk()
    for i in range(5):
        full = np.asarray(Image.open(str(tmp_path / next(order))).convert('RGB'))
        x, y = ref_rng.randint(128), ref_rng.randint(128)
        crop = full[y:y + 128, x:x + 128]
        s8 = np.asarray(Image.fromarray(crop).resize((32, 32), Image.BILINEAR))
        b8 = np.asarray(Image.fromarray(s8).resize((128, 128), Image.BICUBIC))
        np.testing.assert_array_equal(hd[i].cpu().numpy(), O.u8_to_pm1(crop))
        np.testing.assert_array_equal(sd[i].cpu().numpy(), O.u8_to_pm1(s8))
        np.testing.assert_array_equal(bq[i].cpu().numpy(), O.u8_to_pm1(b8))
    sd2, _, _ = next(it)
    assert tuple(sd2.shape) == (5, 32, 32, 3)


# ---- round 4: Adam with its state in device memory; whole train steps replayed as HIP graphs ----------------------------
def test_adam_device_state_matches_host_argument_path():
    """srx_adam_tf_step_dev (step count and learning rate in device memory, lr_t evaluated on the device in double
    precision) against srx_adam_tf_step (lr_t evaluated by the host, a kernel argument) and the float64 oracle: 12 steps,
    a learning-rate change and a step count set from outside on the way."""
    from ml_super_resolution_amd import ops
    g = torch.Generator(device='cuda').manual_seed(3)
    n = 10007                                                   # (not a multiple of 4: the scalar tail runs)
    w0 = torch.randn(n + 1, device='cuda', generator=g)[:n].clone()
    wa, wb = w0.clone(), w0.clone()
    ma, va, mb, vb = (torch.zeros(n, device='cuda') for _ in range(4))
    st = ops.adam_state('cuda', t=0, lr=1e-3)
    wo, mo, vo = w0.double().cpu().numpy(), np.zeros(n), np.zeros(n)
    lr, t = 1e-3, 0
    for i in range(12):
        if i == 5:
            lr = 2.5e-4
            ops.adam_state_set(st, lr=lr)
        if i == 8:
            t = 999                                             # as after a checkpoint load
            ops.adam_state_set(st, t=t)
        grad = torch.randn(n, device='cuda', generator=g)
        t += 1
        ops.adam_tf_step(wa, grad, ma, va, lr, t, 0.5, 0.9, 1e-8)
        ops.adam_tf_step_dev(wb, grad, mb, vb, st, 0.5, 0.9, 1e-8)
        wo, mo, vo = O.adam_tf(wo, grad.double().cpu().numpy(), mo, vo, lr, t, 0.5, 0.9, 1e-8)
        got_t, got_lr, got_lr_t = ops.adam_state_get(st)
        assert got_t == t and abs(got_lr - lr) < 1e-12 * 1e6
        ref_lr_t = lr * np.sqrt(1 - float(np.float32(0.9)) ** t) / (1 - 0.5 ** t)     # (the betas cross the C ABI as floats)
        assert abs(got_lr_t - ref_lr_t) <= 1e-7 * ref_lr_t
    assert torch.equal(ma, mb) and torch.equal(va, vb)          # (no lr_t in the slots)
    # the weights: the same float lr_t unless the device's double-precision pow rounds the other way once in 2^29 times
    assert (wa - wb).abs().max().item() <= 2e-7 * wa.abs().max().item()
    close(wb, wo, 1e-5)


@pytest.mark.parametrize('net', ['espcn', 'srcnn'])
def test_train_step_graph_replay_equals_eager_launches(net):
    """ESPCN / SRCNN train steps replayed as one HIP graph per batch shape (engine.ConvStack.train_step_replay) against
    the same steps as eager launches: weights, Adam slots, gradients and the loss bit-identical after 10 steps; a fed
    learning rate that changes on the way (ESPCN's schedule, espcn/espcn/experiment_train.py:100-113), a batch of another
    shape in between (buffers are replaced: the captured step is dropped and rebuilt) and a step count set from outside."""
    from ml_super_resolution_amd.espcn import model_espcn
    from ml_super_resolution_amd.srcnn import srcnn
    g = torch.Generator(device='cuda').manual_seed(11)
    if net == 'espcn':
        ma, mb = model_espcn.EspcnModel(3, device='cuda', seed=5), model_espcn.EspcnModel(3, device='cuda', seed=5)
        xs = [torch.rand((64, 17, 17, 3), device='cuda', generator=g) * 2 - 1 for _ in range(3)]
        ts = [torch.rand((64, 17, 17, 27), device='cuda', generator=g) * 2 - 1 for _ in range(3)]
        x2, t2 = torch.rand((8, 9, 13, 3), device='cuda', generator=g), torch.rand((8, 9, 13, 27), device='cuda', generator=g)
        step = lambda m, x, t, lr: m.train_step(x, t, lr)
    else:
        fl = srcnn._flags().parse_args(['--train', '--crop-image-size', '33'])
        srcnn.sanity_check(fl)
        ma, mb = srcnn.SrcnnModel(fl, device='cuda', seed=5), srcnn.SrcnnModel(fl, device='cuda', seed=5)
        for m in (ma, mb):
            for i in range(3):
                m.stack.kernel(i).mul_(60.0)                  # O(1) activations instead of the reference's sigma 1e-3
        xs = [torch.rand((16, 33, 33, 3), device='cuda', generator=g) * 2 - 1 for _ in range(3)]
        ts = [torch.rand((16, 21, 21, 3), device='cuda', generator=g) * 2 - 1 for _ in range(3)]
        x2, t2 = torch.rand((2, 40, 37, 3), device='cuda', generator=g), torch.rand((2, 28, 25, 3), device='cuda', generator=g)
        step = lambda m, x, t, lr: m.train_step(x, t)
    assert torch.equal(ma.stack.params, mb.stack.params)
    ma.stack.use_step_graph = False
    mb.stack.use_step_graph = True           # (whatever SRX_STEP_GRAPH says)
    mb.stack.step_graph_max_pixels = None    # (and whatever size the model stops replaying at)
    losses = []
    for i in range(14):
        lr = 1e-3 if i < 6 else 3e-4
        if i == 9:
            x, t = x2, t2                                     # another batch shape in between
        else:
            x, t = xs[i % 3], ts[i % 3]
        if i == 11:
            ma.stack.global_step = mb.stack.global_step = 5000
        la = step(ma, x, t, lr).clone()
        lb = step(mb, x, t, lr).clone()
        losses.append((la, lb))
        assert ma.stack.global_step == mb.stack.global_step
    replayed = [k for k, e in mb.stack._step_graphs.items() if e['graph'] is not None]
    assert replayed, 'no step was replayed from a graph'
    assert not any(e['graph'] is not None for e in ma.stack._step_graphs.values())
    for la, lb in losses:
        assert torch.equal(la, lb)
    for name in ('params', 'grads', 'opt_m', 'opt_v'):
        assert torch.equal(getattr(ma.stack, name), getattr(mb.stack, name)), name
    from ml_super_resolution_amd import ops
    assert ops.adam_state_get(ma.stack._adam_state)[0] == ops.adam_state_get(mb.stack._adam_state)[0] == ma.stack.global_step == 5003


@pytest.mark.parametrize('fmt', ['state_dict', 'tf_checkpoint'])
@pytest.mark.parametrize('net', ['espcn', 'srcnn', 'vdsr6_momentum'])
def test_restore_into_a_model_that_has_trained_replays_the_restored_state(net, fmt, tmp_path):
    """A checkpoint restored into a stack whose train step is already captured (mid-run restore, train - evaluate - reload):
    the captured step holds the addresses of params / grads / opt_m / opt_v, so the restore must land in those buffers
    (param_pool.ParamPool.restore_slot; tests/test_host_logic.py has the pointer half).  Model R (replayed steps): 5 steps, save,
    3 more steps, restore INTO R, the same 3 batches again.  Model E (a fresh twin, eager launches): load, the same 3 batches.
    R's two passes and E agree bit for bit in params, slots, gradients, every loss and the step count.  The fix restores in
    place and keeps the captured steps: static_step_inputs still returns the tensors the next replay reads -- the second
    pass writes its first batch straight into them.  ESPCN: Adam through srx_adam_tf_step_dev (step count on the device);
    SRCNN: the row-norm loss; VDSR, 6 layers on 16 x 41 x 41: Momentum on clipped gradients, one slot."""
    from ml_super_resolution_amd.espcn import model_espcn
    from ml_super_resolution_amd.srcnn import srcnn
    from ml_super_resolution_amd.vdsr import model_vdsr
    g = torch.Generator(device='cuda').manual_seed(23)
    rnd = lambda *s: torch.rand(s, device='cuda', generator=g) * 2 - 1
    if net == 'espcn':
        make = lambda: model_espcn.EspcnModel(3, device='cuda', seed=5).stack
        xs, ts = [rnd(64, 17, 17, 3) for _ in range(8)], [rnd(64, 17, 17, 27) for _ in range(8)]
        step = lambda s, x, t: s.train_step_replay(x, t, 1e-3)
    elif net == 'srcnn':
        fl = srcnn._flags().parse_args(['--train', '--crop-image-size', '33'])
        srcnn.sanity_check(fl)

        def make():
            m = srcnn.SrcnnModel(fl, device='cuda', seed=5)
            for i in range(3):
                m.stack.kernel(i).mul_(60.0)                  # O(1) activations instead of the reference's sigma 1e-3
            return m.stack
        xs, ts = [rnd(16, 33, 33, 3) for _ in range(8)], [rnd(16, 21, 21, 3) for _ in range(8)]
        step = lambda s, x, t: s.train_step_replay(x, t, 0.001, beta1=0.5, beta2=0.9)
    else:
        make = lambda: model_vdsr.VdsrModel(num_layers=6, use_adam=False, device='cuda', seed=5).stack
        xs = [rnd(16, 41, 41, 3) for _ in range(8)]
        ts = [(x + 0.1 * rnd(16, 41, 41, 3)).clamp_(-1, 1) for x in xs]
        step = lambda s, x, t: s.train_step_replay(x, t, 0.01, momentum=0.9, gradient_cap=0.01)
    slots = ('opt_m',) if net == 'vdsr6_momentum' else ('opt_m', 'opt_v')
    names = ('params', 'grads') + slots

    def snapshot(s, losses):
        return {'step': s.global_step, 'losses': losses, **{k: getattr(s, k).clone() for k in names}}

    def same(a, b, what):
        assert a['step'] == b['step'], what
        for la, lb in zip(a['losses'], b['losses']):
            assert torch.equal(la, lb), what + ': loss'
        for k in names:
            assert torch.equal(a[k], b[k]), what + ': ' + k

    R = make()
    R.use_step_graph, R.step_graph_max_pixels = True, None
    for i in range(5):
        step(R, xs[i], ts[i])
    assert any(e['graph'] is not None for e in R._step_graphs.values()), 'no step was captured'
    assert R.global_step == 5
    path = str(tmp_path / ('model.ckpt-5' if fmt == 'tf_checkpoint' else 'model.pt'))
    if fmt == 'tf_checkpoint':
        R.save_tf_checkpoint(path)
    else:
        torch.save(R.state_dict(), path)
    first = snapshot(R, [step(R, xs[i], ts[i]).clone() for i in range(5, 8)])
    assert first['step'] == 8 and not torch.equal(first['params'], torch.zeros_like(first['params']))
    # restore into R itself
    ptrs = {k: getattr(R, k).data_ptr() for k in names}
    R.load_checkpoint(path)
    assert R.global_step == 5 and {k: getattr(R, k).data_ptr() for k in names} == ptrs
    if net == 'vdsr6_momentum':
        assert R.opt_v is None
    static = R.static_step_inputs(xs[5].shape, ts[5].shape)
    assert static is not None, 'the in-place restore keeps the captured step'
    sx, st = static
    sx.copy_(xs[5]); st.copy_(ts[5])                            # (no other copy of this batch reaches the replay)
    losses = [step(R, sx, st).clone()] + [step(R, xs[i], ts[i]).clone() for i in range(6, 8)]
    second = snapshot(R, losses)
    same(second, first, 'replayed after the restore vs replayed before it')
    # the eager twin
    E = make()
    E.use_step_graph = False
    E.load_checkpoint(path)
    assert E.global_step == 5
    eager = snapshot(E, [step(E, xs[i], ts[i]).clone() for i in range(5, 8)])
    assert not any(e['graph'] is not None for e in E._step_graphs.values())
    same(eager, first, 'fresh eager twin vs the trained model')
