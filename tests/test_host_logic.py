"""Host-side logic that needs no GPU: variable fetches without feeds, checkpoint naming / state file / beta powers,
flag parsing.  (The C ABI's threading promise is checked in tests/test_tsan_host.py.)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_and_learning_rate_fetch_need_no_feed():
    """`step = session.run(model['step'])` is the first line of the reference's loops
    (vdsr/vdsr/experiment_train.py:126, espcn/espcn/experiment_train.py:92): no placeholder is fed."""
    from ml_super_resolution_amd import graph
    from ml_super_resolution_amd.espcn import model_espcn
    from ml_super_resolution_amd.vdsr import model_vdsr
    sd, hd = graph.placeholder(name='sd'), graph.placeholder(name='hd')
    model = model_vdsr.build_model(sd, hd, num_layers=3, use_adam=True, device='cpu', seed=0)
    with graph.Session() as session:
        assert session.run(model['step']) == 0
        assert session.run(model['learning_rate']) == pytest.approx(0.1)        # model_vdsr.py:136-141
        assert session.run({'s': model['step']}, feed_dict={model['learning_rate']: 0.01}) == {'s': 0}
        with pytest.raises(ValueError, match='sd_images must be fed'):
            session.run(model['sr_images'])
        with pytest.raises(ValueError, match='sd_images must be fed'):
            session.run([model['step'], model['loss']])
    lr_src, hr_t = graph.placeholder(name='lr'), graph.placeholder(name='hr')
    em = model_espcn.build_model(lr_src, 3, hr_t, device='cpu', seed=0)
    with graph.Session() as session:
        assert session.run(em['step']) == 0
        with pytest.raises(ValueError, match='lr_source must be fed'):
            session.run(em['sr_result'])


def test_tf_checkpoint_names_state_file_and_beta_powers(tmp_path):
    from ml_super_resolution_amd import tf_bundle
    from ml_super_resolution_amd.engine import ConvStack
    from ml_super_resolution_amd.vdsr import model_vdsr
    stack = ConvStack(model_vdsr.layer_specs(3), device='cpu', residual=True, weight_decay=1e-4)
    g = torch.Generator().manual_seed(0)
    stack.params.copy_(torch.randn(stack.flat_size, generator=g))
    stack.opt_m = torch.randn(stack.flat_size, generator=g)
    stack.opt_v = torch.rand(stack.flat_size, generator=g)
    stack.global_step = 7
    d = tmp_path / 'ckpt'
    d.mkdir()
    assert tf_bundle.latest_checkpoint(str(d)) is None
    stack.save_tf_checkpoint(str(d / 'model.ckpt-7'), extra={'learning_rate': np.float32(0.1)})
    vals = tf_bundle.load_checkpoint(str(d / 'model.ckpt-7'))
    # every global variable of the reference's graph: 3 x (kernel, bias) x (value, Adam, Adam_1) + beta powers +
    # global_step + learning_rate (vdsr/vdsr/model_vdsr.py:136-147)
    assert len(vals) == 3 * 2 * 3 + 4
    for key in ('conv2d/kernel', 'conv2d_1/bias', 'conv2d_2/kernel/Adam', 'conv2d_2/bias/Adam_1', 'learning_rate'):
        assert key in vals
    # TF's AdamOptimizer starts the powers at beta and multiplies once per step: beta ** (N + 1)
    np.testing.assert_allclose(vals['beta1_power'], 0.9 ** 8, rtol=1e-6)
    np.testing.assert_allclose(vals['beta2_power'], 0.999 ** 8, rtol=1e-6)
    assert vals['global_step'].dtype == np.int64 and int(vals['global_step']) == 7
    # the `checkpoint` state file (what tf.train.latest_checkpoint reads, experiment_train.py:108)
    text = open(str(d / 'checkpoint')).read()
    assert text == 'model_checkpoint_path: "model.ckpt-7"\nall_model_checkpoint_paths: "model.ckpt-7"\n'
    stack.global_step = 9
    stack.save_tf_checkpoint(str(d / 'model.ckpt-9'))
    text = open(str(d / 'checkpoint')).read().splitlines()
    assert text[0] == 'model_checkpoint_path: "model.ckpt-9"'
    assert text[1:] == ['all_model_checkpoint_paths: "model.ckpt-7"', 'all_model_checkpoint_paths: "model.ckpt-9"']
    assert tf_bundle.latest_checkpoint(str(d)) == str(d / 'model.ckpt-9')
    # restore: weights, slots, step
    other = ConvStack(model_vdsr.layer_specs(3), device='cpu', residual=True, weight_decay=1e-4)
    other.load_tf_checkpoint(str(d / 'model.ckpt-7'))
    assert other.global_step == 7
    for i in range(3):          # (the flat buffers' alignment padding is not part of any variable)
        for buf_a, buf_b in ((None, None), (other.opt_m, stack.opt_m), (other.opt_v, stack.opt_v)):
            assert torch.equal(other.kernel(i, buf_a), stack.kernel(i, buf_b))
            assert torch.equal(other.bias(i, buf_a), stack.bias(i, buf_b))


def test_use_adam_flag_forms():
    """tf.app.flags booleans: bare `--use_adam` (vdsr/makefile:26), `--use_adam=false`, `--use_adam false`."""
    from ml_super_resolution_amd.vdsr.experiment_train import parse_flags
    assert parse_flags([]).use_adam is True
    assert parse_flags(['--use_adam']).use_adam is True
    assert parse_flags(['--use_adam', '--batch_size', '8']).batch_size == 8
    assert parse_flags(['--use_adam=false']).use_adam is False
    assert parse_flags(['--use_adam', 'False']).use_adam is False


def test_forward_buffers_do_not_pile_up_per_image_size():
    """keep=False temporaries are keyed by (parity, channels): a new image size replaces the old buffers."""
    from ml_super_resolution_amd.engine import ConvStack
    from ml_super_resolution_amd.vdsr import model_vdsr
    stack = ConvStack(model_vdsr.layer_specs(6), device='cpu', residual=True)
    shapes = stack._shapes((1, 30, 20, 3))
    for i, s in enumerate(stack.specs):
        stack._buf(('tmp', i & 1, s.cout), shapes[i])
    n = len(stack._bufs)
    for hw in ((31, 21), (50, 60), (8, 8)):
        shapes = stack._shapes((1,) + hw + (3,))
        for i, s in enumerate(stack.specs):
            stack._buf(('tmp', i & 1, s.cout), shapes[i])
    assert len(stack._bufs) == n == 3


def test_blocked_kernel_layout_and_enet_variable_names():
    """Channel-blocked filters <-> TensorFlow's HWIO, and the variable names / checkpoint keys of the EnhanceNet
    training graph (enet/enet/model_enet.py:118-162, 331-343) -- host logic, no kernels."""
    from ml_super_resolution_amd.blocked import BlockedConv, ParamPool
    from ml_super_resolution_amd.enet import model_enet
    rng = np.random.default_rng(0)
    for cin, cout in ((3, 32), (64, 128), (256, 192), (32, 64)):
        shape = BlockedConv.kernel_shape(cin, cout)
        layer = BlockedConv(cin, cout, 1, 'relu', torch.empty(shape), torch.empty(cout))
        k = rng.normal(size=(3, 3, cin, cout)).astype(np.float32)
        layer.set_kernel_hwio(k, np.arange(cout, dtype=np.float32))
        np.testing.assert_array_equal(layer.kernel_hwio().numpy(), k)
        # block [ib][ob] is the HWIO sub-filter of input channels 64 ib.. and output channels 64 ob..
        ib, ob = shape[0] - 1, shape[1] - 1
        np.testing.assert_array_equal(layer.w[ib, ob].numpy(), k[:, :, 64 * ib:64 * ib + shape[4], 64 * ob:64 * ob + shape[5]])
    pool = ParamPool([('k', (3, 3, 3, 32)), ('b', (32,)), ('c', (5,))], 'cpu')
    assert pool.params.numel() == 864 + 32 + 8 and pool.view(2).shape == (5,)
    assert pool.view(1).data_ptr() % 16 == 0 and pool.view(2).data_ptr() % 16 == 0
    D = model_enet.Discriminator(device='cpu', seed=0, width=32, image_size=128, dense_units=1024)
    v = D.variables()
    assert list(v)[:4] == ['d_/conv2d/kernel', 'd_/conv2d/bias', 'd_/conv2d_1/kernel', 'd_/conv2d_1/bias']
    assert tuple(v['d_/conv2d/kernel'].shape) == (3, 3, 3, 32) and tuple(v['d_/conv2d_9/kernel'].shape) == (3, 3, 512, 512)
    assert tuple(v['d_/dense/kernel'].shape) == (8192, 1024) and tuple(v['d_/dense_1/kernel'].shape) == (1024, 1)
    assert [s for _, _, s in model_enet.discriminator_layers()] == [1, 2] * 5
    assert [c for _, c, _ in model_enet.discriminator_layers()] == [32, 32, 64, 64, 128, 128, 256, 256, 512, 512]
    # truncated_normal(0.02): nothing beyond two sigma
    assert float(v['d_/conv2d_9/kernel'].abs().max()) <= 0.04 + 1e-6


def _small_enet(seed=0):
    from ml_super_resolution_amd.enet import model_enet, model_vgg
    return model_enet.EnetModel('pat', model_vgg.random_vgg_weights(0, width=4), device='cpu', seed=seed, d_width=4,
                                image_size=32, dense_units=8)


def _give_adam_state(pool, t, gen):
    pool.t, pool.opt_m, pool.opt_v = t, torch.randn(pool.params.shape, generator=gen), torch.rand(pool.params.shape, generator=gen)


def _same_pool_variables(a, b):
    """Parameters and both Adam slots, variable by variable (the flat buffers' alignment padding belongs to no variable)."""
    return all(torch.equal(a.view(j, x), b.view(j, y)) for j in range(len(a.entries))
               for x, y in ((None, None), (a.opt_m, b.opt_m), (a.opt_v, b.opt_v)))


@pytest.mark.parametrize('g_steps', [999, 5000, 100000])
def test_enet_resume_step_counts_survive_beta_power_underflow(tmp_path, g_steps):
    """enet/enet/experiment_train.py:99-160 saves at step % 1000 == 999; float32 0.9 ** 1000 is 0.0 (TensorFlow would
    store the same), so the Adam step counts must not be recovered by inverting beta1_power."""
    from ml_super_resolution_amd import tf_bundle
    m = _small_enet()
    G, P = m.generator.pool, m.discriminator.pool
    gen = torch.Generator().manual_seed(1)
    m.global_step = g_steps
    _give_adam_state(G, g_steps, gen)
    _give_adam_state(P, (g_steps + 2) // 3 + 5, gen)      # (not what the schedule would give: must come back as stored)
    tensors = m.tf_checkpoint_tensors()
    if g_steps >= 999:
        assert float(tensors['beta1_power']) == 0.0       # the value that used to raise OverflowError on resume
    prefix = str(tmp_path / ('model.ckpt-%d' % g_steps))
    m.save_tf_checkpoint(prefix)
    other = _small_enet(seed=5)
    other.load_tf_checkpoint(prefix)
    assert other.global_step == g_steps and other.generator.pool.t == g_steps and other.discriminator.pool.t == P.t
    assert _same_pool_variables(G, other.generator.pool) and _same_pool_variables(P, other.discriminator.pool)
    # a TensorFlow-written file has no explicit count: beta2_power_1 while it is a normal float, the schedule after that
    del tensors['srx/d_trainer_steps']
    prefix2 = str(tmp_path / 'foreign.ckpt')
    tf_bundle.save_checkpoint(prefix2, tensors)
    third = _small_enet(seed=6)
    third.load_tf_checkpoint(prefix2)
    assert third.generator.pool.t == g_steps
    # (P.t is 5 off the schedule: beta2_power_1 contradicts it and wins while it is a normal float32)
    if 0.999 ** (P.t + 1) > 1.2e-38:
        assert third.discriminator.pool.t == P.t
    else:
        assert third.discriminator.pool.t == (g_steps + 2) // 3


def test_enet_d_steps_guards():
    from ml_super_resolution_amd.enet.model_enet import EnetModel
    f = EnetModel._d_steps_from_checkpoint

    def tf_accumulator(t):
        # what TensorFlow holds after t applies: created as float32(0.999), multiplied by float32(0.999) t times, in float32
        b, p = np.float32(0.999), np.float32(0.999)
        for _ in range(t):
            p = np.float32(p * b)
        return p
    for t in (0, 1, 333, 1667, 20000, 80000):
        # a schedule that does not fit (it would give t + 10): the accumulator decides, and float32's base is the one inverted
        assert f({'beta2_power_1': tf_accumulator(t)}, 3 * (t + 10) - 2) == t
    # a checkpoint the reference wrote: d_trainer ran on steps 0, 3, 6, ... -> the schedule's count, exactly, whatever the
    # accumulator's float32 drift (round-3 advisor: log(0.999) instead of log(float32(0.999)) is off by one from ~40k steps)
    for g in (999, 29999, 119999, 299999):
        t = (g + 2) // 3
        assert f({'beta2_power_1': np.float32(0.999 ** (t + 1))}, g) == t
        assert f({'beta2_power_1': np.float32(float(np.float32(0.999)) ** (t + 1))}, g) == t
    for bad in (np.float32(0.0), np.float32(1e-42), np.float32('nan'), np.float32(1.0)):
        assert f({'beta2_power_1': bad, 'beta1_power_1': np.float32(0.0)}, 2999) == 1000
    assert f({}, 10) == 4
    assert f({'srx/d_trainer_steps': np.int64(77), 'beta2_power_1': np.float32(0.5)}, 10) == 77


def test_load_vgg_weights_reads_the_keras_named_npz(tmp_path):
    """enet/enet/model_vgg.py:39-62: the .npz holds `<layer>_W_1:0` / `<layer>_b_1:0`; scope = first 12 characters,
    constant name = the name without ':0'.  The path a user with the real file takes: npz -> load_vgg_weights -> Vgg19."""
    from ml_super_resolution_amd.enet import model_vgg
    w = model_vgg.random_vgg_weights(3, width=8)
    arrays = {}
    for layer, d in w.items():
        for const, a in d.items():
            arrays[const + ':0'] = a
    path = str(tmp_path / 'vgg19_weights_tf_dim_ordering_tf_kernels_notop.npz')
    np.savez(path, **arrays)
    got = model_vgg.load_vgg_weights(path)
    assert sorted(got) == sorted(n for n in model_vgg.LAYER_NAMES if 'conv' in n) and len(got) == 16
    assert sorted(got['block3_conv4']) == ['block3_conv4_W_1', 'block3_conv4_b_1']
    net = model_vgg.Vgg19(got, device='cpu')
    for layer in w:
        np.testing.assert_array_equal(net.layers[layer].kernel_hwio().numpy(), w[layer][layer + '_W_1'])
        np.testing.assert_array_equal(net.layers[layer].b.numpy(), w[layer][layer + '_b_1'])
    assert model_vgg.load_vgg_weights(str(tmp_path / 'missing.npz')) == {}          # :45-46
    from ml_super_resolution_amd import graph
    from ml_super_resolution_amd.enet import model_enet
    with pytest.raises(ValueError, match='VGG-19 weights not found'):
        model_enet.build_enet(graph.placeholder(name='sd'), graph.placeholder(name='bq'), graph.placeholder(name='hd'),
                              'pat', str(tmp_path / 'missing.npz'), device='cpu')


# ---- the slab oracle and the derived bound of the frame-sized GPU tests, proven without a GPU ------------------------------
@pytest.mark.parametrize('padding', ['SAME', 'VALID'])
@pytest.mark.parametrize('k', [3, 5, 9])
def test_oracle_slabs_equal_the_rows_of_the_whole_image_oracle(k, padding):
    """tests/test_gpu_full_frame.oracle_rows / oracle_rows_bwd_data: bands at row 0, at the last row and in the interior (one
    of a single row, one crossing where SAME padding ends) give EXACTLY the rows of the whole-image oracle -- forward with
    bias, activation and skip operand, and the data gradient."""
    from oracle import oracle as O
    from tests.test_gpu_full_frame import bands, oracle_rows, oracle_rows_bwd_data
    rng = np.random.default_rng(100 * k + len(padding))
    n, h, w, cin, cout = 2, 29, 21, 3, 5
    x = rng.uniform(-1, 1, (n, h, w, cin)).astype(np.float32)
    wt = rng.normal(0, 0.2, (k, k, cin, cout)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, (cout,)).astype(np.float32)
    _, _, oh, ow = O.conv_geometry(h, w, k, k, padding)
    skip = rng.uniform(-1, 1, (n, oh, ow, cout)).astype(np.float32)
    cuts = [(0, 1), (0, 6), (2, 9), (7, 8), (oh // 2, oh // 2 + 5), (oh - 7, oh), (oh - 1, oh), (0, oh)]
    for act, sk in ((None, None), ('relu', None), ('tanh', None), (None, skip)):
        whole = O.c_conv2d_fwd(x, wt, b, padding, act, skip=sk)
        for r0, r1 in cuts:
            got = oracle_rows(x, wt, b, padding, act, r0, r1, skip=sk)
            assert got.shape == (n, r1 - r0, ow, cout)
            assert np.array_equal(got, whole[:, r0:r1]), (act, r0, r1)
        # the float64 NumPy oracle on the same slabs (the reference of the derived bound): the same sums; BLAS may block a
        # slab's products differently from the whole image's, so to float64 rounding
        whole64 = O.conv2d_fwd(x, wt, b, padding, act, skip=sk)
        for r0, r1 in cuts:
            got = oracle_rows(x, wt, b, padding, act, r0, r1, skip=sk, oracle=O.conv2d_fwd)
            assert got.dtype == np.float64 and np.abs(got - whole64[:, r0:r1]).max() <= 1e-13
    dpre = rng.normal(0, 1, (n, oh, ow, cout)).astype(np.float32)
    whole = O.c_conv2d_bwd_data(dpre, wt, (h, w), padding)
    for r0, r1 in [(0, 1), (0, 6), (2, 9), (11, 12), (h // 2, h // 2 + 5), (h - 7, h), (h - 1, h), (0, h)]:
        got = oracle_rows_bwd_data(dpre, wt, (h, w), padding, r0, r1)
        assert got.shape == (n, r1 - r0, w, cin)
        assert np.array_equal(got, whole[:, r0:r1]), (r0, r1)
        got = oracle_rows_bwd_data(dpre, wt, (h, w), padding, r0, r1, oracle=O.conv2d_bwd_data)
        assert np.abs(got - O.conv2d_bwd_data(dpre, wt, (h, w), padding)[:, r0:r1]).max() <= 1e-13
    assert bands([0, 1, 2, 7, 9, 10]) == [(0, 3), (7, 8), (9, 11)]


def test_frame_row_sample_covers_edges_a_seam_band_and_a_tenth_of_the_rows():
    from tests.test_gpu_full_frame import MIN_SHARE, bands, sample_rows
    for oh in (720, 712, 708):
        rows = sample_rows(oh)
        assert set(range(16)) <= set(rows) and set(range(oh - 16, oh)) <= set(rows) and set(range(0, oh, 31)) <= set(rows)
        band = [b for b in bands(rows) if b[1] - b[0] >= 48 and b[0] > 16 and b[1] < oh - 16]
        assert len(band) == 1 and band[0][0] % 16 != 0
        # at least two seams of 16-row tiles strictly inside the band, whatever row the tiling starts at
        assert band[0][1] - band[0][0] >= 2 * 16 + 15
        assert len(rows) >= MIN_SHARE * oh


@pytest.mark.parametrize('k,cin', [(3, 3), (3, 64), (5, 32)], ids=['K27', 'K576', 'K800'])
def test_derived_bound_admits_sequential_fp32_and_catches_one_dropped_median_tap(k, cin):
    """tests/test_gpu_ops.close_elementwise is neither wrong nor vacuous: a plain float32 convolution that adds its K products
    one after the other (the longest rounding chain any order has) stays inside it; the same result with ONE tap of ONE output
    element left out -- the tap whose |x * w| is the median of that element's products -- falls outside it."""
    from tests.test_gpu_ops import close_elementwise
    rng = np.random.default_rng(k * 1000 + cin)
    n, h, w, cout = 1, 7, 8, 4
    K = k * k * cin
    assert K in (27, 576, 800)
    x = rng.uniform(-1, 1, (n, h, w, cin)).astype(np.float32)
    wt = rng.normal(0, 1.0 / np.sqrt(K), (k, k, cin, cout)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, (cout,)).astype(np.float32)
    p = (k - 1) // 2
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    patches = np.stack([xp[:, i:i + h, j:j + w, :] for i in range(k) for j in range(k)], axis=3).reshape(n * h * w, K)
    wm = wt.reshape(K, cout)

    def sequential(rows, cols, skip_tap=None):
        acc = np.broadcast_to(b[cols], (len(rows), len(cols))).astype(np.float32)
        for t in range(K):
            if t != skip_tap:
                acc = (acc + patches[rows, t:t + 1] * wm[t:t + 1, cols]).astype(np.float32)
        return acc
    y = sequential(np.arange(n * h * w), np.arange(cout)).reshape(n, h, w, cout)
    assert y.dtype == np.float32
    for act in (None, 'relu'):
        ya = np.maximum(y, 0) if act else y
        worst = close_elementwise(ya, x, wt, b, 'SAME', act)
        assert 0.0 < worst <= 1.0
    # one interior output element (all K taps real) without its median tap
    pix, co = (h // 2) * w + w // 2, 1
    prod = np.abs(patches[pix].astype(np.float64) * wm[:, co])
    tap = int(np.argsort(prod)[K // 2])
    bad = y.copy()
    bad.reshape(n * h * w, cout)[pix, co] = sequential(np.array([pix]), np.array([co]), skip_tap=tap)[0, 0]
    assert np.count_nonzero(bad != y) == 1
    with pytest.raises(AssertionError, match='derived bound'):
        close_elementwise(bad, x, wt, b, 'SAME', None)


# ---- restoring a checkpoint into a stack that has trained: in place -------------------------------------------------------------
def _stack_with_slots(seed, adam=True):
    from ml_super_resolution_amd.engine import ConvStack
    from ml_super_resolution_amd.vdsr import model_vdsr
    stack = ConvStack(model_vdsr.layer_specs(3), device='cpu', residual=True, weight_decay=1e-4)
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        stack.params.copy_(torch.randn(stack.flat_size, generator=g))
        stack.opt_m = torch.randn(stack.flat_size, generator=g)
        stack.opt_v = torch.rand(stack.flat_size, generator=g) if adam else None
        stack.global_step = 10 + seed
    return stack


def _variable_views(stack, buf):
    return [v(i, buf) for i in range(len(stack.specs)) for v in (stack.kernel, stack.bias)]


def _same_variables(stack, buf, want):
    return all(torch.equal(a, b) for a, b in zip(_variable_views(stack, buf), _variable_views(stack, want)))


@pytest.mark.parametrize('fmt', ['state_dict', 'tf_checkpoint'])
def test_restore_into_a_trained_stack_keeps_the_buffers_a_captured_step_points_at(tmp_path, fmt):
    """ConvStack.train_step_replay captures the ADDRESSES of params / grads / opt_m / opt_v.  A restore therefore writes into
    the buffers that exist: same data_ptr() before and after, the checkpoint's values inside, and the captured steps stay.
    Slots that are still None are allocated (no captured step can hold them yet).  with_optimizer=False and a checkpoint
    without slots leave the existing slots alone.  A Momentum checkpoint over Adam slots: opt_m restored in place, opt_v
    dropped, every captured step with it."""
    src = _stack_with_slots(1)
    want = {k: getattr(src, k).clone() for k in ('params', 'opt_m', 'opt_v')}
    prefix = str(tmp_path / 'model.ckpt-11')

    def save(stack, name=prefix):
        if fmt == 'state_dict':
            return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in stack.state_dict().items()}
        stack.save_tf_checkpoint(name)
        return name

    def load(stack, ckpt, **kw):
        if fmt == 'state_dict':
            assert not kw
            stack.load_state_dict(ckpt)
        else:
            stack.load_tf_checkpoint(ckpt, **kw)
    ckpt = save(src)
    # (1) into a stack that holds slots of its own and a captured step
    dst = _stack_with_slots(2)
    ptrs = {k: getattr(dst, k).data_ptr() for k in ('params', 'grads', 'opt_m', 'opt_v')}
    dst._step_graphs['key'] = marker = {'graph': object()}
    load(dst, ckpt)
    assert {k: getattr(dst, k).data_ptr() for k in ptrs} == ptrs
    assert dst.global_step == 11
    for k in want:
        assert _same_variables(dst, getattr(dst, k), want[k]), k
    assert dst._step_graphs.get('key') is marker
    # ... and into the stack that wrote it, after it has moved on (train - evaluate - reload)
    ptrs_src = {k: getattr(src, k).data_ptr() for k in ('params', 'opt_m', 'opt_v')}
    src.params.mul_(2.0); src.opt_m.add_(1.0); src.opt_v.mul_(0.5); src.global_step += 3
    load(src, ckpt)
    assert {k: getattr(src, k).data_ptr() for k in ptrs_src} == ptrs_src and src.global_step == 11
    for k in want:
        assert _same_variables(src, getattr(src, k), want[k]), k       # (the flat buffers' alignment padding is no variable)
    # (2) slots still None: allocated, filled, and stable from then on
    fresh = _stack_with_slots(None)
    assert fresh.opt_m is None and fresh.opt_v is None
    load(fresh, ckpt)
    for k in want:
        assert _same_variables(fresh, getattr(fresh, k), want[k]), k
    ptrs_fresh = (fresh.opt_m.data_ptr(), fresh.opt_v.data_ptr())
    load(fresh, ckpt)
    assert (fresh.opt_m.data_ptr(), fresh.opt_v.data_ptr()) == ptrs_fresh
    # (3) a checkpoint without slots (and with_optimizer=False): the existing slots stay, untouched and at their address
    bare = save(_stack_with_slots(None), str(tmp_path / 'bare.ckpt-0'))
    for ck, kw in ((bare, {}),) + (((ckpt, {'with_optimizer': False}),) if fmt == 'tf_checkpoint' else ()):
        dst = _stack_with_slots(3)
        m0, v0 = dst.opt_m.clone(), dst.opt_v.clone()
        ptrs = (dst.opt_m.data_ptr(), dst.opt_v.data_ptr())
        dst._step_graphs['key'] = marker
        load(dst, ck, **kw)
        assert (dst.opt_m.data_ptr(), dst.opt_v.data_ptr()) == ptrs
        assert torch.equal(dst.opt_m, m0) and torch.equal(dst.opt_v, v0) and dst._step_graphs.get('key') is marker
    # (4) a Momentum checkpoint into a stack that holds Adam slots
    mom = _stack_with_slots(4, adam=False)
    mom_ckpt = save(mom, str(tmp_path / 'momentum.ckpt-14'))
    dst = _stack_with_slots(5)
    ptr_m = dst.opt_m.data_ptr()
    dst._step_graphs['key'] = marker
    load(dst, mom_ckpt)
    assert dst.opt_m.data_ptr() == ptr_m and _same_variables(dst, dst.opt_m, mom.opt_m)
    assert dst.opt_v is None and not dst._step_graphs
    # ... and into one that holds a Momentum accumulator already: in place, the captured steps stay
    dst = _stack_with_slots(6, adam=False)
    ptr_m = dst.opt_m.data_ptr()
    dst._step_graphs['key'] = marker
    load(dst, mom_ckpt)
    assert dst.opt_m.data_ptr() == ptr_m and _same_variables(dst, dst.opt_m, mom.opt_m) and dst.opt_v is None
    assert dst._step_graphs.get('key') is marker


def test_enet_restore_keeps_parameter_and_slot_buffers(tmp_path):
    """EnetModel.load_tf_checkpoint (no captured steps today, the same rule all the same): generator and discriminator
    parameters and both optimizers' slots are restored into the buffers that exist."""
    m = _small_enet()
    G, P = m.generator.pool, m.discriminator.pool
    gen = torch.Generator().manual_seed(3)
    m.global_step = 12
    _give_adam_state(G, 12, gen)
    _give_adam_state(P, 4, gen)
    prefix = str(tmp_path / 'model.ckpt-12')
    m.save_tf_checkpoint(prefix)
    other = _small_enet(seed=5)
    G2, P2 = other.generator.pool, other.discriminator.pool
    G2.t, G2.opt_m, G2.opt_v = 1, torch.zeros_like(G2.params), torch.ones_like(G2.params)
    P2.t, P2.opt_m, P2.opt_v = 1, torch.zeros_like(P2.params), torch.ones_like(P2.params)
    bufs = lambda: (other.generator.params, G2.params, G2.opt_m, G2.opt_v, P2.params, P2.opt_m, P2.opt_v)
    ptrs = [t.data_ptr() for t in bufs()]
    other.load_tf_checkpoint(prefix)
    assert [t.data_ptr() for t in bufs()] == ptrs
    assert other.global_step == 12 and G2.t == 12 and P2.t == 4
    assert _same_pool_variables(G, G2) and _same_pool_variables(P, P2)
