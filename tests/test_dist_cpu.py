"""Data-parallel host logic on CPU: two gloo ranks, each with half of the batch; the averaged flat
gradient must equal the single-process gradient of the whole batch, and replicas must
start identical.  The per-shard gradients come from the oracle here -- the GPU kernels are covered
by the -m gpu tests; this test covers dist.py (shard / broadcast / all-reduce(mean) / hook)."""
import os
import socket

import numpy as np
import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _init_gloo(rank, world, port):
    """Two gloo ranks whose collectives give up after a minute: ranks that disagree on them fail the test, they do not
    hang it."""
    import datetime
    import sys
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from ml_super_resolution_amd import dist as srx_dist
    torch.distributed.init_process_group(backend='gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    assert srx_dist.init_process_group(rank, world, backend='gloo') == 'gloo'
    return srx_dist


def _worker(rank, world, port, out_dir):
    srx_dist = _init_gloo(rank, world, port)
    from ml_super_resolution_amd.param_pool import ParamPool
    from oracle import oracle as O
    from tests.golden.make_golden import vdsr_params
    params = vdsr_params(300, num_layers=4)
    arrays = [a for kb in params for a in kb]
    stack = ParamPool([('v%d' % j, a.shape) for j, a in enumerate(arrays)], 'cpu')
    # rank 1 starts from garbage: attach() must broadcast rank 0's parameters
    if rank == 0:
        for j, a in enumerate(arrays):
            stack.view(j).copy_(torch.from_numpy(a))
    srx_dist.attach(stack, world)
    for j, a in enumerate(arrays):
        assert np.array_equal(stack.view(j).numpy(), a)
    assert stack.t == 0 and stack.opt_m is None and stack.opt_v is None

    rng = np.random.default_rng(7)
    hd = rng.uniform(-1, 1, (4, 9, 9, 3)).astype(np.float32)
    sd = rng.uniform(-1, 1, (4, 9, 9, 3)).astype(np.float32)
    my_sd = srx_dist.shard(torch.from_numpy(sd), rank, world).numpy()
    my_hd = srx_dist.shard(torch.from_numpy(hd), rank, world).numpy()
    assert my_sd.shape[0] == 2
    _, grads, _ = O.vdsr_loss_and_grads(my_sd, my_hd, params)         # local mean loss + L2 term
    # (the oracle's float64 gradient, not the pool's fp32 buffer: the exchange itself is what is compared to 1e-9)
    g = torch.from_numpy(np.concatenate([np.concatenate([dk.ravel(), db.ravel()]) for dk, db in grads]))
    stack.grad_hook(g)                                                   # the DP exchange: ONE all-reduce
    np.save(os.path.join(out_dir, 'g%d.npy' % rank), g.numpy())
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_gradient_equals_single_process(tmp_path):
    from oracle import oracle as O
    from tests.golden.make_golden import vdsr_params
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    g0 = np.load(tmp_path / 'g0.npy')
    g1 = np.load(tmp_path / 'g1.npy')
    np.testing.assert_array_equal(g0, g1)                                # every rank holds the same averaged gradient
    params = vdsr_params(300, num_layers=4)
    rng = np.random.default_rng(7)
    hd = rng.uniform(-1, 1, (4, 9, 9, 3)).astype(np.float32)
    sd = rng.uniform(-1, 1, (4, 9, 9, 3)).astype(np.float32)
    _, grads, _ = O.vdsr_loss_and_grads(sd, hd, params)                  # single process, whole batch
    ref = np.concatenate([np.concatenate([dk.ravel(), db.ravel()]) for dk, db in grads])
    np.testing.assert_allclose(g0, ref, rtol=1e-9, atol=1e-12)


def test_shard_rejects_ragged_batches():
    import pytest
    from ml_super_resolution_amd import dist as srx_dist
    with pytest.raises(ValueError):
        srx_dist.shard(torch.zeros(5, 2), 0, 2)


def _flat_worker(rank, world, port, out_dir):
    """dist.attach_flat on the real EnetModel object (host tensors, no kernels): rank 0 resumed from a checkpoint
    (step 6, slots), rank 1 did not (step 5, other weights, no slots) -- or the other way round for `case` 1."""
    srx_dist = _init_gloo(rank, world, port)
    from ml_super_resolution_amd.enet import model_enet, model_vgg
    for case in (0, 1):
        m = model_enet.EnetModel('pat', model_vgg.random_vgg_weights(0, width=4), device='cpu', seed=10 * rank + case,
                                 d_width=4, image_size=32, dense_units=8)
        G, P = m.generator.pool, m.discriminator.pool
        has_state = (rank == 0) == (case == 0)
        if has_state:
            gen = torch.Generator().manual_seed(5 + rank)
            m.global_step = 6 + rank
            G.t, G.opt_m, G.opt_v = 6 + rank, torch.randn(G.params.shape, generator=gen), torch.rand(G.params.shape, generator=gen)
            P.t, P.opt_m, P.opt_v = 2 + rank, torch.randn(P.params.shape, generator=gen), torch.rand(P.params.shape, generator=gen)
        else:
            m.global_step = 5
        srx_dist.attach_flat(m, world)
        assert m.generator.params is G.params
        out = {'g': G.params.numpy(), 'd': P.params.numpy(), 'step': np.int64(m.global_step), 'has_g': np.int64(G.opt_m is not None),
               'has_d': np.int64(P.opt_m is not None), 'd_t': np.int64(P.t), 'g_t': np.int64(G.t)}
        assert (G.opt_m is None) == (G.opt_v is None) and (P.opt_m is None) == (P.opt_v is None)
        if G.opt_m is not None:
            out.update(g_m=G.opt_m.numpy(), g_v=G.opt_v.numpy(), d_m=P.opt_m.numpy(), d_v=P.opt_v.numpy())
        # the hooks average over the ranks
        g = torch.full((8,), float(rank + 1))
        m.grad_hook_g(g)
        m.grad_hook_d(g)
        out['hooked'] = g.numpy()
        np.savez(os.path.join(out_dir, 'flat%d_%d.npz' % (case, rank)), **out)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_attach_flat_levels_step_counts_and_adam_slots(tmp_path):
    """ADVICE r2 (dist.py:115): EnhanceNet's `global_step` decides which steps run d_trainer
    (enet/enet/experiment_train.py:112); ranks that disagree issue different collectives.  Everything comes from rank 0 --
    also when rank 0 is the one WITHOUT optimizer state (the other rank's slots are dropped)."""
    port = _free_port()
    mp.spawn(_flat_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = np.load(tmp_path / 'flat0_0.npz'), np.load(tmp_path / 'flat0_1.npz')
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert (int(a['step']), int(a['g_t']), int(a['d_t']), int(a['has_g']), int(a['has_d'])) == (6, 6, 2, 1, 1)
    np.testing.assert_array_equal(a['hooked'], np.full(8, 1.5, np.float32))          # mean of 1 and 2, reduced twice: still 1.5
    a, b = np.load(tmp_path / 'flat1_0.npz'), np.load(tmp_path / 'flat1_1.npz')
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert (int(b['step']), int(b['has_g']), int(b['has_d']), int(b['d_t']), int(b['g_t'])) == (5, 0, 0, 0, 0)


def _level_worker(rank, world, port, out_dir):
    """ParamPool.level_from_rank0 from every mix of slots: (slots rank 0 holds, slots rank 1 holds)."""
    srx_dist = _init_gloo(rank, world, port)
    from ml_super_resolution_amd.param_pool import ParamPool
    out = {}
    for case, held in enumerate(((0, 2), (2, 0), (1, 2), (2, 1), (0, 0))):
        pool = ParamPool([('k', (3, 3, 3, 5)), ('b', (5,))], 'cpu')
        gen = torch.Generator().manual_seed(10 * case + rank)
        pool.params.copy_(torch.randn(pool.flat_size, generator=gen))
        pool.t = 7 + 10 * rank
        pool.opt_m = torch.randn(pool.flat_size, generator=gen) if held[rank] >= 1 else None
        pool.opt_v = torch.rand(pool.flat_size, generator=gen) if held[rank] == 2 else None
        mine = [None if b is None else b.data_ptr() for b in (pool.params, pool.opt_m, pool.opt_v)]
        pool.level_from_rank0()
        # what a rank already held is levelled in place (a captured step points at it)
        for b, ptr in zip((pool.params, pool.opt_m, pool.opt_v), mine):
            assert b is None or ptr is None or b.data_ptr() == ptr
        out.update({'params%d' % case: pool.params.numpy(), 't%d' % case: np.int64(pool.t),
                    'slots%d' % case: np.int64((pool.opt_m is not None) + (pool.opt_v is not None))})
        for name in ('opt_m', 'opt_v'):
            if getattr(pool, name) is not None:
                out['%s%d' % (name, case)] = getattr(pool, name).numpy()
    np.savez(os.path.join(out_dir, 'level%d.npz' % rank), **out)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_levelling_follows_rank_zero_whatever_each_rank_held(tmp_path):
    """Rank 0 WITHOUT slots and rank 1 WITH them ends with neither rank holding slots; one slot against two, and two
    against none, end as rank 0 was.  Whether rank 0's slots exist decides which broadcasts happen, so its head is
    broadcast before any slot: no rank waits for a collective the other never issues (the process group gives up after
    a minute instead of hanging)."""
    port = _free_port()
    mp.spawn(_level_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = np.load(tmp_path / 'level0.npz'), np.load(tmp_path / 'level1.npz')
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert [int(a['slots%d' % c]) for c in range(5)] == [0, 2, 1, 2, 0]
    assert all(int(a['t%d' % c]) == 7 for c in range(5))
    assert 'opt_m0' not in a.files and 'opt_v2' not in a.files and 'opt_v1' in a.files
