"""make_param_pool_golden.py -- writes tests/golden/param_layout.json and tests/golden/checkpoint_keys.json.

param_layout.json:    per network, the flat size and [variable name, float offset, shape in memory] of every variable of
                      its flat parameter buffer.  `ConvStack.state_dict()` stores that buffer whole, so the layout is a
                      file format.
checkpoint_keys.json: per case, the sorted [key, dtype, shape] of tf_checkpoint_tensors().

Both were recorded before the three hand-written layouts became param_pool.ParamPool and must not change:
tests/test_param_pool_host.py compares them exactly.  Run from the repository root: python tests/golden/make_param_pool_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def networks():
    """{name: ParamPool} of the layouts on record (host tensors; the discriminator at the reference's 32 / 128 / 1024)."""
    from ml_super_resolution_amd.enet import model_enet
    from ml_super_resolution_amd.espcn import model_espcn
    from ml_super_resolution_amd.srcnn import srcnn
    from ml_super_resolution_amd.vdsr import model_vdsr
    return {'vdsr20': model_vdsr.VdsrModel(num_layers=20, device='cpu', seed=0).stack,
            'espcn3': model_espcn.EspcnModel(scaling_factor=3, device='cpu', seed=0).stack,
            'srcnn915': srcnn.SrcnnModel(device='cpu', seed=0).stack,
            'enet_generator': model_enet.EnetGenerator(device='cpu', seed=0).pool,
            'enet_discriminator': model_enet.Discriminator(device='cpu', seed=0, width=32, image_size=128, dense_units=1024).pool}


def layout(pool):
    return {'flat_size': int(pool.params.numel()), 'variables': [[name, off, list(shape)] for name, off, shape in pool.layout()]}


def give_slots(pool, two=True):
    pool.opt_m = torch.zeros_like(pool.params)
    pool.opt_v = torch.zeros_like(pool.params) if two else None


def small_enet(seed=0):
    from ml_super_resolution_amd.enet import model_enet, model_vgg
    return model_enet.EnetModel('pat', model_vgg.random_vgg_weights(0, width=4), device='cpu', seed=seed, d_width=4,
                                image_size=32, dense_units=8)


def checkpoint_cases():
    """{case: {checkpoint key: ndarray}}."""
    from ml_super_resolution_amd.espcn import model_espcn
    from ml_super_resolution_amd.srcnn import srcnn
    from ml_super_resolution_amd.vdsr import model_vdsr
    out = {}
    for case, two in (('vdsr6_adam', True), ('vdsr6_momentum', False)):
        stack = model_vdsr.VdsrModel(num_layers=6, use_adam=two, device='cpu', seed=0).stack
        give_slots(stack, two)
        out[case] = stack.tf_checkpoint_tensors(extra={'learning_rate': np.float32(0.1)})
    stack = model_espcn.EspcnModel(scaling_factor=3, device='cpu', seed=0).stack
    give_slots(stack)
    out['espcn3'] = stack.tf_checkpoint_tensors()
    stack = srcnn.SrcnnModel(device='cpu', seed=0).stack
    give_slots(stack)
    out['srcnn915'] = stack.tf_checkpoint_tensors(adam_betas=(0.5, 0.9))
    out['enet_small_without_optimizer_state'] = small_enet().tf_checkpoint_tensors()
    m = small_enet()
    give_slots(m.generator.pool)
    give_slots(m.discriminator.pool)
    out['enet_small_with_optimizer_state'] = m.tf_checkpoint_tensors()
    return out


def key_list(tensors):
    return sorted([k, str(np.asarray(v).dtype), list(np.asarray(v).shape)] for k, v in tensors.items())


def write(path, obj):
    """One variable / key per line."""
    text = json.dumps(obj, sort_keys=True).replace('[[', '[\n  [').replace(']], ', ']],\n ').replace('], ["', '],\n  ["')
    with open(path, 'w') as f:
        f.write(text.replace(']}, ', ']},\n ') + '\n')


if __name__ == '__main__':
    write(os.path.join(HERE, 'param_layout.json'), {k: layout(p) for k, p in networks().items()})
    write(os.path.join(HERE, 'checkpoint_keys.json'), {k: key_list(t) for k, t in checkpoint_cases().items()})
