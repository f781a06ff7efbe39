"""What the GPU tests of ESPCN's byte and 4:2:0 routes share (tests/test_gpu_espcn_frames.py, tests/test_gpu_espcn_yuv.py):
the checkpoint their models are built from and output buffers with guard bytes around them.  Each file keeps its own cached
models (a model holds at most eight captured graphs: what one file captures does not evict what the other replays)."""
import torch

from tests.golden.make_golden import espcn_params

GUARD, FILL = 64, 0xA5


def variables(r, seed=None):
    ck = {}
    for name, (k, b) in zip(('f1', 'f2', 'f3'), espcn_params(103 + r if seed is None else seed, r)):
        ck[name + '/kernel:0'] = k
        ck[name + '/bias:0'] = b
    return ck


def guarded(n, offset=0):
    """A uint8 view of n bytes with at least GUARD bytes of FILL on either side, `offset` bytes off a 16-byte boundary."""
    base = torch.full((GUARD + 16 + n + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    assert base.data_ptr() % 16 == 0
    return base, base[GUARD + offset:GUARD + offset + n]
