#!/usr/bin/env python3
"""One 3x3 64 -> 64 layer at batch 256x41x41: forward, data gradient and filter gradient, 10 calls each at precision 0 and
precision 1 -- the program under rocprofv3 for the per-kernel statistics and the counters of the bf16x3 kernels."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_super_resolution_amd import ops  # noqa: E402

dev = torch.device('cuda')
x = torch.randn((256, 41, 41, 64), device=dev)
dpre = torch.randn_like(x)
w = torch.randn((3, 3, 64, 64), device=dev) * 0.06
b = torch.randn((64,), device=dev)
for p in ('highest', 'high'):
    ws = torch.empty((ops.bwd_filter_workspace_bytes(x.shape, w.shape, precision=p) + 3) // 4, device=dev)
    for _ in range(10):
        ops.conv2d_fwd(x, w, b, 'same', 'relu', precision=p)
        ops.conv2d_bwd_data(dpre, w, x.shape, 'same', x_in=x, in_act='relu', precision=p)
        ops.conv2d_bwd_filter(x, dpre, w.shape, 'same', workspace=ws, precision=p)
torch.cuda.synchronize()
print('done')
