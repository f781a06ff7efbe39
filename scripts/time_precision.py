#!/usr/bin/env python3
"""Precision 1 (bf16x3) against precision 0 (exact fp32) on the 3x3 64 -> 64 layer and the VDSR-20 train step.

Per shape and op: median device-event time of >= 20 timed calls after a warm-up, the two precisions alternated call by
call in one process; max and RMS deviation of precision 1 from precision 0 (relative to the exact output's max); and the
fraction of the fp32 MFMA peak (157.3 TF, counting the layer's FLOPs) and of the bf16 peak (2.5 PF, counting 3x the FLOPs:
three bf16 MFMAs per product) that precision 1 reaches.
  python scripts/time_precision.py [--calls 30]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_super_resolution_amd import ops  # noqa: E402
from ml_super_resolution_amd.vdsr import model_vdsr  # noqa: E402

FP32_PEAK, BF16_PEAK = 157.3e12, 2.5e15


def median_alternating(fns, calls, warm=3):
    """fns: {name: fn}; returns {name: median ms}, the functions called in turn."""
    for _ in range(warm):
        for f in fns.values():
            f()
    times = {k: [] for k in fns}
    for _ in range(calls):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def dev_stats(hi, ex):
    d = (hi.double() - ex.double())
    scale = ex.double().abs().max().item()
    return d.abs().max().item() / scale, d.pow(2).mean().sqrt().item() / scale


def layer(N, H, W, calls):
    dev = torch.device('cuda')
    g = torch.Generator(device='cpu').manual_seed(N * 7 + H)
    x = torch.randn((N, H, W, 64), generator=g).to(dev)
    w = (torch.randn((3, 3, 64, 64), generator=g) * 0.06).to(dev)
    b = torch.randn((64,), generator=g).to(dev)
    dpre = torch.randn((N, H, W, 64), generator=g).to(dev)
    flops = 2.0 * N * H * W * 64 * 64 * 9
    outs = {p: torch.empty_like(x) for p in ('highest', 'high')}
    dxs = {p: torch.empty_like(x) for p in ('highest', 'high')}
    dws = {p: torch.empty((3, 3, 64, 64), device=dev) for p in ('highest', 'high')}
    dbs = {p: torch.empty((64,), device=dev) for p in ('highest', 'high')}
    wss = {p: torch.empty((ops.bwd_filter_workspace_bytes(x.shape, w.shape, precision=p) + 3) // 4, device=dev)
           for p in ('highest', 'high')}
    ops_ = {
        'fwd': lambda p: ops.conv2d_fwd(x, w, b, 'same', 'relu', out=outs[p], precision=p),
        'bwd_data': lambda p: ops.conv2d_bwd_data(dpre, w, x.shape, 'same', x_in=x, in_act='relu', out=dxs[p], precision=p),
        'bwd_filter': lambda p: ops.conv2d_bwd_filter(x, dpre, w.shape, 'same', dw=dws[p], dbias=dbs[p], workspace=wss[p],
                                                      precision=p),
    }
    res = {'fwd': outs, 'bwd_data': dxs, 'bwd_filter': dws}
    for name, f in ops_.items():
        t = median_alternating({p: (lambda p=p: f(p)) for p in ('highest', 'high')}, calls)
        mx, rms = dev_stats(res[name]['high'], res[name]['highest'])
        print('%-10s %4dx%4dx%4d  exact %8.1f us  bf16x3 %8.1f us  speed-up %5.2fx  | max dev %.2e  rms dev %.2e | '
              'bf16x3: %5.1f %% of fp32 peak, %5.1f %% of bf16 peak (3x FLOPs)' %
              (name, N, H, W, t['highest'] * 1e3, t['high'] * 1e3, t['highest'] / t['high'], mx, rms,
               100 * flops / (t['high'] * 1e-3) / FP32_PEAK, 100 * 3 * flops / (t['high'] * 1e-3) / BF16_PEAK), flush=True)


def vdsr(batch, calls):
    dev = torch.device('cuda')
    ms = {p: model_vdsr.VdsrModel(20, True, device=dev, seed=1, precision=p) for p in ('highest', 'high')}
    g = torch.Generator(device='cpu').manual_seed(batch)
    hd = (torch.rand((batch, 41, 41, 3), generator=g) * 2 - 1).to(dev)
    sd = (hd + 0.1 * torch.randn(hd.shape, generator=g).to(dev)).clamp(-1, 1)
    sr = {p: ms[p].forward(sd, keep=False).clone() for p in ms}          # the same (seeded) weights: before any step
    mx, rms = dev_stats(sr['high'] - sd, sr['highest'] - sd)
    t = median_alternating({p: (lambda p=p: ms[p].train_step(sd, hd, 1e-4)) for p in ms}, calls)
    print('VDSR-20 train step, batch %3d x 41 x 41: exact %7.3f ms  high %7.3f ms  speed-up %5.2fx  | forward residual '
          '(sr - sd) max dev %.2e  rms dev %.2e' % (batch, t['highest'], t['high'], t['highest'] / t['high'], mx, rms), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    a = ap.parse_args()
    print('device: %s' % torch.cuda.get_device_name(0))
    for shape in ((256, 41, 41), (64, 128, 128), (1, 720, 1280)):
        layer(*shape, calls=a.calls)
    for batch in (64, 256):
        vdsr(batch, a.calls)


if __name__ == '__main__':
    main()
