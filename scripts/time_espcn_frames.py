#!/usr/bin/env python3
"""Times ESPCN 3x on frame sequences, host uint8 arrays in to host uint8 arrays out, and the kernels of the byte path.

End to end (FRAMES frames per sequence, LR 270 x 480 -- the one-launch window --, 360 x 640 and 720 x 1280 -- both on the
per-layer route), three variants taking turns in one process, each figure the median of ROUNDS sequences (min .. max
beside it), a host clock around the whole sequence (the last frame is on the host when it stops):
  (a) the per-frame route that existed: experiment_test.super_resolve_array + `(sr * 255.0 + 0.5).astype(uint8)`
  (b) bytes, FrameResolver depth 1 (upload, compute, download in series)
  (c) bytes, FrameResolver depth 3 (the three overlapped); once more with copy=True
and, from a run of (c) with timed events, how long each of the three streams was busy per frame: the largest bounds (c).

Device only (events around windows of launches, candidates alternating, median of ROUNDS_DEV windows):
  srx_espcn_forward_u8 against srx_espcn_forward and against decode + srx_espcn_forward + encode at [32,17,17], 256 x 256
  and 270 x 480; srx_unit_u8 at 2160 x 3840 x 3 against srx_stream_copy moving the same 5 n bytes; the five-launch graph
  against the three-launch graph at 720 x 1280."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_super_resolution_amd import ops                                     # noqa: E402
from ml_super_resolution_amd.espcn import experiment_test, model_espcn      # noqa: E402
from ml_super_resolution_amd.espcn.frames import FrameResolver              # noqa: E402

FRAMES = int(os.environ.get('SRX_TIME_FRAMES', '256'))
ROUNDS = int(os.environ.get('SRX_TIME_ROUNDS', '3'))
ROUNDS_DEV, WINDOW, WARMUP = 5, 0.2, 10


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters          # us per call


def compare(fns):
    """{name: fn} -> {name: (median, min, max)} in us, the candidates alternating round by round."""
    iters = {}
    for name, fn in fns.items():
        for _ in range(WARMUP):
            fn()
        iters[name] = max(10, int(WINDOW * 1e6 / max(window(fn, 10), 1.0)))
    times = {name: [] for name in fns}
    for _ in range(ROUNDS_DEV):
        for name, fn in fns.items():
            times[name].append(window(fn, iters[name]))
    return {name: (sorted(t)[len(t) // 2], min(t), max(t)) for name, t in times.items()}


def fmt(t):
    return '%.1f (%.1f .. %.1f)' % t


def sequence_seconds(run):
    torch.cuda.synchronize()
    began = time.perf_counter()
    n = run()
    torch.cuda.synchronize()
    assert n == FRAMES
    return time.perf_counter() - began


def end_to_end(m, h, w):
    model = {'_model': m}
    pool = np.random.default_rng(h).integers(0, 256, (8, h, w, 3), dtype=np.uint8)
    frames = [pool[k % 8] for k in range(FRAMES)]

    def float_route():
        n = 0
        for f in frames:
            out = (experiment_test.super_resolve_array(model, f) * 255.0 + 0.5).astype(np.uint8)
            n += out.shape[2] == 3
        return n

    resolvers = {1: FrameResolver(m, h, w, batch=1, depth=1), 3: FrameResolver(m, h, w, batch=1, depth=3)}

    def bytes_route(depth, copy):
        def run():
            n = 0
            for _, out in resolvers[depth].resolve(frames, copy=copy):
                n += out.shape[2] == 3
            return n
        return run

    variants = {'(a) float per frame': float_route, '(b) bytes depth 1': bytes_route(1, False),
                '(c) bytes depth 3': bytes_route(3, False), '(c) depth 3, copy=True': bytes_route(3, True)}
    # the routes give the same bytes; this is also the warm-up of every shape and graph
    want = (experiment_test.super_resolve_array(model, frames[1]) * 255.0 + 0.5).astype(np.uint8)
    for depth in (1, 3):
        got = [out for _, out in resolvers[depth].resolve(frames[:4], copy=True)]
        assert np.array_equal(got[1], want), 'the byte route differs from the float route'
    fps = {name: [] for name in variants}
    for k in range(ROUNDS):
        for name, run in variants.items():
            fps[name].append(FRAMES / sequence_seconds(run))
        print('  (LR %d x %d: round %d of %d done)' % (h, w, k + 1, ROUNDS), file=sys.stderr, flush=True)
    med = {name: sorted(v)[len(v) // 2] for name, v in fps.items()}
    print('LR %d x %d, r = 3, %d frames per sequence, %d sequences each -- frames per second, median (min .. max):' % (h, w, FRAMES, ROUNDS))
    for name, v in fps.items():
        print('  %-24s %8.1f (%.1f .. %.1f)' % (name, med[name], min(v), max(v)))
    print('  (c) / (a) = %.2f   (c) / (b) = %.2f' % (med['(c) bytes depth 3'] / med['(a) float per frame'], med['(c) bytes depth 3'] / med['(b) bytes depth 1']))
    timed = FrameResolver(m, h, w, batch=1, depth=3, timing=True)
    for _ in timed.resolve(frames, copy=False):
        pass
    busy = {op: ms / FRAMES for op, ms in timed.stream_ms.items()}
    print('  (c) with timed events, busy ms per frame: upload %.3f, compute %.3f, download %.3f -> bound by %s (%.1f frames/s at most)'
          % (busy['upload'], busy['compute'], busy['download'], max(busy, key=busy.get), 1e3 / max(busy.values())))
    sys.stdout.flush()


def device_only(m):
    params = [(m.stack.kernel(i), m.stack.bias(i)) for i in range(3)]
    lut = m.lut
    for n, h, w in ((32, 17, 17), (1, 256, 256), (1, 270, 480)):
        b = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device='cuda')
        x = ops.u8_lut_float(b, lut)
        hr = torch.empty((n, 3 * h, 3 * w, 3), device='cuda')
        hr8 = torch.empty((n, 3 * h, 3 * w, 3), dtype=torch.uint8, device='cuda')

        def composition():
            ops.u8_lut_float(b, lut, out=x)
            ops.espcn_forward(x, params, 3, out=hr)
            ops.unit_u8(hr, out=hr8)
        got = compare({'u8': lambda: ops.espcn_forward_u8(b, lut, params, 3, out=hr8), 'float': lambda: ops.espcn_forward(x, params, 3, out=hr),
                       'composition': composition})
        print('one launch [%d,%d,%d] r = 3, us: srx_espcn_forward_u8 %s | srx_espcn_forward %s | decode + float + encode %s'
              % (n, h, w, fmt(got['u8']), fmt(got['float']), fmt(got['composition'])))
    n = 2160 * 3840 * 3
    x = torch.rand((n,), device='cuda') * 2 - 1
    out = torch.empty((n,), dtype=torch.uint8, device='cuda')
    src, dst = torch.rand((n * 5 // 8,), device='cuda'), torch.empty((n * 5 // 8,), device='cuda')      # 2.5 n bytes read, 2.5 n written
    got = compare({'unit_u8': lambda: ops.unit_u8(x, out=out), 'copy': lambda: ops.stream_copy(src, dst),
                   'unit_u8 + 1 byte': lambda: ops.unit_u8(x[:-4], out=out[1:-3])})
    print('srx_unit_u8 2160 x 3840 x 3 (%.1f MB moved): %s us = %.0f GB/s | srx_stream_copy of the same bytes %s us = %.0f GB/s | out one byte off '
          '(byte stores) %s us' % (5 * n * 1e-6, fmt(got['unit_u8']), 5 * n / got['unit_u8'][0] * 1e-3, fmt(got['copy']),
                                   5 * n / got['copy'][0] * 1e-3, fmt(got['unit_u8 + 1 byte'])))
    b = torch.randint(0, 256, (1, 720, 1280, 3), dtype=torch.uint8, device='cuda')
    x = ops.u8_lut_float(b, lut)
    got = compare({'five': lambda: m.super_resolve_u8(b, single_launch=False, use_graph=True),
                   'three': lambda: m.super_resolve(x, single_launch=False, use_graph=True)})
    print('720 x 1280 LR, replayed graphs, us: five launches (bytes to bytes) %s | three launches (floats) %s | + %.1f us'
          % (fmt(got['five']), fmt(got['three']), got['five'][0] - got['three'][0]))
    sys.stdout.flush()


def main():
    torch.cuda.set_device(0)
    m = model_espcn.EspcnModel(3, device='cuda', seed=1)
    for i in range(3):
        m.stack.bias(i).uniform_(-0.1, 0.1)
    what = sys.argv[1:] or ['device', '270x480', '360x640', '720x1280']
    for item in what:
        if item == 'device':
            device_only(m)
        else:
            h, w = (int(v) for v in item.split('x'))
            end_to_end(m, h, w)


if __name__ == '__main__':
    main()
