#!/usr/bin/env python3
"""Times the planar YUV 4:2:0 path of ESPCN 3x: its two kernels beside the byte kernels they stand in for, and frame
sequences with layout='yuv420' beside layout='rgb', host uint8 arrays in to host uint8 arrays out.

Device only (events around windows of launches, candidates alternating, median of ROUNDS_DEV windows, min .. max beside it):
  srx_unit_yuv420 at 810 x 1440 x 3 and 2160 x 3840 x 3 against srx_unit_u8 on the same float tensor and srx_stream_copy of
  the bytes both read (4 per float); srx_yuv420_lut_float against srx_u8_lut_float at the same sizes (both write those floats).

End to end (FRAMES frames per sequence, LR 270 x 480 -- the one-launch window --, 360 x 640 and 720 x 1280, FrameResolver
depth 3, copy=False): the two layouts taking turns in one process, each figure the median of ROUNDS sequences (min .. max
beside it, the run-to-run spread), a host clock around the whole sequence; then, from one run of each layout with timed
events, how long each of the three streams was busy per frame."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_super_resolution_amd import ops                                     # noqa: E402
from ml_super_resolution_amd.espcn import model_espcn                       # noqa: E402
from ml_super_resolution_amd.espcn.frames import FrameResolver              # noqa: E402
# the measuring rules are those of the byte path's script beside this one (the script's directory is on sys.path)
from time_espcn_frames import FRAMES, ROUNDS, compare, fmt, sequence_seconds     # noqa: E402


def device_only(m):
    c = ops.yuv420_coeffs('bt601', False)
    lut = m.lut
    for h, w in ((810, 1440), (2160, 3840)):
        n = h * w * 3
        x = torch.rand((1, h, w, 3), device='cuda') * 2 - 1
        planes = torch.empty((1, ops.yuv420_frame_bytes(h, w)), dtype=torch.uint8, device='cuda')
        rgb = torch.empty((n,), dtype=torch.uint8, device='cuda')
        dst = torch.empty((n,), dtype=torch.float32, device='cuda')
        got = compare({'yuv': lambda: ops.unit_yuv420(x, c, out=planes), 'u8': lambda: ops.unit_u8(x.view(-1), out=rgb),
                       'copy': lambda: ops.stream_copy(x.view(-1), dst)})
        print('encode %d x %d x 3 (%.1f MB of floats read), us: srx_unit_yuv420 %s = %.0f GB/s | srx_unit_u8 %s = %.0f GB/s | srx_stream_copy of '
              'the floats %s | yuv / u8 = %.2f' % (h, w, 4 * n * 1e-6, fmt(got['yuv']), 4.5 * n / got['yuv'][0] * 1e-3, fmt(got['u8']),
                                                    5 * n / got['u8'][0] * 1e-3, fmt(got['copy']), got['yuv'][0] / got['u8'][0]))
        yuv = torch.randint(0, 256, (1, ops.yuv420_frame_bytes(h, w)), dtype=torch.uint8, device='cuda')
        rgb = torch.randint(0, 256, (n,), dtype=torch.uint8, device='cuda')
        got = compare({'yuv': lambda: ops.yuv420_lut_float(yuv, 1, h, w, c, lut, out=x), 'u8': lambda: ops.u8_lut_float(rgb, lut, out=dst)})
        print('decode %d x %d x 3 (%.1f MB of floats written), us: srx_yuv420_lut_float %s | srx_u8_lut_float %s | yuv / u8 = %.2f'
              % (h, w, 4 * n * 1e-6, fmt(got['yuv']), fmt(got['u8']), got['yuv'][0] / got['u8'][0]))
    sys.stdout.flush()


def end_to_end(m, h, w):
    rng = np.random.default_rng(h)
    pools = {'rgb': rng.integers(0, 256, (8, h, w, 3), dtype=np.uint8),
             'yuv420': rng.integers(0, 256, (8, ops.yuv420_frame_bytes(h, w)), dtype=np.uint8)}
    frames = {layout: [pool[k % 8] for k in range(FRAMES)] for layout, pool in pools.items()}
    resolvers = {layout: FrameResolver(m, h, w, batch=1, depth=3, layout=layout) for layout in pools}

    def route(layout):
        def run():
            n = 0
            for _, out in resolvers[layout].resolve(frames[layout], copy=False):
                n += out.dtype == np.uint8
            return n
        return run

    for layout in pools:                                                 # the warm-up of every shape and graph
        for _ in resolvers[layout].resolve(frames[layout][:8], copy=False):
            pass
    fps = {layout: [] for layout in pools}
    for k in range(ROUNDS):
        for layout in pools:
            fps[layout].append(FRAMES / sequence_seconds(route(layout)))
        print('  (LR %d x %d: round %d of %d done)' % (h, w, k + 1, ROUNDS), file=sys.stderr, flush=True)
    med = {layout: sorted(v)[len(v) // 2] for layout, v in fps.items()}
    print('LR %d x %d, r = 3, depth 3, %d frames per sequence, %d sequences each -- frames per second, median (min .. max):' % (h, w, FRAMES, ROUNDS))
    for layout, v in fps.items():
        print('  %-8s %8.1f (%.1f .. %.1f)' % (layout, med[layout], min(v), max(v)))
    print('  yuv420 / rgb = %.2f; the rgb leg spread %.1f frames/s' % (med['yuv420'] / med['rgb'], max(fps['rgb']) - min(fps['rgb'])))
    for layout in pools:
        timed = FrameResolver(m, h, w, batch=1, depth=3, timing=True, layout=layout)
        for _ in timed.resolve(frames[layout], copy=False):
            pass
        busy = {op: ms / FRAMES for op, ms in timed.stream_ms.items()}
        print('  %-8s timed events, busy ms per frame: upload %.3f, compute %.3f, download %.3f -> bound by %s (%.1f frames/s at most)'
              % (layout, busy['upload'], busy['compute'], busy['download'], max(busy, key=busy.get), 1e3 / max(busy.values())))
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
