#!/usr/bin/env python3
"""Times the planar YUV formats beyond 8-bit 4:2:0 of ESPCN 3x beside the 8-bit 4:2:0 path: the yardstick is that path's kernels,
timed in the same run on the same tensors.

Device only (events around windows of launches, candidates alternating, median of ROUNDS_DEV windows, min .. max beside it):
  srx_unit_yuv for each of the eight new formats against srx_unit_yuv420 on the same float tensor, at 810 x 1440 x 3 and
  2160 x 3840 x 3; srx_yuv_lut_float likewise against srx_yuv420_lut_float.  A format moves 12 + bps (1 + 2 / block) bytes per
  pixel (block = the pixels of a chroma sample) against 4:2:0's 13.5; `bound` is that ratio x 1.25, the most an encode
  should take of srx_unit_yuv420's time.

End to end (FRAMES frames per sequence, LR 270 x 480 and 720 x 1280, FrameResolver depth 3, copy=False): layout='yuv' with
yuv420p10le and with yuv444p against layout='yuv420', taking turns in one process, each figure the median of ROUNDS sequences
(min .. max beside it), a host clock around the whole sequence."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_super_resolution_amd import _lib, ops                               # noqa: E402
from ml_super_resolution_amd.espcn import model_espcn                       # noqa: E402
from ml_super_resolution_amd.espcn.frames import FrameResolver              # noqa: E402
# the measuring rules are those of the byte path's script beside this one (the script's directory is on sys.path)
from time_espcn_frames import FRAMES, ROUNDS, compare, fmt, sequence_seconds     # noqa: E402

NEW_FORMATS = ('yuv422p', 'yuv444p', 'yuv420p10le', 'yuv422p10le', 'yuv444p10le', 'yuv420p12le', 'yuv422p12le', 'yuv444p12le')


def bytes_per_pixel(name):
    depth, sub_x, sub_y = _lib.PIXEL_FORMATS[name]
    return 12 + (1 if depth == 8 else 2) * (1 + 2.0 / ((1 << sub_x) * (1 << sub_y)))


def device_only(m):
    c8 = ops.yuv420_coeffs('bt601', False)
    coeffs = {name: ops.yuv_coeffs('bt601', False, _lib.PIXEL_FORMATS[name][0]) for name in NEW_FORMATS}
    luts = {name: m.lut_of(_lib.PIXEL_FORMATS[name][0]) for name in NEW_FORMATS}
    for h, w in ((810, 1440), (2160, 3840)):
        x = torch.rand((1, h, w, 3), device='cuda') * 2 - 1
        planes = {name: torch.empty((1, ops.yuv_frame_bytes(h, w, name)), dtype=torch.uint8, device='cuda') for name in NEW_FORMATS}
        planes8 = torch.empty((1, ops.yuv420_frame_bytes(h, w)), dtype=torch.uint8, device='cuda')
        fns = {'yuv420': lambda: ops.unit_yuv420(x, c8, out=planes8)}
        for name in NEW_FORMATS:
            fns[name] = lambda name=name: ops.unit_yuv(x, name, coeffs[name], out=planes[name])
        got = compare(fns)
        print('encode %d x %d x 3, us: srx_unit_yuv420 %s = %.0f GB/s' % (h, w, fmt(got['yuv420']), 13.5 * h * w / got['yuv420'][0] * 1e-3))
        for name in NEW_FORMATS:
            ratio, bound = got[name][0] / got['yuv420'][0], bytes_per_pixel(name) / 13.5 * 1.25
            print('  srx_unit_yuv %-12s %s = %.0f GB/s | / yuv420 = %.2f, bound %.2f: %s'
                  % (name, fmt(got[name]), bytes_per_pixel(name) * h * w / got[name][0] * 1e-3, ratio, bound, 'within' if ratio <= bound else 'MISSED'))
        # decode: legal samples (the high byte of a 16-bit sample masked to the depth)
        out = torch.empty((1, h, w, 3), device='cuda')
        for name in NEW_FORMATS:
            planes[name].random_(0, 256)
            if _lib.PIXEL_FORMATS[name][0] > 8:
                planes[name].view(-1)[1::2] &= (1 << (_lib.PIXEL_FORMATS[name][0] - 8)) - 1
        planes8.random_(0, 256)
        fns = {'yuv420': lambda: ops.yuv420_lut_float(planes8, 1, h, w, c8, m.lut, out=out)}
        for name in NEW_FORMATS:
            fns[name] = lambda name=name: ops.yuv_lut_float(planes[name], 1, h, w, name, coeffs[name], luts[name], out=out)
        got = compare(fns)
        print('decode %d x %d x 3, us: srx_yuv420_lut_float %s' % (h, w, fmt(got['yuv420'])))
        for name in NEW_FORMATS:
            print('  srx_yuv_lut_float %-12s %s | / yuv420 = %.2f' % (name, fmt(got[name]), got[name][0] / got['yuv420'][0]))
        sys.stdout.flush()


def end_to_end(m, h, w):
    rng = np.random.default_rng(h)
    kinds = {'yuv420': dict(layout='yuv420'), 'yuv420p10le': dict(layout='yuv', pixel_format='yuv420p10le'),
             'yuv444p': dict(layout='yuv', pixel_format='yuv444p')}
    resolvers = {kind: FrameResolver(m, h, w, batch=1, depth=3, **kw) for kind, kw in kinds.items()}
    frames = {}
    for kind, res in resolvers.items():
        pool = rng.integers(0, 256, (8, res.frame_bytes), dtype=np.uint8)
        if kind == 'yuv420p10le':
            pool[:, 1::2] &= 3                                           # legal 10-bit samples
        frames[kind] = [pool[k % 8] for k in range(FRAMES)]

    def route(kind):
        def run():
            n = 0
            for _, out in resolvers[kind].resolve(frames[kind], copy=False):
                n += out.dtype == np.uint8
            return n
        return run

    for kind in kinds:                                                   # the warm-up of every shape and graph
        for _ in resolvers[kind].resolve(frames[kind][:8], copy=False):
            pass
    fps = {kind: [] for kind in kinds}
    for k in range(ROUNDS):
        for kind in kinds:
            fps[kind].append(FRAMES / sequence_seconds(route(kind)))
        print('  (LR %d x %d: round %d of %d done)' % (h, w, k + 1, ROUNDS), file=sys.stderr, flush=True)
    med = {kind: sorted(v)[len(v) // 2] for kind, v in fps.items()}
    print('LR %d x %d, r = 3, depth 3, %d frames per sequence, %d sequences each -- frames per second, median (min .. max):' % (h, w, FRAMES, ROUNDS))
    for kind, v in fps.items():
        print('  %-12s %8.1f (%.1f .. %.1f), %.2f MB down per frame%s' % (kind, med[kind], min(v), max(v), resolvers[kind].hr_frame_bytes * 1e-6,
                                                                     '' if kind == 'yuv420' else ' | / yuv420 = %.2f' % (med[kind] / med['yuv420'])))
    sys.stdout.flush()


def main():
    torch.cuda.set_device(0)
    m = model_espcn.EspcnModel(3, device='cuda', seed=1)
    for i in range(3):
        m.stack.bias(i).uniform_(-0.1, 0.1)
    what = sys.argv[1:] or ['device', '720x1280', '270x480']
    for item in what:
        if item == 'device':
            device_only(m)
        else:
            h, w = (int(v) for v in item.split('x'))
            end_to_end(m, h, w)


if __name__ == '__main__':
    main()
