#!/usr/bin/env python3
"""HIP-event timing of the feature-map mosaic (srx_feature_mosaic_u8) beside the route that existed before it --
ops.saturate_u8(x) followed by torch's reshape / permute / contiguous on the device -- and beside the library's
streaming copy of the input's bytes (srx_stream_copy: the ceiling of a kernel that only moves them).

Shapes: [1,256,256,64] (the reference's figure) and [1,1080,1920,64].  The three routes alternate in ONE process, window
by window (a window = 1000 or 100 back-to-back launches between two events, after a warm-up); per route the median and the
minimum of the windows are reported, and the whole measurement is repeated so the spread between repeats shows beside
the difference between routes.  GB/s over the algorithmic bytes: 4*64 read + 64 written per pixel (copy: 2 * 4*64).
At 256 x 256 everything (21 MB) stays in the 256 MiB Infinity Cache, as it does in use, right behind the forward pass.

  python scripts/time_feature_mosaic.py
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (N, H, W, launches per window): windows of about 10 ms and more of device work
SHAPES = [(1, 256, 256, 1000), (1, 1080, 1920, 100)]
WINDOWS, REPEATS = 9, 2


def main():
    import statistics
    import torch
    from ml_super_resolution_amd import ops
    for n, h, w, launches in SHAPES:
        x = torch.rand((n, h, w, 64), device='cuda') * 3 - 1.5
        out = torch.empty((n, 8 * h, 8 * w), dtype=torch.uint8, device='cuda')
        cpy = torch.empty_like(x)

        def mosaic():
            ops.feature_mosaic_u8(x, out=out)

        def composition():
            return ops.saturate_u8(x).reshape(n, h, w, 8, 8).permute(0, 3, 1, 4, 2).contiguous().reshape(n, 8 * h, 8 * w)

        def copy():
            ops.stream_copy(x, cpy)
        assert torch.equal(composition(), ops.feature_mosaic_u8(x))
        routes = (('mosaic', mosaic, 320), ('saturate_u8+permute', composition, 320), ('stream_copy', copy, 512))

        def window(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(launches): fn()
            e.record(); e.synchronize()
            return s.elapsed_time(e) / launches * 1e3
        for rep in range(REPEATS):
            for _, fn, _ in routes:
                for _ in range(20): fn()
            t = {name: [] for name, _, _ in routes}
            for _ in range(WINDOWS):
                for name, fn, _ in routes:
                    t[name].append(window(fn))
            parts = []
            for name, _, bpp in routes:
                med, lo = statistics.median(t[name]), min(t[name])
                parts.append('%s median %.2f us min %.2f us %.0f GB/s' % (name, med, lo, n * h * w * bpp / med / 1e3))
            print('[%d,%d,%d,64] repeat %d | %s' % (n, h, w, rep, ' | '.join(parts)), flush=True)
        del x, out, cpy


if __name__ == '__main__':
    main()
