#!/usr/bin/env python3
"""HIP-event timing of the summary panel encoder (srx_summary_panel_u8) beside the composition it replaces and beside
the library's streaming copy of the sources' bytes (srx_stream_copy: the ceiling of a kernel that only moves them).

Shapes, the reference's own: VDSR 64 x 41 x 41 x3 sources, EnhanceNet 64 x 128 x 128 x3, ESPCN 64 x 17 x 17 x2 in label
layout (r = 3), and SRCNN's 64 x 231 x 231 x3 with the range pass (sd a crop of the 243-pixel input, read in place).
Composition: torch.cat along the width, then ops.saturate_u8 (which carries the x * 127.5 + 127.5 map itself); for
r = 3 the split / reshape of the reference's graph as one permute in between; for SRCNN contiguous crops, torch's
amin / amax, the rescale in torch and a cast.  Each composition is asserted equal to the panel first.

The routes alternate in ONE process, window by window (a window = `launches` back-to-back calls between two events,
after a warm-up); per route the median and the minimum of the windows are reported, and the whole measurement is
repeated so the spread between repeats shows beside the difference between routes.  GB/s over the algorithmic bytes:
12 read + 3 written per panel pixel (ranged: 24 + 3, the sources are read twice; copy: 12 + 12).

  python scripts/time_summary_panel.py
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS, REPEATS = 9, 2


def cases(torch, ops):
    def rand(*shape):
        return torch.rand(shape, device='cuda') * 3 - 1.5

    def plain(name, n, s, launches):
        src = [rand(n, s, s, 3) for _ in range(3)]
        return name, src, 1, None, (lambda: ops.saturate_u8(torch.cat(src, dim=2)).reshape(n * s, 3 * s, 3)), launches
    yield plain('vdsr 64x41x41 x3', 64, 41, 1000)
    yield plain('enet 64x128x128 x3', 64, 128, 1000)
    n, p, r = 64, 17, 3
    src = [rand(n, p, p, 27) for _ in range(2)]
    yield ('espcn 64x17x17 x2 r=3', src, r, None,
           lambda: ops.saturate_u8(torch.cat(src, dim=2).reshape(n, p, 2 * p, r, r, 3).permute(0, 1, 3, 2, 4, 5).contiguous())
           .reshape(n * p * r, 2 * p * r, 3), 1000)
    n, s, b = 64, 243, 6
    hd, sr, sd_full = rand(n, s - 2 * b, s - 2 * b, 3), rand(n, s - 2 * b, s - 2 * b, 3), rand(n, s, s, 3)
    src = [hd, sd_full[:, b:s - b, b:s - b], sr]

    def ranged():
        x = torch.cat([t.contiguous() for t in src], dim=2)
        lo, hi = x.amin(), x.amax()
        m = torch.maximum(lo.abs(), hi.abs())
        zero = torch.zeros_like(lo)
        # (tensor / tensor: `127.0 / m` is m.reciprocal() * 127.0 in torch, one rounding more)
        scale = torch.where(lo < 0, torch.where(m < 1e-6, zero, (zero + 127.0) / m), torch.where(hi < 1e-6, zero, (zero + 255.0) / hi))
        offset = torch.where(lo < 0, zero + 128.0, zero)
        return (x * scale + offset).to(torch.uint8).reshape(n * (s - 2 * b), 3 * (s - 2 * b), 3)
    yield 'srcnn 64x231x231 x3 ranged', src, 1, 'range', ranged, 100


def main():
    import statistics
    import torch
    from ml_super_resolution_amd import ops
    for name, src, r, mode, composition, launches in cases(torch, ops):
        out = ops.summary_panel_u8(src, r=r)
        pixels = out.numel() // 3
        flat = torch.cat([t.reshape(-1) for t in src])
        cpy = torch.empty_like(flat)
        rbuf = ops.summary_panel_range(src, r=r) if mode else None

        def panel():
            if mode:
                ops.summary_panel_range(src, r=r, out=rbuf)
            ops.summary_panel_u8(src, r=r, range=rbuf, out=out)

        def copy():
            ops.stream_copy(flat, cpy)
        panel()
        assert torch.equal(composition(), out), name
        routes = (('panel', panel, 27 if mode else 15), ('composition', composition, 27 if mode else 15), ('stream_copy', copy, 24))

        def window(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(launches): fn()
            e.record(); e.synchronize()
            return s.elapsed_time(e) / launches * 1e3
        for rep in range(REPEATS):
            for _, fn, _ in routes:
                for _ in range(20): fn()
            t = {n_: [] for n_, _, _ in routes}
            for _ in range(WINDOWS):
                for n_, fn, _ in routes:
                    t[n_].append(window(fn))
            parts = []
            for n_, _, bpp in routes:
                med, lo = statistics.median(t[n_]), min(t[n_])
                parts.append('%s median %.2f us min %.2f us %.0f GB/s' % (n_, med, lo, pixels * bpp / med / 1e3))
            print('[%s] repeat %d | %s' % (name, rep, ' | '.join(parts)), flush=True)
        del src, out, flat, cpy


if __name__ == '__main__':
    main()
