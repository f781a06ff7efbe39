#!/usr/bin/env python3
"""HIP-event timing of the fused image scores (srx_image_scores / ops.image_scores) beside the calls they replace.

Cases:
  vdsr 512x512x3, vdsr 1080x1920x3   (hd, [sd, sr]) with max_val 2: one ops.image_scores call against the evaluation
                                     script's separate path, two ops.psnr plus two ops.ssim
  espcn 170x170x27 y                 one label-layout image (r = 3), unit_clip and the Y space: one call against
                                     espcn/experiment_test.py: scores_in_subpixel_space (affine, clamp, reshape, Y weights,
                                     sum, contiguous for both tensors, then ops.psnr and ops.ssim)
Neither route fetches its numbers: both are timed as enqueued device work.  The two routes' numbers are compared first
(|SSIM| within 1e-4, PSNR within 1e-5 relative).

The routes alternate in ONE process, window by window (a window = `launches` back-to-back calls between two events, after
a warm-up); per route the median and the minimum of the windows are reported, and the whole measurement is repeated so
the spread between repeats shows beside the difference between routes.  The scratch and the LDS of one workgroup are
printed with each case.

  python scripts/time_image_scores.py
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS, REPEATS = 9, 2


def plan_of(shape, n_cand, max_val, space='rgb', unit_clip=False):
    """(tile_h, tile_w, tiles_y, tiles_x, scratch bytes, LDS bytes of one workgroup), all from the library's host functions
    (srx_image_scores_plan, srx_image_scores_scratch_bytes, srx_image_scores_lds_bytes)."""
    import ctypes
    from ml_super_resolution_amd import _lib
    L = _lib.lib()
    d = _lib.ScoresDesc(*shape, n_cand, _lib.SCORES_SPACE_BY_NAME[space], int(unit_clip), max_val)
    v = [ctypes.c_int(0) for _ in range(4)]
    _lib.check(L.srx_image_scores_plan(ctypes.byref(d), *[ctypes.byref(x) for x in v]), 'srx_image_scores_plan')
    return tuple(x.value for x in v) + (L.srx_image_scores_scratch_bytes(ctypes.byref(d)), L.srx_image_scores_lds_bytes(ctypes.byref(d)))


def cases(torch, ops):
    from ml_super_resolution_amd.espcn import experiment_test

    def noisy(shape, n):
        a = torch.rand(shape, device='cuda') * 2.2 - 1.1
        return a, [a + 0.15 * torch.randn(shape, device='cuda') for _ in range(n)]
    for name, shape, launches in (('vdsr 512x512x3', (1, 512, 512, 3), 200), ('vdsr 1080x1920x3', (1, 1080, 1920, 3), 30)):
        hd, (sd, sr) = noisy(shape, 2)

        def separate(hd=hd, sd=sd, sr=sr):
            return torch.stack([torch.stack([ops.psnr(hd, sd, 2.0), ops.ssim(hd, sd, 2.0)], -1),
                                torch.stack([ops.psnr(hd, sr, 2.0), ops.ssim(hd, sr, 2.0)], -1)])

        def separate_timed(hd=hd, sd=sd, sr=sr):
            ops.psnr(hd, sd, 2.0); ops.psnr(hd, sr, 2.0); ops.ssim(hd, sd, 2.0); ops.ssim(hd, sr, 2.0)
        yield name, shape, dict(n_cand=2, max_val=2.0), (lambda hd=hd, sd=sd, sr=sr: ops.image_scores(hd, [sd, sr], 2.0)), separate, separate_timed, launches
    shape = (1, 170, 170, 27)
    hr, (sr,) = noisy(shape, 1)

    def separate():
        p, q = experiment_test.scores_in_subpixel_space(None, sr, hr, 'y')
        return torch.stack([p, q], -1)[None]
    yield ('espcn 170x170x27 y', shape, dict(n_cand=1, space='y', unit_clip=True, max_val=1.0),
           (lambda: ops.image_scores(hr, [sr], 1.0, space='y', unit_clip=True)), separate, separate, 200)


def main():
    import statistics
    import torch
    from ml_super_resolution_amd import ops
    if not torch.cuda.is_available():
        sys.exit('time_image_scores.py needs a GPU')
    for name, shape, kw, fused, separate, separate_timed, launches in cases(torch, ops):
        print('[%s] tile %d x %d, %d x %d tiles, scratch %d bytes, LDS %d bytes per workgroup' % ((name,) + plan_of(shape, **kw)), flush=True)
        a, b = fused().double().cpu(), separate().double().cpu()
        d_ssim = (a[..., 1] - b[..., 1]).abs().max().item()
        d_psnr = ((a[..., 0] - b[..., 0]).abs().max() / b[..., 0].abs().max()).item()
        print('[%s] fused against separate: |ssim| %.3g, |psnr| / max %.3g' % (name, d_ssim, d_psnr), flush=True)
        assert d_ssim <= 1e-4 and d_psnr <= 1e-5, name
        routes = (('fused', fused), ('separate', separate_timed))

        def window(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(launches): fn()
            e.record(); e.synchronize()
            return s.elapsed_time(e) / launches * 1e3
        for rep in range(REPEATS):
            for _, fn in routes:
                for _ in range(10): fn()
            t = {n_: [] for n_, _ in routes}
            for _ in range(WINDOWS):
                for n_, fn in routes:
                    t[n_].append(window(fn))
            parts = ['%s median %.1f us min %.1f us max %.1f us' % (n_, statistics.median(t[n_]), min(t[n_]), max(t[n_])) for n_, _ in routes]
            print('[%s] repeat %d | %s | separate / fused (medians) %.2f' % (name, rep, ' | '.join(parts), statistics.median(t['separate']) / statistics.median(t['fused'])), flush=True)


if __name__ == '__main__':
    main()
