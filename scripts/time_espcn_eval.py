#!/usr/bin/env python3
"""HIP-event timing of ESPCN's evaluation pairs built on the device (srx_espcn_eval_pairs / dataset.DeviceEvalSet) beside
the host route they replace, on five synthetic images of 256 x 256 ... 512 x 768 at r = 3.

  pairs     experiment_test.prepare_image_pair per image (float64 map, scipy's gaussian_filter, decimation, label layout)
            and the upload of its two float arrays, against ONE ops.espcn_eval_pairs launch for the whole resident set
            (the bytes and the table uploaded before, as DeviceEvalSet keeps them)
  evaluate  the whole experiment_scores.evaluate_images call on a directory of PNGs (model built, files decoded, pairs,
            forward passes, scores, the copy back), --pairs host --scores fused against --pairs device
  resident  DeviceEvalSet.evaluate alone (what a validation inside the trainer enqueues), no host route beside it
The two routes' numbers are compared first: labels equal, lr within 2e-5, the scores' difference printed.

The routes alternate in ONE process, window by window (a window = `calls` back-to-back calls between two events, after a
warm-up; the host route's windows include its host time, during which the stream is idle); per route the median, the
minimum and the maximum of the windows are reported, and the whole measurement is repeated.

  python scripts/time_espcn_eval.py
"""
import contextlib, io, os, statistics, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS, REPEATS, R = 7, 2, 3
SHAPES = ((256, 256), (321, 481), (384, 384), (480, 500), (512, 768))


def make_images():
    import numpy as np
    rng = np.random.default_rng(2)
    out = []
    for k, (h, w) in enumerate(SHAPES):
        y, x = np.mgrid[:h, :w]
        smooth = 127.5 + 90 * np.sin(x / (6.0 + k))[..., None] * np.cos(y / 9.0)[..., None] * np.array([1.0, 0.8, 0.6])
        out.append(np.clip(smooth + rng.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


def compare(routes, window, what):
    for rep in range(REPEATS):
        for _, fn, _ in routes:
            for _ in range(2): fn()
        t = {n_: [] for n_, _, _ in routes}
        for _ in range(WINDOWS):
            for n_, fn, calls in routes:
                t[n_].append(window(fn, calls))
        parts = ['%s median %.1f us min %.1f us max %.1f us' % (n_, statistics.median(t[n_]), min(t[n_]), max(t[n_])) for n_, _, _ in routes]
        ratio = ' | %s / %s (medians) %.1f' % (routes[0][0], routes[1][0], statistics.median(t[routes[0][0]]) / statistics.median(t[routes[1][0]])) if len(routes) == 2 else ''
        print('[%s] repeat %d | %s%s' % (what, rep, ' | '.join(parts), ratio), flush=True)


def main():
    import numpy as np
    import torch
    from PIL import Image
    from ml_super_resolution_amd import _lib, ops
    from ml_super_resolution_amd.espcn import dataset, experiment_scores, experiment_test, model_espcn
    if not torch.cuda.is_available():
        sys.exit('time_espcn_eval.py needs a GPU')
    dev = torch.device('cuda')
    images = make_images()
    names = ['im%d.png' % k for k in range(len(images))]
    eval_set = dataset.DeviceEvalSet(images, R, dev, names=names)
    tiles = _lib.lib().srx_espcn_eval_tiles(eval_set.records.ctypes.data, len(eval_set), R)
    print('[set] %d images, %d arena bytes, %d lr floats (%d label floats), %d tiles' %
          (len(eval_set), eval_set.arena.numel(), eval_set.lr.numel(), eval_set.label.numel(), tiles), flush=True)

    def host_pairs():
        out = []
        for im in images:
            lr, hr = experiment_test.prepare_image_pair(im, R)
            out.append((torch.from_numpy(lr[None]).to(dev), torch.from_numpy(hr[None]).to(dev)))
        return out

    worst = 0.0
    for k, (lr, label) in enumerate(host_pairs()):
        assert torch.equal(label, eval_set.views[k][1]), k
        worst = max(worst, (lr - eval_set.views[k][0]).abs().max().item())
    print('[pairs] labels equal; worst |lr device - lr host| %.3g' % worst, flush=True)
    assert worst <= 2e-5

    def window(fn, calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls): fn()
        e.record(); e.synchronize()
        return s.elapsed_time(e) / calls * 1e3
    out = (torch.empty_like(eval_set.lr), torch.empty_like(eval_set.label))
    compare((('host', host_pairs, 1), ('device', lambda: ops.espcn_eval_pairs(eval_set.arena, eval_set.table, out=out), 50)),
            window, 'pairs')

    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, 'images')
        os.makedirs(d)
        for n, im in zip(names, images):
            Image.fromarray(im).save(os.path.join(d, n))
        ckpt = os.path.join(tmp, 'model.ckpt.npz')
        model_espcn.EspcnModel(R, device=dev, seed=7).save(ckpt)
        argv = ['--ckpt_path', ckpt, '--data_path', d]

        def evaluate(extra):
            with contextlib.redirect_stdout(io.StringIO()):
                return experiment_scores.evaluate_images(argv + extra)
        a, b = evaluate(['--scores', 'fused']), evaluate(['--pairs', 'device'])
        print('[evaluate] |device - host| of the scores: psnr %.3g dB, ssim %.3g' %
              (np.abs(np.array(a['psnrs']) - np.array(b['psnrs'])).max(), np.abs(np.array(a['ssims']) - np.array(b['ssims'])).max()), flush=True)
        compare((('host', lambda: evaluate(['--scores', 'fused']), 1), ('device', lambda: evaluate(['--pairs', 'device']), 1)),
                window, 'evaluate')
        m = experiment_test.build_model(experiment_scores.parse_flags(argv))['_model']
        scores = torch.empty((len(eval_set), 2), device=dev)
        compare((('DeviceEvalSet.evaluate', lambda: eval_set.evaluate(m, 'y', out=scores), 20),), window, 'resident')


if __name__ == '__main__':
    main()
