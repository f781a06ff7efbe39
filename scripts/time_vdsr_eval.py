#!/usr/bin/env python3
"""HIP-event timing of VDSR's evaluation pairs built on the device (srx_vdsr_eval_pairs / dataset.DeviceEvalSet) beside the
two routes that existed before, on synthetic images (no files needed) of 256 x 256 ... 512 x 768 at s = 2, 3, 4.

  pairs     per (image, factor): experiment_evaluate.load_image's work on the decoded image (scipy's gaussian_filter, two
            map_coordinates per channel) and the upload of its two float arrays [host]; the device route that existed:
            upload the bytes, ops.u8_to_unit_float, dataset.degrade_on_device (two blur passes, two resizes) and two
            ops.affine, seven launches [launches]; against ONE ops.vdsr_eval_pairs launch for the whole resident set (the
            bytes and the table uploaded before, as DeviceEvalSet keeps them) [device].  The launch's achieved GB/s counts 3
            bytes read and 24 written per pixel of every record.
  evaluate  the whole experiment_evaluate.main call on a directory of PNGs, once per factor (model built, checkpoint read,
            files decoded, pairs, forward passes, fused scores, the copy back): --pairs host against --pairs device
  resident  DeviceEvalSet.evaluate alone on the set at all three factors (what a validation inside the trainer enqueues)
The routes' numbers are compared first: hd equal, sd within 4e-5 of the seven-launch route; the distance to the host
route's float64 result is printed per size (it grows with the side: the fp32 pixel coordinate, which both device routes
share).

The routes alternate in ONE process, window by window (a window = `calls` back-to-back calls between two events, after a
warm-up; the host route's windows include its host time, during which the stream is idle); per route the median, the
minimum and the maximum of the windows are reported, and the whole measurement is repeated.  The last line is one JSON
record of the medians of the last repeat.

  python scripts/time_vdsr_eval.py
  python scripts/time_vdsr_eval.py --sizes 24x31,40x33 --num_layers 4 --windows 2 --repeats 1     # seconds: the test's call
"""
import argparse, contextlib, io, json, os, statistics, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FACTORS = (2.0, 3.0, 4.0)
SIZES = '256x256,321x481,384x384,480x500,512x768'


def make_images(shapes):
    import numpy as np
    rng = np.random.default_rng(2)
    out = []
    for k, (h, w) in enumerate(shapes):
        y, x = np.mgrid[:h, :w]
        smooth = 127.5 + 90 * np.sin(x / (6.0 + k))[..., None] * np.cos(y / 9.0)[..., None] * np.array([1.0, 0.8, 0.6])
        out.append(np.clip(smooth + rng.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


def compare(routes, window, what, windows, repeats, result):
    for rep in range(repeats):
        for _, fn, _ in routes:
            fn()
        t = {n_: [] for n_, _, _ in routes}
        for _ in range(windows):
            for n_, fn, calls in routes:
                t[n_].append(window(fn, calls))
        parts = ['%s median %.1f us min %.1f us max %.1f us' % (n_, statistics.median(t[n_]), min(t[n_]), max(t[n_])) for n_, _, _ in routes]
        print('[%s] repeat %d | %s' % (what, rep, ' | '.join(parts)), flush=True)
        for n_, _, _ in routes:
            result['%s_%s_us' % (what, n_)] = round(statistics.median(t[n_]), 2)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default=SIZES, help='comma-separated HxW list')
    ap.add_argument('--num_layers', type=int, default=20)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=2)
    args = ap.parse_args(argv)
    shapes = tuple(tuple(int(v) for v in s.split('x')) for s in args.sizes.split(','))
    import numpy as np
    import torch
    from PIL import Image
    from ml_super_resolution_amd import _lib, ops
    from ml_super_resolution_amd.vdsr import dataset, experiment_evaluate, model_vdsr
    if not torch.cuda.is_available():
        sys.exit('time_vdsr_eval.py needs a GPU')
    dev = torch.device('cuda')
    images = make_images(shapes)
    names = ['im%d.png' % k for k in range(len(images))]
    eval_set = dataset.DeviceEvalSet(images, FACTORS, dev, names=names)
    tiles = _lib.lib().srx_vdsr_eval_tiles(eval_set.records.ctypes.data, len(eval_set))
    pixels = int(sum(int(r['height']) * int(r['width']) for r in eval_set.records))
    result = {'sizes': args.sizes, 'factors': list(FACTORS), 'records': len(eval_set), 'tiles': int(tiles), 'pixels': pixels}
    print('[set] %d images x %d factors = %d records, %d arena bytes, %d floats in sd and in hd, %d tiles' %
          (len(images), len(FACTORS), len(eval_set), eval_set.arena.numel(), eval_set.sd.numel(), tiles), flush=True)

    def host_pairs():
        out = []
        for s in FACTORS:
            for im in images:
                hd = im.astype(np.float32) / 255.0
                sd = dataset.hd_image_to_sd_image(hd, s)
                out.append((torch.from_numpy((sd * 2.0 - 1.0)[None].astype(np.float32)).to(dev),
                            torch.from_numpy((hd * 2.0 - 1.0)[None].astype(np.float32)).to(dev)))
        return out

    def launches_pairs():
        out = []
        for s in FACTORS:
            for im in images:
                hd01 = ops.u8_to_unit_float(torch.from_numpy(im[None]).to(dev))
                out.append((ops.affine(dataset.degrade_on_device(hd01, s), 2.0, -1.0), ops.affine(hd01, 2.0, -1.0)))
        return out

    host, launches = host_pairs(), launches_pairs()
    worst_launches, worst_host = 0.0, {}
    for k, ((sd_h, hd_h), (sd_l, hd_l)) in enumerate(zip(host, launches)):
        sd, hd = eval_set.views[k]
        assert torch.equal(hd, hd_l), k
        worst_launches = max(worst_launches, (sd - sd_l).abs().max().item())
        size = '%dx%d' % tuple(hd.shape[1:3])
        worst_host[size] = max(worst_host.get(size, 0.0), (sd - sd_h).abs().max().item())
    print('[pairs] hd equal; worst |sd device - sd launches| %.3g; worst |sd device - sd host| per size: %s' %
          (worst_launches, ', '.join('%s %.3g' % kv for kv in worst_host.items())), flush=True)
    assert worst_launches <= 4e-5
    result['sd_device_vs_launches'] = worst_launches
    result['sd_device_vs_host'] = worst_host
    del host, launches

    def window(fn, calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls): fn()
        e.record(); e.synchronize()
        return s.elapsed_time(e) / calls * 1e3
    out = (torch.empty_like(eval_set.sd), torch.empty_like(eval_set.hd))
    compare((('host', host_pairs, 1), ('launches', launches_pairs, 3),
             ('device', lambda: ops.vdsr_eval_pairs(eval_set.arena, eval_set.table, out=out), 50)),
            window, 'pairs', args.windows, args.repeats, result)
    result['pairs_device_GBps'] = round(pixels * 27 / (result['pairs_device_us'] * 1e-6) / 1e9, 1)
    print('[pairs] the launch moves %d bytes (3 read + 24 written per pixel): %.1f GB/s' % (pixels * 27, result['pairs_device_GBps']), flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, 'images')
        os.makedirs(d)
        for n, im in zip(names, images):
            Image.fromarray(im).save(os.path.join(d, n))
        ckpt = os.path.join(tmp, 'model.ckpt-0.pt')
        m = model_vdsr.VdsrModel(args.num_layers, device=dev, seed=7)
        torch.save(m.stack.state_dict(), ckpt)

        def evaluate(pairs):
            got = []
            with contextlib.redirect_stdout(io.StringIO()):
                for s in FACTORS:
                    got.append(experiment_evaluate.main(['--ckpt_path', ckpt, '--hd_image_dir_path', d, '--num_layers', str(args.num_layers),
                                                         '--scaling_factor', str(int(s)), '--scores', 'fused', '--pairs', pairs]))
            return got
        a, b = evaluate('host'), evaluate('device')
        dp = max(np.abs(np.array(x['sr_psnrs']) - np.array(y['sr_psnrs'])).max() for x, y in zip(a, b))
        ds = max(np.abs(np.array(x['sr_ssims']) - np.array(y['sr_ssims'])).max() for x, y in zip(a, b))
        print('[evaluate] |device - host| of the sr scores: psnr %.3g dB, ssim %.3g' % (dp, ds), flush=True)
        result['scores_device_vs_host'] = [float(dp), float(ds)]
        compare((('host', lambda: evaluate('host'), 1), ('device', lambda: evaluate('device'), 1)), window, 'evaluate',
                args.windows, args.repeats, result)
        scores = torch.empty((len(eval_set), 2, 2), device=dev)
        compare((('DeviceEvalSet.evaluate', lambda: eval_set.evaluate(m, out=scores), 3),), window, 'resident', args.windows, args.repeats, result)
    print(json.dumps(result), flush=True)
    return result


if __name__ == '__main__':
    main()
