#!/usr/bin/env python3
"""Timing of VDSR's real-image data path: vdsr/dataset.py image_batches (host crops, one copy and about 17 launches per
batch) beside device_image_batches (resident images, one table upload and ONE launch per batch: srx_vdsr_patch_pairs),
and the train-step rate each of them feeds, beside synthetic_batches (what bench.py measures).

Images: 291 synthetic uint8 images of 200-500 pixels a side, fixed seed (the size of the reference's training set).

Part 1, per batch, at 256 x 41, 64 x 41 and 64 x 128, scaling factors 2 / 3 / 4:
  enqueue   host clock around next(batches) alone: how long the thread that also issues the train step is held
  wall      host clock around next(batches) + a device synchronise
  device    HIP events around next(batches): stream time from the request to the finished batch
Part 2, 20-layer VDSR with Adam at 256 x 41, precision 'highest' and 'high': train steps per second with each source;
a window is WINDOW_STEPS steps (next(batches) + train_step) between two device synchronises.
Every figure is the median of BATCHES batches (part 1) or WINDOWS windows (part 2) after a warm-up, the sources alternating
batch by batch / window by window in ONE process.

  python scripts/time_vdsr_pairs.py
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(256, 41), (64, 41), (64, 128)]
FACTORS = [2.0, 3.0, 4.0]
BATCHES, WARMUP = 30, 5
WINDOWS, WINDOW_STEPS = 20, 5


def make_images():
    import numpy as np
    rng = np.random.default_rng(291)
    return [rng.integers(0, 256, size=(int(rng.integers(200, 501)), int(rng.integers(200, 501)), 3), dtype=np.uint8)
            for _ in range(291)]


def main():
    import statistics
    import time
    import torch
    from ml_super_resolution_amd.vdsr import dataset, model_vdsr
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    images = make_images()
    print('291 images, %.1f MB decoded' % (sum(im.size for im in images) / 1e6), flush=True)

    def one_batch(gen):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        next(gen)
        e.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t0) * 1e3, s.elapsed_time(e)

    print('part 1: ms per batch, median of %d (enqueue / wall / device events)' % BATCHES)
    for B, S in SHAPES:
        gens = {'image_batches': dataset.image_batches(images, FACTORS, S, B, dev, seed=0),
                'device_image_batches': dataset.device_image_batches(images, FACTORS, S, B, dev, seed=0)}
        t = {k: [] for k in gens}
        for i in range(WARMUP + BATCHES):
            for k, g in gens.items():
                r = one_batch(g)
                if i >= WARMUP:
                    t[k].append(r)
        for k in gens:
            med = [statistics.median(x[j] for x in t[k]) for j in range(3)]
            print('  %3d x %3d  %-22s enqueue %7.3f  wall %7.3f  device %7.3f' % (B, S, k, *med), flush=True)

    B, S = SHAPES[0]
    print('part 2: 20-layer VDSR + Adam at %d x %d, train steps/s, median of %d windows of %d steps' % (B, S, WINDOWS, WINDOW_STEPS))
    image_set = dataset.DeviceImageSet(images, S, dev)
    for precision in ('highest', 'high'):
        model = model_vdsr.VdsrModel(num_layers=20, use_adam=True, device=dev, seed=106, precision=precision)
        gens = {'synthetic_batches': dataset.synthetic_batches(S, B, dev),
                'image_batches': dataset.image_batches(images, FACTORS, S, B, dev, seed=0),
                'device_image_batches': dataset.device_image_batches(image_set, FACTORS, S, B, dev, seed=0)}

        def window(g):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(WINDOW_STEPS):
                sd, hd = next(g)
                model.train_step(sd, hd, 5e-5)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / WINDOW_STEPS
        t = {k: [] for k in gens}
        for i in range(2 + WINDOWS):
            for k, g in gens.items():
                r = window(g)
                if i >= 2:
                    t[k].append(r)
        base = statistics.median(t['synthetic_batches'])
        for k in gens:
            med = statistics.median(t[k])
            print('  %-8s %-22s %7.3f ms/step  %7.2f steps/s  %6.1f %% of synthetic  (min %.3f max %.3f ms)'
                  % (precision, k, med * 1e3, 1 / med, 100 * base / med, min(t[k]) * 1e3, max(t[k]) * 1e3), flush=True)
        del model


if __name__ == '__main__':
    main()
