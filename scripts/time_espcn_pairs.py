#!/usr/bin/env python3
"""Timing of ESPCN's real-image data path at the reference's recipe (batch 64 of 17 x 17, r = 3): the train step is about
150 us and latency-bound, so whatever the host does per batch is on the critical path.

Images: 24 synthetic uint8 images of 200-500 pixels a side, fixed seed; every 51 x 51 patch of them in its four flips.

Part 1, per batch:
  enqueue   host clock around next(batches) alone: how long the thread that also issues the train step is held
  wall      host clock around next(batches) + a device synchronise
  device    HIP events around next(batches): stream time from the request to the finished batch
Part 2, step windows: a window is WINDOW_STEPS steps (next(batches) [+ space_to_depth] + train_step) between two device
synchronises, with three sources alternating window by window in ONE process:
  (a) resident      one resident batch reused: the ceiling
  (b) npz_batches   experiment_train.npz_batches on an .npz of the same patches + ops.space_to_depth per step (the
                    real-data path before --patch_source)
  (c) device        espcn/dataset.py device_patch_batches: one launch per batch
Every figure is the median of BATCHES batches / WINDOWS windows after a warm-up, with minimum and maximum.

  python scripts/time_espcn_pairs.py
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, P_LR, BATCH = 3, 17, 64
BATCHES, WARMUP = 50, 10
WINDOWS, WINDOW_STEPS = 30, 20


def make_images():
    import numpy as np
    rng = np.random.default_rng(24)
    return [rng.integers(0, 256, size=(int(rng.integers(200, 501)), int(rng.integers(200, 501)), 3), dtype=np.uint8)
            for _ in range(24)]


def write_npz(path, images):
    """The .npz experiment_train.npz_batches reads: lr_patches [M,17,17,3] and hr_patches [M,51,51,3] (not yet in label
    layout), the same patches in the same order as the device set's records."""
    import numpy as np
    from ml_super_resolution_amd.espcn import dataset
    P = R * P_LR
    lr = np.stack([a for im in images for a, _ in dataset.extract_image_patches(im, R, P)])
    hr = []
    for im in images:
        rec = dataset.patch_records([im.shape[0]], [im.shape[1]], [0], R, P_LR)
        f = (im / 127.5 - 1.0).astype(np.float32)
        hr += [f[t['y']:t['y'] + P, t['x']:t['x'] + P][::(-1 if t['flip'] & 2 else 1), ::(-1 if t['flip'] & 1 else 1)] for t in rec]
    np.savez(path, lr_patches=lr, hr_patches=np.stack(hr))
    return len(lr)


def main():
    import statistics
    import tempfile
    import time
    import torch
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.espcn import dataset, experiment_train, model_espcn
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    images = make_images()
    tmp = tempfile.mkdtemp()
    npz = os.path.join(tmp, 'patches.npz')
    n = write_npz(npz, images)
    patch_set = dataset.DevicePatchSet(images, R, P_LR, dev)
    assert len(patch_set) == n
    print('%d images, %.1f MB decoded, %d patches of %d x %d (r %d), batch %d' % (len(images), sum(im.size for im in images) / 1e6, n,
                                                                                  P_LR, P_LR, R, BATCH), flush=True)

    def labelled(gen):                       # the parent path: HR patches -> label layout on the device, per step
        for lr, hr in gen:
            yield lr, ops.space_to_depth(hr, R)

    def sources():
        return {'npz_batches': labelled(experiment_train.npz_batches(npz, BATCH, dev)),
                'host_patch_batches': dataset.host_patch_batches(images, R, P_LR, BATCH, dev, seed=0),
                'device_patch_batches': dataset.device_patch_batches(patch_set, R, P_LR, BATCH, dev, seed=0)}

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
        return (t1 - t0) * 1e6, (t2 - t0) * 1e6, s.elapsed_time(e) * 1e3

    print('part 1: us per batch, median of %d (enqueue / wall / device events)' % BATCHES)
    gens = sources()
    t = {k: [] for k in gens}
    for i in range(WARMUP + BATCHES):
        for k, g in gens.items():
            r = one_batch(g)
            if i >= WARMUP:
                t[k].append(r)
    for k in gens:
        med = [statistics.median(x[j] for x in t[k]) for j in range(3)]
        print('  %-22s enqueue %8.1f  wall %8.1f  device %8.1f' % (k, *med), flush=True)

    print('part 2: ESPCN train step at %d x %d x %d, r %d: us per step, median of %d windows of %d steps' % (BATCH, P_LR, P_LR, R, WINDOWS,
                                                                                                        WINDOW_STEPS))
    model = model_espcn.EspcnModel(R, device=dev, seed=7)
    gens = sources()
    fixed = next(gens['device_patch_batches'])

    def resident():
        while True:
            yield fixed
    gens = {'(a) resident': resident(), '(b) npz_batches': gens['npz_batches'], '(c) device': gens['device_patch_batches']}

    def window(g):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(WINDOW_STEPS):
            lr, target = next(g)
            model.train_step(lr, target, 1e-4)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / WINDOW_STEPS
    t = {k: [] for k in gens}
    for i in range(3 + WINDOWS):
        for k, g in gens.items():
            r = window(g)
            if i >= 3:
                t[k].append(r)
    base = statistics.median(t['(a) resident'])
    for k in gens:
        med = statistics.median(t[k])
        print('  %-18s %8.1f us/step  %8.1f steps/s  %6.1f %% of resident  (min %.1f max %.1f us)'
              % (k, med * 1e6, 1 / med, 100 * base / med, min(t[k]) * 1e6, max(t[k]) * 1e6), flush=True)
    os.remove(npz)
    os.rmdir(tmp)


if __name__ == '__main__':
    main()
