#!/usr/bin/env python3
"""Timing of SRCNN's training data path at the reference's shape (batch 64 of 243 x 243 x 3, factor 3, border 6): the host
route train() runs by default beside --patch-source device (resident images, one table upload and ONE launch per batch:
srx_srcnn_patch_pairs), and one whole training step fed by each.

Images: IMAGES synthetic decoded images of 375 x 500 from a fixed seed (smooth colour fields plus noise), written once as
JPEGs to a temporary directory because dataset_reader reads a directory; nothing else is read.

Per batch, median and minimum of BATCHES after a warm-up, the routes alternating batch by batch in ONE process:
  (a) host route    next(dataset_reader), torch.from_numpy(...).to(device), degrade (two srx_resize_bicubic_tf launches), the
                    border slice with .contiguous(), a device synchronise -- train()'s four lines
      of which      next(dataset_reader) alone (host only)
  (b) copy alone    torch.from_numpy(batch).to(device) of such a batch and a synchronise
  (c) device route  patch_table (the batch's random draws), check + table upload + launch (ops.srcnn_patch_pairs), a synchronise
      of which      patch_table alone (host only)
      kernel alone  HIP events around ROUNDS back-to-back launches on a table that is already on the device, per launch; its
                    GB/s over the bytes it must read (the crops) and write (sd, hd), and that as a share of 8 TB/s
  (d) train step    one whole step -- batch from the source, then SrcnnModel.train_step -- ended by a synchronise, per source

  python scripts/time_srcnn_pairs.py
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAGES = 32
B, FACTOR = 64, 3
BATCHES, WARMUP = 30, 5
ROUNDS = 20
HBM_BYTES_PER_S = 8e12


def write_images(directory):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(243)
    for i in range(IMAGES):
        h, w = 375, 500
        coarse = rng.integers(0, 256, size=((h + 15) // 16 + 1, (w + 15) // 16 + 1, 3)).astype(np.uint8)
        field = np.asarray(Image.fromarray(coarse).resize((w, h), Image.BICUBIC)).astype(np.int16)
        im = np.clip(field + rng.integers(-6, 7, size=field.shape), 0, 255).astype(np.uint8)
        Image.fromarray(im).save(os.path.join(directory, 'im%04d.jpg' % i), quality=95)


def main():
    import ctypes
    import statistics
    import tempfile
    import time
    import numpy as np
    import torch
    from ml_super_resolution_amd import ops
    from ml_super_resolution_amd.srcnn import srcnn
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    with tempfile.TemporaryDirectory() as directory:
        write_images(directory)
        flags = srcnn.sanity_check(srcnn._flags().parse_args(['--train', '--training-images-path', directory, '--batch-size', str(B),
                                                               '--upscaling-factor', str(FACTOR)]))
        S = flags.crop_image_size
        model = srcnn.SrcnnModel(flags, device=dev, seed=0)
        side = model.crop_side()
        T = S - 2 * side
        print('batch %d of %d x %d x 3, factor %d, border %d; %d images of 375 x 500' % (B, S, S, FACTOR, side, IMAGES), flush=True)

        t0 = time.perf_counter()
        image_set = srcnn.DeviceImageSet(srcnn.decode_training_images(flags), S, dev)
        torch.cuda.synchronize()
        print('DeviceImageSet: %.1f MB on the device, decoded and uploaded in %.2f s' % (image_set.nbytes / 1e6, time.perf_counter() - t0), flush=True)
        reader = srcnn.dataset_reader(flags, seed=7)
        batches = srcnn.device_batches(flags, dev, seed=7, image_set=image_set)
        rng, state = np.random.default_rng(8), {}
        fixed = next(srcnn.dataset_reader(flags, seed=9))
        print('host batch: %.1f MB of float32' % (fixed.nbytes / 1e6))

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def host_batch():
            hd_full = torch.from_numpy(next(reader)).to(dev)
            sd_full = model.degrade(hd_full)
            return sd_full, hd_full[:, side:hd_full.shape[1] - side, side:hd_full.shape[2] - side].contiguous()

        def device_route():
            ops.srcnn_patch_pairs(image_set.arena, srcnn.patch_table(image_set, flags, rng, state), S, FACTOR, side)

        routes = {
            '(a) host route': host_batch,
            '    next(dataset_reader) alone': lambda: next(reader),
            '(b) copy alone': lambda: torch.from_numpy(fixed).to(dev),
            '(c) device route': device_route,
            '    patch_table alone': lambda: srcnn.patch_table(image_set, flags, rng, state),
            '(d) train step, host source': lambda: model.train_step(*host_batch()),
            '(d) train step, device source': lambda: model.train_step(*next(batches)),
        }
        t = {k: [] for k in routes}
        for i in range(WARMUP + BATCHES):
            for k, fn in routes.items():
                r = clock(fn)
                if i >= WARMUP:
                    t[k].append(r)
        print('ms per batch of %d: median and minimum of %d' % (B, BATCHES))
        for k in routes:
            print('  %-32s median %9.3f  min %9.3f' % (k, statistics.median(t[k]), min(t[k])), flush=True)

        # the kernel alone: the table already on the device, the outputs allocated
        words = ops.srcnn_patch_table_check(srcnn.patch_table(image_set, flags, rng, state), S, FACTOR, side, image_set.nbytes)
        table_dev = torch.from_numpy(words).to(dev)
        sd = torch.empty((B, S, S, 3), dtype=torch.float32, device=dev)
        hd = torch.empty((B, T, T, 3), dtype=torch.float32, device=dev)
        L = ops.lib()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def launch():
            ops.check(L.srx_srcnn_patch_pairs(ctypes.c_void_p(image_set.arena.data_ptr()), ctypes.c_void_p(table_dev.data_ptr()), B, S, FACTOR,
                                              side, ctypes.c_void_p(sd.data_ptr()), ctypes.c_void_p(hd.data_ptr()), stream), 'srx_srcnn_patch_pairs')
        per_launch = []
        for i in range(WARMUP + BATCHES):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(ROUNDS):
                launch()
            e.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                per_launch.append(s.elapsed_time(e) / ROUNDS)
        nbytes = B * (S * S * 3 + 4 * S * S * 3 + 4 * T * T * 3)
        med, low = statistics.median(per_launch), min(per_launch)
        rate = nbytes / (med * 1e-3)
        print('  %-32s median %9.3f  min %9.3f   (HIP events, %d launches back to back)' % ('    kernel alone', med, low, ROUNDS))
        print('  kernel: %.1f MB read + written per batch, %.0f GB/s at the median = %.1f %% of 8 TB/s; %d workgroups, %d bytes of LDS each'
              % (nbytes / 1e6, rate / 1e9, 100 * rate / HBM_BYTES_PER_S, B * -(-S // L.srx_srcnn_pairs_band(S, FACTOR)),
                 L.srx_srcnn_pairs_lds_bytes(S, FACTOR)))
        c, b = statistics.median(t['(c) device route']), statistics.median(t['(b) copy alone'])
        print('  (c) / (b) = %.4f: building the batch on the device %s copying the host-built batch' % (c / b, 'costs less than' if c < b else 'DOES NOT cost less than'))


if __name__ == '__main__':
    main()
