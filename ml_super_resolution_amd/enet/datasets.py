"""
datasets.py -- mirror of enet/enet/datasets.py (reference): training batches for EnhanceNet from a directory of images.

`image_batches(source_dir_path, scale_factor, batch_size)` (:79-127) yields (sd_images, bq_images, hd_images): per image
a random 128x128 crop (x, y = np.random.randint(128): the images are at least 255 pixels on a side), `sd =
scipy.misc.imresize(hd, 25)` (Pillow BILINEAR, antialiased, to 32x32), `bq = scipy.misc.imresize(sd, 400, 'bicubic')`
(Pillow BICUBIC, back to 128x128), all three as float32 / 127.5 - 1.  Here the file decode and the crop stay on the host
(Pillow), the crops go to the GPU as uint8 and both resizes and the float conversion run there
(`ops.resize_pil_u8`, `ops.u8_to_pm1`): the same bytes as the reference's CPU path (pinned by assets/enet_eagle_bq.png,
tests/test_oracle_pins.py), without the per-image Python resizes on the training loop's critical path.
(`build_image_batch_iterator`, the unused tf.data variant of :33-76, is not mirrored.)  File decoding runs on a small
thread pool a couple of batches ahead of the consumer.

`DeviceImageSet` / `device_image_batches` are the same source with the decoded images resident on the device: every file
is decoded once, the region a crop can reach (rows and columns 0 .. 254 of each image: 195 KB) is kept in one uint8
tensor, and per batch the host draws a table in `image_batches`'s order and ONE launch builds the batch
(ops.enet_patch_pairs): for the same RandomState the same tensors, bit for bit, with no file, no pool and no image copy
inside the training loop.  A set that does not fit the device fails in torch's allocation.
"""
import os

import numpy as np
import torch

from .. import image_arena, ops


def is_image_name(name):
    return os.path.splitext(name)[1].lower() in ('.png', '.jpg', '.jpeg')


def build_path_generator(dir_path, rng=None):
    """Endless generator over the directory's image paths, reshuffled every pass (:10-30)."""
    rng = rng if rng is not None else np.random
    names = [n for n in sorted(os.listdir(dir_path)) if is_image_name(n)]
    if not names:
        raise ValueError('no .png / .jpg / .jpeg images in %s' % dir_path)

    def paths_generator():
        while True:
            rng.shuffle(names)
            for name in names:
                yield os.path.join(dir_path, name)
    return paths_generator


def degrade_on_device(hd_u8):
    """hd_u8 [N,128,128,3] uint8 on the GPU -> (sd, bq, hd) float32 in [-1, 1]: sd [N,32,32,3], bq and hd [N,128,128,3]."""
    n, h, w, _ = hd_u8.shape
    sd_u8 = ops.resize_pil_u8(hd_u8, h // 4, w // 4, 'bilinear')          # imresize(hd, 25): default interp 'bilinear'
    bq_u8 = ops.resize_pil_u8(sd_u8, (h // 4) * 4, (w // 4) * 4, 'bicubic')   # imresize(sd, 400, 'bicubic')
    return ops.u8_to_pm1(sd_u8), ops.u8_to_pm1(bq_u8), ops.u8_to_pm1(hd_u8)


EVAL_MIN_SIDE = 12      # the scores need the 11 positions of SSIM's window, and a trimmed side is a multiple of 4


def trimmed_eval_images(images_u8, names=None):
    """Decoded images trimmed at the bottom and right to multiples of 4 (the top-left pixel stays, as ESPCN's trimming
    does): (trimmed views, names).  Refuses an image that is not uint8 [h, w, 3] or whose trimmed side is below
    EVAL_MIN_SIDE, naming it."""
    images_u8, names = image_arena.eval_images(images_u8, names)
    out = []
    for name, im in zip(names, images_u8):
        image_arena.refuse_unless_rgb_u8(name, im)
        h, w = im.shape[0] - im.shape[0] % 4, im.shape[1] - im.shape[1] % 4
        if min(h, w) < EVAL_MIN_SIDE:
            raise ValueError('image %s of %d x %d pixels trims to %d x %d: too small to score (a side is below %d)'
                             % (name, im.shape[0], im.shape[1], h, w, EVAL_MIN_SIDE))
        out.append(im[:h, :w])
    return out, names


def eval_records(trimmed):
    """The packed arena and the srx_enet_eval_image records of a list of trimmed images: (image_arena.pack's tuple,
    records).  Host only."""
    packed = image_arena.pack(trimmed)
    _, offsets, widths, heights = packed
    return packed, ops.enet_eval_records(np.stack([heights, widths], axis=1), offsets)


class DeviceEvalSet(image_arena.ResidentEvalSet):
    """A held-out image set as evaluation pairs resident on the device: the training degradation of the reference
    (enet/enet/datasets.py:95-127) applied to every whole image, once.  The images (a directory, listed and decoded as
    image_arena.eval_image_names / decode_rgb do, or decoded uint8 arrays) are trimmed to multiples of 4 and packed into one
    uint8 arena; `table` is their checked table and `pairs` (ops.EnetEvalPairs: flat `sd`, `bq`, `hd`) is built by ONE launch
    at construction (image_arena.ResidentEvalSet); `views[k]` = (sd, bq, hd) of image k as [1, ., ., 3] views in place.
    Nothing of it is float on the host."""

    def __init__(self, dir_or_arrays, device, names=None):
        trimmed, self.names = trimmed_eval_images(dir_or_arrays, names)
        super().__init__(*eval_records(trimmed), device, ops.enet_eval_table, ops.enet_eval_pairs)
        self.sd, self.bq, self.hd = self.pairs.sd, self.pairs.bq, self.pairs.hd

    def evaluate(self, generator, out=None):
        """generator.forward(sd, bq) on every image's views, then one ops.image_scores call per image: hd the reference,
        [bq, sr] the candidates, mapped to [0, 1] and clipped by the kernel, max_val 1, RGB.  Returns [n, 2 (bq, sr),
        2 (psnr, ssim)] on the device; nothing here waits for the GPU."""
        if out is None:
            out = torch.empty((len(self), 2, 2), dtype=torch.float32, device=self.device)
        for k, (sd, bq, hd) in enumerate(self.views):
            ops.image_scores(hd, [bq, generator.forward(sd, bq)], 1.0, space='rgb', unit_clip=True, out=out[k].view(2, 1, 2))
        return out


def _decode_crop(path, x, y):
    from PIL import Image
    hd = np.asarray(Image.open(path).convert('RGB'))
    crop = hd[y:y + 128, x:x + 128, :]
    if crop.shape != (128, 128, 3):
        raise ValueError('%s is smaller than 255 pixels on a side: crop %s' % (path, crop.shape))
    return crop


def image_batches(source_dir_path, scale_factor=4, batch_size=32, device='cuda', rng=None, workers=8, prefetch=2):
    """(sd_images, bq_images, hd_images) device tensors, forever.  scale_factor is accepted and ignored, as in the
    reference (:79: the 25 % / 400 % are literals).
    The reference decodes its batch_size files one after the other inside the training loop (a 256x256 PNG costs a
    millisecond or two: 64 of them are longer than a training step on this GPU).  Here the random numbers are drawn in
    the reference's order on the calling thread, the decode + crop jobs they define run on `workers` threads (Pillow
    releases the GIL) and `prefetch` batches are kept in flight: the same bytes, off the critical path."""
    import collections
    from concurrent.futures import ThreadPoolExecutor
    rng = rng if rng is not None else np.random
    paths = build_path_generator(source_dir_path, rng)()
    pool = ThreadPoolExecutor(max_workers=max(1, workers))

    def submit_batch():
        jobs = []
        for _ in range(batch_size):
            path = next(paths)
            x, y = rng.randint(128), rng.randint(128)          # (:104-105, in this order)
            jobs.append(pool.submit(_decode_crop, path, x, y))
        return jobs
    pending = collections.deque(submit_batch() for _ in range(max(1, prefetch)))
    try:
        while True:
            jobs = pending.popleft()
            pending.append(submit_batch())
            crops = np.stack([j.result() for j in jobs], axis=0)
            yield degrade_on_device(torch.from_numpy(crops).to(device))
    finally:
        pool.shutdown(wait=False, cancel_futures=True)


def _decode_reachable(item, side):
    """One image (a path, or a decoded uint8 array [h,w,3]) -> its [:side, :side] as a contiguous array."""
    if isinstance(item, (str, os.PathLike)):
        from PIL import Image
        name, hd = str(item), np.asarray(Image.open(item).convert('RGB'))
    else:
        name, hd = None, np.asarray(item)
        if hd.dtype != np.uint8 or hd.ndim != 3 or hd.shape[2] != 3:
            raise ValueError('images must be uint8 [h,w,3] arrays or paths')
    return name, hd.shape, np.ascontiguousarray(hd[:side, :side, :])


def pack_images(items, hd_size=128, workers=16):
    """The host side of DeviceImageSet: (arena uint8 [bytes], offsets uint64, widths int32, heights int32, names).  Of each
    image only [:2 hd_size - 1, :2 hd_size - 1] is kept: x, y < hd_size, so no crop reads past row or column
    2 hd_size - 2 (enet/enet/datasets.py:107-110).  An image smaller than that on a side raises ValueError naming it --
    here, at start-up, where `image_batches` raises only when a draw reaches past the edge."""
    from concurrent.futures import ThreadPoolExecutor
    items = list(items)
    if not items:
        raise ValueError('no images')
    side = 2 * int(hd_size) - 1
    with ThreadPoolExecutor(max_workers=max(1, min(16, workers, len(items)))) as pool:
        decoded = list(pool.map(lambda it: _decode_reachable(it, side), items))
    for k, (name, shape, _) in enumerate(decoded):
        if shape[0] < side or shape[1] < side:
            raise ValueError('%s is smaller than %d pixels on a side: %d x %d' % (name or 'image %d' % k, side, shape[1], shape[0]))
    return image_arena.pack([d[2] for d in decoded]) + ([d[0] for d in decoded],)


class DeviceImageSet(image_arena.ImageArena):
    """The decoded training images, resident on `device` (image_arena.ImageArena): the reachable region of each
    (pack_images), 195 KB per image at hd_size 128.  The host also keeps `index`, the path -> position map of the images
    that came as paths.  `source_dir` is the directory the set was listed from (DeviceImageSet.from_directory), else None."""

    def __init__(self, paths_or_arrays, device, hd_size=128):
        self.hd_size = int(hd_size)
        if self.hd_size < 4 or self.hd_size > 128 or self.hd_size % 4:
            raise ValueError('hd_size must be a multiple of 4 in 4..128')
        *packed, self.names = pack_images(paths_or_arrays, self.hd_size)
        super().__init__(packed, device)
        self.index = {name: k for k, name in enumerate(self.names) if name is not None}
        self.source_dir = None

    @classmethod
    def from_directory(cls, dir_path, device, hd_size=128):
        """Every image `build_path_generator(dir_path)` walks, in its sorted order."""
        names = [n for n in sorted(os.listdir(dir_path)) if is_image_name(n)]
        if not names:
            raise ValueError('no .png / .jpg / .jpeg images in %s' % dir_path)
        image_set = cls([os.path.join(dir_path, n) for n in names], device, hd_size)
        image_set.source_dir = dir_path
        return image_set


class DeviceImageBatches:
    """Iterator behind `device_image_batches`; `last_table` is the table of the batch yielded last."""

    def __init__(self, image_set, batch_size, rng=None, flips=False):
        rng = rng if rng is not None else np.random
        self.image_set, self.batch_size, self.rng = image_set, int(batch_size), rng
        # the flips come from a stream of their own, seeded from rng's state without drawing from it
        self.flip_rng = np.random.RandomState(rng.get_state()[1]) if flips else None
        # build_path_generator's walk on positions instead of names: shuffle's draws depend on the list's length alone,
        # and a set listed from a directory (from_directory) holds the names in the generator's sorted order
        self.order, self.pos = list(range(len(image_set))), len(image_set)
        self.last_table = None

    def __iter__(self):
        return self

    def next_table(self):
        """The draws of one batch as srx_patch_src records, in `image_batches`'s order: per entry the next image of the
        shuffled walk, then x, then y (:107-108); no launch.  Between two reshuffles nothing but the (x, y) pairs is drawn,
        so they are drawn in one call per run of entries: randint(n, size=(m, 2)) is the next 2 m scalar draws."""
        s, side, n = self.image_set, self.image_set.hd_size, len(self.image_set)
        k = np.empty(self.batch_size, np.int64)
        xy = np.empty((self.batch_size, 2), np.int64)
        filled = 0
        while filled < self.batch_size:
            if self.pos == n:
                self.rng.shuffle(self.order)
                self.pos = 0
            m = min(self.batch_size - filled, n - self.pos)
            k[filled:filled + m] = self.order[self.pos:self.pos + m]
            xy[filled:filled + m] = self.rng.randint(side, size=(m, 2))
            self.pos += m
            filled += m
        table = np.empty(self.batch_size, ops.PATCH_SRC_DTYPE)
        table['offset'], table['width'], table['height'] = s.offsets[k], s.widths[k], s.heights[k]
        table['x'], table['y'], table['flip'], table['scaling_factor'] = xy[:, 0], xy[:, 1], 0, 4.0
        if self.flip_rng is not None:
            table['flip'] = self.flip_rng.randint(4, size=self.batch_size)
        self.last_table = table
        return table

    def __next__(self):
        return ops.enet_patch_pairs(self.image_set.arena, self.next_table(), self.image_set.hd_size)


def device_image_batches(source_dir_path_or_set, scale_factor=4, batch_size=32, device='cuda', rng=None, flips=False):
    """`image_batches` from a device-resident image set: (sd_images, bq_images, hd_images) device tensors, forever, one
    table upload and ONE launch per batch (ops.enet_patch_pairs).  source_dir_path_or_set: a directory (decoded, packed and
    uploaded here, once) or a DeviceImageSet.  The draws are `image_batches`'s in its order -- the shuffled walk of
    build_path_generator(dir, rng), then x and y per entry -- so the same RandomState yields the same batches, bit for bit.  flips=True additionally reverses each crop's rows and / or columns by a 2-bit draw per entry (the
    augmentation of the reference's unused build_image_batch_iterator, :66-68) from a second stream derived from rng's
    state, which leaves image, x and y as they are.  The iterator's `.last_table` is the table of the batch just yielded."""
    if scale_factor != 4:
        raise ValueError('the device sampler resizes by 25 %% and 400 %% only (scale_factor 4), got %r' % (scale_factor,))
    if isinstance(source_dir_path_or_set, DeviceImageSet):
        image_set = source_dir_path_or_set
        if image_set.device != torch.device(device):
            raise ValueError('the image set lives on %s, not on %s' % (image_set.device, torch.device(device)))
    else:
        image_set = DeviceImageSet.from_directory(source_dir_path_or_set, device)
    return DeviceImageBatches(image_set, batch_size, rng, flips)
