"""
dataset.py -- mirror of espcn/espcn/dataset.py: a set of images becomes (lr patch, sub-pixel label) training pairs.

The reference extracts every pair ahead of training and writes one TFRecord per pair (dataset.py:81-158, :198-222); the
trainer then reads them shuffled and repeated (:54-78).  The whole image is mapped to [-1, 1] and blurred with
sigma = 0.5 (r - 1) ('nearest' borders), tiled into P x P patches (P = p r; a patch that would end on the image's edge is
not produced), each in its four flips; the lr patch is the blurred image decimated at offset r // 2 and the label is the
HR patch in sub-pixel layout.  This module offers:
  * extract_image_patches: the host restatement (scipy's gaussian_filter, as experiment_test.py: prepare_image_pair);
  * patch_records: every patch of a set as srx_patch_src records (ops.PATCH_SRC_DTYPE) in the reference's order;
  * DevicePatchSet: the decoded images packed into one uint8 arena on the device and their checked records, uploaded once;
  * host_patch_batches: all pairs extracted on the host once (the TFRecords' role), gathered and uploaded per batch;
  * device_patch_batches: the same pairs built by ONE launch per batch from the resident set (ops.espcn_patch_pairs) --
    one index upload per epoch, none per batch.
Both iterators sample without replacement and reshuffle per epoch (Dataset.list_files(shuffle=True).repeat(), one record
per file), draw rng.permutation(n) from np.random.default_rng(seed) epoch by epoch -- one seed, the same patches in the
same order from either -- and yield (lr, hr_target) device tensors with the target already in label layout.
"""
import itertools

import numpy as np
import torch

from ..image_arena import ResidentEvalSet
from ..vdsr.dataset import DeviceImageSet


def extract_image_patches(hr_image_u8, upscaling_factor, hr_patch_size):
    """dataset.py:81-158 on an already decoded uint8 image [h, w, 3]: generates (lr_patch [p,p,3], hr_label [p,p,3 r^2])
    float32, p = hr_patch_size // r, x outermost, then y, then the row flip, then the column flip."""
    from scipy.ndimage import gaussian_filter
    r, P = int(upscaling_factor), int(hr_patch_size)
    p = P // r
    hr = hr_image_u8 / 127.5 - 1.0
    sigma = max(0.0, 0.5 * (r - 1.0))
    bl = gaussian_filter(hr, sigma=(sigma, sigma, 0), mode='nearest', truncate=4.0) if sigma > 0 else hr
    off = r // 2
    h, w, c = hr.shape
    for x, y, u, v in itertools.product(range(0, w - P, P), range(0, h - P, P), (-1, 1), (-1, 1)):
        hr_patch = hr[y:y + P, x:x + P][::u, ::v]
        lr_patch = bl[y + off:y + off + P:r, x + off:x + off + P:r][::u, ::v]
        label = hr_patch.reshape(p, r, p, r, c).transpose(0, 2, 1, 3, 4).reshape(p, p, r * r * c)
        yield lr_patch.astype(np.float32), label.astype(np.float32)


def patch_records(heights, widths, offsets, r, p):
    """Every patch of a set of images (arrays of heights, widths and arena byte offsets) as one ops.PATCH_SRC_DTYPE array,
    image by image in extract_image_patches' order, without a Python loop per patch.  flip: bit 0 mirrors along the width
    (v = -1), bit 1 along the height (u = -1); scaling_factor holds r."""
    from .. import ops
    heights, widths = np.asarray(heights, np.int64), np.asarray(widths, np.int64)
    offsets = np.asarray(offsets, np.uint64)
    P = int(p) * int(r)
    nx, ny = np.maximum((widths - 1) // P, 0), np.maximum((heights - 1) // P, 0)     # len(range(0, w - P, P))
    counts = nx * ny * 4
    image = np.repeat(np.arange(len(counts)), counts)
    q = np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)   # index within the image
    records = np.empty(len(q), ops.PATCH_SRC_DTYPE)
    records['offset'], records['width'], records['height'] = offsets[image], widths[image], heights[image]
    records['x'] = q // (4 * ny[image]) * P
    records['y'] = q // 4 % ny[image] * P
    records['flip'] = 2 * (q // 2 % 2 == 0) + (q % 2 == 0)                             # u, v run over (-1, 1): -1 first
    records['scaling_factor'] = r
    return records


def epoch_index_batches(n, batch_size, seed):
    """The patch indices of batch after batch: permutations of range(n) drawn from np.random.default_rng(seed) epoch by
    epoch, cut into runs of batch_size (a batch may straddle epochs)."""
    rng = np.random.default_rng(seed)
    perm, pos = None, n
    while True:
        idx = np.empty(batch_size, np.int64)
        filled = 0
        while filled < batch_size:                      # once per epoch boundary inside the batch, not per patch
            if pos == n:
                perm, pos = rng.permutation(n), 0
            k = min(batch_size - filled, n - pos)
            idx[filled:filled + k] = perm[pos:pos + k]
            pos += k
            filled += k
        yield idx


def _checked_images(images_u8):
    for im in images_u8:
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError('images must be uint8 arrays [h, w, 3]')
    return list(images_u8)


class DevicePatchSet:
    """The training images resident on the device with the records of all their patches: the images that yield at least
    one patch (h > P and w > P) packed into one uint8 arena (DeviceImageSet's packing), `records` (host, patch_records'
    order) checked by srx_espcn_patch_table_check and uploaded once as `table` (ops.EspcnPatchTable)."""

    def __init__(self, images_u8, r, p, device):
        from .. import ops
        self.r, self.p = int(r), int(p)
        P = self.r * self.p
        kept = [im for im in _checked_images(images_u8) if im.shape[0] > P and im.shape[1] > P]
        if not kept:
            raise ValueError('no image is larger than %dx%d: no patch' % (P, P))
        self.images = DeviceImageSet(kept, P + 1, device)
        self.device, self.arena = self.images.device, self.images.arena
        self.records = patch_records(self.images.heights, self.images.widths, self.images.offsets, self.r, self.p)
        self.table = ops.espcn_patch_table(self.records, self.r, self.p, self.arena)

    def __len__(self):
        return len(self.records)


def host_patch_batches(images_u8, r, p, batch_size, device, seed=None):
    """All pairs extracted on the host once, then per batch one gather and one upload.  Yields (lr [B,p,p,3],
    hr_target [B,p,p,3 r^2]) device tensors."""
    pairs = [pair for im in _checked_images(images_u8) for pair in extract_image_patches(im, r, p * r)]
    if not pairs:
        raise ValueError('no image is larger than %dx%d: no patch' % (p * r, p * r))
    lr_all, label_all = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    for idx in epoch_index_batches(len(pairs), batch_size, seed):
        yield torch.from_numpy(lr_all[idx]).to(device), torch.from_numpy(label_all[idx]).to(device)


class DevicePatchBatches:
    """Iterator behind `device_patch_batches`; `last_indices` holds the patch indices (rows of the set's records) of the
    batch yielded last."""

    def __init__(self, patch_set, batch_size, seed=None):
        self.patch_set, self.batch_size = patch_set, int(batch_size)
        self.rng = np.random.default_rng(seed)
        self.perm, self.tab, self.pos = None, None, len(patch_set)
        self.last_indices = None

    def __iter__(self):
        return self

    def _new_epoch(self):
        self.perm = self.rng.permutation(len(self.patch_set))
        self.tab = self.patch_set.table.permuted(torch.from_numpy(self.perm).to(self.patch_set.device))   # once per epoch
        self.pos = 0

    def next_rows(self):
        """Advance by one batch: (table, start) such that rows [start, start + batch_size) are the batch.  Inside an epoch
        that is the epoch's permuted table; a batch that straddles epochs gets the tail and the head joined on the device."""
        n, B = len(self.patch_set), self.batch_size
        if self.pos == n:
            self._new_epoch()
        if self.pos + B <= n:
            start, self.pos = self.pos, self.pos + B
            self.last_indices = self.perm[start:start + B]
            return self.tab, start
        parts, idx, need = [], [], B
        while need:
            if self.pos == n:
                self._new_epoch()
            k = min(need, n - self.pos)
            parts.append(self.tab.rows(self.pos, k))
            idx.append(self.perm[self.pos:self.pos + k])
            self.pos += k
            need -= k
        self.last_indices = np.concatenate(idx)
        return type(self.tab).concat(parts), 0

    def __next__(self):
        from .. import ops
        tab, start = self.next_rows()
        return ops.espcn_patch_pairs(self.patch_set.arena, tab, start, self.batch_size)


def device_patch_batches(images_u8_or_set, r, p, batch_size, device, seed=None):
    """The same pairs as host_patch_batches, in the same order for the same seed, from a device-resident set: one launch
    per batch.  images_u8_or_set: a list of decoded uint8 images [h,w,3] (packed, checked and uploaded here, once) or a
    DevicePatchSet.  The iterator's `.last_indices` are the patch indices of the batch just yielded."""
    if isinstance(images_u8_or_set, DevicePatchSet):
        patch_set = images_u8_or_set
        if (patch_set.r, patch_set.p) != (int(r), int(p)) or patch_set.device != torch.device(device):
            raise ValueError('the patch set was built for r %d, p %d on %s' % (patch_set.r, patch_set.p, patch_set.device))
    else:
        patch_set = DevicePatchSet(images_u8_or_set, r, p, device)
    return DevicePatchBatches(patch_set, batch_size, seed)


EVAL_MIN_SIDE = 11      # the side of tf.image.ssim's gaussian window: an image in score layout below it has no window


def trimmed_eval_images(images_u8, r, names=None):
    """experiment_test.py:68-71 on decoded images: views trimmed to multiples of r (h -= h % r; w -= w % r).  An image whose
    score layout [h', w' r^2] has a side below 11 is refused by name: neither srx_image_scores nor the reference's
    tf.image.ssim can score it."""
    from .. import image_arena
    r = int(r)
    images_u8 = _checked_images(images_u8)
    names = image_arena.eval_names(len(images_u8), names)
    out = []
    for name, im in zip(names, images_u8):
        h, w = im.shape[0] - im.shape[0] % r, im.shape[1] - im.shape[1] % r
        if h // r < EVAL_MIN_SIDE or (w // r) * r * r < EVAL_MIN_SIDE:
            raise ValueError('image %s of %d x %d pixels trims to an lr of %d x %d at r = %d: too small to score (a side of the '
                             '[h, w r^2] score layout is below %d)' % (name, im.shape[0], im.shape[1], h // r, w // r, r, EVAL_MIN_SIDE))
        out.append(im[:h, :w])
    return out, names


def eval_records(trimmed, r):
    """The packed arena and the srx_eval_image records of a list of trimmed images: (image_arena.pack's tuple, records).
    Host only."""
    from .. import image_arena, ops
    packed = image_arena.pack(trimmed)
    _, offsets, widths, heights = packed
    return packed, ops.espcn_eval_records(heights, widths, offsets, r)


class DeviceEvalSet(ResidentEvalSet):
    """A held-out image set as evaluation pairs resident on the device (experiment_test.py:60-98 for every image, once):
    the images trimmed to multiples of r and packed into one uint8 arena, their checked table, and `pairs`
    (ops.EspcnEvalPairs: flat `lr`, `label` and per-image `views`) built by ONE launch at construction
    (image_arena.ResidentEvalSet).  Nothing of it is float on the host."""

    def __init__(self, images_u8, r, device, names=None):
        from .. import ops
        self.r = int(r)
        trimmed, self.names = trimmed_eval_images(images_u8, self.r, names)
        packed, records = eval_records(trimmed, self.r)
        super().__init__(packed, records, device, lambda rec, arena: ops.espcn_eval_table(rec, self.r, arena), ops.espcn_eval_pairs)
        self.lr, self.label = self.pairs.lr, self.pairs.label
        # what model.forward reads: the convolutions ask for 16-byte-aligned base pointers, and an image's lr starts
        # 3 h' w' floats after the one before it, which is a multiple of four floats only by chance.  A view that is not
        # aligned is copied once, here, on the device (lr is the small half of a pair); the scores read the label views.
        self.inputs = [lr if lr.data_ptr() % 16 == 0 else lr.clone() for lr, _ in self.views]

    def evaluate(self, model, score_space='y', out=None):
        """model.forward on every lr view, then one ops.image_scores call per image against its label (max_val 1, the map to
        [0, 1] and the clip applied by the kernel).  Returns [n, 2] (psnr, ssim) on the device; nothing here waits for
        the GPU."""
        from .. import ops
        if out is None:
            out = torch.empty((len(self), 2), dtype=torch.float32, device=self.device)
        space = 'y' if score_space == 'y' else 'rgb'
        for k, (lr, (_, label)) in enumerate(zip(self.inputs, self.views)):
            ops.image_scores(label, [model.forward(lr)], 1.0, space=space, unit_clip=True, out=out[k].view(1, 1, 2))
        return out


def load_images(dir_path):
    """The .png / .jpg / .bmp images of a directory, decoded with PIL to uint8 [h, w, 3], in name order."""
    import os
    from PIL import Image
    names = sorted(n for n in os.listdir(dir_path) if n.lower().endswith(('.png', '.jpg', '.jpeg', '.bmp')))
    return [np.asarray(Image.open(os.path.join(dir_path, n)).convert('RGB')) for n in names]
