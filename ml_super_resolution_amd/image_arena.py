"""
image_arena.py -- what the device-side batch samplers (VDSR, ESPCN, EnhanceNet, SRCNN) share on the host: the packing of
decoded images into one uint8 arena and the base of their resident image sets.  Which images a set keeps or refuses, and
what a sampler draws, stays with each model.  Likewise the listing and decoding of an evaluation directory and the base
of the four resident evaluation sets (ESPCN, VDSR, EnhanceNet, SRCNN): what an image must satisfy and how a set is scored
stays with each.  EnhanceNet and SRCNN score a bicubic baseline (bq) beside sr: their validation tags and the report of
their evaluation commands are here once.
"""
import os

import numpy as np
import torch


def pack(images):
    """Decoded uint8 images [h, w, 3] back to back: (arena uint8 [bytes], offsets uint64, widths int32, heights int32), all
    numpy; image k is arena[offsets[k] : offsets[k] + 3 widths[k] heights[k]], rows of 3 widths[k] bytes."""
    heights = np.array([im.shape[0] for im in images], np.int32)
    widths = np.array([im.shape[1] for im in images], np.int32)
    sizes = heights.astype(np.uint64) * widths.astype(np.uint64) * np.uint64(3)
    offsets = np.concatenate([np.zeros(1, np.uint64), np.cumsum(sizes, dtype=np.uint64)[:-1]])
    arena = np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images])
    return arena, offsets, widths, heights


class ImageArena:
    """Packed images resident on `device`: `arena`, ONE uint8 tensor uploaded once, and on the host each image's byte
    offset, width and height (numpy arrays `offsets`, `widths`, `heights`).  `packed` is what `pack` returns."""

    def __init__(self, packed, device):
        arena, self.offsets, self.widths, self.heights = packed
        self.device = torch.device(device)
        self.arena = torch.from_numpy(arena).to(self.device)

    def __len__(self):
        return len(self.widths)

    @property
    def nbytes(self):
        return self.arena.numel()


def eval_image_names(dir_path):
    """An evaluation directory's image files, sorted, by the reference's filter (experiment_test.py, experiment_evaluate.py)."""
    return [n for n in sorted(os.listdir(dir_path)) if n[-4:] in ['.png', '.jpg', '.bmp']]


def decode_rgb(path):
    """An image file decoded with PIL to uint8 [h, w, 3]."""
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def eval_names(n_images, names):
    """An evaluation set's names: '0', '1', ... unless given.  Refuses another count than the images' and an empty set."""
    names = [str(k) for k in range(n_images)] if names is None else list(names)
    if len(names) != n_images:
        raise ValueError('%d names for %d images' % (len(names), n_images))
    if not n_images:
        raise ValueError('no image to evaluate')
    return names


def eval_images(dir_or_arrays, names=None):
    """An evaluation set's decoded images and their names: (list, names) of a directory (listed by eval_image_names unless
    `names` says which files, decoded by decode_rgb) or of decoded arrays (named '0', '1', ... unless given).  Refuses as
    eval_names does."""
    if isinstance(dir_or_arrays, (str, os.PathLike)):
        if names is None:
            names = eval_image_names(dir_or_arrays)
        dir_or_arrays = [decode_rgb(os.path.join(dir_or_arrays, n)) for n in names]
    images = list(dir_or_arrays)
    return images, eval_names(len(images), None if names is None else [str(n) for n in names])


def refuse_unless_rgb_u8(name, im):
    """The refusal by name of an evaluation image that is not uint8 [h, w, 3]."""
    if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
        raise ValueError('image %s must be uint8 [h, w, 3], got %s %s' % (name, im.dtype, im.shape))


def bq_sr_tags(mean):
    """{tag: device scalar} of a set's mean scores [2 (bq, sr), 2 (psnr, ssim)]: what EnhanceNet's and SRCNN's Validator
    write to the event file."""
    return {'valid_psnr': mean[1, 0:1], 'valid_ssim': mean[1, 1:2], 'valid_psnr_bq': mean[0, 0:1], 'valid_ssim_bq': mean[0, 1:2]}


def report_bq_sr_scores(names, scores, data_path):
    """The end of EnhanceNet's and SRCNN's evaluation commands: `scores` [n, 2 (bq, sr), 2 (psnr, ssim)] on the device
    comes to the host in one copy, is printed per image and as means, and returned as {'names', 'bq_psnrs', 'bq_ssims',
    'sr_psnrs', 'sr_ssims'} (lists of floats in name order)."""
    got = scores.cpu().numpy()                                              # the one device-to-host copy
    out = {'names': names}
    for c, cand in enumerate(('bq', 'sr')):
        out[cand + '_psnrs'], out[cand + '_ssims'] = [float(v) for v in got[:, c, 0]], [float(v) for v in got[:, c, 1]]
    for k, name in enumerate(names):
        print('name: {:>32}, psnr (bq, sr): {:.4f}, {:.4f}, ssim (bq, sr): {:.4f}, {:.4f}'.format(
            name, out['bq_psnrs'][k], out['sr_psnrs'][k], out['bq_ssims'][k], out['sr_ssims'][k]))
    print('data: {}'.format(data_path))
    print('psnr (bq, sr): {:.4f}, {:.4f}'.format(float(np.mean(out['bq_psnrs'])), float(np.mean(out['sr_psnrs']))))
    print('ssim (bq, sr): {:.4f}, {:.4f}'.format(float(np.mean(out['bq_ssims'])), float(np.mean(out['sr_ssims']))))
    return out


class ResidentEvalSet:
    """A held-out image set as evaluation pairs resident on `device`: the packed images (`images`, an ImageArena; its
    `device` and `arena`), their host `records`, the checked `table`, `pairs` built by ONE launch at construction and
    `views[k]` = pairs.views(k).  Which images a set accepts, its records and its scoring are the model's DeviceEvalSet's."""

    def __init__(self, packed, records, device, make_table, launch_pairs):
        self.records = records
        self.images = ImageArena(packed, device)
        self.device, self.arena = self.images.device, self.images.arena
        self.table = make_table(records, self.arena)
        self.pairs = launch_pairs(self.arena, self.table)
        self.views = [self.pairs.views(k) for k in range(len(records))]

    def __len__(self):
        return len(self.records)
