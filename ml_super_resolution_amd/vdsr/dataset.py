"""
dataset.py -- batch sources for the VDSR entry points.

The reference's `vdsr/vdsr/dataset.py` builds (sd, hd) pairs on the host with scikit-image
(gaussian blur sigma = 0.5*(s-1), bilinear resize down then up with mode='edge', random 41x41 crop
and flip: dataset.py:13-38,82-128).  scikit-image is not part of this image and that CPU pipeline is
outside the hot path, so this module offers:
  * synthetic_batches: the benchmark's synthetic patches, generated on the GPU;
  * npz_batches: pre-extracted patch pairs ({'sd': [M,h,w,3], 'hd': [M,h,w,3]} in [-1,1]);
  * hd_image_to_sd_image: the same degradation restated with scipy.ndimage (parity with skimage
    unpinned) for the evaluate / resolve entry points;
  * image_batches: the reference's image source with the float work on the GPU (host crops, one copy and about 17
    launches per batch);
  * DeviceImageSet / patch_table / device_image_batches: the same source with the decoded images resident on the
    device: per batch the host draws a table (vectorised) and ONE launch builds the pairs (srx_vdsr_patch_pairs).
Every generator yields device tensors: nothing is copied host->device per step.
"""
import numpy as np
import torch

from .. import image_arena


def synthetic_batches(image_size, batch_size, device, seed=104):
    g = torch.Generator(device=device).manual_seed(seed)
    while True:
        hd = torch.rand((batch_size, image_size, image_size, 3), device=device, generator=g) * 2 - 1
        sd = (hd + 0.1 * torch.randn(hd.shape, device=device, generator=g)).clamp(-1, 1)
        yield sd, hd


def npz_batches(path, batch_size, device, seed=0):
    z = np.load(path)
    sd_all, hd_all = z['sd'].astype(np.float32), z['hd'].astype(np.float32)
    rng = np.random.default_rng(seed)
    while True:
        idx = rng.integers(0, sd_all.shape[0], size=batch_size)
        yield torch.from_numpy(sd_all[idx]).to(device), torch.from_numpy(hd_all[idx]).to(device)


def hd_image_to_sd_image(hd_image, scaling_factor):
    """dataset.py:13-38 restated with scipy: blur (nearest borders), bilinear resize down and back up
    (edge mode, no anti-aliasing).  float image in, float image out."""
    from scipy.ndimage import gaussian_filter, map_coordinates
    hd_h, hd_w, _ = hd_image.shape
    sd_h, sd_w = int(hd_h / scaling_factor), int(hd_w / scaling_factor)
    sigma = max(0.0, 0.5 * (scaling_factor - 1.0))
    bl = gaussian_filter(hd_image, sigma=(sigma, sigma, 0), mode='nearest', truncate=4.0) if sigma > 0 else hd_image

    def resize(img, oh, ow):
        ih, iw, c = img.shape
        # skimage.transform.resize (order 1): output pixel centre -> input coordinate, half-pixel mapping
        ys = (np.arange(oh) + 0.5) * ih / oh - 0.5
        xs = (np.arange(ow) + 0.5) * iw / ow - 0.5
        yy, xx = np.meshgrid(ys, xs, indexing='ij')
        out = np.empty((oh, ow, c), img.dtype)
        for ch in range(c):
            out[:, :, ch] = map_coordinates(img[:, :, ch], [yy, xx], order=1, mode='nearest')
        return out

    return resize(resize(bl, sd_h, sd_w), hd_h, hd_w)


def degrade_on_device(hd01, scaling_factor):
    """dataset.py:13-38 on the GPU for a batch [N,H,W,3] of float images in [0,1]: gaussian blur
    sigma = 0.5*(s-1) ('nearest' borders), bilinear resize to (int(H/s), int(W/s)) and back ('edge')."""
    from .. import ops
    N, H, W, C = hd01.shape
    sd_h, sd_w = int(H / scaling_factor), int(W / scaling_factor)
    bl = ops.gaussian_blur(hd01, max(0.0, 0.5 * (scaling_factor - 1.0)))
    return ops.resize_bilinear(ops.resize_bilinear(bl, sd_h, sd_w), H, W)


def image_batches(images_u8, scaling_factors, image_size, batch_size, device, seed=None):
    """The reference's `image_batches` (dataset.py:41-128) with the float work moved to the GPU.
    images_u8: list of decoded uint8 images [h,w,3] (host).  Per patch, as the reference: random crop,
    random horizontal flip (host, uint8 slicing), then ON DEVICE: /255, degrade with a randomly chosen
    scaling factor, map both to [-1,1].  Patches are grouped by scaling factor so that every device op runs
    on a uniform batch.  Yields (sd_images, hd_images) device tensors [batch_size, S, S, 3]."""
    from .. import ops
    if not scaling_factors:
        scaling_factors = [2.0, 3.0, 4.0]
    if any(s <= 1 for s in scaling_factors):
        raise Exception('invalide scaling factors')
    rng = np.random.default_rng(seed)
    images_u8 = [im for im in images_u8 if im.shape[0] >= image_size and im.shape[1] >= image_size and im.shape[2] == 3]
    if not images_u8:
        raise ValueError('no image is at least %dx%d' % (image_size, image_size))
    order = np.arange(len(images_u8))
    pos = len(order)
    while True:
        crops, factors = [], []
        while len(crops) < batch_size:
            if pos == len(order):
                rng.shuffle(order)
                pos = 0
            im = images_u8[order[pos]]
            pos += 1
            h, w, _ = im.shape
            x = rng.integers(0, max(w - image_size, 1))
            y = rng.integers(0, max(h - image_size, 1))
            crop = im[y:y + image_size, x:x + image_size]
            if rng.integers(0, 2) == 1:
                crop = crop[:, ::-1]
            crops.append(crop)
            factors.append(rng.choice(scaling_factors))
        factors = np.asarray(factors)
        idx = np.argsort(factors, kind='stable')
        hd_u8 = torch.from_numpy(np.ascontiguousarray(np.stack(crops)[idx])).to(device)
        hd01 = ops.u8_to_unit_float(hd_u8)
        sd01 = torch.empty_like(hd01)
        f_sorted = factors[idx]
        start = 0
        while start < batch_size:
            end = start
            while end < batch_size and f_sorted[end] == f_sorted[start]:
                end += 1
            sd01[start:end] = degrade_on_device(hd01[start:end].contiguous(), float(f_sorted[start]))
            start = end
        yield ops.affine(sd01, 2.0, -1.0), ops.affine(hd01, 2.0, -1.0)


EVAL_MIN_SIDE = 11      # the side of SSIM's gaussian window: a smaller image has no window to score


def eval_records(images_u8, scaling_factors):
    """The packed arena and the srx_vdsr_eval_image records of a list of decoded images at a list of scaling factors:
    (image_arena.pack's tuple, records).  The arena holds each image once; the records are factor-major, record
    f * len(images) + k being image k at scaling_factors[f].  Host only."""
    from .. import ops
    packed = image_arena.pack(images_u8)
    _, offsets, widths, heights = packed
    n, factors = len(images_u8), [float(s) for s in scaling_factors]
    return packed, ops.vdsr_eval_records(np.tile(heights, len(factors)), np.tile(widths, len(factors)), np.tile(offsets, len(factors)),
                                         np.repeat(np.asarray(factors, np.float32), n))


class DeviceEvalSet(image_arena.ResidentEvalSet):
    """A held-out image set as evaluation pairs resident on the device (experiment_evaluate.py:14-33 of the reference for
    every image at every scaling factor, once): the images packed into one uint8 arena, each once; a checked table with a
    record per (factor, image), factor-major; and `pairs` (ops.VdsrEvalPairs: flat `sd`, `hd` and per-record `views`) built
    by ONE launch at construction (image_arena.ResidentEvalSet).  Nothing of it is float on the host.  `names[k]`,
    `factors[k]` describe record k."""

    def __init__(self, images_u8, scaling_factors, device, names=None):
        from .. import ops
        images_u8, names = image_arena.eval_images(images_u8, names)
        factors = [float(s) for s in scaling_factors]
        if not factors or any(not (1.0 < s <= 8.0) for s in factors):
            raise ValueError('scaling factors must lie in (1, 8], got %s' % (list(scaling_factors),))
        for name, im in zip(names, images_u8):
            image_arena.refuse_unless_rgb_u8(name, im)
            if min(im.shape[:2]) < EVAL_MIN_SIDE:
                raise ValueError('image %s of %d x %d pixels is too small to score: a side is below %d, the side of the SSIM window'
                                 % (name, im.shape[0], im.shape[1], EVAL_MIN_SIDE))
        self.scaling_factors = factors
        self.names = names * len(factors)
        self.factors = [s for s in factors for _ in images_u8]
        # every record starts at a multiple of 4 floats: the views are what ConvStack.forward reads, without a copy
        super().__init__(*eval_records(images_u8, factors), device, ops.vdsr_eval_table, ops.vdsr_eval_pairs)
        self.sd, self.hd = self.pairs.sd, self.pairs.hd

    def evaluate(self, model, out=None):
        """model.forward on every record's sd view, then one ops.image_scores(hd, [sd, sr], 2.0) per record.  Returns
        [n_records, 2 (sd, sr), 2 (psnr, ssim)] on the device; nothing here waits for the GPU."""
        from .. import ops
        if out is None:
            out = torch.empty((len(self), 2, 2), dtype=torch.float32, device=self.device)
        for k, (sd, hd) in enumerate(self.views):
            ops.image_scores(hd, [sd, model.forward(sd)], 2.0, out=out[k].view(2, 1, 2))
        return out


class DeviceImageSet(image_arena.ImageArena):
    """The decoded training images, resident on the device (image_arena.ImageArena): the images `image_batches` would
    keep (at least image_size x image_size, 3 channels -- dataset.py:90-93 of the reference); smaller ones are dropped."""

    def __init__(self, images_u8, image_size, device):
        images_u8 = [im for im in images_u8 if im.shape[0] >= image_size and im.shape[1] >= image_size and im.shape[2] == 3]
        if not images_u8:
            raise ValueError('no image is at least %dx%d' % (image_size, image_size))
        if any(im.dtype != np.uint8 for im in images_u8):
            raise ValueError('images must be uint8')
        self.image_size = int(image_size)
        super().__init__(image_arena.pack(images_u8), device)


def sampler_state(image_set):
    """The image order `patch_table` walks: a permutation of the set and the position in it (exhausted: reshuffle)."""
    return {'order': np.arange(len(image_set)), 'pos': len(image_set)}


def patch_table(image_set, scaling_factors, batch_size, rng, state):
    """The random draws of one batch as a table of srx_patch_src records (ops.PATCH_SRC_DTYPE), without a Python loop
    per patch.  As the reference (dataset.py:59-63,96-109) and `image_batches`: the images come in a shuffled order
    without replacement, reshuffled when exhausted (`state`: sampler_state(image_set), advanced in place); x is uniform
    in [0, max(w - S, 1)), y in [0, max(h - S, 1)); flip and scaling factor are uniform.  The draws are made per batch
    (all images, then all x, all y, all flips, all factors), so for a given seed this is a NEW random stream, not the
    patch sequence `image_batches` yields."""
    from .. import ops
    n, S = len(image_set), image_set.image_size
    idx = np.empty(batch_size, np.int64)
    filled = 0
    while filled < batch_size:                      # once per epoch boundary inside the batch, not per patch
        if state['pos'] == n:
            rng.shuffle(state['order'])
            state['pos'] = 0
        k = min(batch_size - filled, n - state['pos'])
        idx[filled:filled + k] = state['order'][state['pos']:state['pos'] + k]
        state['pos'] += k
        filled += k
    table = np.empty(batch_size, ops.PATCH_SRC_DTYPE)
    w, h = image_set.widths[idx], image_set.heights[idx]
    table['offset'], table['width'], table['height'] = image_set.offsets[idx], w, h
    table['x'] = rng.integers(0, np.maximum(w - S, 1))
    table['y'] = rng.integers(0, np.maximum(h - S, 1))
    table['flip'] = rng.integers(0, 2, size=batch_size)
    table['scaling_factor'] = np.asarray(scaling_factors, np.float32)[rng.integers(0, len(scaling_factors), size=batch_size)]
    return table


class DeviceImageBatches:
    """Iterator behind `device_image_batches`; `last_table` is the table of the batch yielded last."""

    def __init__(self, image_set, scaling_factors, batch_size, seed=None):
        if not scaling_factors:
            scaling_factors = [2.0, 3.0, 4.0]
        if any(s <= 1 for s in scaling_factors):
            raise Exception('invalide scaling factors')
        self.image_set, self.scaling_factors, self.batch_size = image_set, list(scaling_factors), batch_size
        self.rng = np.random.default_rng(seed)
        self.state = sampler_state(image_set)
        self.last_table = None

    def __iter__(self):
        return self

    def __next__(self):
        from .. import ops
        self.last_table = patch_table(self.image_set, self.scaling_factors, self.batch_size, self.rng, self.state)
        return ops.vdsr_patch_pairs(self.image_set.arena, self.last_table, self.image_set.image_size)


def device_image_batches(images_u8_or_set, scaling_factors, image_size, batch_size, device, seed=None):
    """The reference's `image_batches` (dataset.py:41-128) from a device-resident image set: per batch one vectorised
    host draw (`patch_table`), one small table upload and ONE launch (ops.vdsr_patch_pairs) that crops, flips, converts,
    degrades each patch with its own scaling factor and maps both to [-1, 1] -- no host loop per patch, no sort by
    factor.  images_u8_or_set: a list of decoded uint8 images [h,w,3] (packed and uploaded here, once) or a
    DeviceImageSet.  Yields (sd_images, hd_images) device tensors [batch_size, S, S, 3] in table order; the iterator's
    `.last_table` is the table of the batch just yielded.  The random stream is `patch_table`'s, not `image_batches`'s."""
    if isinstance(images_u8_or_set, DeviceImageSet):
        image_set = images_u8_or_set
        if image_set.image_size != image_size or image_set.device != torch.device(device):
            raise ValueError('the image set was built for image_size %d on %s' % (image_set.image_size, image_set.device))
    else:
        image_set = DeviceImageSet(images_u8_or_set, image_size, device)
    return DeviceImageBatches(image_set, scaling_factors, batch_size, seed)
