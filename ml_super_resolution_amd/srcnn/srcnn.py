"""
srcnn.py -- mirror of srcnn/srcnn.py (reference) on the MI355X engine.

Keeps the reference's flag names/defaults (srcnn.py:8-23, dashes become underscores as tf.app.flags
does), `sanity_check()` (:28-43) and `build_srcnn()` with its result keys
{step, loss, trainer, hd_images, sd_images, sr_images} (:159-166).

The network (srcnn.py:100-130) is three VALID convolutions: 9x9 -> 64 ReLU, 1x1 -> 32 ReLU,
5x5 -> 3 tanh; the loss (:142-144) is the mean over rows of ||reshape(sr - hd, [-1, bb*bb])||_2;
the optimizer Adam(1e-3, beta1 .5, beta2 .9) (:155-157).
The reference builds its inputs in-graph (JPEG queue, random crop + flip, :46-82; bicubic down / up, :89-93).  Here
`hd_images` is fed (or drawn by `dataset_reader`, the host-side stand-in of the JPEG queue) and `sd_images`, when it
is not fed too, is computed ON THE GPU the way the reference's graph does: tf.image.resize_bicubic down by the
factor and up again (`srx_resize_bicubic_tf`; pinned against the reference's own panels).
`train()`, `super_resolution()` and `main()` mirror :208-298: checkpoints every 5000 steps under
`<ckpt-dir-path>/model.ckpt-<step>` in tf.train.Saver format with the graph's variable names
(`patch_extraction/weights`, `.../biases`, ...), resume from the latest, the hd | sd | sr panel as JPEG.
Not in the reference: `DeviceEvalSet` keeps a held-out directory as evaluation pairs on the device (one launch,
ops.srcnn_eval_pairs) and `--valid-images-path DIR --valid-every K` scores it while training (`Validator`); evaluate.py
scores a directory with a checkpoint.
"""
import argparse
import glob
import os

import numpy as np
import torch

from .. import graph, image_arena, ops
from ..engine import ConvStack, LayerSpec, truncated_normal_


def _flags():
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument('--ckpt-dir-path', default='./ckpts/')
    ap.add_argument('--logs-dir-path', default='./logs/')
    ap.add_argument('--training-images-path', default=None)
    ap.add_argument('--sr-source-path', default=None)
    ap.add_argument('--sr-target-path', default=None)
    ap.add_argument('--train', action='store_true')
    ap.add_argument('--batch-size', type=int, default=64)
    ap.add_argument('--upscaling-factor', type=int, default=3)
    ap.add_argument('--crop-image-size', type=int, default=256)
    ap.add_argument('--crop-image-side', type=int, default=6)
    ap.add_argument('--srcnn-fsub', type=int, default=33)
    ap.add_argument('--srcnn-f1', type=int, default=9)
    ap.add_argument('--srcnn-f2', type=int, default=1)
    ap.add_argument('--srcnn-f3', type=int, default=5)
    ap.add_argument('--srcnn-n1', type=int, default=64)
    ap.add_argument('--srcnn-n2', type=int, default=32)
    ap.add_argument('--save-every', type=int, default=5000)      # the reference's constant (step % 5000 == 0, :253)
    # not in the reference: where train() builds its batches.  host: dataset_reader, an upload and the in-graph degradation per
    # step; device: the decoded images stay on the GPU and ONE launch builds (sd, cropped hd) per step (device_batches)
    ap.add_argument('--patch-source', choices=('host', 'device'), default='host')
    # not flags of the reference: after the update of every step that is a multiple of --valid-every (0: never), train()
    # scores the images of --valid-images-path as evaluate.py --pairs device scores them, and the means go to the event file
    # as the scalars valid_psnr, valid_ssim (sr against hd) and valid_psnr_bq, valid_ssim_bq (the bicubic input against hd)
    # -- tags of this project, the reference's graph has none for a held-out set
    ap.add_argument('--valid-images-path', default=None)
    ap.add_argument('--valid-every', type=int, default=0)
    return ap


FLAGS = _flags().parse_args([])


def sanity_check(flags=None):
    """srcnn.py:28-43 (the reference's `/` is Python-2 integer division)."""
    f = flags or FLAGS
    smaller_output_size = f.srcnn_fsub - f.srcnn_f1 - f.srcnn_f2 - f.srcnn_f3 + 3
    boundary = (f.srcnn_fsub - smaller_output_size) // 2
    crop_size = (f.crop_image_size - boundary * 2) // smaller_output_size
    f.crop_image_side = boundary
    f.crop_image_size = crop_size * smaller_output_size + boundary * 2
    if not f.train:
        f.batch_size = 1
    return f


def layer_specs(flags=None):
    f = flags or FLAGS
    return [LayerSpec(f.srcnn_f1, 3, f.srcnn_n1, 'valid', 'relu', 'patch_extraction'),
            LayerSpec(f.srcnn_f2, f.srcnn_n1, f.srcnn_n2, 'valid', 'relu', 'non_linear_mapping'),
            LayerSpec(f.srcnn_f3, f.srcnn_n2, 3, 'valid', 'tanh', 'reconstruction')]


class SrcnnModel(object):
    def __init__(self, flags=None, device='cuda', seed=None):
        self.flags = flags or FLAGS
        self.stack = ConvStack(layer_specs(self.flags), device=device, residual=False, weight_decay=0.0,
                               leaf_names=('weights', 'biases'))                # tf.contrib.layers.convolution2d
        self.stack.loss_kind = 'rownorm'
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        for i in range(3):
            truncated_normal_(self.stack.kernel(i), 0.001, gen)    # srcnn.py:84; biases zero
        self.placeholders = {}
        self.use_single_launch = os.environ.get('SRX_SRCNN_FUSED', '1') != '0'
        # ONE launch (srx_srcnn_forward) for batches of small patches only.  Measured (scripts/time_srcnn.py, round 4): since the
        # per-layer route has its own kernels for the 9x9 3->64 and 5x5 32->3 layers, three launches win on single images of every
        # size (1 x 243^2: 52 against 58 us; 1 x 170^2: 43 against 58 -- a 15 x 15 tile costs the one-launch kernel ~55 us however few
        # of them there are); the one launch wins on many small patches (64 x 33^2: 46 against 54 us; 128 x 33^2: level).
        self.single_launch_max_pixels = int(os.environ.get('SRX_SRCNN_FUSED_MAX_PIXELS', '57600'))
        self.single_launch_min_pixels = int(os.environ.get('SRX_SRCNN_FUSED_MIN_PIXELS', '8000'))
        self.single_launch_max_patch = int(os.environ.get('SRX_SRCNN_FUSED_MAX_PATCH', '1024'))     # output pixels per image

    def crop_side(self):
        f = self.flags
        return (f.srcnn_f1 - 1 + f.srcnn_f2 - 1 + f.srcnn_f3 - 1) // 2

    def degrade(self, hd_images):
        """lo_images of srcnn.py:89-93: resize_bicubic to crop_image_size / upscaling_factor (Python-2 integer division)
        and back, on the device."""
        n, h, w, _ = hd_images.shape
        f = self.flags.upscaling_factor
        lo = ops.resize_bicubic_tf(hd_images.contiguous(), h // f, w // f)
        return ops.resize_bicubic_tf(lo, h, w)

    def forward(self, sd_images, keep=False, single_launch=None):
        """[N,S,S,3] bicubic-interpolated input -> [N,S-12,S-12,3] (VALID 9-1-5).
        Three launches (BASELINE configs[0]'s one 243 x 243 image: conv_pack3_kernel, the 1x1 layer, conv_kwrows_kernel).
        Inference (keep=False) on batches of small patches -- at most `single_launch_max_patch` output pixels per image,
        `single_launch_min_pixels` .. `single_launch_max_pixels` in all -- runs as ONE launch that chains the three layers
        through LDS (srx_srcnn_forward; bit-identical to the three launches on conv path 0, equal to rounding on the default
        path); training keeps the per-layer launches, whose activations backward needs."""
        f = self.flags
        if single_launch is None:
            n, h, w, _ = sd_images.shape
            single_launch = (self.use_single_launch and not keep and sd_images.is_cuda and (f.srcnn_f1, f.srcnn_f2, f.srcnn_f3) == (9, 1, 5)
                             and (f.srcnn_n1, f.srcnn_n2) == (64, 32) and h >= 13 and w >= 13
                             and (h - 12) * (w - 12) <= self.single_launch_max_patch
                             and self.single_launch_min_pixels <= n * (h - 12) * (w - 12) <= self.single_launch_max_pixels)
        if single_launch:
            params = [(self.stack.kernel(i), self.stack.bias(i)) for i in range(3)]
            return ops.srcnn_forward(sd_images.contiguous(), params)
        return self.stack.forward(sd_images, keep=keep)

    def forward_ensemble(self, sd_images):
        """forward averaged over the eight flips / transposes of sd_images (ensemble.self_ensemble; not in the
        reference).  The VALID network crops the same margin on every side, so cropping commutes with the transforms:
        [N,S,T,3] -> [N,S-12,T-12,3], a new tensor."""
        from .. import ensemble
        return ensemble.self_ensemble(self.forward, sd_images)

    def train_step(self, sd_images, hd_images_cropped):
        """hd_images_cropped: ground truth cropped to the VALID region (srcnn.py:132-136)."""
        # srcnn.py:155-157: AdamOptimizer(0.001, beta1=0.5, beta2=0.9); one replayed HIP graph per batch shape
        return self.stack.train_step_replay(sd_images, hd_images_cropped, 0.001, beta1=0.5, beta2=0.9)

    def run(self, keys, feed_dict):
        from .. import ops
        dev = self.stack.device
        feeds = {name: feed_dict[ph] for name, ph in self.placeholders.items() if ph in feed_dict}
        if 'sd_images' not in feeds and 'hd_images' not in feeds:
            raise ValueError('hd_images must be fed (sd_images is then derived on the GPU as in the reference), or sd_images '
                             '(the bicubic down / up-sampled input, full size)')
        side = self.crop_side()
        hd = hd_full = None
        if 'hd_images' in feeds:
            hd_full = graph.to_device(feeds['hd_images'], dev)
            hd = hd_full[:, side:hd_full.shape[1] - side, side:hd_full.shape[2] - side].contiguous()
        sd = graph.to_device(feeds['sd_images'], dev) if 'sd_images' in feeds else self.degrade(hd_full)
        loss = None
        if 'trainer' in keys:
            loss = self.train_step(sd, hd)
            sr = self.stack.acts[-1]
        else:
            sr = self.stack.forward(sd, keep=True)
            if 'loss' in keys:
                loss = self.stack.loss
                ops.rownorm_loss_fwd_bwd(sr, hd, sr.shape[1] * sr.shape[2], loss, want_grad=False)
        out = {}
        for k in keys:
            if k == 'trainer':
                out[k] = None
            elif k == 'loss':
                out[k] = float(loss.item())
            elif k == 'step':
                out[k] = self.stack.global_step
            elif k == 'sr_images':
                out[k] = sr.detach().cpu().numpy()
            elif k == 'hd_images':      # cropped to the valid region, as the reference returns them
                out[k] = hd.detach().cpu().numpy()
            elif k == 'sd_images':
                out[k] = sd[:, side:sd.shape[1] - side, side:sd.shape[2] - side].detach().cpu().numpy()
            else:
                raise KeyError(k)
        return out


def build_srcnn(hd_images=None, sd_images=None, flags=None, device='cuda', seed=None):
    """-> {'step','loss','trainer','hd_images','sd_images','sr_images'} (srcnn.py:159-166).
    hd_images / sd_images: graph.placeholders for the full-size ground truth and the bicubic
    down/up-sampled input (created here when omitted)."""
    m = SrcnnModel(flags, device=device, seed=seed)
    hd_images = hd_images or graph.placeholder([None, None, None, 3], name='hd_images')
    sd_images = sd_images or graph.placeholder([None, None, None, 3], name='sd_images')
    m.placeholders['hd_images'] = hd_images
    m.placeholders['sd_images'] = sd_images
    return {
        'step': graph.Tensor('global_step', owner=m, key='step'),
        'loss': graph.Tensor('loss', owner=m, key='loss'),
        'trainer': graph.Tensor('trainer', owner=m, key='trainer'),
        'hd_images': graph.Tensor('hd_images', owner=m, key='hd_images'),
        'sd_images': graph.Tensor('sd_images', owner=m, key='sd_images'),
        'sr_images': graph.Tensor('sr_images', owner=m, key='sr_images'),
        '_model': m, '_feed_hd_images': hd_images, '_feed_sd_images': sd_images,
    }


# ---------------------------------------------------------------------------------------------------------------------
# the script: dataset reader, train(), super_resolution(), main()   (srcnn/srcnn.py:46-82, 169-298)
# ---------------------------------------------------------------------------------------------------------------------
def dataset_reader(flags, seed=None):
    """Host-side stand-in of build_dataset_reader (:46-82): JPEGs of --training-images-path (training) or the one
    --sr-source-path image, random crop to crop_image_size, random left-right flip, / 127.5 - 1; yields [B,S,S,3]."""
    from PIL import Image
    f = flags
    paths = sorted(glob.glob(os.path.join(f.training_images_path, '*.jpg'))) if f.train else [f.sr_source_path]
    if not paths:
        raise SystemExit('no *.jpg under %r' % (f.training_images_path,))
    rng = np.random.default_rng(seed)
    images = [np.asarray(Image.open(p).convert('RGB')) for p in paths]
    s, k = f.crop_image_size, 0
    while True:
        batch = []
        for _ in range(f.batch_size):
            im = images[k % len(images)]
            k += 1
            if im.shape[0] < s or im.shape[1] < s:
                raise SystemExit('image smaller than the %d-pixel crop' % s)
            y, x = int(rng.integers(0, im.shape[0] - s + 1)), int(rng.integers(0, im.shape[1] - s + 1))
            crop = im[y:y + s, x:x + s]
            if rng.random() < 0.5:
                crop = crop[:, ::-1]
            batch.append(crop.astype(np.float32) / np.float32(127.5) - np.float32(1.0))
        yield np.stack(batch)


def decode_training_images(flags):
    """The decoded *.jpg of --training-images-path, in dataset_reader's (sorted) order."""
    from PIL import Image
    paths = sorted(glob.glob(os.path.join(flags.training_images_path, '*.jpg')))
    if not paths:
        raise SystemExit('no *.jpg under %r' % (flags.training_images_path,))
    return [np.asarray(Image.open(p).convert('RGB')) for p in paths]


class DeviceImageSet(image_arena.ImageArena):
    """The decoded training images, resident on `device` (image_arena.ImageArena).  An image smaller than the crop is
    refused here, with dataset_reader's message.  device='cpu' keeps the arena on the host (tables can be drawn, nothing
    launched)."""

    def __init__(self, images_u8, crop_size, device):
        self.crop_size = int(crop_size)
        images = [np.ascontiguousarray(im) for im in images_u8]
        if not images:
            raise ValueError('no images')
        for im in images:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError('images must be uint8 [h, w, 3] arrays')
            if im.shape[0] < self.crop_size or im.shape[1] < self.crop_size:
                raise SystemExit('image smaller than the %d-pixel crop' % self.crop_size)
        super().__init__(image_arena.pack(images), device)


def patch_table(image_set, flags, rng, state):
    """The draws of one batch as srx_patch_src records, in dataset_reader's order: images cycle with k % len (`state['k']`
    carries over between batches), and per patch y = rng.integers(0, h - s + 1), then x, then rng.random() < 0.5 for the
    flip.  No launch."""
    s, n = image_set.crop_size, len(image_set)
    table = np.empty(flags.batch_size, ops.PATCH_SRC_DTYPE)
    k = state.get('k', 0)
    for e in range(flags.batch_size):
        i = k % n
        k += 1
        h, w = int(image_set.heights[i]), int(image_set.widths[i])
        y, x = int(rng.integers(0, h - s + 1)), int(rng.integers(0, w - s + 1))
        table[e] = (image_set.offsets[i], w, h, x, y, int(rng.random() < 0.5), float(flags.upscaling_factor))
    state['k'] = k
    return table


class DeviceBatches:
    """Iterator behind `device_batches`; `last_table` is the table of the batch yielded last."""

    def __init__(self, image_set, flags, border, seed=None):
        self.image_set, self.flags, self.border = image_set, flags, int(border)
        self.rng, self.state, self.last_table = np.random.default_rng(seed), {'k': 0}, None

    def __iter__(self):
        return self

    def __next__(self):
        f = self.flags
        self.last_table = patch_table(self.image_set, f, self.rng, self.state)
        return ops.srcnn_patch_pairs(self.image_set.arena, self.last_table, f.crop_image_size, f.upscaling_factor, self.border)


def device_batches(flags, device='cuda', seed=None, image_set=None):
    """dataset_reader + degrade + the border slice from a device-resident image set: (sd_full [B,S,S,3], hd_cropped
    [B,S-2b,S-2b,3]) device tensors, forever, one table upload and ONE launch per batch (ops.srcnn_patch_pairs); b is the
    VALID network's margin.  The files are decoded once, here (or pass a DeviceImageSet).  The draws are dataset_reader's in
    its order, so the same seed yields the same batches, bit for bit.  `.last_table` is the table of the batch just yielded."""
    f = flags
    if image_set is None:
        image_set = DeviceImageSet(decode_training_images(f), f.crop_image_size, device)
    else:
        want, have = torch.device(device), image_set.arena.device
        if have.type != want.type or (want.index is not None and have.index != want.index) or image_set.crop_size != f.crop_image_size:
            raise ValueError('the image set was built for %s and a crop of %d' % (have, image_set.crop_size))
    border = (f.srcnn_f1 - 1 + f.srcnn_f2 - 1 + f.srcnn_f3 - 1) // 2        # SrcnnModel.crop_side
    return DeviceBatches(image_set, f, border, seed)


EVAL_MIN_EXTENT = 11      # the scores need the 11 positions of SSIM's window inside the margin


def eval_records(images_u8, f, border):
    """The packed arena and the srx_srcnn_eval_image records of a list of decoded images: (image_arena.pack's tuple,
    records).  Host only."""
    packed = image_arena.pack(images_u8)
    _, offsets, widths, heights = packed
    return packed, ops.srcnn_eval_records(heights, widths, offsets, f, border)


class DeviceEvalSet(image_arena.ResidentEvalSet):
    """A held-out image set as evaluation pairs resident on the device: the reference's in-graph degradation
    (srcnn/srcnn.py:89-93) and the margin of its VALID network (:132-139) applied to every whole image, once.  The images (a
    directory, listed and decoded as image_arena.eval_image_names / decode_rgb do, or decoded uint8 arrays) are packed into
    one uint8 arena; `table` is their checked table for the factor `f` and the margin `border` (SrcnnModel.crop_side()),
    and `pairs` (ops.SrcnnEvalPairs: flat `sd`, `bq`, `hd`) is built by ONE launch at construction
    (image_arena.ResidentEvalSet); `views[k]` = (sd [1,H,W,3], bq and hd [1,H-2b,W-2b,3]) of image k in place.  An image that
    is not uint8 [h, w, 3], or of which less than EVAL_MIN_EXTENT pixels a side are left inside the margin, or with no
    low-resolution pixel (side < f), is refused by name before any GPU work.  Nothing of it is float on the host."""

    def __init__(self, dir_or_arrays, f, border, device, names=None):
        images, self.names = image_arena.eval_images(dir_or_arrays, names)
        self.f, self.border = int(f), int(border)
        for name, im in zip(self.names, images):
            image_arena.refuse_unless_rgb_u8(name, im)
            h, w = im.shape[:2]
            if min(h, w) - 2 * self.border < EVAL_MIN_EXTENT or min(h, w) < self.f:
                raise ValueError('image %s of %d x %d pixels is too small to score: a side leaves fewer than %d pixels inside the '
                                 'border of %d, or fewer than the factor %d' % (name, h, w, EVAL_MIN_EXTENT, self.border, self.f))
        packed, records = eval_records(images, self.f, self.border)
        super().__init__(packed, records, device, lambda rec, arena: ops.srcnn_eval_table(rec, self.f, self.border, arena),
                         ops.srcnn_eval_pairs)
        self.sd, self.bq, self.hd = self.pairs.sd, self.pairs.bq, self.pairs.hd

    def evaluate(self, model, out=None):
        """model.forward(sd) on every image's view, then one ops.image_scores call per image: hd the reference, [bq, sr] the
        candidates, max_val 2.0 ([-1, 1]), RGB.  Inference only: forward keeps nothing, so a trainer's activations stay as
        they are.  Returns [n, 2 (bq, sr), 2 (psnr, ssim)] on the device; nothing here waits for the GPU."""
        if model.crop_side() != self.border:
            raise ValueError('the set was built for a border of %d, the model removes %d' % (self.border, model.crop_side()))
        if out is None:
            out = torch.empty((len(self), 2, 2), dtype=torch.float32, device=self.device)
        for k, (sd, bq, hd) in enumerate(self.views):
            ops.image_scores(hd, [bq, model.forward(sd)], 2.0, out=out[k].view(2, 1, 2))
        return out


def latest_checkpoint(ckpt_dir):
    from .. import tf_bundle
    return tf_bundle.latest_checkpoint(ckpt_dir) if ckpt_dir and os.path.isdir(ckpt_dir) else None


def build_sr_result(model, hd_full, sd_full, sr):
    """The panel hd | sd | sr (:169-184): three [B*width, width, 3] strips side by side, width = crop_image_size - 2 * side."""
    side = model.crop_side()
    crop = lambda t: t[:, side:t.shape[1] - side, side:t.shape[2] - side]
    strips = [t.reshape(1, -1, t.shape[2], 3) for t in (crop(hd_full), crop(sd_full), sr)]
    return torch.cat(strips, dim=2)


VALID_TAGS = ('valid_psnr', 'valid_ssim', 'valid_psnr_bq', 'valid_ssim_bq')


class Validator:
    """A held-out set scored with the weights being trained, without touching the trainer: the pairs are resident
    (DeviceEvalSet) and the forward passes run in a SrcnnModel of their own that SHARES the trained parameter tensor, so
    its buffers are its own and the train step's activations, its captured graph and that graph's buffers stay as they
    are.  It draws no random number of the trainer's and takes no batch.  mean_scores() returns {tag: device scalar};
    nothing waits for the GPU."""

    def __init__(self, train_model, images_path, device):
        self.model = SrcnnModel(train_model.flags, device=device, seed=0)
        self.model.stack.params = train_model.stack.params
        self.eval_set = DeviceEvalSet(images_path, train_model.flags.upscaling_factor, train_model.crop_side(), device)
        self.scores = torch.empty((len(self.eval_set), 2, 2), dtype=torch.float32, device=device)

    def mean_scores(self):
        mean = self.eval_set.evaluate(self.model, out=self.scores).mean(dim=0)      # [2 (bq, sr), 2 (psnr, ssim)]
        return image_arena.bq_sr_tags(mean)


def train(flags, device='cuda', max_steps=None, seed=None, log=None, reporter=None):
    """srcnn.py:208-260: restore the latest checkpoint if there is one, then loop: one Adam(1e-3, .5, .9) step per batch,
    the loss every 100 steps, a checkpoint whenever step % 5000 == 0.  `max_steps` (not in the reference, whose loop
    never ends) stops after that many steps; `log`: optional callable receiving (step, loss).  --patch-source device draws
    the same batches from a device-resident image set (device_batches) instead of dataset_reader + upload + degrade.
    `reporter`: a summary.EventFileWriter (main() builds it from --logs-dir-path; None writes nothing) that receives the
    reference's summaries (:187-200,224-248): a session-log START, `loss` every step and, when the step before the update is
    a multiple of 500, in the same event the hd | sd | sr panel `image/image/0` -- a FLOAT image in the reference, so
    encoded with TensorFlow's rescale (ops.summary_panel_range); the crop of sd is passed as a view, not copied.
    With --valid-images-path DIR --valid-every K the directory is scored after the update of every step that is a multiple
    of K, once that step's summaries and panel have been taken (Validator): the scalars VALID_TAGS go to the reporter at
    that step, in an event of their own.  Training is bit-identical with and without it."""
    valid_every = getattr(flags, 'valid_every', 0)
    if valid_every > 0 and not getattr(flags, 'valid_images_path', None):
        raise ValueError('--valid-every %d needs --valid-images-path, a directory of images' % valid_every)
    m = SrcnnModel(flags, device=device, seed=seed)
    source = latest_checkpoint(flags.ckpt_dir_path)
    if source is not None:
        m.stack.load_tf_checkpoint(source)
    if reporter is not None:
        reporter.add_session_log_start(m.stack.global_step)
    on_device = getattr(flags, 'patch_source', 'host') == 'device'
    batches = device_batches(flags, m.stack.device, seed) if on_device else dataset_reader(flags, seed)
    side = m.crop_side()
    validator = Validator(m, flags.valid_images_path, m.stack.device) if valid_every > 0 else None
    done = 0
    while max_steps is None or done < max_steps:
        if on_device:
            sd_full, hd = next(batches)
        else:
            hd_full = torch.from_numpy(next(batches)).to(m.stack.device)
            sd_full = m.degrade(hd_full)
            hd = hd_full[:, side:hd_full.shape[1] - side, side:hd_full.shape[2] - side].contiguous()
        with_image = m.stack.global_step % 500 == 0
        loss = m.train_step(sd_full, hd)
        step = m.stack.global_step
        done += 1
        if reporter is not None:
            values = [('loss', loss)]
            if with_image:
                sources = [hd, sd_full[:, side:sd_full.shape[1] - side, side:sd_full.shape[2] - side], m.stack.acts[-1]]
                values.append(('image/image/0', ops.summary_panel_u8(sources, range=ops.summary_panel_range(sources))))
            reporter.add_summary(step, values)
        if validator is not None and step % valid_every == 0:
            valid = validator.mean_scores()
            if reporter is not None:
                reporter.add_summary(step, list(valid.items()))
        if log is not None:
            log(step, loss.item())
        if step % 100 == 0:
            print('loss[{}]: {}'.format(step, loss.item()), flush=True)
        if step % flags.save_every == 0:
            os.makedirs(flags.ckpt_dir_path, exist_ok=True)
            m.stack.save_tf_checkpoint(os.path.join(flags.ckpt_dir_path, 'model.ckpt-%d' % step), adam_betas=(0.5, 0.9))
    return m


def super_resolution(flags, device='cuda', seed=None):
    """srcnn.py:263-287: restore the latest checkpoint, run one (randomly cropped / flipped) crop of --sr-source-path
    through the net and write the hd | sd | sr panel to --sr-target-path as JPEG, pixels
    saturate_cast((x + 1) * 127.5, uint8)."""
    from PIL import Image
    m = SrcnnModel(flags, device=device, seed=seed)
    source = latest_checkpoint(flags.ckpt_dir_path)
    if source is None:
        raise SystemExit('no checkpoint under %r' % (flags.ckpt_dir_path,))
    m.stack.load_tf_checkpoint(source, with_optimizer=False)
    hd_full = torch.from_numpy(next(dataset_reader(flags, seed))).to(m.stack.device)
    sd_full = m.degrade(hd_full)
    sr = m.forward(sd_full)
    panel = build_sr_result(m, hd_full, sd_full, sr)[0].cpu().numpy()
    px = np.clip((panel + np.float32(1.0)) * np.float32(127.5), 0, 255).astype(np.uint8)      # clamp, truncate
    Image.fromarray(px).save(flags.sr_target_path, format='JPEG')
    return px


def main(argv=None):
    flags = sanity_check(_flags().parse_args(argv))
    if flags.train:
        from .. import summary
        with summary.EventFileWriter(flags.logs_dir_path) as reporter:      # tf.summary.FileWriter(FLAGS.logs_dir_path) (:213)
            train(flags, reporter=reporter)
    else:
        super_resolution(flags)


if __name__ == '__main__':
    main()
