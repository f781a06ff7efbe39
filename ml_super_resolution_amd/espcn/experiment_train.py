"""
experiment_train.py -- mirror of espcn/espcn/experiment_train.py: flags, LR schedule
lr0 * factor ** (step // decay_steps) (:101-107), resume from the latest checkpoint under ckpt_path when
one exists (:78-88), loop until stop_training_at_k_step, one checkpoint at the end (:130) -- a TensorFlow
V2 bundle `model.ckpt-<step>` with the reference's variable names (f1..f3 kernel / bias, Adam slots,
beta powers, global_step) plus the `checkpoint` state file.  The reference reads pre-shuffled TFRecords; here batches come from a
synthetic generator or an .npz of (lr_patches, hr_patches): HR patches are mapped to the sub-pixel
label layout ON THE GPU with space_to_depth (dataset.py:140-156).  With --patch_source host / device, --data_path is a
directory of images and the pairs come from espcn/dataset.py (host_patch_batches / device_patch_batches), the target
already in label layout.  With --valid_data_path DIR --valid_every K a held-out directory is scored every K steps from
device-resident pairs (dataset.DeviceEvalSet): the reference offers this only as "stop, save a checkpoint, run
experiment_test on it".
"""
import argparse
import os

import numpy as np
import torch

from .. import image_arena, ops, summary
from . import dataset, model_espcn


def synthetic_batches(batch_size, lr_patch_size, scaling_factor, device, seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    hp = lr_patch_size * scaling_factor
    while True:
        hr = torch.rand((batch_size, hp, hp, 3), device=device, generator=g) * 2 - 1
        off = scaling_factor // 2
        lr = hr[:, off::scaling_factor, off::scaling_factor].contiguous()
        yield lr, hr


def npz_batches(path, batch_size, device, seed=0):
    z = np.load(path)
    lr_all, hr_all = z['lr_patches'].astype(np.float32), z['hr_patches'].astype(np.float32)
    rng = np.random.default_rng(seed)
    while True:
        idx = rng.integers(0, lr_all.shape[0], size=batch_size)
        yield torch.from_numpy(lr_all[idx]).to(device), torch.from_numpy(hr_all[idx]).to(device)


def parse_flags(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--data_path', default=None)
    # npz: --data_path is an .npz of patches (none: synthetic); host / device: a directory of .png / .jpg / .bmp images
    ap.add_argument('--patch_source', choices=('npz', 'host', 'device'), default='npz')
    ap.add_argument('--ckpt_path', default=None)
    ap.add_argument('--logs_path', default=None)
    ap.add_argument('--batch_size', type=int, default=64)
    ap.add_argument('--scaling_factor', type=int, default=3)
    ap.add_argument('--lr_patch_size', type=int, default=17)
    ap.add_argument('--initial_learning_rate', type=float, default=0.1)
    ap.add_argument('--learning_rate_decay_factor', type=float, default=0.1)
    ap.add_argument('--learning_rate_decay_steps', type=int, default=2560)
    ap.add_argument('--stop_training_at_k_step', type=int, default=10000)
    # not flags of the reference: after the update of every step that is a multiple of --valid_every (0: never), the images of
    # --valid_data_path are scored as experiment_scores --pairs device scores them and the means go to the event file as
    # the scalars valid_psnr and valid_ssim -- tags of this project, the reference's graph has none for a held-out set
    ap.add_argument('--valid_data_path', default=None)
    ap.add_argument('--valid_every', type=int, default=0)
    return ap.parse_args(argv)


class Validator:
    """A held-out set scored with the weights being trained, without touching the trainer: the pairs are resident
    (dataset.DeviceEvalSet) and the forward passes run in a model of their own that SHARES the trained parameter tensor,
    so its buffers are its own and the captured train step keeps its pointers.  mean_scores() returns the device tensor
    [2] (psnr, ssim) of the set's means; nothing waits for the GPU."""

    def __init__(self, train_model, data_path, scaling_factor, device):
        names = image_arena.eval_image_names(data_path)     # experiment_test's filter
        images = [image_arena.decode_rgb(os.path.join(data_path, n)) for n in names]
        self.eval_set = dataset.DeviceEvalSet(images, scaling_factor, device, names=names)
        self.model = model_espcn.EspcnModel(scaling_factor, device=device, seed=0)
        self.model.stack.params = train_model.stack.params
        self.scores = torch.empty((len(self.eval_set), 2), dtype=torch.float32, device=device)

    def mean_scores(self):
        return self.eval_set.evaluate(self.model, 'y', out=self.scores).mean(dim=0)


def latest_checkpoint(ckpt_path):
    """tf.train.latest_checkpoint(ckpt_path): the state file first, then the highest-numbered bundle."""
    from .. import tf_bundle
    if not ckpt_path or not os.path.isdir(ckpt_path):
        return None
    found = tf_bundle.latest_checkpoint(ckpt_path)
    if found is not None:
        return found
    steps = {}
    for name in os.listdir(ckpt_path):
        if name.startswith('model.ckpt-') and name.endswith('.index'):
            steps[int(name[len('model.ckpt-'):-len('.index')])] = os.path.join(ckpt_path, name[:-len('.index')])
    return steps[max(steps)] if steps else None


def main(argv=None, log=None):
    """`log`: optional callable receiving one dict per step (tests).  With --logs_path the reference's TensorBoard
    summaries are written (:32-65,95-128; summary.EventFileWriter): a session-log START at the restored step, `loss` every
    step and, when the step before the update is a multiple of 1000, a separate event with the sr | hr panel
    `patches/image`; both at the step after the update."""
    FLAGS = parse_flags(argv)
    device = torch.device('cuda')
    m = model_espcn.EspcnModel(FLAGS.scaling_factor, device=device)
    source = latest_checkpoint(FLAGS.ckpt_path)
    if source is not None:
        m.stack.load_tf_checkpoint(source)               # weights, Adam slots, global_step (:78-88)
    labelled = FLAGS.patch_source != 'npz'            # the source yields the target in label layout
    if labelled:
        if not FLAGS.data_path:
            raise ValueError('--patch_source %s needs --data_path, a directory of images' % FLAGS.patch_source)
        source_fn = dataset.device_patch_batches if FLAGS.patch_source == 'device' else dataset.host_patch_batches
        batches = source_fn(dataset.load_images(FLAGS.data_path), FLAGS.scaling_factor, FLAGS.lr_patch_size, FLAGS.batch_size,
                            device, seed=0)
    else:
        batches = (npz_batches(FLAGS.data_path, FLAGS.batch_size, device) if FLAGS.data_path
                   else synthetic_batches(FLAGS.batch_size, FLAGS.lr_patch_size, FLAGS.scaling_factor, device))
    step = m.stack.global_step
    validator = None
    if FLAGS.valid_every > 0:
        if not FLAGS.valid_data_path:
            raise ValueError('--valid_every %d needs --valid_data_path, a directory of images' % FLAGS.valid_every)
        validator = Validator(m, FLAGS.valid_data_path, FLAGS.scaling_factor, device)
    reporter = summary.EventFileWriter(FLAGS.logs_path) if FLAGS.logs_path else None
    if reporter is not None:
        reporter.add_session_log_start(step)
    while step < FLAGS.stop_training_at_k_step:
        with_patches = step % 1000 == 0
        lr_rate = FLAGS.initial_learning_rate * (FLAGS.learning_rate_decay_factor ** (step // FLAGS.learning_rate_decay_steps))
        lr_patch, hr_patch = next(batches)
        hr_target = hr_patch if labelled else ops.space_to_depth(hr_patch, FLAGS.scaling_factor)
        loss = m.train_step(lr_patch, hr_target, lr_rate)
        step = m.stack.global_step
        if reporter is not None:
            reporter.add_summary(step, [('loss', loss)])
            if with_patches:
                panel = ops.summary_panel_u8([m.stack.acts[-1], hr_target], r=FLAGS.scaling_factor)
                reporter.add_summary(step, [('patches/image', panel)])
        valid = None
        if validator is not None and step % FLAGS.valid_every == 0:
            valid = validator.mean_scores()
            if reporter is not None:
                reporter.add_summary(step, [('valid_psnr', valid[0:1]), ('valid_ssim', valid[1:2])])
        if log is not None:
            rec = {'step': step, 'lr': lr_rate, 'loss': loss.item()}
            if valid is not None:
                rec['valid_psnr'], rec['valid_ssim'] = (float(v) for v in valid.cpu())
            log(rec)
        if step % 100 == 0:
            print('step %d loss %.6f lr %g' % (step, loss.item(), lr_rate), flush=True)
    if reporter is not None:
        reporter.close()                                   # reporter.flush() (:128)
    if FLAGS.ckpt_path:
        os.makedirs(FLAGS.ckpt_path, exist_ok=True)
        # saver.save(session, ckpt_path/model.ckpt, global_step=step) (:130)
        m.stack.save_tf_checkpoint(os.path.join(FLAGS.ckpt_path, 'model.ckpt-%d' % step))
    return m


if __name__ == '__main__':
    main()
