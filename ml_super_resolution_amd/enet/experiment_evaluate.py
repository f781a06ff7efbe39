"""
experiment_evaluate.py -- this project's own entry point: the reference's EnhanceNet has no quantitative evaluation
(enet/enet/experiment_resolve.py writes pictures, experiment_train.py logs losses).  Every image of a directory is trimmed
to multiples of 4, degraded as a training crop is (enet/enet/datasets.py:95-127 on the whole image: sd = Pillow BILINEAR
down by 4, bq = Pillow BICUBIC back up), super-resolved by the generator, and bq and sr are scored against the image: PSNR
and SSIM on [0, 1], clipped, RGB, max_val 1 (ops.image_scores).

--pairs {host,device}: where an image's (sd, bq, hd) is built.  'host' (the default) decodes one image at a time and runs
datasets.degrade_on_device on it: four resample launches and three conversions per image.  'device' decodes the directory,
uploads the bytes once and builds every image's pair in ONE launch (datasets.DeviceEvalSet, ops.enet_eval_pairs); the
[n, 2, 2] scores are copied to the host once.  Both give the same bits.

--target_dir_path: also write <name>_bq.png and <name>_sr.png, encoded as experiment_resolve encodes them.

--self_ensemble: sr is EnetGenerator.forward_ensemble(sd, bq), the mean over the eight flips / transposes of the pair
(ensemble.py), on either --pairs route; bq's own scores do not change.

  python -m ml_super_resolution_amd.enet.experiment_evaluate --source_ckpt_path ckpt/extracted/model.ckpt \
         --hd_dir_path Set5 --pairs device
"""
import argparse
import os

import numpy as np
import torch

from .. import ensemble, image_arena, ops
from . import datasets, experiment_resolve


def parse_flags(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--source_ckpt_path', required=True)
    ap.add_argument('--hd_dir_path', required=True)
    ap.add_argument('--pairs', choices=('host', 'device'), default='host')
    ap.add_argument('--precision', choices=('highest', 'high'), default='highest')
    ap.add_argument('--target_dir_path', default=None)
    # not a flag of the reference: geometric self-ensemble -- the mean over the eight flips / transposes (ensemble.py)
    ap.add_argument('--self_ensemble', action='store_true')
    return ap.parse_args(argv)


def host_pair(image_u8, device, name=None):
    """One decoded image -> (sd, bq, hd) of its trimmed self by the per-image launches (datasets.degrade_on_device)."""
    (trimmed,), _ = datasets.trimmed_eval_images([image_u8], None if name is None else [name])
    return datasets.degrade_on_device(torch.from_numpy(np.array(trimmed[None])).to(device))


def _write_pngs(target_dir_path, file_name, bq, sr):
    from PIL import Image
    name = os.path.splitext(file_name)[0]
    # saturate_cast(x * 127.5 + 127.5): clamp, then truncate (experiment_resolve.super_resolve)
    Image.fromarray(ops.saturate_u8(bq)[0].cpu().numpy()).save(os.path.join(target_dir_path, name + '_bq.png'))
    Image.fromarray(ops.saturate_u8(sr)[0].cpu().numpy()).save(os.path.join(target_dir_path, name + '_sr.png'))


def evaluate_images(FLAGS, generator=None):
    """Scores every image of FLAGS.hd_dir_path; FLAGS is the parsed flags or an argv list.  Returns {'names', 'bq_psnrs',
    'bq_ssims', 'sr_psnrs', 'sr_ssims'} (lists of floats in name order)."""
    if isinstance(FLAGS, (list, tuple)):
        FLAGS = parse_flags(FLAGS)
    device = torch.device('cuda')
    if generator is None:
        generator = experiment_resolve.load_generator(FLAGS.source_ckpt_path, device)
        generator.set_precision(FLAGS.precision)
    if FLAGS.self_ensemble:
        generator = ensemble.Ensembled(generator)
    names = image_arena.eval_image_names(FLAGS.hd_dir_path)
    if FLAGS.target_dir_path:
        os.makedirs(FLAGS.target_dir_path, exist_ok=True)
    scores = torch.empty((len(names), 2, 2), dtype=torch.float32, device=device)
    if FLAGS.pairs == 'device':
        eval_set = datasets.DeviceEvalSet(FLAGS.hd_dir_path, device, names=names)
        eval_set.evaluate(generator, out=scores)
        for name, (sd, bq, _) in zip(names, eval_set.views if FLAGS.target_dir_path else ()):
            _write_pngs(FLAGS.target_dir_path, name, bq, generator.forward(sd, bq))
    else:
        for k, name in enumerate(names):
            sd, bq, hd = host_pair(image_arena.decode_rgb(os.path.join(FLAGS.hd_dir_path, name)), device, name)
            sr = generator.forward(sd, bq)
            ops.image_scores(hd, [bq, sr], 1.0, space='rgb', unit_clip=True, out=scores[k].view(2, 1, 2))
            if FLAGS.target_dir_path:
                _write_pngs(FLAGS.target_dir_path, name, bq, sr)
    return image_arena.report_bq_sr_scores(names, scores, FLAGS.hd_dir_path)


def main(argv=None):
    return evaluate_images(parse_flags(argv))


if __name__ == '__main__':
    main()
