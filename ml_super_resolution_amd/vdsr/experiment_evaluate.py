"""
experiment_evaluate.py -- mirror of vdsr/vdsr/experiment_evaluate.py: mean PSNR of (sd, sr) against
hd over a directory of images and the mean forward time per image (:64-123).  PSNR and SSIM use
max_val 2.0 on [-1,1] images as the reference does (:57-60); both are computed on the GPU.
--scores fused scores an image with one ops.image_scores call (hd against sd and sr) and fetches the
numbers once, after the loop; --scores separate (the default) makes the four calls of the reference.
--pairs device decodes the directory, uploads the bytes once and takes every image's (sd, hd) from a
dataset.DeviceEvalSet -- one launch for the whole directory (ops.vdsr_eval_pairs) -- where --pairs host (the
default) runs load_image per image: a scipy blur, two map_coordinates per channel and two float uploads.
--self_ensemble scores VdsrModel.forward_ensemble(sd) -- the mean over the eight flips / transposes of sd
(ensemble.py) -- in place of forward(sd); sd's own scores do not change.

  python -m ml_super_resolution_amd.vdsr.experiment_evaluate --ckpt_path model.ckpt-25600.pt \
         --hd_image_dir_path Set5 --scaling_factor 2
"""
import argparse
import os
import time

import numpy as np
import torch

from .. import image_arena, ops
from . import dataset, model_vdsr


def load_image(path, scaling_factor):
    """experiment_evaluate.py:14-33: read, to float [0,1], degrade, map both to [-1,1], batch of 1."""
    hd = image_arena.decode_rgb(path).astype(np.float32) / 255.0
    sd = dataset.hd_image_to_sd_image(hd, scaling_factor)
    return (sd * 2.0 - 1.0)[None].astype(np.float32), (hd * 2.0 - 1.0)[None].astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--meta_path', default=None)       # accepted for flag compatibility; unused
    ap.add_argument('--ckpt_path', required=True)
    ap.add_argument('--hd_image_dir_path', required=True)
    ap.add_argument('--scaling_factor', type=int, default=2)
    ap.add_argument('--num_layers', type=int, default=20)
    # not a flag of the reference: 'high' runs the 3x3 64 -> 64 body layers on bf16x3 products (include/srx.h)
    ap.add_argument('--precision', choices=('highest', 'high'), default='highest')
    # not a flag of the reference: 'fused' scores (hd, [sd, sr]) in one call per image and crosses to the host once
    ap.add_argument('--scores', choices=('separate', 'fused'), default='separate')
    # not a flag of the reference: 'device' builds every image's (sd, hd) in one launch from the uploaded bytes
    ap.add_argument('--pairs', choices=('host', 'device'), default='host')
    # not a flag of the reference: geometric self-ensemble -- the mean over the eight flips / transposes (ensemble.py)
    ap.add_argument('--self_ensemble', action='store_true')
    FLAGS = ap.parse_args(argv)
    device = torch.device('cuda')
    model = model_vdsr.VdsrModel(FLAGS.num_layers, device=device, precision=FLAGS.precision)
    model.stack.load_checkpoint(FLAGS.ckpt_path)      # TF V2 prefix (reference checkpoints) or .pt
    forward = model.forward_ensemble if FLAGS.self_ensemble else model.forward
    names = image_arena.eval_image_names(FLAGS.hd_image_dir_path)
    sd_psnrs, sr_psnrs, sd_ssims, sr_ssims, total = [], [], [], [], 0.0
    fused = []                                         # per image [2 (sd, sr), 1, 2 (psnr, ssim)], on the device
    eval_set = None
    if FLAGS.pairs == 'device' and names:
        images = [image_arena.decode_rgb(os.path.join(FLAGS.hd_image_dir_path, n)) for n in names]
        eval_set = dataset.DeviceEvalSet(images, [FLAGS.scaling_factor], device, names=names)
    for k, n in enumerate(names):
        if eval_set is not None:
            sd, hd = eval_set.views[k]
        else:
            sd_np, hd_np = load_image(os.path.join(FLAGS.hd_image_dir_path, n), FLAGS.scaling_factor)
            sd, hd = torch.from_numpy(sd_np).to(device), torch.from_numpy(hd_np).to(device)
        torch.cuda.synchronize()
        t0 = time.time()
        sr = forward(sd)
        torch.cuda.synchronize()
        total += time.time() - t0
        if FLAGS.scores == 'fused':
            fused.append(ops.image_scores(hd, [sd, sr], 2.0))
            continue
        sd_psnrs.append(ops.psnr(hd, sd, 2.0).item())
        sr_psnrs.append(ops.psnr(hd, sr, 2.0).item())
        sd_ssims.append(ops.ssim(hd, sd, 2.0).item())
        sr_ssims.append(ops.ssim(hd, sr, 2.0).item())
    if fused:
        got = torch.stack(fused).cpu().numpy().astype(np.float64)          # the one copy to the host
        sd_psnrs, sr_psnrs = got[:, 0, 0, 0].tolist(), got[:, 1, 0, 0].tolist()
        sd_ssims, sr_ssims = got[:, 0, 0, 1].tolist(), got[:, 1, 0, 1].tolist()
    print('x{}'.format(FLAGS.scaling_factor))
    print('time (s)     : {}'.format(total / max(len(names), 1)))
    print('psnr (sd, sr): {}, {}'.format(np.mean(sd_psnrs), np.mean(sr_psnrs)))
    print('ssim (sd, sr): {}, {}'.format(np.mean(sd_ssims), np.mean(sr_ssims)))
    return {'names': names, 'sd_psnrs': sd_psnrs, 'sr_psnrs': sr_psnrs, 'sd_ssims': sd_ssims, 'sr_ssims': sr_ssims,
            'time': total / max(len(names), 1)}


if __name__ == '__main__':
    main()
