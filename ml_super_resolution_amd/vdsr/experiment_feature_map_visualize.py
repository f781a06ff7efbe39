"""
experiment_feature_map_visualize.py -- mirror of vdsr/vdsr/experiment_feature_map_visualize.py: degrade one image,
super-resolve it and write what every layer produced: sd_image.png, sr_image.png, conv.N.png / relu.N.png (the 64 maps
of layer N as an 8 x 8 mosaic, :80-110) and conv.<num_layers>.png (the residual), every byte encoded as
tf.saturate_cast(x * 127.5 + 127.5, uint8) (:73,106).  The mosaics are built on the device (srx_feature_mosaic_u8):
only bytes cross to the host.

  python -m ml_super_resolution_amd.vdsr.experiment_feature_map_visualize --ckpt_path model.ckpt-25600 \
         --hd_image_path in.png --result_dir_path maps/ --scaling_factor 2
"""
import argparse
import os

import numpy as np
import torch

from . import dataset, model_vdsr


def load_sd_images(hd_image_path, scaling_factor):
    """[1,H,W,3] float32 in [-1,+1]: the degraded image (load_sd_images, :13-32)."""
    from PIL import Image
    hd = np.asarray(Image.open(hd_image_path).convert('RGB')).astype(np.float32) / 255.0
    sd = dataset.hd_image_to_sd_image(hd, scaling_factor)
    return (sd * 2.0 - 1.0)[None].astype(np.float32)


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument('--meta_path', default=None)
    ap.add_argument('--ckpt_path', required=True)
    ap.add_argument('--hd_image_path', required=True)
    ap.add_argument('--result_dir_path', required=True)
    ap.add_argument('--scaling_factor', type=int, default=2)
    # not flags of the reference: it reads the depth from the meta graph; 'high' runs the body layers on bf16x3 products
    ap.add_argument('--num_layers', type=int, default=20)
    ap.add_argument('--precision', choices=('highest', 'high'), default='highest')
    FLAGS = ap.parse_args(argv)
    device = torch.device('cuda')
    model = model_vdsr.VdsrModel(FLAGS.num_layers, device=device, precision=FLAGS.precision)
    model.stack.load_checkpoint(FLAGS.ckpt_path)      # TF V2 prefix (reference checkpoints) or .pt
    sd_images = torch.from_numpy(load_sd_images(FLAGS.hd_image_path, FLAGS.scaling_factor)).to(device)
    maps = model.feature_maps(sd_images)
    os.makedirs(FLAGS.result_dir_path, exist_ok=True)
    host = {}
    for key, u8 in maps.items():
        # 'conv.3:0' -> conv.3.png (build_feature_maps, :121-158); conv.N and relu.N are one tensor: copied once, written twice
        if id(u8) not in host:
            host[id(u8)] = Image.fromarray(u8[0].cpu().numpy())
        name = key[:-2] if key.endswith(':0') else key
        host[id(u8)].save(os.path.join(FLAGS.result_dir_path, name + '.png'))


if __name__ == '__main__':
    main()
