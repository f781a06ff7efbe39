"""
experiment_video.py -- super-resolve a frame sequence: the image files of a directory, in name order, all of one size
(espcn/espcn/experiment_test.py:148-184 per frame; the reference resolves one image per process).  Frames travel as bytes
both ways and several are in flight (frames.FrameResolver); `--io float` runs experiment_test's per-frame route instead,
for A/B: both write the same files.

  python -m ml_super_resolution_amd.espcn.experiment_video --ckpt_path model.npz \
         --frames_dir_path frames/ --result_dir_path sr/ [--batch 1] [--depth 3] [--io bytes|float]

Or a YUV4MPEG2 stream of planar frames (y4m.py: 4:2:0, 4:2:2 or 4:4:4 at 8, 10 or 12 bits, by the stream's C tag) in and one
of the same format out, `-` for stdin / stdout, so that the run sits in a pipe between a decoder and an encoder; the planes
travel as they are and the colour conversion runs on the device (EspcnModel.super_resolve_yuv420 for 8-bit 4:2:0,
EspcnModel.super_resolve_yuv for the others).  The range is the stream's XCOLORRANGE tag when it has one, else --range:

  decoder ... | python -m ml_super_resolution_amd.espcn.experiment_video --ckpt_path model.npz \
         --y4m_path - --result_y4m_path - [--matrix bt601|bt709] [--range limited|full] [--batch 1] [--depth 3] | encoder ...
"""
import argparse
import itertools
import os
import sys
import time

import numpy as np

from .. import image_arena
from . import experiment_test, frames, model_espcn, y4m


def read_frames(dir_path, names):
    """The decoded frames, one at a time; a frame of another size than the first is refused by name."""
    size = None
    for name in names:
        image = image_arena.decode_rgb(os.path.join(dir_path, name))
        if size is None:
            size = image.shape
        elif image.shape != size:
            raise ValueError('%s is %s, the sequence began with %s' % (name, tuple(image.shape), tuple(size)))
        yield image


def resolve_y4m(FLAGS):
    """--y4m_path to --result_y4m_path: the header is read first, the frames are read into a small ring of host arrays as
    the resolver asks for them and written as they come back."""
    to_stdout = FLAGS.result_y4m_path == '-'
    src = sys.stdin.buffer if FLAGS.y4m_path == '-' else open(FLAGS.y4m_path, 'rb')
    dst = None
    try:
        header = y4m.read_header(src, formats=y4m.PLANAR_FORMATS)
        full_range = header.full_range if header.full_range is not None else FLAGS.range == 'full'
        model = model_espcn.build_test_model(FLAGS.meta_path, FLAGS.ckpt_path)
        m = model['_model']
        # 8-bit 4:2:0 keeps its own layout and kernels; every other format names itself
        layout = {'layout': 'yuv420'} if header.pixel_format == 'yuv420p' else {'layout': 'yuv', 'pixel_format': header.pixel_format}
        resolver = frames.FrameResolver(m, header.height, header.width, batch=FLAGS.batch, depth=FLAGS.depth,
                                        matrix=FLAGS.matrix, full_range=full_range, **layout)
        out_header = header.scaled(m.scaling_factor)
        dst = sys.stdout.buffer if to_stdout else open(FLAGS.result_y4m_path, 'wb')
        writer = y4m.Y4MWriter(dst, out_header)
        # a frame is copied into the pinned ring when its batch is uploaded, before the next batch is read
        ring = [np.empty((header.frame_bytes,), dtype=np.uint8) for _ in range(FLAGS.batch + 1)]
        began = time.perf_counter()
        for _, hr in resolver.resolve(y4m.read_frames(src, header, buffers=itertools.cycle(ring)), copy=False):
            writer.write(hr)
        dst.flush()
        seconds = time.perf_counter() - began
    finally:
        if src is not sys.stdin.buffer:
            src.close()
        if dst is not None and dst is not sys.stdout.buffer:
            dst.close()
    print('frames: {}, seconds: {:.3f}, io: y4m {}x{} -> {}x{}, matrix: {}, range: {}{}'.format(
        writer.frames, seconds, header.width, header.height, out_header.width, out_header.height, FLAGS.matrix,
        'full' if full_range else 'limited', '' if header.pixel_format == 'yuv420p' else ', format: ' + header.pixel_format),
        file=sys.stderr if to_stdout else sys.stdout)
    return {'frames': writer.frames, 'seconds': seconds, 'header': out_header, 'full_range': full_range}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--meta_path', default=None)
    ap.add_argument('--ckpt_path', required=True)
    ap.add_argument('--frames_dir_path', default=None)
    ap.add_argument('--result_dir_path', default=None)
    ap.add_argument('--y4m_path', default=None)
    ap.add_argument('--result_y4m_path', default=None)
    ap.add_argument('--matrix', choices=('bt601', 'bt709'), default='bt601')
    ap.add_argument('--range', choices=('limited', 'full'), default='limited')
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--depth', type=int, default=3)
    ap.add_argument('--io', choices=('bytes', 'float'), default='bytes')
    FLAGS = ap.parse_args(argv)
    if (FLAGS.frames_dir_path is None) == (FLAGS.y4m_path is None):
        ap.error('exactly one of --frames_dir_path and --y4m_path must be given')
    if FLAGS.y4m_path is not None:
        if FLAGS.result_y4m_path is None:
            ap.error('--y4m_path needs --result_y4m_path')
        return resolve_y4m(FLAGS)
    if FLAGS.result_dir_path is None:
        ap.error('--frames_dir_path needs --result_dir_path')
    from PIL import Image
    names = image_arena.eval_image_names(FLAGS.frames_dir_path)
    if not names:
        raise ValueError('no image file in %s' % FLAGS.frames_dir_path)
    model = model_espcn.build_test_model(FLAGS.meta_path, FLAGS.ckpt_path)
    os.makedirs(FLAGS.result_dir_path, exist_ok=True)

    def save(index, hr_u8):
        Image.fromarray(hr_u8).save(os.path.join(FLAGS.result_dir_path, os.path.splitext(names[index])[0] + '.png'))

    began = time.perf_counter()
    sequence = read_frames(FLAGS.frames_dir_path, names)
    if FLAGS.io == 'float':
        for index, image in enumerate(sequence):
            sr = experiment_test.super_resolve_array(model, image)
            save(index, (sr * 255.0 + 0.5).astype(np.uint8))              # experiment_test.py:85
    else:
        for index, hr_u8 in frames.resolve_frames(model['_model'], sequence, batch=FLAGS.batch, depth=FLAGS.depth, copy=False):
            save(index, hr_u8)
    seconds = time.perf_counter() - began
    print('frames: {}, seconds: {:.3f}, io: {}'.format(len(names), seconds, FLAGS.io))
    return {'names': names, 'frames': len(names), 'seconds': seconds}


if __name__ == '__main__':
    main()
