"""
make_pin_p8.py -- P8: the reference's own feature-map figures pin the mosaic encoder (srx_feature_mosaic_u8).

BUILD CONTAINER ONLY (reads /root/reference/assets, which does not travel).  Output: DATA only (uint8 pixel crops of the
reference's PNGs and two hashes of their pixels; no reference source text):

  tests/golden/pin_p8_fig2_mosaic.npz    for layers 1, 2, 10 and 19: 'conv%d' [4, 8, 8, 24, 24] uint8 -- for each image
                                         corner (top-left, top-right, bottom-left, bottom-right, the order of P7's
                                         corners) the 24 x 24 crop of each of the 8 x 8 tiles, cut by PLAIN SLICING of
                                         the mosaic PNG: tile (r, c) is png[r*256 : (r+1)*256, c*256 : (c+1)*256].  No
                                         reshape, no transpose: the layout under test is not restated here.
  tests/golden/pin_p8_fig2_mosaic.json   sha256 of the [2048, 2048] pixel bytes of vdsr-fig2-conv.1.png and conv.19.png,
                                         and the image side.

What the pins say: P7's fixtures hold the same maps channel-last (pin_p7_vdsr_fig2.npz corners, pin_p7_layer1_full.npz,
pin_p7_layer20_full.npz).  Decoding those bytes to the midpoints of their intervals and encoding them again is the
identity on all 256 codes, so an encoder that lays channel k at tile (k // 8, k % 8) must reproduce the PNGs: the two
whole images by hash, the corners of four layers by value.

Run:  python tests/golden/make_pin_p8.py     (seconds)
"""
import hashlib
import json
import os
import sys

import numpy as np
from PIL import Image

ASSETS = '/root/reference/assets'
HERE = os.path.dirname(os.path.abspath(__file__))
C = 24                      # side of a corner crop (P7's)
S = 256                     # image side
LAYERS = (1, 2, 10, 19)
# sha256 of the pixel bytes, as measured when the pin was designed: a different asset must not pass silently
EXPECT = {
    'conv1': '1eb04609d94dcf8792ff4debff4137f8ef3876b5860a1c3b9fbdcd349c84f374',
    'conv19': '737aaa956bd1786f7f3c3744d3a1ad28f1cff026bec616f8e81e3d940eda165f',
}


def main():
    out, hashes = {}, {}
    for n in LAYERS:
        png = np.asarray(Image.open(os.path.join(ASSETS, 'vdsr-fig2-conv.%d.png' % n)))
        assert png.shape == (8 * S, 8 * S) and png.dtype == np.uint8, (n, png.shape, png.dtype)
        crops = np.zeros((4, 8, 8, C, C), np.uint8)
        for k, (y0, x0) in enumerate(((0, 0), (0, S - C), (S - C, 0), (S - C, S - C))):
            for r in range(8):
                for c in range(8):
                    crops[k, r, c] = png[r * S + y0:r * S + y0 + C, c * S + x0:c * S + x0 + C]
        out['conv%d' % n] = crops
        if 'conv%d' % n in EXPECT:
            hashes['conv%d' % n] = hashlib.sha256(np.ascontiguousarray(png).tobytes()).hexdigest()
    assert hashes == EXPECT, hashes
    dst = os.path.join(HERE, 'pin_p8_fig2_mosaic.npz')
    np.savez_compressed(dst, **out)
    print('wrote', dst, os.path.getsize(dst), 'bytes')
    dst = os.path.join(HERE, 'pin_p8_fig2_mosaic.json')
    with open(dst, 'w') as f:
        json.dump({'side': S, 'sha256': hashes}, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', dst)


if __name__ == '__main__':
    sys.exit(main())
