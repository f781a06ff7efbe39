"""What the tests of the four device batch samplers (VDSR, ESPCN, EnhanceNet, SRCNN) share: tables of srx_patch_src
records over an arena of images given by their (height, width) shapes, and the geometry rows of the BAD lists -- the
refusals every srx_*_patch_table_check owes to the one check they share.  A plain module, imported by the test files."""
import numpy as np


def offsets_of(shapes):
    """(byte offset of each image, the arena's byte count) for [h, w, 3] uint8 images packed back to back."""
    sizes = [h * w * 3 for h, w in shapes]
    return [int(v) for v in np.cumsum([0] + sizes[:-1])], int(sum(sizes))


def entry_for(shapes, default_factor):
    """entry(image, x, y, flip=0, factor=default_factor): one record, as a tuple in PATCH_SRC_DTYPE's field order, on image
    `image` of an arena of `shapes`."""
    offs, _ = offsets_of(shapes)

    def entry(image, x, y, flip=0, factor=default_factor):
        h, w = shapes[image]
        return (offs[image], w, h, x, y, flip, float(factor))
    return entry


def table_of(entries):
    from ml_super_resolution_amd import ops
    return np.array(entries, dtype=ops.PATCH_SRC_DTYPE)


def bad_geometry_rows(shapes, side, factor, letter='S'):
    """The rows (name, the bad entry, arena_bytes) every sampler's BAD list starts with, for a crop or patch of `side`
    (called `letter` in the names) on the second image of `shapes`, the arena's end tested on the last: each differs from
    a valid entry in ONE respect of the geometry."""
    entry = entry_for(shapes, factor)
    offs, total = offsets_of(shapes)
    last = len(shapes) - 1
    (h1, w1), (hl, wl) = shapes[1], shapes[last]
    factor = float(factor)
    return [
        ('x < 0', entry(1, -1, 0), total),
        ('y < 0', entry(1, 0, -1), total),
        ('x + %s > width' % letter, entry(1, w1 - side + 1, 0), total),
        ('y + %s > height' % letter, entry(1, 0, h1 - side + 1), total),
        ('x + %s overflows int32' % letter, entry(1, 2 ** 31 - 1, 0), total),
        ('image ends one byte past the arena', entry(last, 0, 0), total - 1),
        ('offset one byte too far', (offs[last] + 1, wl, hl, 0, 0, 0, factor), total),
        ('offset + size wraps around 2^64', (2 ** 64 - 1, w1, h1, 0, 0, 0, factor), total),
        ('width * height * 3 far above the arena', (offs[1], 2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 0, factor), total),
        ('zero width', (offs[1], 0, h1, 0, 0, 0, factor), total),
    ]
