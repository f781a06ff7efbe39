"""
image_arena.py -- what the device-side batch samplers (VDSR, ESPCN, EnhanceNet, SRCNN) share on the host: the packing of
decoded images into one uint8 arena and the base of their resident image sets.  Which images a set keeps or refuses, and
what a sampler draws, stays with each model.
"""
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
