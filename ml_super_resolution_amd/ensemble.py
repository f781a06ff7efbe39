"""Geometric self-ensemble inference (the "+" variants of the super-resolution literature): the model runs on the eight
flips and transposes of its input, each result is transformed back, and the eight are averaged.  No retraining, any
checkpoint.  Not part of the reference.

The transforms and their average are one launch each (ops.dihedral_expand / ops.dihedral_merge; include/srx.h); the
eight forward passes are two batched calls: the four images that keep the input's shape (group A) and the four
transposed ones (group B)."""
from . import ops


def self_ensemble(fn, *inputs):
    """fn(*inputs) averaged over the dihedral group.  inputs: [N,H,W,C] device tensors (C <= 8), all transformed
    alike -- EnhanceNet takes two, at different sizes; fn maps batches to a batch [., h, w, c] and must commute with
    the transforms up to its weights (any convolutional net with square kernels and symmetric padding or cropping).
    Returns [N,h,w,c].

    The models here return buffers they own and overwrite on the next call of the same shape, which for square images
    is the B call: the A result is copied before fn runs again.  Two calls of 4N images, never one of 8N: every image
    then takes the route -- and so gets the bits -- that a plain batch of 4N takes."""
    if not inputs:
        raise ValueError('self_ensemble: no input')
    groups = [ops.dihedral_expand(x.contiguous()) for x in inputs]
    ya = fn(*[g[0] for g in groups]).clone()
    yb = fn(*[g[1] for g in groups])
    return ops.dihedral_merge(ya.contiguous(), yb.contiguous())


class Ensembled(object):
    """A model seen through its self-ensemble: `forward` is the model's `forward_ensemble`, everything else is the
    model's own.  What the evaluation sets take where they take a model."""

    def __init__(self, model):
        self._model = model

    def forward(self, *inputs):
        return self._model.forward_ensemble(*inputs)

    def __getattr__(self, name):
        return getattr(self._model, name)
