"""The eight dihedral transforms of an image, and what srx_dihedral_expand / srx_dihedral_merge compute, in numpy
(include/srx.h).  Images are [H,W,C], batches [N,H,W,C]; T and T_inv take either (the two image axes are the two
before the last)."""
import numpy as np


def T(k, x):
    """T_k(x) = flipH^(k&1)( flipV^((k>>1)&1)( transpose^((k>>2)&1)(x) ) )."""
    x = np.asarray(x)
    if k & 4:
        x = np.swapaxes(x, -3, -2)
    if k & 2:
        x = x[..., ::-1, :, :]
    if k & 1:
        x = x[..., :, ::-1, :]
    return x


def T_inv(k, y):
    """The inverse: the same steps undone in the opposite order."""
    y = np.asarray(y)
    if k & 1:
        y = y[..., :, ::-1, :]
    if k & 2:
        y = y[..., ::-1, :, :]
    if k & 4:
        y = np.swapaxes(y, -3, -2)
    return y


def expand_ref(x):
    """x [N,H,W,C] -> (a [4N,H,W,C], b [4N,W,H,C]), transform-major."""
    x = np.asarray(x)
    a = np.ascontiguousarray(np.concatenate([T(k, x) for k in range(4)]))
    b = np.ascontiguousarray(np.concatenate([T(k, x) for k in range(4, 8)]))
    return a, b


def merge_ref(a, b):
    """a [4N,H,W,C], b [4N,W,H,C] -> [N,H,W,C]: float32 adds of the eight inverses in the order 0..7, then * 0.125."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n = a.shape[0] // 4
    assert a.shape[0] == b.shape[0] == 4 * n and a.shape[1:] == (b.shape[2], b.shape[1], b.shape[3])
    acc = None
    for k in range(8):
        g = a if k < 4 else b
        u = np.ascontiguousarray(T_inv(k, g[(k & 3) * n:(k & 3) * n + n]), dtype=np.float32)
        acc = u if acc is None else (acc + u).astype(np.float32)
    return (acc * np.float32(0.125)).astype(np.float32)
