"""numpy model of option "depth_resolve" (include/bibim_hip.h): which sample of an output pixel's n x n
block gives the pixel its depth and its winning primitive.  The block of output pixel (x, y) is the fine pixels (nx + i, ny + j)
and k = j * n + i, as in resolve_reference.py.  Depths are compared as the unsigned 32-bit integers their bit patterns are:

  SAMPLE_ZERO  k* = 0
  MIN          k* = the first k, in index order, whose bit pattern is smallest
  MAX          k* = the first k, in index order, whose bit pattern is largest

numpy's argmin / argmax return the first occurrence, which is the tie rule.  The values are Vulkan's VkResolveModeFlagBits."""
import numpy as np

NONE, SAMPLE_ZERO, AVERAGE, MIN, MAX = 0, 1, 2, 4, 8
MODES = (SAMPLE_ZERO, MIN, MAX)
NAMES = {SAMPLE_ZERO: "zero", MIN: "min", MAX: "max"}
NO_PRIM = np.uint32(0xFFFFFFFF)


def bits(depth):
    """float32 depths as the uint32 the rule compares (a uint32 array passes through)"""
    depth = np.ascontiguousarray(depth)
    if depth.dtype == np.uint32:
        return depth
    assert depth.dtype == np.float32, depth.dtype
    return depth.view(np.uint32)


def blocks(fine, n):
    """[n*H, n*W] -> [H, W, n*n], sample k = j * n + i of the block last"""
    fine = np.ascontiguousarray(fine)
    assert fine.ndim == 2 and fine.shape[0] % n == 0 and fine.shape[1] % n == 0, (fine.shape, n)
    h, w = fine.shape[0] // n, fine.shape[1] // n
    return fine.reshape(h, n, w, n).transpose(0, 2, 1, 3).reshape(h, w, n * n)


def select(fine_depth, n, mode):
    """k* of every output pixel: [H, W] int64"""
    b = blocks(bits(fine_depth), n)
    if mode == SAMPLE_ZERO:
        return np.zeros(b.shape[:2], np.int64)
    if mode == MIN:
        return b.argmin(axis=2)
    if mode == MAX:
        return b.argmax(axis=2)
    raise ValueError(f"depth_resolve {mode}: no sample is selected (0 keeps no depth, 2 is an average)")


def resolve(fine_depth, fine_prim, n, mode):
    """(fine depth float32 [n*H, n*W], fine winners uint32 or None) -> (depth float32 [H, W], winners uint32 [H, W] or None):
    the bit pattern and the winner of sample k*.  n = 1 is the identity in every mode."""
    k = select(fine_depth, n, mode)[..., None]
    depth = np.take_along_axis(blocks(bits(fine_depth), n), k, axis=2)[..., 0].view(np.float32)
    prim = None
    if fine_prim is not None:
        prim = np.take_along_axis(blocks(np.ascontiguousarray(fine_prim, np.uint32), n), k, axis=2)[..., 0]
    return np.ascontiguousarray(depth), prim
