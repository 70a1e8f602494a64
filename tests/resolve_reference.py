"""numpy model of the resolve of option "supersample" (include/bibim_hip.h): the n x n samples of an
output pixel are added one after the other in binary32, first sample first, row-major (i fastest), then multiplied once by
R[n].  No fused operation anywhere: numpy's float32 add and multiply are the IEEE ones."""
import numpy as np

F = np.float32
# R[1] = 1, R[2] = 0.25f, R[3] = the binary32 nearest 1/9, R[4] = 0.0625f
R = {1: F(1.0), 2: F(0.25), 3: F(1.0) / F(9.0), 4: F(0.0625)}
assert R[3].view(np.uint32) == 0x3DE38E39


def sample_order(n):
    """(i, j) of the samples in the order they are added: row-major, i (x) fastest"""
    return [(i, j) for j in range(n) for i in range(n)]


def resolve(fine, n, order=None):
    """fine [n*H, n*W, C] float32 -> [H, W, C] float32.  `order`: another order of the samples (the tests permute it to
    show that the order is observable); default sample_order(n)."""
    fine = np.ascontiguousarray(fine, F)
    assert fine.ndim == 3 and fine.shape[0] % n == 0 and fine.shape[1] % n == 0
    if n == 1:
        return fine.copy()
    order = sample_order(n) if order is None else list(order)
    assert sorted(order) == sorted(sample_order(n))
    with np.errstate(invalid="ignore", over="ignore"):
        i0, j0 = order[0]
        acc = fine[j0::n, i0::n].copy()
        for i, j in order[1:]:
            acc = acc + fine[j::n, i::n]        # float32 + float32: one rounding per addition
        return (acc * R[n]).astype(F, copy=False)
