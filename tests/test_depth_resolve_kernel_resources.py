"""Register, scratch and LDS footprint of k_resolve_depth (option "depth_resolve"), from the compiler's own device listing, built
the way tests/test_kernel_resources.py builds it (its fixture, compiled once more for this module).  No GPU is needed.

k_resolve_depth is a streaming kernel like k_resolve: a lane holds one fine row of its pixel's depths at a time, the best so
far and its index.  Every instantiation -- n = 2, 3, 4; SAMPLE_ZERO (1), MIN (4), MAX (8); the plain form and the dumping one
-- owns no scratch and no LDS and stays at or under 64 registers, the allocation step of eight waves per SIMD.

Counts of the listing this was written against (vector registers, plain / dumping form):
    n = 2   SAMPLE_ZERO 4 / 6    MIN 10 / 11    MAX 10 / 11
    n = 3   SAMPLE_ZERO 4 / 6    MIN  9 / 15    MAX  9 / 15
    n = 4   SAMPLE_ZERO 4 / 6    MIN 10 / 17    MAX 10 / 17"""
import pytest

from test_kernel_resources import _one, kernels  # noqa: F401  (the fixture)

RESOLVE_DEPTH_VGPR_MAX = 64


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("mode", [1, 4, 8])
@pytest.mark.parametrize("prim", [0, 1])
def test_k_resolve_depth_footprint(kernels, n, mode, prim):  # noqa: F811
    k = _one(kernels, f"_ZN3bbr15k_resolve_depthILi{n}ELi{mode}ELb{prim}EEE")
    print(f"k_resolve_depth<{n},{mode},{prim}>: {k}")
    assert k["private_segment_fixed_size"] == 0, "k_resolve_depth owns scratch"
    assert k["group_segment_fixed_size"] == 0, "k_resolve_depth owns LDS"
    assert k["vgpr_count"] + k["agpr_count"] <= RESOLVE_DEPTH_VGPR_MAX


def test_every_instantiation_is_there(kernels):  # noqa: F811
    names = [n for n in kernels if n.startswith("_ZN3bbr15k_resolve_depthILi")]
    assert len(names) == 18, names
