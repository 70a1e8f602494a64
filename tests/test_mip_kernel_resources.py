"""Register and scratch footprint of the mip kernels (option "mip_levels"), from the compiler's own device listing, built
the way tests/test_kernel_resources.py builds it (its fixture, compiled once more for this module).  No GPU is needed.

k_shade_mip holds level d's filtered channels while it runs the tap loop of level d + 1: it must still fit the 128-register
allocation step of four waves per SIMD that k_shade_aniso runs at, without scratch and without LDS."""
import pytest

from test_kernel_resources import _one, kernels  # noqa: F401  (the fixture)

MIP_VGPR_MAX = 128


@pytest.mark.parametrize("deferred,present", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_k_shade_mip_fits_four_waves(kernels, deferred, present):  # noqa: F811
    k = _one(kernels, f"_ZN3bbr11k_shade_mipILi32ELi32ELb{deferred}ELb{present}ELb0EEE")
    print(f"k_shade_mip<32,32,{deferred},{present},false>: {k}")
    assert k["private_segment_fixed_size"] == 0, "k_shade_mip owns scratch"
    assert k["group_segment_fixed_size"] == 0
    assert k["vgpr_count"] + k["agpr_count"] <= MIP_VGPR_MAX


@pytest.mark.parametrize("name", ["_ZN3bbr12k_mip_reduceE", "_ZN3bbr10k_mip_packE"])
def test_chain_kernels_have_no_scratch(kernels, name):  # noqa: F811
    k = _one(kernels, name)
    print(f"{name}: {k}")
    assert k["private_segment_fixed_size"] == 0
