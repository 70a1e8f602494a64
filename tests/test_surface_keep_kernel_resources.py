"""Register, scratch and LDS footprint of the kernels of option "surface_keep", from the compiler's device listing: the fixture
and the metadata of tests/test_kernel_resources.py.  No GPU.

k_shade_lit is a streaming kernel in front of a light loop: four coalesced loads, then arithmetic on what they brought.  What
hides its one round trip is the number of waves, so it stays inside the 64 registers of eight waves per SIMD, and it owns
neither LDS nor scratch.  k_surface_store runs once per stop of the camera and slot: it may hold what it likes of the register
file, but a spill would turn its stores into scratch traffic."""
import pytest

from test_kernel_resources import _one, kernels  # noqa: F401  (the module-scoped fixture)

LIT_VGPR_MAX = 64


def test_k_shade_lit_footprint(kernels):  # noqa: F811
    k = _one(kernels, "_ZN3bbr11k_shade_litILb0EEE")
    print(f"k_shade_lit<false>: {k}")
    assert k["vgpr_count"] <= LIT_VGPR_MAX
    assert k["agpr_count"] == 0
    assert k["private_segment_fixed_size"] == 0, "k_shade_lit owns scratch"
    assert k["group_segment_fixed_size"] == 0, "k_shade_lit owns LDS"


@pytest.mark.parametrize("tile", [32, 64])
def test_k_surface_store_has_no_scratch(kernels, tile):  # noqa: F811
    k = _one(kernels, f"_ZN3bbr15k_surface_storeILi{tile}ELi{tile}EEE")
    print(f"k_surface_store<{tile},{tile}>: {k}")
    assert k["private_segment_fixed_size"] == 0, "k_surface_store owns scratch"
