"""Register, scratch and LDS footprint of the bloom kernels (option "bloom"), from the compiler's device listing: the fixture
and the metadata of tests/test_kernel_resources.py.  No GPU.

The four are streaming kernels that wait for memory: what they hold of the register file decides how many of their waves
hide that wait.  64 registers is the allocation step of eight waves per SIMD; k_resolve<n, true>, which carries the same
present_pixel as k_present_bloom, stays inside it."""
import pytest

from test_kernel_resources import _one, kernels  # noqa: F401  (the module-scoped fixture)

BLOOM_VGPR_MAX = 64
# k_present_bloom's header comment: the sRGB tables and nothing else -- 256 thresholds of 4 bytes and the 13 x 256 keyed bytes
PRESENT_BLOOM_LDS = 256 * 4 + 13 * 256

KERNELS = {"k_bloom_first": "_ZN3bbr13k_bloom_firstE", "k_bloom_down": "_ZN3bbr12k_bloom_downE", "k_bloom_up": "_ZN3bbr10k_bloom_upE",
           "k_present_bloom": "_ZN3bbr15k_present_bloomE"}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_bloom_kernel_footprint(kernels, name):  # noqa: F811
    k = _one(kernels, KERNELS[name])
    print(f"{name}: {k}")
    assert k["private_segment_fixed_size"] == 0, f"{name} owns scratch"
    assert k["agpr_count"] == 0
    assert k["vgpr_count"] <= BLOOM_VGPR_MAX
    assert k["group_segment_fixed_size"] == (PRESENT_BLOOM_LDS if name == "k_present_bloom" else 0)


def test_the_resolve_that_presents_meets_the_same_bound(kernels):  # noqa: F811
    for n in (2, 3, 4):
        assert _one(kernels, f"_ZN3bbr9k_resolveILi{n}ELb1EEE")["vgpr_count"] <= BLOOM_VGPR_MAX
