"""Register, scratch and LDS footprint of the auto exposure kernels (option "auto_exposure"), from the compiler's device
listing: the fixture and the metadata of tests/test_kernel_resources.py.  No GPU.

k_luminance and the two present kernels stream and wait for memory: 64 registers is the allocation step of eight waves per
SIMD.  k_luminance's LDS is what its header comment states, 257 words; the present kernels hold the sRGB tables as the
kernels they restate do."""
import pytest

from test_kernel_resources import _one, kernels  # noqa: F401  (the module-scoped fixture)

VGPR_MAX = 64
LUMINANCE_LDS = 257 * 4
TABLES_LDS = 256 * 4 + 13 * 256

KERNELS = {"k_luminance": "_ZN3bbr11k_luminanceE", "k_exposure": "_ZN3bbr10k_exposureE", "k_present_auto": "_ZN3bbr14k_present_autoE",
           "k_present_bloom_auto": "_ZN3bbr20k_present_bloom_autoE"}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_exposure_kernel_footprint(kernels, name):  # noqa: F811
    k = _one(kernels, KERNELS[name])
    print(f"{name}: {k}")
    assert k["private_segment_fixed_size"] == 0, f"{name} owns scratch"
    assert k["agpr_count"] == 0
    if name != "k_exposure":
        assert k["vgpr_count"] <= VGPR_MAX
    if name == "k_luminance":
        assert k["group_segment_fixed_size"] == LUMINANCE_LDS
    elif name != "k_exposure":
        assert k["group_segment_fixed_size"] == TABLES_LDS


def test_the_restated_present_kernels_keep_their_footprint(kernels):  # noqa: F811
    """present_body / present_bloom_body are shared: the plain kernels use no more than their _auto forms and the same LDS"""
    for plain, auto in [("_ZN3bbr9k_presentE", "k_present_auto"), ("_ZN3bbr15k_present_bloomE", "k_present_bloom_auto")]:
        a, b = _one(kernels, plain), _one(kernels, KERNELS[auto])
        assert a["group_segment_fixed_size"] == b["group_segment_fixed_size"] == TABLES_LDS
        assert a["vgpr_count"] <= VGPR_MAX and a["private_segment_fixed_size"] == 0
