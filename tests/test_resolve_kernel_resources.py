"""Register, scratch and LDS footprint of k_resolve (option "supersample"), from the compiler's own device listing, built the
way tests/test_kernel_resources.py builds it (its fixture, compiled once more for this module).  No GPU is needed.

k_resolve is a streaming kernel: nothing it loads is used twice, so it has no reason to hold more than one fine row of its
pixel at a time.  Both forms, every n: no scratch; no LDS in the fp32 form and the sRGB tables alone in the PRESENT form; at
most 64 registers, the allocation step of eight waves per SIMD."""
import pytest

from test_kernel_resources import _one, kernels  # noqa: F401  (the fixture)

RESOLVE_VGPR_MAX = 64
SRGB_TABLES_BYTES = 256 * 4 + 13 * 256      # sizeof(SrgbTables): float thr[256] + uint8_t lut[13 * 256]


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("present", [0, 1])
def test_k_resolve_footprint(kernels, n, present):  # noqa: F811
    k = _one(kernels, f"_ZN3bbr9k_resolveILi{n}ELb{present}EEE")
    print(f"k_resolve<{n},{present}>: {k}")
    assert k["private_segment_fixed_size"] == 0, "k_resolve owns scratch"
    if present:
        lds = k["group_segment_fixed_size"]
        assert SRGB_TABLES_BYTES <= lds < SRGB_TABLES_BYTES + 16      # the tables, rounded up to the allocation's alignment
    else:
        assert k["group_segment_fixed_size"] == 0
    assert k["vgpr_count"] + k["agpr_count"] <= RESOLVE_VGPR_MAX
