"""Register, scratch and LDS footprint of k_shade_shadow_casters (bbr_render_shadow_caster), from the compiler's own device
listing, built the way tests/test_kernel_resources.py builds it (its fixture, compiled once more for this module).  No GPU is
needed.

k_shade_shadow_casters is k_shade_aniso's fragment stage plus a uniform loop over the eight caster slots round the face loop of
k_shade_shadow_pcf; the number of casters, F and R are run-time scalars, so there are 16 instantiations -- both tile shapes,
forward and deferred, fp32 and presented output, the shipped form and the dumping one.  Each owns no scratch and no LDS and stays
at or under 128 vector registers, the allocation step of the four waves per SIMD k_shade_shadow_pcf lives at (ANISO_VGPR_MAX)."""
import pytest

from test_kernel_resources import ANISO_VGPR_MAX, _one, kernels  # noqa: F401  (the fixture)


@pytest.mark.parametrize("dump", [0, 1])
@pytest.mark.parametrize("present", [0, 1])
@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("tile", [32, 64])
def test_k_shade_shadow_casters_footprint(kernels, tile, deferred, present, dump):  # noqa: F811
    k = _one(kernels, f"_ZN3bbr22k_shade_shadow_castersILi{tile}ELi{tile}ELb{deferred}ELb{present}ELb{dump}EEE")
    print(f"k_shade_shadow_casters<{tile},{tile},{deferred},{present},{dump}>: {k}")
    assert k["private_segment_fixed_size"] == 0, "k_shade_shadow_casters owns scratch"
    assert k["group_segment_fixed_size"] == 0, "k_shade_shadow_casters owns LDS"
    assert k["vgpr_count"] + k["agpr_count"] <= ANISO_VGPR_MAX


def test_every_instantiation_is_there(kernels):  # noqa: F811
    names = [n for n in kernels if n.startswith("_ZN3bbr22k_shade_shadow_castersILi")]
    assert len(names) == 16, names
