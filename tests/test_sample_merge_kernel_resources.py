"""Register, scratch and LDS footprint of the two kernels of option "sample_shading" 0, from the compiler's own device
listing, built the way tests/test_kernel_resources.py builds it (its fixture, compiled once more for this module).  No GPU
is needed.

k_resolve_merged is k_resolve with one more load per pixel: a streaming kernel that holds one fine row of its block at a
time.  Both forms, n = 2 and 4: no scratch; no LDS in the fp32 form and the sRGB tables alone in the PRESENT form; at most 64
registers, the allocation step of eight waves per SIMD.

k_sample_merge keeps a tile's list in registers (4 words per thread at 32 x 32 tiles, 16 at 64 x 64) and the winners in LDS:
no scratch, and LDS = the primitive array (4 bytes per fine pixel of the tile) + the staging it declares: the tile's map words
(2 bytes per output pixel at n = 2, 8 at n = 4), one count per run of 64 list words, and the list's first word."""
import pytest

from test_kernel_resources import _one, kernels  # noqa: F401  (the fixture)

RESOLVE_VGPR_MAX = 64
SRGB_TABLES_BYTES = 256 * 4 + 13 * 256      # sizeof(SrgbTables): float thr[256] + uint8_t lut[13 * 256]
MAP_WORD_BYTES = {2: 2, 4: 8}               # a 4-bit field per sample


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("present", [0, 1])
def test_k_resolve_merged_footprint(kernels, n, present):  # noqa: F811
    k = _one(kernels, f"_ZN3bbr16k_resolve_mergedILi{n}ELb{present}EEE")
    print(f"k_resolve_merged<{n},{present}>: {k}")
    assert k["private_segment_fixed_size"] == 0, "k_resolve_merged owns scratch"
    if present:
        lds = k["group_segment_fixed_size"]
        assert SRGB_TABLES_BYTES <= lds < SRGB_TABLES_BYTES + 16      # the tables, rounded up to the allocation's alignment
    else:
        assert k["group_segment_fixed_size"] == 0
    assert k["vgpr_count"] + k["agpr_count"] <= RESOLVE_VGPR_MAX


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("tile", [32, 64])
def test_k_sample_merge_footprint(kernels, tile, n):  # noqa: F811
    k = _one(kernels, f"_ZN3bbr14k_sample_mergeILi{tile}ELi{tile}ELi{n}EEE")
    print(f"k_sample_merge<{tile},{tile},{n}>: {k}")
    assert k["private_segment_fixed_size"] == 0, "k_sample_merge owns scratch"
    pixels = tile * tile
    prim_array = 4 * pixels
    staging = (pixels // (n * n)) * MAP_WORD_BYTES[n] + 4 * (pixels // 64) + 8
    lds = k["group_segment_fixed_size"]
    assert prim_array + staging <= lds < prim_array + staging + 32    # (alignment of the four arrays)
    assert k["vgpr_count"] + k["agpr_count"] <= 128                   # four workgroups of 256 threads per CU at the least
