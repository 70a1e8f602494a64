"""The resolve rule of option "supersample" as tests/resolve_reference.py states it.  No GPU."""
import numpy as np
import pytest

import resolve_reference as RR
from bibim_renderer_amd import partition as P

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_one_sample_is_the_identity_on_bits():
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 2**32, (7, 5, 4), dtype=np.uint64).astype(np.uint32)   # every kind of bit pattern, NaN payloads included
    fine = raw.view(F)
    assert np.array_equal(bits(RR.resolve(fine, 1)), raw)


def constants(rng, count):
    """full 24-bit significands of both signs over a wide range of exponents, subnormals among them, below FLT_MAX / 16"""
    raw = rng.integers(0, 2**32, count, dtype=np.uint64).astype(np.uint32)
    c = raw.view(F).copy()
    c[~(np.abs(c) < F(2.0**123))] = F(1.5)                                     # (NaN, inf and what 16 c would overflow)
    c[:8] = (0.0, -0.0, 2.0**-149, -(2.0**-149), 2.0**-140 * 3, 65504.0, 2.0**-126, 1.0 + 2.0**-23)
    return c


@pytest.mark.parametrize("n", [2, 4])
def test_a_constant_block_resolves_to_the_constant(n):
    """n = 2: exactly, for EVERY finite constant c whose 4 c is finite.  c + c and 4 c are exact; 3 c rounds by at most half an
    ulp of 3 c, which is at most half an ulp of 4 c, and a tie goes to the even neighbour 4 c; 4 c x 0.25 is exact
    (subnormals: every sum of subnormal-spaced values is exact).  Full 24-bit significands, both signs, subnormals.

    n = 4: NOT for every c -- 3 c, 5 c, ... round and sixteen additions do not make up for it (two thirds of random 24-bit
    constants come back in another bit pattern).  Exactly where every partial sum k c, k <= 16, is a binary32 value: c of at
    most 20 significant bits (k adds at most four), which is what frames hold in flat regions -- alpha 0 and 1, clear
    colours, binary16 values.  The unrestricted figure is printed."""
    rng = np.random.default_rng(2)
    c = constants(rng, 3 * 5000 * 4)
    if n == 4:
        full = c.reshape(3, 5000, 4)
        fine = np.repeat(np.repeat(full, n, axis=0), n, axis=1)
        print("n = 4, full 24-bit constants that do not come back bit for bit:",
              float((bits(RR.resolve(fine, n)) != bits(full)).mean()))
        c = (c.view(np.uint32) & np.uint32(0xFFFFFFF0)).view(F)                # 20 significant bits
    const = c.reshape(3, 5000, 4)
    fine = np.repeat(np.repeat(const, n, axis=0), n, axis=1)
    assert np.array_equal(bits(RR.resolve(fine, n)), bits(const))


def test_three_by_three_is_within_one_ulp_of_the_mean():
    """Where the bound of one ulp is a theorem: nine samples of one sign whose partial sums are binary32 values (here: integers
    below 2^20 times one power of two per pixel, so every sum stays below 2^24 units).  The additions are then exact and
    two roundings are left: R[3] = (1/9)(1 + 2^-27) and the product, half an ulp -- at most 0.75 ulp of the mean together.

    On general one-sign inputs the pinned sequence does NOT stay within one ulp: each of the eight additions may round by
    2^-24 of a partial sum that is at most the total, so the bound is (8 + 1/8 + 1) * 2^-24 relative, 9.125 ulp of the mean
    at worst; the uniform samples in [1e-3, 1e3) below measure 2.55 and 3.0 ulp.  That bound is asserted for them, and the
    figure printed."""
    rng = np.random.default_rng(3)

    def err_in_ulp(fine):
        got = RR.resolve(fine, 3).astype(np.float64)
        mean = fine.astype(np.float64).reshape(40, 3, 30, 3, 4).mean(axis=(1, 3))
        return (np.abs(got - mean) / np.spacing(np.abs(mean).astype(F)).astype(np.float64)).max()

    for sign in (1.0, -1.0):
        scale = np.repeat(np.repeat(2.0 ** rng.integers(-60, 60, (40, 30, 4)), 3, axis=0), 3, axis=1)
        exact = (sign * rng.integers(1, 2**20, (3 * 40, 3 * 30, 4)) * scale).astype(F)
        e = err_in_ulp(exact)
        print("n = 3, sign", sign, "exact partial sums: max error in ulp of the mean:", e)
        assert e <= 1.0
        general = (sign * rng.uniform(1e-3, 1e3, (3 * 40, 3 * 30, 4))).astype(F)
        g = err_in_ulp(general)
        print("n = 3, sign", sign, "general samples: max error in ulp of the mean:", g)
        assert g <= 9.125


def test_the_order_of_the_additions_is_observable():
    big = F(2.0**24)
    block = np.array([[big, 1.0], [1.0, -big]], F).reshape(2, 2, 1)            # row-major: 2^24, 1, 1, -2^24
    got = RR.resolve(block, 2)
    assert got[0, 0, 0] == F(0.0)                                              # 2^24 + 1 = 2^24 (tie to even), + 1 likewise, - 2^24 = 0
    permuted = np.array([[1.0, 1.0], [big, -big]], F).reshape(2, 2, 1)         # the same values in another row-major order
    other = RR.resolve(permuted, 2)
    assert other[0, 0, 0] == F(0.5)                                            # (1 + 1 + 2^24) - 2^24 = 2, x 0.25
    assert bits(got)[0, 0, 0] != bits(other)[0, 0, 0]
    # the same through the model's own `order`: column-major over the original block
    column_major = RR.resolve(block, 2, order=[(0, 0), (0, 1), (1, 0), (1, 1)])
    assert np.array_equal(bits(column_major), bits(got))                       # (here the two ones swap: same result)
    last_first = RR.resolve(block, 2, order=[(1, 1), (0, 0), (1, 0), (0, 1)])  # -2^24 + 2^24 + 1 + 1 = 2
    assert last_first[0, 0, 0] == F(0.5)


def test_inf_minus_inf_is_nan_and_a_nan_stays():
    block = np.zeros((2, 4, 1), F)
    block[0, 0], block[1, 1] = np.inf, -np.inf
    block[0, 2] = np.inf
    got = RR.resolve(block, 2)
    assert np.isnan(got[0, 0, 0]) and np.isposinf(got[0, 1, 0])
    block[0, 2] = np.nan
    assert np.isnan(RR.resolve(block, 2)[0, 1, 0])


@pytest.mark.parametrize("world", [1, 3, 5])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_the_shard_of_the_resolved_frame_is_the_resolved_fine_shard(world, n):
    H, W, band_rows = 100, 6, 32
    rng = np.random.default_rng(4 + n)
    fine = rng.standard_normal((n * H, n * W, 4)).astype(F)
    whole = RR.resolve(fine, n)
    for rank in range(world):
        want = P.pack_shard(whole, rank, world, band_rows)
        fine_shard = P.pack_shard(fine, rank, world, n * band_rows)            # bands of n x band_rows fine rows
        assert fine_shard.shape[0] == n * want.shape[0]                        # the fine shard is n x the output shard
        got = RR.resolve(fine_shard, n)
        assert np.array_equal(bits(got), bits(want))
        owned = P.shard_row_of(H, world, band_rows)
        rows = np.zeros(want.shape[0], bool)
        rows[owned[1][owned[0] == rank]] = True
        assert not got[~rows].any()                                            # padding rows: zero stays zero
