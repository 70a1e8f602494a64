"""The CPU statement of the anisotropic filter rule (tests/aniso_reference.py) against hand-derived cases and against the
oracle's sampler.  No GPU."""
import numpy as np
import pytest

import aniso_reference as A
from oracle import bbo

F = np.float32
T = F(1.0) / F(64.0)        # one texel of a 64 x 64 map, in uv


def count(dudx, dvdx, dudy, dvdy, max_aniso=16, w=64, h=64):
    n, axis = A.tap_count(F(dudx), F(dvdx), F(dudy), F(dvdy), w, h, max_aniso)
    return int(n.reshape(-1)[0]), int(axis.reshape(-1)[0])


def test_fmaf_is_one_rounding():
    # 1 + 2^-24 is a tie of the binary32 grid; the product's tail decides it, which two roundings (binary64, then binary32) lose
    a = F(1.0) + F(2.0 ** -12)
    exact = float(a) * float(a) + 2.0 ** -60                        # (1 + 2^-11 + 2^-24) + 2^-60: just above the tie
    assert exact == float(a) * float(a)                             # binary64 cannot hold it ...
    assert A.fmaf(a, a, F(2.0 ** -60)) == F(1.0) + F(2.0 ** -11) + F(2.0 ** -23)   # ... the fma still rounds up
    assert A.fmaf(a, a, F(-2.0 ** -60)) == F(1.0) + F(2.0 ** -11)                  # and down just below it
    rng = np.random.default_rng(1)
    x, y, z = (rng.standard_normal(4096).astype(F) for _ in range(3))
    from fractions import Fraction
    got = A.fmaf(x, y, z)
    for i in range(0, 4096, 16):
        q = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        lo, hi = np.nextafter(got[i], F(-np.inf)), np.nextafter(got[i], F(np.inf))
        assert abs(Fraction(float(got[i])) - q) <= min(abs(Fraction(float(lo)) - q), abs(Fraction(float(hi)) - q))


def test_tap_counts_by_hand():
    assert count(2 * T, 0, 0, 2 * T)[0] == 1                         # isotropic, minified: one tap
    assert count(4 * T, 0, 0, 2 * T) == (2, 0)                       # exactly 2:1 (16 against 4: 4 * 4 < 16 is false)
    assert count(np.nextafter(4 * T, F(1)), 0, 0, 2 * T) == (3, 0)   # just above 2:1
    assert count(0, 2 * T, np.nextafter(4 * T, F(1)), 0) == (3, 1)   # the same, the long axis being y
    assert count(32 * T, 0, 0, 2 * T)[0] == 16                       # exactly 16:1: 15^2 * 4 < 1024
    assert count(64 * T, 0, 0, 2 * T)[0] == 16                       # beyond: still 16
    for cap in (1, 2, 4, 15):
        assert count(64 * T, 0, 0, 2 * T, cap)[0] == cap
    assert count(3 * T, 0, 0, 0)[0] == 16                            # a line footprint longer than a texel
    assert count(T, 0, 0, 0)[0] == 1                                 # mx = 1 exactly: !(mx > 1)
    assert count(0.5 * T, 0, 0, 0.01 * T)[0] == 1                    # magnified, however anisotropic
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            d = [8 * T, 0, 0, T]
            d[k] = bad
            assert count(*d)[0] == 1, (bad, k)
    # per-map sizes: the same differences are 2:1 on a 64 x 64 map and isotropic on a 128 x 32 one
    assert count(4 * T, 0, 0, 2 * T, w=64, h=64)[0] == 2 and count(4 * T, 0, 0, 16 * T, w=128, h=32)[0] == 1
    # the count is the ceiling of the ratio for ratios 1 .. 16
    for r in range(2, 17):
        assert count(F(r) * 2 * T, 0, 0, 2 * T)[0] == r
        assert count(np.nextafter(F(r) * 2 * T, F(9)), 0, 0, 2 * T)[0] == min(r + 1, 16)


def test_axis_choice_and_the_tie():
    assert count(5 * T, 0, 0, 2 * T)[1] == 0
    assert count(2 * T, 0, 0, 5 * T)[1] == 1
    assert count(3 * T, 4 * T, 5 * T, 0) == (1, 1)                   # px2 = py2 = 25: not (px2 > py2), the axis is y
    assert count(0, 3 * T, 3 * T, 0) == (1, 1)


def test_tap_offsets_for_two_taps():
    u, v, du, dv = F(0.3), F(0.7), F(0.06), F(-0.03)
    n = np.array([2])
    for i, sign in ((1, -1.0), (2, 1.0)):
        ui, vi = A.tap_positions(u, v, du, dv, n, i)
        assert abs(float(ui[0]) - (0.3 + sign * 0.06 / 6)) < 1e-7 and abs(float(vi[0]) - (0.7 + sign * -0.03 / 6)) < 1e-7
    o1 = A.fmaf(F(1), A.R[3], F(-0.5)).reshape(-1)[0]
    assert o1 == F(np.float64(A.R[3]) - 0.5) and abs(float(o1) + 1 / 6) < 2.0 ** -25
    ui, vi = A.tap_positions(u, v, F(np.inf), F(np.nan), np.array([1]), 1)          # one tap: (u, v), no arithmetic
    assert ui[0] == u and vi[0] == v
    assert all(A.R[k] == F(1.0) / F(k) for k in range(1, 18))


@pytest.mark.parametrize("size", [(64, 64), (40, 24), (1, 1), (7, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_tap_is_the_oracle_sampler(size):
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    tex = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    n = 10000
    uv = rng.uniform(-3.0, 3.0, (n, 2)).astype(F)
    uv[:8] = [(0, 0), (1, 1), (-1, 0.5), (0.5 / w, 0.5 / h), (np.nan, 0.2), (np.inf, -np.inf), (3e9, 0.1), (-0.0, 1e-30)]
    want = np.stack([bbo.sample(tex, 0, float(a), float(b)) for a, b in uv])
    got = A.bilinear(tex, uv[:, 0], uv[:, 1])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # ... and through the filter with a footprint that asks for one tap
    fp = np.zeros((n, 6), F)
    fp[:, :2] = uv
    fp[:, 2], fp[:, 5] = F(0.5) / F(w), F(0.5) / F(h)
    cnt, axis = A.tap_count(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], w, h, 16)
    assert (cnt == 1).all()
    assert np.array_equal(A.filter_texture(tex, fp, cnt, axis).view(np.uint32), want.view(np.uint32))


def test_column_stripes_by_hand():
    """8 x 4 texels, even columns 0, odd columns 255.  u = 0.4375 is the centre of column 3: one tap reads 1.  A footprint of
    4 x 2 texels, long axis x, has two taps at u -+ 0.5 / 6, i.e. x = 3 -+ 2/3: column 2 | 3 at weight 1/3 -> 1/3, and column
    3 | 4 at weight 2/3 -> 1/3; their average is 1/3.  With four texels along y instead the axis is y and every tap reads 1."""
    tex = np.zeros((4, 8, 4), np.uint8)
    tex[:, 1::2] = 255
    one = F(255.0) * (F(1.0) / F(255.0))                               # what a tap on a 255 texel reads
    fp = np.array([[0.4375, 0.5, 0.5, 0, 0, 0.5]], F)
    n, axis = A.tap_count(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], 8, 4, 16)
    assert (int(n[0]), int(axis[0])) == (2, 0)
    assert np.allclose(A.filter_texture(tex, fp, n, axis), 1 / 3, atol=1e-6)
    assert np.array_equal(A.filter_texture(tex, fp, np.array([1]), axis), np.full((1, 4), one))
    fp = np.array([[0.4375, 0.5, 0.25, 0, 0, 1.0]], F)
    n, axis = A.tap_count(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], 8, 4, 16)
    assert (int(n[0]), int(axis[0])) == (2, 1)
    assert np.array_equal(A.filter_texture(tex, fp, n, axis), np.full((1, 4), one))
    # through filter_maps: a packed material of that one map; the absent maps are uniform and stay what they are up to the
    # rounding of (t + t) / 2, which is exact
    out = A.filter_maps({"albedo": tex}, np.array([[0.4375, 0.5, 0.5, 0, 0, 0.5]], F), 1, False, 16)
    assert np.allclose(out[0, :3], 1 / 3, atol=1e-6) and out[0, 3] == 0 and out[0, 5] == one and out[0, 6] == 0
    assert list(out[0, 10:]) == [2, 2, 2, 2, 2, 0]
    assert np.allclose(out[0, 7:10], np.array([127, 127, 255]) / 255 * 2 - 1, atol=1e-6)


def test_per_map_counts_and_the_height_map():
    rng = np.random.default_rng(3)
    maps = {"albedo": rng.integers(0, 256, (64, 64, 4), dtype=np.uint8), "roughness": rng.integers(0, 256, (16, 16, 4), dtype=np.uint8),
            "height": rng.integers(0, 256, (32, 32, 4), dtype=np.uint8)}
    fp = np.array([[0.3, 0.6, 8 * T, 0, 0, 2 * T]], F)     # 8 x 2 texels of the 64 x 64 map, 2 x 0.5 of the 16 x 16 one
    out = A.filter_maps(maps, fp, 1, True, 16)
    assert list(out[0, 10:]) == [4, 1, 4, 1, 1, 4]          # roughness: 4:1 and longer than a texel; 1 x 1 defaults: one tap
    out = A.filter_maps(maps, fp, 0, False, 2)
    assert list(out[0, 10:]) == [2, 1, 2, 1, 0, 0] and not out[0, 6:10].any()


def test_average_against_binary64():
    rng = np.random.default_rng(7)
    tex = rng.integers(0, 256, (48, 40, 4), dtype=np.uint8)
    m = 2000
    fp = np.zeros((m, 6), F)
    fp[:, :2] = rng.uniform(-2, 2, (m, 2))
    fp[:, 2:] = rng.uniform(-0.3, 0.3, (m, 4)) * rng.uniform(0, 1, (m, 1))
    n, axis = A.tap_count(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], 40, 48, 16)
    assert set(range(1, 17)) <= set(n.tolist())
    got = A.filter_texture(tex, fp, n, axis).astype(np.float64)
    du, dv = np.where(axis == 0, fp[:, 2], fp[:, 4]), np.where(axis == 0, fp[:, 3], fp[:, 5])
    total = np.zeros((m, 4))
    for i in range(1, 17):
        ui, vi = A.tap_positions(fp[:, 0], fp[:, 1], du, dv, n, i)
        total += np.where((i <= n)[:, None], A.bilinear(tex, ui, vi).astype(np.float64), 0.0)
    mean = total / n[:, None]
    assert (np.abs(got - mean) <= n[:, None] * 2.0 ** -24 * mean).all()
