"""tests/bloom_reference.py against a scalar restatement of the rule in exact arithmetic: every + - * is done on
fractions.Fraction and its exact result rounded once to binary32 (nearest, ties to even, denormals kept).  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import bloom_reference as B
from oracle import bbo

F32 = np.float32


def r32(q):
    """the binary32 nearest to the exact rational q, ties to even, as a Fraction (math.inf past the largest finite value)"""
    if q == 0:
        return Fraction(0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()     # 2^(e-1) <= a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1                                                     # 2^e <= a < 2^(e+1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = a / quantum
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    v = fl * quantum
    if v >= Fraction(2) ** 128:
        return math.inf
    return v if q > 0 else -v


def test_r32_is_binary32_rounding():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(300).astype(F32) * F32(1e3)
    b = (rng.standard_normal(300) * 1e-3).astype(F32)
    a[:6] = [1e30, 1e-45, 1e-39, 65504.0, 1.0, 16777216.0]
    b[:6] = [1e-30, 1e-45, -1e-40, 1.0, 2.0 ** -24, 1.0]
    for x, y in zip(a, b):
        fx, fy = Fraction(float(x)), Fraction(float(y))
        assert float(r32(fx + fy)) == float(x + y)
        assert float(r32(fx - fy)) == float(x - y)
        assert float(r32(fx * fy)) == float(x * y)
        assert float(r32(fx * Fraction(1, 4))) == float(x * F32(0.25))


# ---- the scalar restatement: Fractions that are binary32 values ----
def s_add(a, b):
    return r32(a + b)


def s_sub(a, b):
    return r32(a - b)


def s_mul(a, b):
    return r32(a * b)


def s_bright(value, t):
    v = float(value)
    if math.isnan(v):
        return Fraction(0)
    if math.isinf(v):
        return Fraction(65504) if v > 0 else Fraction(0)
    d = s_sub(Fraction(v), t)
    return min(d, Fraction(65504)) if d > 0 else Fraction(0)


def s_box(g, w, h):
    wd, hd = (w + 1) >> 1, (h + 1) >> 1
    out = {}
    for y in range(hd):
        for x in range(wd):
            x0, x1, y0, y1 = min(2 * x, w - 1), min(2 * x + 1, w - 1), min(2 * y, h - 1), min(2 * y + 1, h - 1)
            out[x, y] = s_mul(s_add(s_add(g[x0, y0], g[x1, y0]), s_add(g[x0, y1], g[x1, y1])), Fraction(1, 4))
    return out, wd, hd


def s_lerp4(a, b):
    return s_add(a, s_mul(s_sub(b, a), Fraction(1, 4)))


def s_up(g, w, h, x, y):
    px, py = x >> 1, y >> 1
    qx = min(max(px + (1 if x & 1 else -1), 0), w - 1)
    qy = min(max(py + (1 if y & 1 else -1), 0), h - 1)
    return s_lerp4(s_lerp4(g[px, py], g[qx, py]), s_lerp4(g[px, qy], g[qx, qy]))


def scalar_pyramid(frame, channel, levels, threshold):
    """([None, U_1 .. U_L] as dicts (x, y) -> Fraction, sizes) for one channel"""
    h, w = frame.shape[:2]
    t = Fraction(float(F32(threshold)))
    e = {(x, y): s_bright(frame[y, x, channel], t) for y in range(h) for x in range(w)}
    d, sizes = [None], [(w, h)]
    g, gw, gh = e, w, h
    for _ in range(levels):
        g, gw, gh = s_box(g, gw, gh)
        d.append(g)
        sizes.append((gw, gh))
    u = list(d)
    for k in range(levels - 1, 0, -1):
        wk, hk = sizes[k]
        wc, hc = sizes[k + 1]
        u[k] = {(x, y): s_add(d[k][x, y], s_up(u[k + 1], wc, hc, x, y)) for y in range(hk) for x in range(wk)}
    return u, sizes


def as_array(level, w, h):
    return np.array([[float(level[x, y]) for x in range(w)] for y in range(h)], F32)


@pytest.mark.parametrize("levels", B.CHART_LEVELS)
@pytest.mark.parametrize("w,h", B.SMALL_FRAMES)
def test_model_equals_exact_arithmetic(w, h, levels):
    for variant in range(3):
        frame = B.chart_frame(w, h, variant=variant)
        got = B.pyramid(frame, levels, B.CHART_THRESHOLD)
        assert [(g.shape[1], g.shape[0]) for g in got[1:]] == B.level_sizes(w, h, levels)[1:]
        v = B.bloomed(frame, levels, B.CHART_THRESHOLD, B.CHART_INTENSITY)
        for c in range(3):
            want, sizes = scalar_pyramid(frame, c, levels, B.CHART_THRESHOLD)
            assert sizes == B.level_sizes(w, h, levels)
            for k in range(1, levels + 1):
                assert B.same_bits(got[k][..., c], as_array(want[k], *sizes[k])), (variant, c, k)
            for y in range(h):                       # the pixel: F + I * up(U_1), where F is finite
                for x in range(w):
                    if np.isfinite(frame[y, x, c]):
                        b = s_up(want[1], *sizes[1], x, y)
                        pixel = s_add(Fraction(float(frame[y, x, c])), s_mul(Fraction(float(B.CHART_INTENSITY)), b))
                        assert float(pixel) == float(v[y, x, c]), (variant, c, x, y)
        assert B.same_bits(v[..., 3], frame[..., 3])


def test_level_sizes_repeat_at_one():
    assert B.level_sizes(1, 1, 3) == [(1, 1)] * 4
    assert B.level_sizes(3, 5, 8) == [(3, 5), (2, 3), (1, 2), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1)]
    assert B.level_sizes(7, 4, 3) == [(7, 4), (4, 2), (2, 1), (1, 1)]
    assert B.level_sizes(257, 131, 8)[1:] == [(129, 66), (65, 33), (33, 17), (17, 9), (9, 5), (5, 3), (3, 2), (2, 1)]
    assert B.level_sizes(32768, 1, 2) == [(32768, 1), (16384, 1), (8192, 1)]


@pytest.mark.parametrize("levels", B.CHART_LEVELS)
@pytest.mark.parametrize("w,h", B.SMALL_FRAMES + [(33, 17)])
def test_levels_are_finite_and_not_negative(w, h, levels):
    for variant in range(4):
        frame = B.chart_frame(w, h, variant=variant)
        assert not np.isfinite(frame[..., :3]).all() or w * h < 2        # the hazards are in
        for u in B.pyramid(frame, levels, B.CHART_THRESHOLD)[1:] + B.down_levels(frame, levels, B.CHART_THRESHOLD)[1:]:
            assert np.isfinite(u).all() and (u >= 0).all() and not np.signbit(u).any()
        b = B.up(B.pyramid(frame, levels, B.CHART_THRESHOLD)[1], w, h)
        assert np.isfinite(b).all() and not np.signbit(b).any()
        # a NaN or inf of the frame reaches only its own pixel
        v = B.bloomed(frame, levels, B.CHART_THRESHOLD, B.CHART_INTENSITY)
        assert np.array_equal(np.isfinite(v), np.isfinite(frame))


@pytest.mark.parametrize("hdr16", [False, True])
@pytest.mark.parametrize("enable", [0, 1])
def test_identities_through_present(enable, hdr16):
    for (w, h) in B.SMALL_FRAMES + [(33, 17)]:
        frame = B.chart_frame(w, h)
        plain = bbo.present(frame.reshape(-1, 4), enable, 0.7, hdr16).reshape(h, w, 4)
        for levels in B.CHART_LEVELS:
            assert np.array_equal(B.image(frame, 0, 1.0, 0.25, enable, 0.7, hdr16), plain)
            assert np.array_equal(B.image(frame, levels, 1.0, 0.0, enable, 0.7, hdr16), plain)          # I = 0
            # T >= every finite channel (a +inf channel passes any threshold as 65504: the identity is about frames without one)
            capped = np.where(np.isposinf(frame), F32(7.0), frame).astype(F32)
            plain_capped = bbo.present(capped.reshape(-1, 4), enable, 0.7, hdr16).reshape(h, w, 4)
            big = np.where(np.isfinite(capped[..., :3]), capped[..., :3], 0).max()
            assert np.array_equal(B.image(capped, levels, F32(big), 0.25, enable, 0.7, hdr16), plain_capped)
            assert np.array_equal(B.image(capped, levels, 3e38, 0.25, enable, 0.7, hdr16), plain_capped)
            assert (B.image(frame, levels, 1.0, 0.25, enable, 0.7, hdr16) != plain).any() or w * h <= 4


@pytest.mark.parametrize("levels", [1, 2, 3, 5, 8])
def test_constant_frame_adds_the_levels(levels):
    frame = np.full((12, 20, 4), 3.5, F32)
    u = B.pyramid(frame, levels, 1.0)
    assert np.array_equal(u[1], np.full((6, 10, 3), levels * 2.5, F32))       # U_1 = L * e: nothing is normalised
    assert np.array_equal(B.bloomed(frame, levels, 1.0, 0.5)[..., :3], np.full((12, 20, 3), 3.5 + 0.5 * levels * 2.5, F32))
