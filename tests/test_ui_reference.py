"""tests/ui_reference.py, the CPU statement of the GUI pass (bbr_draw_ui), against cases derived by hand and against a
binary64 evaluation on the committed draw data (tests/golden/ui_drawdata.npz, tools/ui_fixture_mint.cpp).

The closed forms are binary64 throughout (exact EOTF / OETF, round to nearest byte) and every hand-derived case asserts that
its values sit far from an encode threshold, so that the binary32 rule has to give the same bytes."""
import json
import os

import numpy as np
import pytest

import ui_reference as U
from conftest import GOLDEN

F = np.float32
WHITE = {1: np.full((1, 1, 4), 255, np.uint8)}
TAU = 16.0 * 2.0 ** -24       # the roundings of the attribute, fragment and blend steps on values in [0, 1]


def eotf(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def oetf(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.0031308, x * 12.92, 1.055 * np.maximum(x, 1e-30) ** (1 / 2.4) - 0.055)


T64 = eotf((np.arange(1, 256) - 0.5) / 255.0)     # the encode thresholds in binary64


def closed_blend(dst, colour):
    """one fragment of a white-textured primitive over bytes, in binary64: (bytes, distance of the nearest threshold)"""
    dst, colour = np.asarray(dst, np.float64), np.asarray(colour, np.float64)
    s, sa = colour[:3] / 255.0, colour[3] / 255.0
    o = s * sa + eotf(dst[:3] / 255.0) * (1.0 - sa)
    oa = sa * (1.0 - sa)
    margin = min(np.abs(o[:, None] - T64[None, :]).min(), np.abs(255.0 * oa - (np.arange(256) + 0.5)).min() / 255.0)
    rgb = np.searchsorted(T64, o, side="right")
    return np.array(list(rgb) + [int(np.rint(255.0 * oa))], np.uint8), margin


def background(h, w, px=(100, 150, 200, 255)):
    img = np.empty((h, w, 4), np.uint8)
    img[...] = px
    return img


def one_quad(x0, y0, x1, y1, col, size, clip=None, flip=False):
    w, h = size
    return U.assemble([(clip or (0, 0, w, h), 1, [U.quad(x0, y0, x1, y1, U.rgba(*col), flip=flip)])], (w, h))


def test_encode_inverts_decode_for_every_byte():
    assert np.array_equal(U.srgb8(U.DEC), np.arange(256))


def test_decode_table_is_the_committed_one():
    bits = json.load(open(os.path.join(GOLDEN, "ui_tables.json")))["dec_bits"]
    assert [int(x) for x in U.DEC.view(np.uint32)] == bits
    assert np.array_equal(U.DEC, eotf(np.arange(256) / 255.0).astype(F))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("offset", [0.0, 0.5])
def test_quad_covers_its_pixels_exactly_once(flip, offset):
    """integer bounds: no centre on an outer edge, the diagonal through centres; bounds at + 0.5: the centres of column x0 and
    row y0 ON the left / top edge (in), those of column x1 and row y1 on the right / bottom edge (out)"""
    img = background(16, 20)
    col = (255, 128, 0, 128)
    out = U.render(img, one_quad(3 + offset, 2 + offset, 11 + offset, 9 + offset, col, (20, 16), flip=flip), WHITE)
    once, margin = closed_blend(img[0, 0], col)
    twice, _ = closed_blend(once, col)
    assert margin > 1e-4 and not np.array_equal(once[:3], twice[:3])          # a double blend would show
    expect = img.copy()
    expect[2:9, 3:11] = once
    assert np.array_equal(out, expect)


def test_scissor_truncates_the_difference_not_the_ends():
    img = background(16, 32)
    col = (10, 200, 30, 200)
    out = U.render(img, one_quad(-5, -5, 40, 40, col, (32, 16), clip=(10.9, -3.0, 20.1, 9.9)), WHITE)
    expect = img.copy()
    expect[0:9, 10:19] = closed_blend(img[0, 0], col)[0]                        # x in [10, 19), not [10, 20); y from 0
    assert np.array_equal(out, expect)
    assert U.scissor((10.9, -3.0, 20.1, 9.9), one_quad(0, 0, 1, 1, col, (32, 16)), 32, 16) == (10, 0, 19, 9)


@pytest.mark.parametrize("clip", [(32.0, 0.0, 50.0, 10.0), (0.0, 16.0, 10.0, 30.0), (-9.0, 0.0, -1.0, 10.0), (0.0, -9.0, 10.0, -0.5),
                                  (12.0, 0.0, 5.0, 10.0), (float("nan"), 0.0, 10.0, 10.0)])
def test_command_that_cannot_draw_is_skipped(clip):
    img = background(16, 32)
    out = U.render(img, one_quad(-5, -5, 40, 40, (1, 2, 3, 200), (32, 16), clip=clip), WHITE)
    assert np.array_equal(out, img)


def test_order_matters_and_each_order_has_its_closed_form():
    img = background(8, 8)
    A, B = (240, 30, 20, 150), (20, 40, 250, 96)
    results = []
    for first, second in ((A, B), (B, A)):
        d = U.assemble([((0, 0, 8, 8), 1, [U.quad(1, 1, 6, 6, U.rgba(*first)), U.quad(3, 3, 8, 8, U.rgba(*second), flip=True)])], (8, 8))
        out = U.render(img, d, WHITE)
        b1, m1 = closed_blend(img[0, 0], first)
        b2, m2 = closed_blend(img[0, 0], second)
        b12, m12 = closed_blend(b1, second)
        assert min(m1, m2, m12) > 1e-4
        expect = img.copy()
        expect[1:6, 1:6] = b1
        expect[3:8, 3:8] = b2
        expect[3:6, 3:6] = b12
        assert np.array_equal(out, expect)
        results.append(out[4, 4])
    assert not np.array_equal(results[0][:3], results[1][:3])


def test_requantising_per_fragment_differs_from_accumulating_in_float():
    """an 8-bit attachment rounds after every fragment: a three-layer stack whose bytes differ from the ones a float
    accumulator would give -- searched for, found, and rendered"""
    def in_float(dst, colour):
        d = U.DEC[np.asarray(dst[:3])]
        for _ in range(3):
            s, sa = (F(colour[:3]) * (F(1) / F(255))).astype(F), F(colour[3]) * (F(1) / F(255))
            d = U.fmaf(s, sa, (d * (F(1) - sa)).astype(F))
        return U.srgb8(d)

    found = None
    for dst in ((7, 60, 200, 255), (128, 33, 90, 255), (250, 3, 17, 255)):
        for colour in ((200, 100, 50, 40), (13, 240, 77, 25), (90, 90, 90, 10), (255, 0, 128, 70)):
            b = np.array(dst, np.uint8)
            margin = 1.0
            for _ in range(3):
                b, m = closed_blend(b, colour)
                margin = min(margin, m)
            if margin > 1e-4 and not np.array_equal(b[:3], in_float(dst, colour)):
                found = found or (dst, colour, b)
    assert found is not None
    dst, colour, b = found
    img = background(4, 4, dst)
    d = U.assemble([((0, 0, 4, 4), 1, [U.quad(0, 0, 4, 4, U.rgba(*colour))] * 3)], (4, 4))
    assert np.array_equal(U.render(img, d, WHITE)[2, 1], b)


def test_transparent_source_keeps_rgb_and_opaque_source_replaces_it():
    img = np.zeros((16, 16, 4), np.uint8)
    img[..., 0] = np.arange(256).reshape(16, 16)           # every byte value as a destination
    img[..., 1] = img[..., 0][::-1]
    img[..., 2] = 77
    img[..., 3] = 255
    out = U.render(img, one_quad(0, 0, 16, 16, (9, 99, 199, 0), (16, 16)), WHITE)
    assert np.array_equal(out[..., :3], img[..., :3]) and not out[..., 3].any()     # sa = 0: o = d, alpha = sa (1 - sa) = 0
    out = U.render(img, one_quad(0, 0, 16, 16, (9, 99, 199, 255), (16, 16)), WHITE)
    opaque = np.searchsorted(T64, np.array([9, 99, 199]) / 255.0, side="right")      # sa = 1: the encode of the LINEAR colour
    assert list(opaque) == [53, 167, 229] and np.array_equal(out[..., :3], np.broadcast_to(opaque.astype(np.uint8), (16, 16, 3)))
    assert not out[..., 3].any()


def test_alpha_byte_is_the_back_ends_own_factor():
    """srcAlphaBlendFactor ONE_MINUS_SRC_ALPHA, dstAlphaBlendFactor ZERO: oa = sa (1 - sa), whatever the destination's alpha"""
    for a in range(256):
        sa = a / 255.0
        x = 255.0 * sa * (1.0 - sa)
        if abs(x - np.floor(x) - 0.5) < 1e-3:
            continue                                           # (a tie of rint in binary64: left to the margin layer)
        for dst_a in (0, 255):
            out = U.blend(np.array([[5, 6, 7, dst_a]], np.uint8), np.array([[0.25, 0.5, 0.75, F(a) * (F(1) / F(255))]], F))
            assert out[0, 3] == int(np.rint(x)), a


# ---- margin layer: every fragment step of the committed draw data against binary64 ----

def load_fixture():
    z = np.load(os.path.join(GOLDEN, "ui_drawdata.npz"))
    draw = U.DrawData(z["vertices"].copy().view(U.VERTEX_DTYPE).reshape(-1), z["indices"], z["cmds"].copy().view(U.CMD_DTYPE).reshape(-1),
                      z["display_pos"], z["display_size"], z["framebuffer_scale"])
    atlas = np.full(z["atlas_alpha"].shape + (4,), 255, np.uint8)
    atlas[..., 3] = z["atlas_alpha"]
    return draw, atlas


def bilinear64(tex, u, v):
    h, w = tex.shape[:2]
    x, y = u * w - 0.5, v * h - 0.5
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    ix, iy = xf.astype(np.int64), yf.astype(np.int64)
    t = tex.astype(np.float64)
    a, b, c, d = t[iy % h, ix % w], t[iy % h, (ix + 1) % w], t[(iy + 1) % h, ix % w], t[(iy + 1) % h, (ix + 1) % w]
    top, bot = a + fx * (b - a), c + fx * (d - c)
    return (top + fy * (bot - top)) / 255.0


def test_fixture_is_what_the_mint_tool_describes():
    draw, atlas = load_fixture()
    assert draw.extent() == (1280, 720) and atlas.shape == (64, 512, 4)
    assert len(draw.cmds) == 4 and set(draw.cmds["texture"]) == {1, 2} and (draw.cmds["vtx_offset"] != 0).any()
    assert (draw.cmds["elem_count"] % 3 == 0).all() and draw.vertices["pos"][:, 1].min() < 0          # partly off the top edge


def test_every_fragment_step_against_binary64(maps64):
    draw, atlas = load_fixture()
    img = background(720, 1280, (40, 90, 160, 255))
    img[::3, ::2, :3] = (200, 30, 120)
    stats = {"values": 0, "undecided": 0, "wrong": 0, "fragments": 0}

    def observe(f):
        X, Y = [float(x) for x in f.X], [float(y) for y in f.Y]
        S = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
        dx = f.px * 256.0 + 128.0 - X[0]
        dy = f.py * 256.0 + 128.0 - Y[0]
        l1 = ((Y[2] - Y[0]) * dx - (X[2] - X[0]) * dy) / S
        l2 = ((X[1] - X[0]) * dy - (Y[1] - Y[0]) * dx) / S
        A = f.attr.astype(np.float64)
        attr = A[0][None, :] + l1[:, None] * (A[1] - A[0])[None, :] + l2[:, None] * (A[2] - A[0])[None, :]
        src = attr[:, 2:6] * bilinear64(f.texture, attr[:, 0], attr[:, 1])
        sa = src[:, 3:4]
        o = src[:, :3] * sa + eotf(f.dst[:, :3] / 255.0) * (1.0 - sa)
        decided = np.abs(o[:, :, None] - T64[None, None, :]).min(axis=2) > TAU
        byte = np.searchsorted(T64, o.ravel(), side="right").reshape(o.shape)
        oa = np.clip(sa[:, 0] * (1.0 - sa[:, 0]), 0.0, 1.0)
        a_decided = np.abs(255.0 * oa - np.floor(255.0 * oa) - 0.5) > 255.0 * TAU
        stats["fragments"] += len(f.px)
        stats["values"] += decided.size + a_decided.size
        stats["undecided"] += int((~decided).sum() + (~a_decided).sum())
        stats["wrong"] += int((decided & (byte != f.out[:, :3])).sum() + (a_decided & (np.rint(255.0 * oa) != f.out[:, 3])).sum())

    U.render(img, draw, {1: atlas, 2: maps64["albedo"]}, observe)
    print(stats)
    assert stats["fragments"] > 200000
    assert stats["undecided"] <= 0.01 * stats["values"]        # thresholds are >= 1 / (255 * 12.92) apart: 2 tau over that is 0.63 %
    assert stats["wrong"] == 0
