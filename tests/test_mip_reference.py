"""The mip model (tests/mip_reference.py) against hand-made cases, against aniso_reference where the two must agree, and the
census of the GPU scenes on the oracle's uv frame: all without a GPU.  tests/test_gpu_mip.py holds the kernels to it."""
import functools

import numpy as np
import pytest

import aniso_reference as A
import mip_reference as M
import surface_chart as SC
import texture_chart as TC
from oracle import bbo

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def grey(values, w, h):
    """uint8 [h, w, 4] with every channel of texel i = values[i]"""
    return np.repeat(np.asarray(values, np.uint8).reshape(h, w, 1), 4, axis=2)


# ---------------------------------------------------------------------------------------------------------------------
# chain by hand
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("texels,want", [((0, 0, 0, 1), 0), ((0, 1, 0, 1), 1), ((1, 1, 1, 0), 1), ((255, 255, 255, 255), 255)],
                         ids=["sum 1", "sum 2", "sum 3", "sum 1020"])
def test_two_by_two_rounds_half_up(texels, want):
    assert sum(texels) in (1, 2, 3, 1020)
    levels = M.chain(grey(texels, 2, 2), 15)
    assert [l.shape for l in levels] == [(2, 2, 4), (1, 1, 4)]
    assert (levels[1] == want).all()            # (1 + 2) >> 2 = 0, (2 + 2) >> 2 = 1, (3 + 2) >> 2 = 1, 1022 >> 2 = 255


def test_five_by_three_and_one_by_seven():
    t = grey(np.arange(15) * 10, 5, 3)          # rows 0 10 20 30 40 / 50 .. 90 / 100 .. 140
    levels = M.chain(t, 15)
    assert [l.shape[:2] for l in levels] == [(3, 5), (1, 2), (1, 1)]
    # 2 x 1: columns (0, 1) and (2, 3) of rows 0 and 1; column 4 and row 2 belong to no texel of the level below
    assert levels[1][0, :, 0].tolist() == [(0 + 10 + 50 + 60 + 2) >> 2, (20 + 30 + 70 + 80 + 2) >> 2]
    # 1 x 1 from 2 x 1: the row index clamps (rows min(0, 0), min(1, 0)): each column counts twice
    a, b = levels[1][0, :, 0].astype(int)
    assert levels[2][0, 0, 0] == (2 * a + 2 * b + 2) >> 2
    t = grey([1, 2, 3, 4, 50, 60, 255], 1, 7)   # one column, seven rows
    levels = M.chain(t, 15)
    assert [l.shape[:2] for l in levels] == [(7, 1), (3, 1), (1, 1)]
    # the column index clamps on every level: each row counts twice; row 6 belongs to no texel of the level below
    assert levels[1][:, 0, 0].tolist() == [(2 * 1 + 2 * 2 + 2) >> 2, (2 * 3 + 2 * 4 + 2) >> 2, (2 * 50 + 2 * 60 + 2) >> 2]
    a, b = levels[1][:2, 0, 0].astype(int)
    assert levels[2][0, 0, 0] == (2 * a + 2 * b + 2) >> 2


def test_level_counts():
    assert M.level_count(1, 1, 15) == 1
    assert M.level_count(64, 2, 15) == 7 and M.level_size(64, 2, 6) == (1, 1) and M.level_size(64, 2, 2) == (16, 1)
    assert M.level_count(16384, 3, 15) == 15 and M.level_size(16384, 3, 14) == (1, 1)
    for cap in range(1, 16):
        assert M.level_count(16384, 3, cap) == cap
        assert M.level_count(64, 2, cap) == min(cap, 7)
        assert M.level_count(1, 1, cap) == 1
        assert len(M.chain(np.zeros((3, 100, 4), np.uint8), cap)) == min(cap, 7)
    assert len(M.material_chains({}, 15)["albedo"]) == 1          # a defaulted map is 1 x 1 and has one level


# ---------------------------------------------------------------------------------------------------------------------
# level rule
# ---------------------------------------------------------------------------------------------------------------------
def test_level_rule_by_hand():
    L = 9
    for k in range(0, 8):
        d, delta = M.level_of(F(4.0) ** k, True, L)
        assert (d.item(), delta.item()) == (k, 0.0)
    d, delta = M.level_of(F(2.0), True, L)
    assert (d.item(), delta.item()) == (0, 0.5)
    d, delta = M.level_of(F(3.0), True, L)
    assert (d.item(), delta.item()) == (0, 0.75)                    # e = 1, mantissa 0.5: 0.5 (1 + 0.5)
    for P in (F(1.0), F(0.5), F(0.0), F(np.nan), F(-4.0), np.nextafter(F(1.0), F(0.0))):
        d, delta = M.level_of(P, True, L)
        assert (d.item(), delta.item()) == (0, 0.0), P
    d, delta = M.level_of(F(64.0), False, L)                      # a difference that is not finite
    assert (d.item(), delta.item()) == (0, 0.0)
    for P in (F(np.inf), F(4.0) ** 8, F(4.0) ** 9, F(3e38), np.nextafter(F(4.0) ** 8, F(np.inf))):
        d, delta = M.level_of(P, True, L)
        assert (d.item(), delta.item()) == (L - 1, 0.0), P
    d, delta = M.level_of(np.nextafter(F(4.0) ** 8, F(0.0)), True, L)
    assert d.item() == L - 2 and 0.99 < delta.item() < 1.0
    d, delta = M.level_of(F(1e6), True, 1)                        # a one-level map
    assert (d.item(), delta.item()) == (0, 0.0)


def test_level_rule_is_monotone_and_within_its_bound():
    rng = np.random.default_rng(5)
    P = np.sort(np.exp2(rng.uniform(0.0, 28.0, 100000)).astype(F))
    P = P[P > 1]
    d, delta = M.level_of(P, np.ones(len(P), bool), 15)
    lam = d.astype(np.float64) + delta.astype(np.float64)
    assert (np.diff(lam) >= 0).all()
    exact = 0.5 * np.log2(P.astype(np.float64))
    # the bound is derived, not fitted: log2(1 + t) - t on [0, 1) peaks at t = 1 / ln 2 - 1
    t = 1.0 / np.log(2.0) - 1.0
    bound = 0.5 * (np.log2(1.0 + t) - t)
    assert abs(bound - 0.043) < 1e-3 and bound == M.LEVEL_BOUND
    err = exact - lam
    print(f"d + delta against 1/2 log2 P on {len(P)} values: low by at most {err.max():.5f} (bound {bound:.5f}), high by {-err.min():.2e}")
    assert err.max() <= bound + 1e-12 and err.min() >= -1e-12
    assert err.max() > 0.9 * bound                                # the bound is reached: the deviation is real


def test_r2_is_the_nearest_binary32():
    for k in range(1, 17):
        assert float(M.R2[k]) == float(F(1.0 / (k * k)))


# ---------------------------------------------------------------------------------------------------------------------
# one level, and level 0 alone: the bits of aniso_reference
# ---------------------------------------------------------------------------------------------------------------------
def random_footprints(rng, n, scale):
    fp = np.zeros((n, 6), F)
    fp[:, :2] = rng.uniform(-3, 3, (n, 2))
    fp[:, 2:] = rng.normal(size=(n, 4)) * np.exp2(rng.uniform(-12, scale, (n, 1)))
    return fp


@pytest.mark.parametrize("max_aniso", [1, 16])
def test_a_one_level_chain_is_the_anisotropic_filter(max_aniso):
    rng = np.random.default_rng(1)
    maps = TC.materials("five sizes")[0]
    fp = random_footprints(rng, 4000, 2)
    want = A.filter_maps(maps, fp, 1, True, max_aniso)
    got = M.filter_maps(maps, fp, 1, True, max_aniso, 1)
    assert np.array_equal(bits(got[:, :16]), bits(want)) and not got[:, 16:].any()


@pytest.mark.parametrize("layout", ["packed 48x80", "five sizes"])
def test_pixels_on_level_zero_alone_keep_their_bits(layout):
    rng = np.random.default_rng(2)
    maps = TC.materials(layout)[0]
    fp = random_footprints(rng, 6000, -2)
    want = A.filter_maps(maps, fp, 1, True, 16)
    got = M.filter_maps(maps, fp, 1, True, 16, 15)
    shared = A.shared_size(maps)
    # per column of the record: the map that decides it
    columns = [("albedo", [0, 1, 2]), ("metallic", [3]), ("roughness", [4]), ("ao", [5]), ("height", [6]), ("normal", [7, 8, 9])]
    seen = moved = 0
    for name, cols in columns:
        tex = A.texture_of(maps.get(name), name)
        w, h = shared if (shared is not None and name != "height") else (tex.shape[1], tex.shape[0])
        n, _ = A.tap_count(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], w, h, 16)
        d, delta, _ = M.level_rule(fp, w, h, n, M.level_count(w, h, 15))
        same = (d == 0) & (delta == 0)
        seen += int(same.sum())
        assert np.array_equal(bits(got[same][:, cols]), bits(want[same][:, cols])), name
        if (~same).sum() > 100:                                   # (a small map leaves level 0 on few of these footprints)
            assert (bits(got[~same][:, cols]) != bits(want[~same][:, cols])).any(), name
            moved += 1
    assert seen > 6000 and moved >= 2
    assert np.array_equal(got[:, 10:16], want[:, 10:16])          # N is the anisotropic rule's on the level-0 size


# ---------------------------------------------------------------------------------------------------------------------
# stripes
# ---------------------------------------------------------------------------------------------------------------------
def test_stripes_of_period_two_are_constant_from_level_one_on():
    tex = np.zeros((16, 16, 4), np.uint8)
    tex[:, ::2] = 255                                             # columns 255 0 255 0 ...
    levels = M.chain(tex, 15)
    for l in levels[1:]:
        assert (l == 128).all()                                   # (255 + 0 + 255 + 0 + 2) >> 2
    u = (np.arange(200, dtype=F) * F(0.013)).astype(F)
    fp = np.zeros((200, 6), F)
    fp[:, 0], fp[:, 1] = u, F(0.3)
    fp[:, 2], fp[:, 5] = F(8.0 / 16.0), F(8.0 / 16.0)             # minified 8 x on both axes: P = 64, d = 3
    n, axis = A.tap_count(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], 16, 16, 1)
    d, delta, P = M.level_rule(fp, 16, 16, n, len(levels))
    assert (P == 64).all() and (d == 3).all() and (delta == 0).all()
    got = M.filter_chain(levels, fp, n, axis, d, delta)
    assert (bits(got) == bits(F(128.0) * (F(1.0) / F(255.0)))).all()
    level0 = A.filter_texture(tex, fp, n, axis)
    assert level0[:, 0].max() - level0[:, 0].min() > 0.9          # the level-0 tap aliases between 0 and 1


# ---------------------------------------------------------------------------------------------------------------------
# packed levels
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_PACKED = [(2, 2), (4, 4), (5, 3), (3, 5), (6, 10), (7, 1), (1, 7), (17, 5), (48, 80), (64, 2), (130, 2)]


@pytest.mark.parametrize("wh", CHAIN_PACKED, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_packed_levels_are_the_host_pack_of_the_level_maps(wh):
    maps = TC.materials(f"packed {wh[0]}x{wh[1]}")[0]
    chains = M.material_chains(maps, 15)
    levels = M.packed_levels(maps, 15)
    assert len(levels) == M.level_count(wh[0], wh[1], 15)
    for k, want in enumerate(levels):
        ok, w, h, n, got = TC.host_pack({name: chains[name][k] for name in A.SHADED})
        assert ok and (w, h) == M.level_size(wh[0], wh[1], k) and n == len(want) == TC.packed_bytes_needed(w, h)
        assert np.array_equal(got, want)


def test_packed_levels_of_partly_and_wholly_defaulted_materials():
    assert M.packed_levels(TC.materials("five sizes")[0], 15) is None
    levels = M.packed_levels({}, 15)
    assert len(levels) == 1 and np.array_equal(levels[0], TC.host_pack({})[4])
    maps = TC.materials("normal only 6x10")[0]
    levels = M.packed_levels(maps, 15)
    assert len(levels) == 4
    for k, want in enumerate(levels):
        assert np.array_equal(TC.host_pack({"normal": M.chain(maps["normal"], 15)[k]})[4], want)


# ---------------------------------------------------------------------------------------------------------------------
# index safety: must hold before any packed chain goes to a GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", CHAIN_PACKED + [(1024, 1024), (16384, 3), (3, 16384)], ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_every_record_load_stays_inside_its_level(wh):
    """The column of a tap depends on u alone and its row on v alone, so every value of the hazard lists is taken on each
    axis by itself and the record index is then checked on EVERY pair of a reached column and a reached row.  The lists: those
    of the level-0 extents (what the texture chart plants) and of the level's own extents (which stand on that level's wraps)."""
    w, h = wh
    table = M.level_table(w, h, 15)
    assert len(table) == M.level_count(w, h, 15)
    layout = f"packed {w}x{h}"
    planted = [TC.arriving_uv(TC.planted_uv(layout), chart) for chart in TC.POINT_CHARTS] if layout in TC.LAYOUTS else []
    for k, (wk, hk, first, n_bytes) in enumerate(table):
        assert (wk, hk) == M.level_size(w, h, k) and n_bytes == TC.packed_bytes_needed(wk, hk)
        with np.errstate(all="ignore"):
            us = np.concatenate([TC.hazard_list(n) for n in dict.fromkeys((w, h, wk, hk))]).astype(F)
        x0, x1, y0, y1 = TC.wrapped_taps(us, us, wk, hk)
        for x, n in ((x0, wk), (x1, wk), (y0, hk), (y1, hk)):
            assert x.min() >= 0 and x.max() < n
            assert {0, n - 1} <= set(x.tolist()), f"level {k}: the taps do not reach both ends of an axis of {n}"
        cols, rows = np.union1d(x0, x1), np.union1d(y0, y1)
        assert len(cols) == wk or wk > 600, f"level {k}: {len(cols)} of {wk} columns reached"    # (long lists are thinned: TC.hazard_list)
        assert len(rows) == hk or hk > 600
        X, Y = np.meshgrid(cols, rows)
        at = first + TC.packed_index(X.ravel(), Y.ravel(), wk) * TC.PACKED_TEXEL_BYTES
        assert at.min() >= first and (at + TC.TAP_LOAD_BYTES).max() <= first + n_bytes, f"level {k}: a 12-byte tap load leaves the level"
        for uv in planted:                                        # the chart's planted pairs themselves, as they arrive
            px0, px1, py0, py1 = TC.wrapped_taps(uv[:, 0], uv[:, 1], wk, hk)
            for x, y in ((px0, py0), (px1, py0), (px0, py1), (px1, py1)):
                at = first + TC.packed_index(x, y, wk) * TC.PACKED_TEXEL_BYTES
                assert at.min() >= first and (at + TC.TAP_LOAD_BYTES).max() <= first + n_bytes, f"level {k}: a planted uv leaves the level"
        # the last texel's load fits, and with it every texel's: the index is largest there
        every = TC.packed_index(np.arange(wk * hk) % wk, np.arange(wk * hk) // wk, wk)
        assert int(every.max()) == int(TC.packed_index(wk - 1, hk - 1, wk)) and len(np.unique(every)) == wk * hk
        assert first + TC.PACKED_TEXEL_BYTES * int(every.max()) + TC.TAP_LOAD_BYTES <= first + n_bytes
        assert TC.PACKED_TEXEL_BYTES * int(every.max()) + TC.TAP_LOAD_BYTES <= 2 ** 32 - 1                # uint32 byte offsets
        if k + 1 < len(table):
            assert first + n_bytes == table[k + 1][2]


# ---------------------------------------------------------------------------------------------------------------------
# census of the GPU scenes on the oracle's uv frame with the model's differences
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def oracle_uv(name):
    sc = M.scene(name, (M.maps64(),))
    uv, prim, _, _ = bbo.render(sc, flags=bbo.FLAG_OUTPUT_UV)
    return sc, uv, prim


# (scene, texture size, option): the textures of tests/test_gpu_mip.py's layouts on which a scene claims its classes -- the
# 64^2 set and its 16^2 height map, the 1024^2 set, and the 64^2 set under a cap of three levels (where `tilted` is clamped
# everywhere and claims nothing, as on the 16^2 map)
CENSUS = [(name, size, cap) for name in M.SCENES for size, cap in (((64, 64), 15), ((1024, 1024), 15), ((16, 16), 15), ((64, 64), 3))
          if not (name == "tilted" and (cap == 3 or size == (16, 16)))]   # (16^2: its many taps leave it magnified)


@pytest.mark.parametrize("name,size,levels", CENSUS, ids=lambda v: str(v).replace(" ", ""))
def test_census_of_the_gpu_scenes(name, size, levels):
    sc, uv, prim = oracle_uv(name)
    diff, ok = M.model_differences(uv, prim)
    # (a strip's last row has another winner below it: seven rows of eight qualify)
    assert ok.sum() >= 0.75 * (prim != bbo.NO_PRIM).sum() and (prim != bbo.NO_PRIM).sum() >= 0.95 * M.N_PIX
    fp = np.concatenate([np.asarray(uv, F)[..., :2][ok], diff[ok]], -1)
    w, h = size
    count = M.level_count(w, h, levels)
    for max_aniso in (1, 16):
        n, _ = A.tap_count(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], w, h, max_aniso)
        d, delta, P = M.level_rule(fp, w, h, n, count)
        _, finite = M.long_axis(fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5], w, h)
        out = M.census(name, d, delta, P, finite, count)
        print(f"{name} {w}x{h} cap {levels} max_anisotropy {max_aniso}: {out}")
        if name == "steps":                                       # P = 4^k exactly: no pixel between two levels
            assert out["blended"] == 0
