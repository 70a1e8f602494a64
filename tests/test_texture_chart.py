"""CPU side of the texture charts (tests/texture_chart.py; the GPU side is tests/test_gpu_texture_chart.py).

  * the point chart is what it claims, on the oracle: every pixel covered by its own primitive, the planted uv arrives bit
    for bit (+-inf as NaN on flat, -0 as +0 on steep), the census minimums hold for every layout
  * the sampler model (aniso_reference.bilinear) equals the oracle's sampler (bbo.sample) bit for bit on every planted pair
    of every layout, through every map of each of its materials, non-finite pairs included; it agrees with the Vulkan text in binary64 (np_bilinear) where both
    coordinates are below 2^20 texels, and with the two closed forms where a coordinate is dead
  * the block-linear index model stays inside what the host pack function reports, for every packed layout and every
    planted pair: the test that has to pass before a packed layout goes to a GPU
  * the host pack function (bbr_pack_material, csrc/bb_pack.h): decision, dims, bytes, defaults, padding, both orders of
    a supplied 1 x 1 map -- and, compiled stand-alone under AddressSanitizer + UBSan, on heap images of the exact size"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import aniso_reference as A
import surface_chart as SC
import texture_chart as TC
from conftest import GOLDEN, ROOT
from test_oracle_contract import np_bilinear
from oracle import bbo

F = np.float32
PACKED_LAYOUTS = [l for l in TC.LAYOUTS if l != "both" and TC.expect_packed(l)[0]]


def all_pairs(layout):
    """the layout's planted pairs as they arrive on both point charts, bit-distinct, [n, 2]"""
    p = TC.planted_uv(layout)
    both = np.concatenate([TC.arriving_uv(p, "flat"), TC.arriving_uv(p, "steep")])
    return np.unique(SC.bits(both), axis=0).view(F)


# ---------------------------------------------------------------------------------------------------------------------
# the chart
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart", TC.POINT_CHARTS)
@pytest.mark.parametrize("layout", TC.LAYOUTS)
def test_point_chart_on_the_oracle(layout, chart):
    sc = TC.scene(layout, chart)
    uv, prim, depth, st = bbo.render(sc, flags=bbo.FLAG_OUTPUT_UV)
    assert np.array_equal(prim, TC.expected_prim(layout)), "a pixel is not covered by its own primitive"
    assert st["n_shaded"] == TC.N_PIX and st["n_prims"] == sc.n_prims == TC.N_PIX and st["n_clipped_prims"] == 0
    assert 0.25 <= depth.min() and depth.max() <= 0.75
    planted = TC.planted_uv(layout)
    want = TC.arriving_uv(planted, chart)
    got = uv[..., :2].reshape(-1, 2)
    finite = np.isfinite(planted)
    assert np.array_equal(SC.bits(got)[finite & (planted != 0)], SC.bits(planted)[finite & (planted != 0)])
    assert SC.equal_but_for_nan_payload(got, want)
    if chart == "steep":
        inf = np.isinf(planted)
        assert inf.sum() >= 2 * TC.MIN_CLASS and np.array_equal(got[inf], planted[inf])
        assert not np.signbit(got[planted == 0]).any()
    else:
        assert np.isnan(got[np.isinf(planted)]).all()
        assert np.array_equal(np.signbit(got[planted == 0]), np.signbit(planted[planted == 0]))
    c = TC.check_census(layout, chart, got)
    rec = json.load(open(os.path.join(GOLDEN, "texture_chart.json")))
    assert rec["seeds"] == TC.SEEDS and rec["layouts"] == TC.LAYOUTS
    # (a change detector on the chart's construction -- the counts come from the planted inputs, not from a sampler)
    assert rec["census"][f"{layout} {chart}"] == c, "tools/texture_chart_record.py rewrites the record"


@pytest.mark.parametrize("layout", TC.LAYOUTS)
def test_every_list_value_is_planted(layout):
    uv = TC.planted_uv(layout)
    for axis in (0, 1):
        have = set(SC.bits(uv[:, axis][~np.isnan(uv[:, axis])]).tolist())
        for _, wh in TC.layout_sizes(layout):
            lst = TC.hazard_list(wh[axis])
            assert set(SC.bits(lst[~np.isnan(lst)]).tolist()) <= have
        assert np.isnan(uv[:, axis]).any()


def test_hazard_list_holds_what_it_names():
    for n in (1, 2, 5, 130, 16384):
        lst = TC.hazard_list(n)
        b = set(SC.bits(lst).tolist())
        assert len(lst) <= 3 * (2 * 256 + 18) + 1
        for v in (0.0, -0.0, -0.5 / n, -1e-30, 1e-45, -1e-45, 2.0 ** 30 / n, -(2.0 ** 30) / n, (2.0 ** 30 - 64) / n,
                  (2.0 ** 24 + 0.5) / n, 1e6, -1e6, 3e38, -3e38, np.inf, -np.inf, 1.0, (n - 1 + 0.5) / n, -2.0, 3.0):
            v = F(v)
            assert SC.bits(v).item() in b, (n, v)
            for w in (np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))):
                assert SC.bits(w).item() in b, (n, v, w)
        assert np.isnan(lst).sum() == 1
        c = TC.classes(lst, n)
        assert all(c[i].any() for i in range(9) if not (n == 1 and i == 6)), (n, c.sum(1))
    # the classes on hand-made values, n = 4: x = 4 u - 0.5
    u = F([0.125, 0.375, -0.0625, 0.875, 1.9, -0.5, 2.0 ** 19 + 0.25, 2.0 ** 28, 3e38, np.inf, np.nan])
    want = ["a", "a", "b", "ac", "c", "d", "e", "f", "g", "h", "i"]
    got = ["".join(TC.CLASSES[i] for i in range(9) if col[i]) for col in TC.classes(u, 4).T]
    assert got == want, got


@pytest.mark.parametrize("chart", TC.GRADIENT_CHARTS)
def test_gradient_chart_on_the_oracle(chart):
    sc = TC.scene("packed 6x10", chart)
    uv, prim, _, st = bbo.render(sc, flags=bbo.FLAG_OUTPUT_UV)
    assert (prim != bbo.NO_PRIM).all() and st["n_prims"] == 2
    assert (st["n_clipped_prims"] >= 1) == (chart == "clipped")
    u, v = uv[..., 0], uv[..., 1]
    if chart == "nanvertex":          # the triangle with the NaN vertex is NaN in u and huge in v; the other is plain
        assert np.isnan(u[prim == 0]).all() and np.isfinite(u[prim == 1]).all() and (np.abs(v[prim == 0]) > 1e30).any()
        assert 8000 <= (prim == 0).sum() <= 8400
    else:
        x, y = SC.pixel_xy()
        assert np.allclose(u, -40 + 10 * (x + 4), atol=2e-3) and np.allclose(v, -33 + 10 * (4 - y), atol=2e-3)


# ---------------------------------------------------------------------------------------------------------------------
# the sampler model against the oracle, the Vulkan text and the closed forms
# ---------------------------------------------------------------------------------------------------------------------
def oracle_sample(tex, name, uv):
    img = np.ascontiguousarray(tex, np.uint8)
    im = bbo.Image(img.ctypes.data, img.shape[1], img.shape[0])
    out = np.zeros((len(uv), 4), F)
    fn, ref, kind = bbo.lib().bbo_sample, C.byref(im), A.MAP_NAMES.index(name)
    for i, (u, v) in enumerate(uv.tolist()):
        fn(ref, kind, u, v, out[i].ctypes.data)
    return out


@pytest.mark.parametrize("layout", TC.LAYOUTS)
def test_model_is_the_oracles_sampler_on_the_planted_pairs(layout):
    """every planted pair of the layout through every map of every one of its materials (an absent map once per size)"""
    uv = all_pairs(layout)
    for maps in TC.materials(layout):
        seen = set()
        for name in A.MAP_NAMES:
            tex = A.texture_of(maps.get(name), name)
            if maps.get(name) is None and tex.shape[:2] in seen:
                continue
            seen.add(tex.shape[:2])
            assert np.array_equal(SC.bits(A.bilinear(tex, uv[:, 0], uv[:, 1])), SC.bits(oracle_sample(tex, name, uv))), name


@pytest.mark.parametrize("layout", TC.LAYOUTS)
def test_model_against_binary64_and_the_closed_forms(layout):
    uv = all_pairs(layout)
    fp = np.concatenate([uv, np.zeros((len(uv), 4), F)], 1)
    worst = 0.0
    for maps in TC.materials(layout):
        one_tap = A.filter_maps(maps, fp, 1, True, 1)
        assert (one_tap[:, 10:] == 1).all()
        worst = max(worst, TC.check_values(maps, uv, one_tap, True, np_bilinear, layout))
    assert 0 <= worst <= 1


def test_closed_forms_reject_a_wrong_sampler():
    """check_values itself: a sampler with the cutoff at 2^31, and one that keeps the weight of a dead axis, fail it"""
    maps = TC.materials("packed 6x10")[0]
    uv = all_pairs("packed 6x10")
    good = A.filter_maps(maps, np.concatenate([uv, np.zeros((len(uv), 4), F)], 1), 1, True, 1)
    TC.check_values(maps, uv, good, True, np_bilinear)
    dead_u = TC.dead(uv[:, 0], 6) & ~TC.dead(uv[:, 1], 10)
    bad = good.copy()
    bad[dead_u, 0:3] = A.bilinear(maps["albedo"], np.full(dead_u.sum(), F(0.0)), uv[dead_u, 1])[:, :3]    # x = -0.5 instead of 0
    with pytest.raises(AssertionError):
        TC.check_values(maps, uv, bad, True, np_bilinear)
    bad = good.copy()
    both = TC.dead(uv[:, 0], 6) & TC.dead(uv[:, 1], 10)
    bad[both, 4] = (maps["roughness"][1, 0, 0] * (F(1) / F(255)))
    with pytest.raises(AssertionError):
        TC.check_values(maps, uv, bad, True, np_bilinear)


# ---------------------------------------------------------------------------------------------------------------------
# addressing of the packed form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", PACKED_LAYOUTS)
def test_index_model_stays_inside_the_packed_form(layout):
    maps = TC.materials(layout)[0]
    ok, w, h, n_bytes, packed = TC.host_pack(maps)
    assert ok and (w, h) == A.shared_size(maps)
    uv = all_pairs(layout)
    x0, x1, y0, y1 = TC.wrapped_taps(uv[:, 0], uv[:, 1], w, h)
    for x in (x0, x1):
        assert x.min() >= 0 and x.max() < w
    for y in (y0, y1):
        assert y.min() >= 0 and y.max() < h
    assert {0, w - 1} <= set(x0.tolist()) and {0, w - 1} <= set(x1.tolist()) and {0, h - 1} <= set(y0.tolist()) and {0, h - 1} <= set(y1.tolist())
    rec = packed[:n_bytes - TC.PACKED_PAD].reshape(-1, TC.PACKED_TEXEL_BYTES)
    t = {k: np.broadcast_to(A.texture_of(maps.get(k), k), (h, w, 4)) for k in A.SHADED}
    for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
        i = TC.packed_index(x, y, w)
        assert i.min() >= 0 and (TC.PACKED_TEXEL_BYTES * i + TC.TAP_LOAD_BYTES <= n_bytes).all(), "a 12-byte tap load leaves the allocation"
        # and the record there is the texel the sampler means
        assert np.array_equal(rec[i, 0:3], t["albedo"][y, x, :3]) and np.array_equal(rec[i, 3], t["metallic"][y, x, 0])
        assert np.array_equal(rec[i, 4:7], t["normal"][y, x, :3]) and np.array_equal(rec[i, 7], t["roughness"][y, x, 0])
        assert np.array_equal(rec[i, 8], t["ao"][y, x, 0])
    assert (TC.PACKED_TEXEL_BYTES * TC.packed_index(w - 1, h - 1, w) + TC.TAP_LOAD_BYTES) <= n_bytes
    assert int(TC.packed_index(np.arange(w * h) % w, np.arange(w * h) // w, w).max()) * 9 + 12 <= 2 ** 32 - 1     # uint32 byte offsets


# ---------------------------------------------------------------------------------------------------------------------
# the host pack function
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", TC.LAYOUTS)
def test_host_pack_function(layout):
    for maps, expect in zip(TC.materials(layout), TC.expect_packed(layout)):
        ok, w, h, n_bytes, packed = TC.host_pack(maps)
        size = A.shared_size(maps)
        assert ok == expect == (size is not None)
        if not ok:
            assert (w, h, n_bytes, packed) == (0, 0, 0, None)
            continue
        assert (w, h) == size and n_bytes == TC.packed_bytes_needed(w, h) == len(packed)
        want = TC.pack_bytes(maps)
        assert np.array_equal(packed, want)
        # what the equality above contains, said separately
        rec = packed[:-TC.PACKED_PAD].reshape(-1, 9)
        inside = np.zeros(len(rec), bool)
        y, x = np.divmod(np.arange(w * h), w)
        inside[TC.packed_index(x, y, w)] = True
        assert inside.sum() == w * h and not rec[~inside].any() and not packed[-TC.PACKED_PAD:].any(), "padding is not zero"
        for k, cols in (("albedo", [0, 1, 2]), ("metallic", [3]), ("normal", [4, 5, 6]), ("roughness", [7]), ("ao", [8])):
            if maps.get(k) is None:
                assert (rec[inside][:, cols] == np.array(A.DEFAULT_TEXEL[k][:len(cols)], np.uint8)).all(), f"{k}: not the default texel"


def test_a_supplied_1x1_map_beside_a_larger_one_is_unpacked_in_either_order():
    rng = np.random.Generator(np.random.PCG64(3))
    big = lambda: rng.integers(0, 256, (10, 6, 4), dtype=np.uint8)
    one = lambda: rng.integers(0, 256, (1, 1, 4), dtype=np.uint8)
    for small in A.SHADED:
        for others in (A.SHADED, ("albedo", "normal"), ("ao",)):
            maps = {k: big() for k in others if k != small}
            if not maps:
                continue
            maps[small] = one()
            assert A.shared_size(maps) is None
            assert TC.host_pack(maps)[:4] == (False, 0, 0, 0), (small, others)
    assert TC.host_pack({"height": big(), "albedo": one()})[:3] == (True, 1, 1)       # the height map is not one of the five
    assert TC.host_pack({"albedo": one(), "ao": one()})[:3] == (True, 1, 1)


def test_pack_entry_point_arguments():
    from bibim_renderer_amd import _capi
    L = _capi.lib()
    ok, w, h, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
    arr = (_capi.BbrImage * 6)()
    assert L.bbr_pack_material(None, C.byref(ok), C.byref(w), C.byref(h), C.byref(n), None, 0) == -1
    assert L.bbr_pack_material(arr, None, C.byref(w), C.byref(h), C.byref(n), None, 0) == -1
    out = np.zeros(64, np.uint8)
    assert L.bbr_pack_material(arr, C.byref(ok), C.byref(w), C.byref(h), C.byref(n), out.ctypes.data, 24) == -8    # capacity
    assert (ok.value, w.value, h.value, n.value) == (1, 1, 1, 9 * 16 + 16) and not out.any()
    a = np.zeros((1, 4, 4), np.uint8)
    arr[0] = _capi.BbrImage(a.ctypes.data, 16385, 1)
    assert L.bbr_pack_material(arr, C.byref(ok), C.byref(w), C.byref(h), C.byref(n), None, 0) == -1


def test_pack_header_under_address_and_ub_sanitizers(tmp_path):
    """tests/pack_material_check.cpp with the host compiler: heap images at their exact sizes through csrc/bb_pack.h"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pack_material_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing to preload
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "bibim_renderer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pack_material_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(" ok") == 7 and "WRONG" not in p.stdout
