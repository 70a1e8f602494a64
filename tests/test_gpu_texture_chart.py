"""GPU: the texture sampler (`bilinear_taps`, `wrap_repeat`, the block-linear addressing, `filter_channel`; csrc/bb_kernels.hip.h)
on hazard texture coordinates and every material layout, through all six of its call forms: the packed taps and the per-map
path of k_shade, the height fetch of the deferred pass, PackedFetch and MapFetch of k_shade_aniso, and the dumping
instantiation behind bbr_read_surface.

tests/texture_chart.py builds the frames (128 x 128: one primitive per pixel with a planted uv, or one quad with a uv
gradient).  Every layout x chart x pass is rendered with max_anisotropy 1 and 16, one renderer per frame, and held against
(the numbers return in the messages):
  1  the whole pipeline at max_anisotropy 1: frame, winner, depth bits, n_shaded (deferred: the G-buffer) equal the oracle's
  2  the dumped vUV equals the oracle's (FLAG_OUTPUT_UV) and, on the point charts, the planted values; the census on the dump
  3  slots 12..27 of the dump equal aniso_reference.filter_maps on the dump's own uv and differences, bit for bit
  4  the production kernel is tied to the dump: the frame equals the oracle's light loop on the dumped surface
  5  at max_anisotropy 1 the dumped values (the normal sample included) agree with the Vulkan text in binary64 and with the
     two closed forms
  6  tile shape, item route and a partition of three do not change a bit
"equal": surface_chart.equal_but_for_nan_payload.  The wall time of this file is recorded in tests/golden/texture_chart.json."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import surface_chart as SC
import texture_chart as TC
from test_oracle_contract import np_bilinear
from bibim_renderer_amd import Renderer
from bibim_renderer_amd import partition as P
from oracle import bbo

pytestmark = pytest.mark.gpu

W, H, N_PIX = TC.W, TC.H, TC.N_PIX
equal = SC.equal_but_for_nan_payload
bits = SC.bits
pass_id = lambda d: "deferred" if d else "forward"


def gpu(layout, chart, deferred, max_aniso, **opts):
    """one frame and its read-backs"""
    sc = TC.scene(layout, chart)
    r = Renderer(W, H)
    r.set_option("render_pass", deferred)
    r.set_option("max_anisotropy", max_aniso)
    for k, v in opts.items():
        r.set_option(k, v)
    r.render_scene(sc)
    g = SimpleNamespace(frame=r.read_framebuffer(), surf=r.read_surface(), stats=r.stats())
    g.prim, g.depth = r.read_visibility()
    g.gbuf = r.read_gbuffer() if deferred else None
    again = r.read_framebuffer()           # the dumps re-render the frame: the same bits
    r.close()
    assert equal(again, g.frame)
    assert not g.surf[..., 28:].any()
    return g


@functools.lru_cache(None)
def oracle_of(layout, chart, deferred):
    sc = TC.scene(layout, chart)
    if deferred:
        ref, gbuf, prim, depth, st = bbo.render_deferred(sc)
    else:
        ref, prim, depth, st = bbo.render(sc)
        gbuf = None
    uv = bbo.render(sc, flags=bbo.FLAG_OUTPUT_UV, want_prim=False, want_depth=False)[0][..., :2]
    return SimpleNamespace(frame=ref, gbuf=gbuf, prim=prim, depth=depth, stats=st, uv=np.ascontiguousarray(uv))


def mismatch(got, want):
    ng, nw = np.isnan(got), np.isnan(want)
    diff = (ng != nw) | (~nw & ~ng & (bits(got) != bits(want)))
    return f"{int(diff.reshape(N_PIX, -1).any(-1).sum())} pixels differ, first at {np.argwhere(diff.reshape(N_PIX, -1).any(-1))[:3].ravel().tolist()}"


def check_frame(layout, chart, deferred, max_aniso, g):
    """assertions 1-5 on one frame; returns the worst error / tolerance of 5 (None at max_anisotropy 16)"""
    sc = TC.scene(layout, chart)
    o = oracle_of(layout, chart, deferred)
    rec = g.surf.reshape(N_PIX, 32)
    # -- 1 (the parts that do not depend on the option) and 2 --
    assert (o.prim != bbo.NO_PRIM).all(), "the chart does not cover the frame"
    assert np.array_equal(g.prim, o.prim), f"1: {int((g.prim != o.prim).sum())} pixels pick another primitive"
    assert np.array_equal(bits(g.depth), bits(o.depth)), "1: depth"
    assert g.stats["n_shaded"] == o.stats["n_shaded"] == N_PIX and g.stats["n_clipped_prims"] == o.stats["n_clipped_prims"]
    assert equal(rec[:, :2], o.uv.reshape(-1, 2)), f"2: the dumped vUV is not the oracle's ({mismatch(rec[:, :2], o.uv.reshape(-1, 2))})"
    if chart in TC.POINT_CHARTS:
        assert np.array_equal(g.prim, TC.expected_prim(layout))
        assert equal(rec[:, :2], TC.arriving_uv(TC.planted_uv(layout), chart)), "2: the dumped vUV is not the planted one"
        TC.check_census(layout, chart, rec[:, :2])
    # -- 3 --
    want = TC.filter_rows(layout, chart, g.prim, rec, deferred, max_aniso)
    counts = rec[:, 22:28]
    assert np.array_equal(counts, want[:, 10:]), f"3: tap counts ({int((counts != want[:, 10:]).any(-1).sum())} pixels)"
    assert np.array_equal(bits(rec[:, 12:28]), bits(want)), f"3: filtered values ({mismatch(rec[:, 12:28], want)})"
    sampled = counts[:, [0, 1, 2, 3, 4] + ([5] if deferred else [])]
    assert (sampled >= 1).all() and counts.max() <= max_aniso and (deferred or not counts[:, 5].any())
    if chart == "flat" or max_aniso == 1:
        assert (sampled == 1).all(), "3: more than one tap without a footprint"
    elif chart == "steep":
        wild = ~np.isfinite(rec[:, 2:6]).all(-1)
        assert wild.sum() >= TC.MIN_CLASS and (sampled[wild] == 1).all(), "3: a non-finite difference must give one tap"
        assert (sampled[~wild] > 1).any()
    # (the gradient charts: the uv gradient is the same along both axes, so a second tap is asked for where w != h only --
    #  the counts are the model's, above)
    # -- 4 --
    if not deferred:
        inputs = rec[:, 6:18]
    else:
        tex = g.gbuf.reshape(N_PIX, 4, 4)
        for a, cols in enumerate((slice(6, 9), slice(9, 12), slice(12, 15))):
            assert equal(tex[:, a, :3], bbo.half_round(rec[:, cols])), f"4: G-buffer attachment {a} is not the rounded dump"
        assert equal(tex[:, 3], bbo.half_round(rec[:, 15:19])), "4: G-buffer attachment 3 is not the rounded dump"
        inputs = SC.gbuffer_values(g.gbuf)
    lit = bbo.light_surface(sc.frame, sc.view, inputs, literal=False).reshape(H, W, 4)
    assert equal(g.frame, lit), f"4: the frame is not the oracle's loop on the dumped surface ({mismatch(g.frame, lit)})"
    if max_aniso != 1:
        return None
    # -- 1, the rest --
    if deferred:
        assert equal(g.gbuf, o.gbuf), f"1: G-buffer texels differ ({mismatch(g.gbuf, o.gbuf)})"
    assert equal(g.frame, o.frame), f"1: the frame is not the oracle's ({mismatch(g.frame, o.frame)})"
    # -- 5 --
    which = TC.pixel_material(layout, chart, g.prim)
    worst = 0.0
    for i, maps in enumerate(TC.materials(layout)):
        at = np.flatnonzero(which == i)
        worst = max(worst, TC.check_values(maps, rec[at, :2], rec[at, 12:22], deferred, np_bilinear, f"5: {layout}"))
    return worst


@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("chart", TC.CHARTS)
@pytest.mark.parametrize("layout", TC.LAYOUTS)
def test_sampler(layout, chart, deferred):
    for max_aniso in (1, 16):
        g = gpu(layout, chart, deferred, max_aniso)
        worst = check_frame(layout, chart, deferred, max_aniso, g)
        if worst is not None:
            print(f"5: {layout} | {chart} | {pass_id(deferred)}: worst error / tolerance against binary64 {worst:.4g}")
            assert worst <= 1


# ---------------------------------------------------------------------------------------------------------------------
# 6. invariances
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("chart", ["steep", "coarse"])
@pytest.mark.parametrize("layout", TC.INVARIANCE_LAYOUTS)
def test_tile_shape_item_route_and_partition_do_not_change_a_bit(layout, chart, deferred):
    sc = TC.scene(layout, chart)
    base = gpu(layout, chart, deferred, 16)
    for opts in ({"tile_mode": 0}, {"no_tail_items": 0}, {"no_tail_items": 0, "heavy_tiles": 4}):
        g = gpu(layout, chart, deferred, 16, **opts)
        assert equal(g.frame, base.frame), opts
        assert equal(g.surf, base.surf), opts
    shards = []
    for rank in range(3):
        r = Renderer(W, H)
        r.set_option("render_pass", deferred)
        r.set_option("max_anisotropy", 16)
        band_rows = r.tile_height()
        r.set_partition(rank, 3, band_rows)
        r.render_scene(sc)
        shards.append(r.read_shard())
        r.close()
    assert equal(P.unpack_gathered(np.stack(shards), H, band_rows), base.frame), "partition of three"
