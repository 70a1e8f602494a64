"""GPU: what the library allocates for itself is given back -- all of it when a context is destroyed, and exactly the stated
groups when an option or a resize drops buffers (csrc/bb_own.h, bbr_debug_live_resources).  Small extents, one-triangle meshes,
8 x 8 and 5 x 3 maps: the counts do not depend on the sizes."""
import functools
import gc

import numpy as np
import pytest

import resolve_reference as RR
import ui_reference as U
from bibim_renderer_amd import Renderer
from bibim_renderer_amd.renderer import TBN_SEGMENT_DTYPE, UiDrawData, live_resources
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 64
W2, H2 = 96, 64


def same(a, b):
    """bit for bit; NaN by placement"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


@functools.lru_cache(None)
def scene(w, h):
    """the triangle scene, one object per extent: a Renderer's handles are keyed by the scene's arrays"""
    return scenes.triangle_scene(w, h)


def gizmo():
    """a one-triangle gizmo: float32 [3, 9] = pos, colour, normal"""
    v = np.zeros((3, 9), F)
    v[:, 0:3] = [(0, 1, 0), (1, -1, 0), (-1, -1, 0)]
    v[:, 3:6] = (0.9, 0.2, 0.1)
    v[:, 6:9] = (0, 0, 1)
    return v, np.arange(3, dtype=np.uint32)


def ui_draw(w, h, texture):
    d = U.assemble([((0, 0, w, h), texture, [U.quad(3.25, 2.5, 30.0, 20.75, U.rgba(40, 220, 130, 150))])], (w, h))
    return UiDrawData(d.vertices, d.indices, d.cmds, d.display_pos, d.display_size, d.framebuffer_scale)


def use_every_owner(rng):
    """one context from bbr_create to bbr_destroy that has held every kind of thing the library owns"""
    image = lambda h, w: rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    r = Renderer(W, H)
    r.upload_gizmo(*gizmo())
    # materials: packed (the supplied maps agree on a size) and not, chains built by the option and by the upload, freed and kept
    packed = r.upload_material({"albedo": image(8, 8), "normal": image(8, 8)})
    unpacked = r.upload_material({"albedo": image(8, 8), "roughness": image(3, 5)})
    r.set_option("mip_levels", 3)
    under_mip = r.upload_material({"albedo": image(3, 5), "ao": image(3, 5)})
    assert r.read_material_level(packed, 0, 2).shape == (2, 2, 4) and len(r.read_packed_level(packed, 1)) > 0
    assert len(r.read_packed_level(unpacked, 0)) == 0
    r.set_option("mip_levels", 1)
    r.free_material(unpacked)
    r.free_material(under_mip)
    tri = scene(W, H)
    v = tri.draws[0].vertices
    r.free_mesh(r.upload_mesh(v, np.arange(3, dtype=np.uint32)))
    r.upload_mesh(v)                                               # alive at destroy, like `packed`
    freed = r.upload_ui_texture(image(8, 8))
    kept = r.upload_ui_texture(image(3, 5))                        # alive at destroy
    r.free_ui_texture(freed)

    # overlays + TBN lines + presentation + GUI; the dumps of the read-backs
    r.set_option("overlays", 1)
    r.set_option("tbn", 1)
    handles = r.render_scene(tri)
    r.present()
    r.draw_overlays(16)
    r.draw_ui(ui_draw(W, H, kept))
    assert r.read_presented().shape == (H, W, 4)
    assert (r.read_visibility()[0] != 0xFFFFFFFF).any() and r.read_surface().shape == (H, W, 32)
    r.set_option("render_pass", 1)
    r.render_scene(tri, handles)
    assert r.read_gbuffer().shape == (H, W, 4, 4)
    r.set_option("render_pass", 0)

    # merged supersampling with a depth rule, timed
    r.set_option("supersample", 2)
    r.set_option("sample_shading", 0)
    r.set_option("depth_resolve", 8)
    r.set_option("timing", 1)
    r.render_scene(scene(2 * W, 2 * H), handles)
    r.present()
    r.draw_overlays(16)
    assert (r.read_visibility()[0] != 0xFFFFFFFF).any() and r.resolve_timing()[0] >= 1
    r.set_option("timing", 0)

    # the option changes that drop buffers, and every slot
    r.set_option("tile_mode", 0)
    r.render_scene(scene(2 * W, 2 * H), handles)
    r.resize(W2, H2)
    r.set_option("frames_in_flight", 4)
    for _ in range(4):
        r.render_scene(scene(2 * W2, 2 * H2), handles)
    assert r.read_framebuffer().shape == (H2, W2, 4)

    # the self-tests' scratch
    assert r.selftest_rcp(0x3F800000, 0x3F800000 + 4000) == 0
    seg = np.zeros(1, TBN_SEGMENT_DTYPE)
    seg[0] = (256 * 4, 256 * 5, 256 * 40, 256 * 30, 0.25, 0.25, 7, 0)
    assert r.selftest_lines(seg, W, H, np.ones((H, W), F)).shape == (H, W)
    r.close()


def test_live_counts_return_to_the_base_after_destroy():
    gc.collect()
    base = live_resources()
    rng = np.random.default_rng(5)
    for cycle in range(3):
        use_every_owner(rng)
        gc.collect()
        assert live_resources() == base, cycle                     # a condition, not a measurement


# What each step frees, counted by name from the lists the library kept by hand before its buffers were grouped at their
# declarations (FrameSlot::release_tile_buffers, drop_extent_buffers, TbnPass::release; today TileSized, ExtentSized, TbnRecords and
# ExtentDumps in csrc/bibim_hip.hip), for a context at n = 1 with options "overlays" and "tbn", two frames in flight, both slots
# rendered and presented, overlays drawn, visibility read:
TILE = ["d_tile_count", "d_bins", "d_frags", "d_frag_count", "d_items", "d_item_groups", "d_cooked", "d_heavy"]  # release_tile_buffers' eight
OV_TILE = TILE[:4]          # ... of which the overlay slot holds what ensure_pass_buffers allocates
EXTENT = ["d_frame", "d_present", "d_depth"]         # drop_extent_buffers' own six, less d_fine, d_sample_map, d_fine_depth (n = 1)
TBN = ["d_staging", "d_segs", "d_tile_count", "d_bins", "d_ctr", "d_keys"]   # TbnPass::release's six
DUMPS = ["d_vis_prim", "d_vis_depth"]                # drop_extent_buffers' five of the context, less the fine pair (n = 1) and d_gbuffer (forward)
SLOTS = 2
FREED_BY_TILE_MODE = SLOTS * len(TILE) + len(OV_TILE)                                       # 20
FREED_BY_EXTENT = SLOTS * (len(TILE) + len(EXTENT)) + len(OV_TILE) + len(TBN) + len(DUMPS)  # 34


def test_the_drop_sets_are_the_stated_groups():
    assert (FREED_BY_TILE_MODE, FREED_BY_EXTENT) == (20, 34)
    gc.collect()
    base = live_resources()
    r = Renderer(W, H)
    r.upload_gizmo(*gizmo())
    r.set_option("overlays", 1)
    r.set_option("tbn", 1)
    handles = {"mesh": {}, "mat": {}}
    for extent in ((W, H), (W2, H2), (2 * W2, 2 * H2)):            # every mesh and material is uploaded before anything is counted
        r.render_scene(scene(*extent), handles)

    def frame(w, h):
        r.render_scene(scene(w, h), handles)
        return r.read_framebuffer()

    def full_use(w, h):
        """both slots hold a presented frame, the overlay slot, the TBN pass and the visibility dump are allocated"""
        for _ in range(SLOTS):
            out = frame(w, h)
            r.present()
            r.draw_overlays(16)
        r.read_visibility()
        assert same(r.read_framebuffer(), out)
        return out, live_resources()

    def fixed(c):
        return tuple(c[k] - base[k] for k in ("pinned_blocks", "events", "streams"))

    before_frame, full = full_use(W, H)
    assert fixed(full) == (2 * SLOTS, 4 * SLOTS, 4)                # per slot: staging and flag words; three edges and ev_done

    # option "tile_mode": the tile group of every slot, nothing else; the next frame brings back its slot's
    r.set_option("tile_mode", 0)
    after = live_resources()
    assert after["device_allocs"] == full["device_allocs"] - FREED_BY_TILE_MODE and after["device_bytes"] < full["device_bytes"]
    assert fixed(after) == fixed(full)
    assert same(frame(W, H), before_frame)
    assert live_resources()["device_allocs"] == after["device_allocs"] + len(TILE)
    before_frame, again = full_use(W, H)
    assert again["device_allocs"] == full["device_allocs"] and fixed(again) == fixed(full)

    # bbr_resize to the same extent drops nothing
    r.resize(W, H)
    assert live_resources() == again
    assert same(frame(W, H), before_frame) and live_resources() == again

    # bbr_resize to another extent: the tile and the extent group of every slot, the TBN pass, the dumps
    r.resize(W2, H2)
    after = live_resources()
    assert after["device_allocs"] == again["device_allocs"] - FREED_BY_EXTENT and after["device_bytes"] < again["device_bytes"]
    assert fixed(after) == fixed(full)
    oracle = bbo.render(scene(W2, H2))[0]
    assert same(frame(W2, H2), oracle)
    assert live_resources()["device_allocs"] == after["device_allocs"] + len(TILE) + len(["d_frame", "d_depth"])
    before_frame, again = full_use(W2, H2)
    assert same(before_frame, oracle) and again["device_allocs"] == full["device_allocs"] and fixed(again) == fixed(full)

    # option "supersample": the same sets as a resize (no rule in "depth_resolve": a frame at n = 2 keeps no depth)
    r.set_option("supersample", 2)
    after = live_resources()
    assert after["device_allocs"] == again["device_allocs"] - FREED_BY_EXTENT and fixed(after) == fixed(full)
    fine = bbo.render(scene(2 * W2, 2 * H2))[0]
    assert same(frame(2 * W2, 2 * H2), RR.resolve(fine, 2))
    assert live_resources()["device_allocs"] == after["device_allocs"] + len(TILE) + len(["d_frame", "d_fine"])
    r.close()
