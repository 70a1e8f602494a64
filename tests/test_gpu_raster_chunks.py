"""GPU: k_raster's chunk loop with three chunks on one tile.

k_raster stages a tile's entries (class 0 | class 1 | class 2 | every-tile list) through LDS 256 at a time and fetches ahead:
the triangles of chunk k + 1 and the bin references of chunk k + 2 are asked for while chunk k is rasterised.  The references
fetched two chunks ahead are first consumed by a tile's THIRD chunk, i.e. with more than 512 entries on one tile, and no other
small scene is known to get there with 32 x 32 tiles (the margin scenes have at most 393 distinct winners per such tile).

Scene: one 32 x 32 frame -- one 32 x 32 tile, or one 64 x 64 tile three quarters outside the frame.  676 tiny triangles
(class 0), one around each pixel centre of a 26 x 26 block, nearest; behind them four triangles spanning 80 pixels
(class 2, one wave each), one over each edge of the frame so that each wins a strip of the border, and behind those six
spanning 33..64 pixels (class 1); three slivers through the near plane in the two outer columns, nearest of all.  With 676 + 6 + 4 bin entries the class boundaries lie strictly inside the third chunk.  A frame
of a single tile has no triangle that touches more tiles than `broad_threshold`, so the every-tile list holds exactly what
the clipper puts there: the slivers' sub-triangles."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from bibim_renderer_amd import Renderer, textures
from oracle import bbo, scenes

W = H = 32
GRID0, GRID = 3, 26                       # the block of pixels with a tiny triangle each
N_SMALL, N_MID, N_LARGE, N_CLIP = GRID * GRID, 6, 4, 3
N_TRI = N_SMALL + N_MID + N_LARGE + N_CLIP
NO = bbo.NO_PRIM
TAN = np.tan(np.radians(30.0))            # scenes.view_uniforms: fov 60 degrees, aspect 1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def world(px, py, z):
    """the point at depth z whose projection is the pixel coordinate (px, py); the camera looks down +z from the origin"""
    return ((px / (W / 2) - 1.0) * TAN * z, (py / (H / 2) - 1.0) * TAN * z, z)


def upright(cx, cy, s, z):
    """a triangle around pixel coordinate (cx, cy), s pixels to each side, in the winding of the other one-tile scenes"""
    return [world(cx - s, cy + s, z), world(cx + s, cy + s, z), world(cx, cy - s, z)]


@functools.lru_cache(None)
def scene(light_in_front=False):
    rng = np.random.default_rng(5)
    tris = [upright(GRID0 + i + 0.5, GRID0 + j + 0.5, 0.45, 2.0) for j in range(GRID) for i in range(GRID)]
    tris += [upright(*rng.uniform(4, 28, 2), rng.uniform(17, 31), 3.0) for _ in range(N_MID)]      # spans 34..62 pixels
    # spans of 80 pixels, one over each edge of the frame, so that each wins pixels of the border the grid leaves free
    tris += [upright(cx, cy, 40.0, 2.5 + 0.1 * k) for k, (cx, cy) in enumerate([(-20, 16), (52, 16), (16, -25), (16, 60)])]
    for k in range(N_CLIP):                                                                        # the apex: behind the camera
        cx, s = (1.3, 30.7, 1.5)[k], 1.2
        tris.append([world(cx - s, 20 + 3 * k + s, 1.0), world(cx + s, 20 + 3 * k + s, 1.0), (world(cx, 0, 1.0)[0], -6.0 * TAN, -0.5)])
    v = np.zeros(3 * N_TRI, bbo.VERTEX_DTYPE)
    v["pos"] = np.asarray(tris, np.float32).reshape(-1, 3)
    v["uv"] = rng.uniform(-2, 2, (3 * N_TRI, 2))
    v["normal"], v["tangent"] = (0, 0, -1), (1, 0, 0)
    inst = np.zeros(1, bbo.INSTANCE_DTYPE)
    inst[0] = scenes.instance(np.eye(4, dtype=np.float32))
    pos = (0.1, 0.1, 1.5) if light_in_front else (0.3, 0.5, 0.0)
    fu = scenes.frame_uniforms([scenes.light(0, pos=pos, color=(1.0, 0.9, 0.8), intensity=6.0)], 1, 1.2)
    vu = scenes.view_uniforms((0, 0, 0), 0, 0, W, H, 1)
    return bbo.Scene(fu, vu, [bbo.DrawData(v, None, inst, bbo.MaterialData(textures.make_material(16)))], W, H, "raster chunks")


@functools.lru_cache(None)
def oracle(light_in_front=False):
    o = SimpleNamespace()
    o.frame, o.prim, o.depth, o.stats = bbo.render(scene(light_in_front))
    return o


def test_the_scene_puts_three_chunks_of_every_kind_on_the_tile():
    """on the oracle alone, no GPU: every winner is a bin entry of the one tile, so 513 distinct winners are three chunks;
    and a winner of each kind -- small, class 2, every-tile list = clipped"""
    o = oracle()
    won = np.unique(o.prim[o.prim != NO])
    small, mid, large = N_SMALL, N_SMALL + N_MID, N_SMALL + N_MID + N_LARGE
    kinds = {"small": int((won < small).sum()), "class 1": int(((won >= small) & (won < mid)).sum()),
             "class 2": int(((won >= mid) & (won < large)).sum()), "clipped": int((won >= large).sum())}
    print(f"distinct winners {len(won)}: {kinds}; clipped primitives {o.stats['n_clipped_prims']}, raster triangles {o.stats['n_raster_tris']}")
    assert len(won) >= 513
    assert kinds["small"] >= 513 and kinds["class 1"] >= 1 and kinds["class 2"] == N_LARGE and kinds["clipped"] >= 1
    assert o.stats["n_clipped_prims"] == N_CLIP          # the every-tile list of a one-tile frame: the clipper's sub-triangles
    # the raster classes (k_geometry's raster_class): larger side of the bounding box in pixels
    p = scene().draws[0].vertices["pos"].reshape(N_TRI, 3, 3)[:large]
    px = (p[..., :2] / (p[..., 2:3] * TAN) + 1.0) * (W / 2)
    span = (px.max(axis=1) - px.min(axis=1)).max(axis=1)
    assert (span[:small] < 1.0).all()
    assert ((span[small:mid] > 32.5) & (span[small:mid] < 63.5)).all()
    assert (span[mid:] > 64.5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("tile_mode", [0, 1])
def test_forward_frame_winner_depth_and_count(tile_mode, item_route):
    sc, o = scene(), oracle()
    r = Renderer(W, H)
    r.set_option("tile_mode", tile_mode)
    r.render_scene(sc)
    frame = r.read_framebuffer()
    prim, depth = r.read_visibility()
    st = r.stats()
    r.close()
    assert np.array_equal(prim, o.prim) and np.array_equal(depth.view(np.uint32), o.depth.view(np.uint32))
    assert st["n_shaded"] == o.stats["n_shaded"] and st["n_clipped_prims"] == N_CLIP
    assert np.array_equal(bits(frame), bits(o.frame))


@pytest.mark.gpu
@pytest.mark.parametrize("tile_mode", [0, 1])
def test_overlay_marker_over_the_stored_depth(tile_mode, item_route):
    """option "overlays": k_raster stores the resolved depth and the overlay pass reads it again -- a light marker in front
    of the grid, as tests/test_gpu_overlays.py expects it"""
    sc, o = scene(True), oracle(True)
    base = bbo.present(o.frame, 1, 1.2)
    want, _ = bbo.overlay(sc.frame, sc.view, o.depth, base, None, None, 0)
    assert (want != base).any()
    r = Renderer(W, H)
    r.set_option("tile_mode", tile_mode)
    r.set_option("overlays", 1)
    r.render_scene(sc)
    r.present()
    assert np.array_equal(r.read_presented(), base)
    r.draw_overlays(0)
    got = r.read_presented()
    r.close()
    assert np.array_equal(got, want)
