"""GPU: how many references k_geometry's bin loop writes and where it routes primitives -- the bin chart.

`bbr_stats` reports n_bin_refs (references written to tile bins) and n_broad_tris (entries of the every-tile list); this
file pins them, with n_raster_tris and n_clipped_prims, on the vertex chart's two 160 x 128 views (tests/vertex_chart.py: 154
primitives, twelve draws), forward pass, both tile sizes, three values of option `broad_threshold`, whole and partitioned.

The model is independent of the code under test: the snapped coordinates are VC.setup() of the oracle's clip positions, the
fate is VC.fate(); on top of them it restates in numpy
    box    pixels whose centres lie in the triangle's bounding box, clamped to the frame: first = (min - 128 + 255) >> 8,
           last = (max - 128) >> 8 in 24.8 fixed point
    tiles  box / tile size; a survivor of more tiles than broad_threshold goes to the every-tile list, every other one to
           the bin of each of its tiles
    bands  tile row ty belongs to rank (ty / band_tiles) mod world; a rank keeps a survivor that has a row of its own and
           writes the references of its own rows only.  Every rank clips every primitive that crosses the guard band, and the
           clipper's sub-triangles go to the every-tile list: their number is the oracle's n_raster_tris minus the unclipped
           survivors (zero for the main view).
The last test outgrows the TBN overlay's bins (1024 entries per 32 x 32 tile to begin with) at the smallest size: the
one-tile scene of tests/test_gpu_raster_chunks.py puts several thousand segments on its tile, so the shared reservation's
overflow branch and the host's redo run."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import tbn_reference as tr
import vertex_chart as VC
from bibim_renderer_amd import Renderer
from oracle import bbo
from test_gpu_raster_chunks import oracle as one_tile_oracle, scene as one_tile_scene
from test_gpu_tbn_overlay import same_records

W, H = VC.W, VC.H
TILE = {0: 64, 1: 32}                     # option tile_mode -> tile size
DEFAULT_THRESHOLD = 16                    # option broad_threshold as a context starts
THRESHOLDS = (1, DEFAULT_THRESHOLD, 100000)
TBN_BIN_START = 1024                      # entries per TBN bin before the first overflow
WHOLE = [(v, m, t) for v in VC.VIEWS for m in (0, 1) for t in THRESHOLDS]
PARTS = [(v, m, w) for v in VC.VIEWS for m in (0, 1) for w in (2, 3)]


@functools.lru_cache(None)
def survivors(view, tile):
    """tile ranges [n] of the view's unclipped survivors, and the number of sub-triangles its clipper leaves"""
    clip, _ = VC.stage(view, 0)
    st = VC.setup(clip)
    u = (VC.fate(clip) == "unclipped") & st.ok
    X, Y = st.X[u].astype(np.int64), st.Y[u].astype(np.int64)
    px0, px1 = np.maximum((X.min(1) - 128 + 255) >> 8, 0), np.minimum((X.max(1) - 128) >> 8, W - 1)
    py0, py1 = np.maximum((Y.min(1) - 128 + 255) >> 8, 0), np.minimum((Y.max(1) - 128) >> 8, H - 1)
    assert (px0 <= px1).all() and (py0 <= py1).all()
    o = VC.oracle_frame(view, 0).stats
    return SimpleNamespace(tx0=px0 // tile, tx1=px1 // tile, ty0=py0 // tile, ty1=py1 // tile, n=int(u.sum()),
                           clipped_sub=int(o["n_raster_tris"]) - int(u.sum()), n_clipped_prims=int(o["n_clipped_prims"]),
                           n_raster_tris=int(o["n_raster_tris"]))


def model(view, tile, threshold, world=1, rank=0, band_tiles=1):
    s = survivors(view, tile)
    width = s.tx1 - s.tx0 + 1
    ntiles = width * (s.ty1 - s.ty0 + 1)
    rows = np.arange(-(-H // tile))
    mine = (rows // band_tiles) % world == rank
    own_rows = np.array([int(mine[a:b + 1].sum()) for a, b in zip(s.ty0, s.ty1)])
    kept = own_rows > 0
    binned = kept & (ntiles <= threshold)
    return {"n_bin_refs": int((width * own_rows)[binned].sum()), "n_broad_tris": int((kept & ~binned).sum()) + s.clipped_sub,
            "n_raster_tris": int(kept.sum()) + s.clipped_sub, "n_clipped_prims": s.n_clipped_prims}


@functools.lru_cache(None)
def gpu_stats(view, tile_mode, threshold, world=1, rank=0):
    r = Renderer(W, H)
    r.set_option("tile_mode", tile_mode)
    r.set_option("broad_threshold", threshold)
    if world > 1:
        r.set_partition(rank, world, TILE[tile_mode])            # a band of one tile row
    r.render_scene(VC.scene(view))
    st = r.stats()
    r.close()
    assert st["tile_w"] == st["tile_h"] == TILE[tile_mode]
    return st


def test_the_model_is_not_vacuous():
    """CPU: one-tile and several-tile primitives, both sides of a threshold, references on every rank"""
    for tile in TILE.values():
        s = survivors("main", tile)
        ntiles = (s.tx1 - s.tx0 + 1) * (s.ty1 - s.ty0 + 1)
        print(f"main view, {tile} x {tile} tiles: {s.n} survivors, {int((ntiles == 1).sum())} of one tile, {int((ntiles > 1).sum())} of "
              f"more, {int((ntiles > DEFAULT_THRESHOLD).sum())} above the default threshold")
        assert s.n >= 138 and s.clipped_sub == 0 and s.n_clipped_prims == 0
        assert (ntiles == 1).any() and (ntiles > 1).any()
        assert (ntiles > DEFAULT_THRESHOLD).any() or (ntiles > 1).any()      # above the default threshold, or else above 1
        a, b = model("main", tile, 1), model("main", tile, 100000)
        assert 0 < a["n_bin_refs"] < b["n_bin_refs"] and a["n_broad_tris"] > 0 and b["n_broad_tris"] == 0
        assert b["n_bin_refs"] == int(ntiles.sum()) and a["n_raster_tris"] == b["n_raster_tris"] == s.n
        for world in (2, 3):
            parts = [model("main", tile, DEFAULT_THRESHOLD, world, rank) for rank in range(world)]
            assert sum(p["n_bin_refs"] for p in parts) == model("main", tile, DEFAULT_THRESHOLD)["n_bin_refs"]
            assert sum(p["n_raster_tris"] for p in parts) > s.n              # a primitive across a band border is kept twice
    assert all(model("main", 32, DEFAULT_THRESHOLD, 3, rank)["n_bin_refs"] > 0 for rank in range(3))
    near = survivors("near", 32)
    assert near.n_clipped_prims == 8 and near.clipped_sub >= 8 and near.n >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("view,tile_mode,threshold", WHOLE, ids=lambda v: str(v))
def test_references_and_routes(view, tile_mode, threshold):
    got, want = gpu_stats(view, tile_mode, threshold), model(view, TILE[tile_mode], threshold)
    print(f"{view} tile_mode {tile_mode} broad_threshold {threshold}: got " + ", ".join(f"{k} {got[k]}" for k in want) + f"; want {want}")
    assert {k: got[k] for k in want} == want
    assert want["n_raster_tris"] == survivors(view, TILE[tile_mode]).n_raster_tris      # the oracle's


@pytest.mark.gpu
@pytest.mark.parametrize("view,tile_mode,world", PARTS, ids=lambda v: str(v))
def test_partitioned_references(view, tile_mode, world):
    whole = gpu_stats(view, tile_mode, DEFAULT_THRESHOLD)
    total = 0
    for rank in range(world):
        got = gpu_stats(view, tile_mode, DEFAULT_THRESHOLD, world, rank)
        want = model(view, TILE[tile_mode], DEFAULT_THRESHOLD, world, rank)
        print(f"{view} tile_mode {tile_mode} rank {rank} of {world}: got " + ", ".join(f"{k} {got[k]}" for k in want) + f"; want {want}")
        assert {k: got[k] for k in want} == want
        total += got["n_bin_refs"]
    assert total == whole["n_bin_refs"]


@functools.lru_cache(None)
def one_tile_tbn():
    sc = one_tile_scene()
    want = tr.tbn_records(sc)
    return sc, want


def tbn_tile_entries(segs, width, height):
    """segments whose pixel bounding box, one pixel of slack each side, meets the target (the TBN bins' rule)"""
    x0 = np.maximum((np.minimum(segs["x0"], segs["x1"]) >> 8) - 1, 0); x1 = np.minimum((np.maximum(segs["x0"], segs["x1"]) >> 8) + 1, width - 1)
    y0 = np.maximum((np.minimum(segs["y0"], segs["y1"]) >> 8) - 1, 0); y1 = np.minimum((np.maximum(segs["y0"], segs["y1"]) >> 8) + 1, height - 1)
    return int(((x0 <= x1) & (y0 <= y1)).sum())


def test_the_one_tile_scene_outgrows_a_tbn_bin():
    """CPU: the reference puts more segments on the one 32 x 32 tile than a TBN bin starts with"""
    sc, want = one_tile_tbn()
    n = tbn_tile_entries(want, sc.width, sc.height)
    print(f"one-tile scene: {len(want)} segments, {n} on the tile")
    assert sc.width == sc.height == 32 and n > TBN_BIN_START


@pytest.mark.gpu
def test_tbn_bins_outgrown_on_one_tile():
    sc, want = one_tile_tbn()
    o = one_tile_oracle()
    base = bbo.present(o.frame, 1, 1.2)
    lines = tr.composite(base, tr.resolve(want, sc.width, sc.height, o.depth))
    want_img, _ = bbo.overlay(sc.frame, sc.view, o.depth, lines, None, None, 0)
    assert (lines != base).any()
    r = Renderer(sc.width, sc.height)
    r.set_option("overlays", 1)
    r.set_option("tbn", 1)
    r.render_scene(sc)
    r.present()
    assert np.array_equal(r.read_presented(), base)
    r.draw_overlays(0)
    got, img = r.read_tbn_segments(), r.read_presented()
    r.close()
    same_records(got, want)
    bad = (img != want_img).any(axis=2)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5])
