"""TBN line overlay (option "tbn"; tbn.vert / tbn.geom / tbn.frag): the GPU's segment records, its line raster and
resolve, and the presented bytes against the CPU restatement in tbn_reference.py, exactly."""
import os

import numpy as np
import pytest

import tbn_reference as tr
from conftest import GOLDEN
from bibim_renderer_amd import BibimError, Renderer, configs
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

CFG = configs.C3.scaled(640, 360, 64)
FIELDS = ("x0", "y0", "x1", "y1", "za", "zb", "key")


def gizmo():
    g = np.load(os.path.join(GOLDEN, "gizmo.npz"))
    gv = np.zeros(len(g["vertices"]), bbo.GIZMO_VERTEX_DTYPE)
    gv["pos"], gv["color"], gv["normal"] = g["vertices"][:, 0:3], g["vertices"][:, 3:6], g["vertices"][:, 6:9]
    return g["vertices"], g["indices"], gv


def scene(maps, enable, cfg=CFG):
    sc = scenes.shaderball_scene(cfg, bbo.MaterialData(maps))
    sc.view["enable_normal_map"] = enable
    return sc


@pytest.fixture(scope="module")
def cpu_records(maps64):
    return {e: tr.tbn_records(scene(maps64, e)) for e in (0, 1)}


def same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in FIELDS:
        a, b = got[f], want[f]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.nonzero(a != b)[0]
        assert not len(bad), (f, len(bad), got[bad[:3]], want[bad[:3]])


def tbn_renderer(cfg, deferred=False, tile_mode=1):
    r = Renderer(cfg.width, cfg.height)
    r.set_option("tile_mode", tile_mode)
    r.set_option("render_pass", int(deferred))
    r.set_option("overlays", 1)
    r.set_option("tbn", 1)
    return r


def test_selftest_lines_hand_set_random_segments_and_depth_ties():
    from test_tbn_line_rule import HAND, random_segments
    W, H = 100, 70                                                 # not a multiple of the 32-pixel tile
    hand = np.zeros(len(HAND), tr.TBN_SEGMENT_DTYPE)
    for i, (s, _) in enumerate(HAND):
        hand[i] = (s[0] + 256 * 40, s[1] + 256 * 30, s[2] + 256 * 40, s[3] + 256 * 30, 0.5, 0.5, 10 * i + 3, 0)
    rng = np.random.default_rng(11)
    rnd = random_segments(6000, 5, span=8)
    shift_x, shift_y = 256 * rng.integers(-6, W - 4, len(rnd)), 256 * rng.integers(-6, H - 4, len(rnd))
    for f, sh in (("x0", shift_x), ("x1", shift_x), ("y0", shift_y), ("y1", shift_y)):
        rnd[f] += sh.astype(np.int32)
    rnd["za"] = rng.choice([0.25, 0.5, 0.75], len(rnd)).astype(np.float32)  # exact ties with the depth buffer
    rnd["zb"] = np.where(rng.random(len(rnd)) < 0.5, rnd["za"], rng.random(len(rnd))).astype(np.float32)
    rnd["key"] = rng.permutation(1 << 20)[:len(rnd)].astype(np.uint32) + 1000
    long = np.zeros(3, tr.TBN_SEGMENT_DTYPE)                       # across several tiles and out of the target
    long[0] = (-256 * 50, 256 * 10 + 77, 256 * 150, 256 * 60 + 3, 0.1, 0.9, 7, 0)
    long[1] = (256 * 99 + 200, -256 * 20, 256 * 3, 256 * 90, 0.9, 0.1, 9, 0)
    long[2] = (256 * 20, 256 * 5, 256 * 20 + 13, 256 * 69 + 255, 0.5, 0.5, 11, 0)
    segs = np.concatenate([hand, rnd, long])
    depth = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 2.0], np.float32), (H, W))
    want = tr.resolve(segs, W, H, depth)
    r = Renderer(64, 64)
    got = r.selftest_lines(segs, W, H, depth)
    assert (want != 0).sum() > 2000 and np.array_equal(got, want), int((got != want).sum())
    r.set_option("bin_cap", 8)                                     # (the context's bin option does not apply here)
    got = r.selftest_lines(segs[::-1].copy(), W, H, depth)         # order of the records does not matter
    assert np.array_equal(got, want)
    got = r.selftest_lines(segs[:0], W, H, depth)
    assert not got.any()
    r.close()


@pytest.mark.parametrize("tile_mode", [0, 1])
@pytest.mark.parametrize("enable", [0, 1])
@pytest.mark.parametrize("deferred", [False, True])
def test_records_equal_the_cpu(maps64, cpu_records, deferred, enable, tile_mode):
    r = tbn_renderer(CFG, deferred, tile_mode)
    r.render_scene(scene(maps64, enable))
    r.present()
    r.draw_overlays(0)
    got = r.read_tbn_segments()
    same_records(got, cpu_records[enable])
    assert len(got) > 900000
    r.close()


@pytest.mark.parametrize("deferred", [False, True])
def test_presented_bytes_equal_the_cpu_composite(maps64, cpu_records, deferred):
    raw, gi, gv = gizmo()
    sc = scene(maps64, 1)
    sc.frame["enable_tone_mapping"], sc.frame["exposure"] = 1, 1.3
    if deferred:
        hdr, _, _, depth, _ = bbo.render_deferred(sc)
    else:
        hdr, _, depth, _ = bbo.render(sc)
    base = bbo.present(hdr, 1, 1.3)
    keys = tr.resolve(cpu_records[1], CFG.width, CFG.height, depth)
    lines = tr.composite(base, keys)
    want, _ = bbo.overlay(sc.frame, sc.view, depth, lines, gv, gi, 100)
    everything = tr.resolve(cpu_records[1], CFG.width, CFG.height, np.full_like(depth, -np.inf))
    assert (keys != 0).sum() > 5000                                # lines are really there ...
    assert (everything != 0).sum() > (keys != 0).sum() + 1000      # ... and the depth test hid some
    assert (lines != want).any()                                   # the markers and the gizmo are drawn over them
    r = tbn_renderer(CFG, deferred)
    r.upload_gizmo(raw, gi)
    r.render_scene(sc)
    r.present()
    assert np.array_equal(r.read_presented(), base)
    r.draw_overlays(100)
    got = r.read_presented()
    bad = (got != want).any(axis=2)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5])
    r.close()


def test_near_camera_clipping_and_guard_band(maps64):
    """camera inside the ball grid, close to a ball: segments cross z = w, some start behind the camera, some leave
    the guard band"""
    sc = scene(maps64, 1)
    sc.view = scenes.view_uniforms((-1.0, -0.6, 1.55), 10.0, -20.0, CFG.width, CFG.height, 1, 90.0, 0.1, 1000.0)
    want = tr.tbn_records(sc)
    n_prims = sc.n_prims
    assert len(want) < 6 * n_prims - 1000                          # many were clipped away entirely
    assert (np.maximum(want["za"], want["zb"]) > 0.999).sum() > 10   # cut at z = w (reverse-Z near plane)
    lim = 256 * 640 * 2
    assert ((np.abs(want["x0"]) > lim) | (np.abs(want["x1"]) > lim)).any()  # ends out at the guard band
    sc.frame["num_lights"] = 0                                     # no markers: the lines alone (gizmo_extent 0)
    hdr, _, depth, _ = bbo.render(sc)
    base = bbo.present(hdr, 0, 1.0)
    want_img = tr.composite(base, tr.resolve(want, CFG.width, CFG.height, depth))
    r = tbn_renderer(CFG)
    r.render_scene(sc)
    r.present()
    r.draw_overlays(0)
    same_records(r.read_tbn_segments(), want)
    assert np.array_equal(r.read_presented(), want_img)
    r.close()


def test_full_size_c3_image(maps64):
    cfg = configs.C3.scaled(3840, 2160, 64)
    sc = scene(maps64, 1, cfg)
    r = tbn_renderer(cfg)
    r.render_scene(sc)
    _, _, depth, _ = bbo.render(sc)
    r.present()
    base = r.read_presented()
    r.draw_overlays(0)
    got = r.read_presented()
    recs = tr.tbn_records(sc)
    same_records(r.read_tbn_segments(), recs)
    want = tr.composite(base, tr.resolve(recs, cfg.width, cfg.height, depth))
    want, _ = bbo.overlay(sc.frame, sc.view, depth, want, None, None, 0)
    bad = (got != want).any(axis=2)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5])
    assert (got != base).any(axis=2).sum() > 100000
    r.close()


def test_option_off_again_and_errors(maps64):
    sc = scene(maps64, 1, configs.C2.scaled(320, 180, 64))
    raw, gi, _ = gizmo()
    imgs = []
    for setting in (None, (1, 0)):
        r = Renderer(320, 180)
        r.set_option("overlays", 1)
        r.upload_gizmo(raw, gi)
        if setting:
            for v in setting:
                r.set_option("tbn", v)
        r.render_scene(sc)
        r.present()
        r.draw_overlays(100)
        imgs.append(r.read_presented())
        with pytest.raises(BibimError):
            r.read_tbn_segments()                                  # no TBN draw yet
        r.close()
    assert np.array_equal(imgs[0], imgs[1])
    r = Renderer(320, 180)
    r.set_option("overlays", 1)
    r.set_option("tbn", 1)
    h = r.render_scene(sc)
    r.present()
    r.draw_overlays(0)
    assert len(r.read_tbn_segments()) > 0
    r.resize(160, 90)
    with pytest.raises(BibimError):
        r.read_tbn_segments()                                      # the records had the old extent
    r.close()
    r = Renderer(320, 180)
    r.set_option("overlays", 1)
    r.set_option("tbn", 1)
    r.set_partition(0, 2)
    r.render_scene(sc, None)
    with pytest.raises(BibimError):
        r.draw_overlays(0)                                         # not available with a partition
    r.close()
