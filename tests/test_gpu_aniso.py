"""GPU: anisotropic texture filtering (option "max_anisotropy", k_shade_aniso) and the surface read-back (bbr_read_surface).

No reference decides the extra taps of a one-mip sampler, so the rule is pinned and tested exactly,
in pieces that each have a reference of their own:
  uv            the dump's vUV against the oracle's (FLAG_OUTPUT_UV), bit for bit
  differences   against the dump's own uv where the neighbouring pixels belong to the same unclipped primitive (bit for bit),
                against the exact rasteriser's gradient on the clipped ground plane (within 2e-2 of its length), and
                against themselves with and without an occluder in front (the extrapolated ones)
  taps, values  tests/aniso_reference.py on the dump's own uv and differences, bit for bit
  colour        the oracle's light loop on the dump's surface values, bit for bit
and the frame's bits must not depend on tile shape, item route, fused presentation, a partition or frames in flight.

Scenes (small: every test takes a few seconds at most):
  Q   128 x 96, a 12 x 12 quad 0.6 below the camera seen at grazing angles, uv x 16, 64^2 maps: every tap count 1..16 occurs
  B   C2 at 160 x 90 with 64^2 maps: sub-pixel ball triangles, a clipped ground plane, many one-tap pixels
  QO  Q plus a nearer triangle drawn after it over the middle of the view
  M   Q with maps of different sizes (one not a power of two) and a height map: the per-map path"""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import aniso_reference as A
import raster_reference as RR
from conftest import GOLDEN
from bibim_renderer_amd import BibimError, Renderer, configs, textures
from bibim_renderer_amd import partition as P
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

W, H = 128, 96
NO = bbo.NO_PRIM
PASSES = [0, 1]
pass_id = lambda d: "deferred" if d else "forward"


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def maps64():
    return textures.make_material(64)


@functools.lru_cache(None)
def mixed_maps():
    rng = np.random.default_rng(11)
    m = maps64()
    return {"albedo": m["albedo"], "metallic": m["metallic"][::4, ::4].copy(), "roughness": rng.integers(40, 256, (32, 32, 4), dtype=np.uint8),
            "normal": rng.integers(100, 156, (40, 48, 4), dtype=np.uint8), "height": rng.integers(0, 256, (12, 24, 4), dtype=np.uint8)}


def quad_scene(maps, occluder=False):
    v, idx = scenes.plane_mesh()
    v["uv"] *= np.float32(16.0)
    inst = np.zeros(1, bbo.INSTANCE_DTYPE)
    inst[0] = scenes.instance(bbo.mat_mul(bbo.mat_translate(0.0, -0.6, 7.0), bbo.mat_scale(12.0)))
    mat = bbo.MaterialData(maps)
    draws = [bbo.DrawData(v, idx, inst, mat)]
    if occluder:
        t = np.zeros(3, bbo.VERTEX_DTYPE)
        t["pos"] = [(0.0, -0.2, 2.0), (1.6, -0.55, 2.0), (-1.6, -0.55, 2.0)]     # above the quad's plane: in front of it
        t["uv"] = [(0.5, 1), (1, 0), (0, 0)]
        t["normal"], t["tangent"] = (0, 0, -1), (1, 0, 0)
        one = np.zeros(1, bbo.INSTANCE_DTYPE)
        one[0] = scenes.instance(np.eye(4, dtype=np.float32))
        draws.append(bbo.DrawData(t, None, one, mat))
    fu = scenes.frame_uniforms([scenes.light(0, pos=(0.5, 1.5, 5.0), color=(1.0, 0.9, 0.8), intensity=40.0)], 1, 1.3)
    vu = scenes.view_uniforms((0, 0, 0), 0.0, 0.0, W, H, 1)
    return bbo.Scene(fu, vu, draws, W, H, "Q+occluder" if occluder else "Q")


@functools.lru_cache(None)
def scene(name):
    if name == "Q":
        return quad_scene(maps64())
    if name == "QO":
        return quad_scene(maps64(), occluder=True)
    if name == "M":
        return quad_scene(mixed_maps())
    assert name == "B"
    sc = scenes.shaderball_scene(configs.C2.scaled(160, 90, 64), bbo.MaterialData(maps64()))
    sc.frame["enable_tone_mapping"], sc.frame["exposure"] = 1, 0.9
    return sc


def material_of(name):
    return mixed_maps() if name == "M" else maps64()


@functools.lru_cache(None)
def gpu(name, deferred, max_aniso, **opts):
    """one frame of a scene and its read-backs"""
    sc = scene(name)
    r = Renderer(sc.width, sc.height)
    r.set_option("render_pass", deferred)
    r.set_option("max_anisotropy", max_aniso)
    for k, v in opts.items():
        r.set_option(k, v)
    r.render_scene(sc)
    out = SimpleNamespace(frame=r.read_framebuffer(), surf=r.read_surface())
    out.prim, _ = r.read_visibility()
    out.gbuf = r.read_gbuffer() if deferred else None
    again = r.read_framebuffer()       # the dumps re-render the frame: the same bits
    r.close()
    assert np.array_equal(again.view(np.uint32), out.frame.view(np.uint32))
    out.covered = out.prim != NO
    assert not out.surf[~out.covered].any(), "an uncovered pixel's record is not 32 zeros"
    assert not out.surf[..., 28:].any()
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_on_both_neighbours(prim):
    """pixels whose winner also wins the right and the lower neighbour"""
    ok = np.zeros(prim.shape, bool)
    ok[:-1, :-1] = (prim[:-1, :-1] != NO) & (prim[:-1, :-1] == prim[:-1, 1:]) & (prim[:-1, :-1] == prim[1:, :-1])
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# 1. uv
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_aniso", [1, 16])
@pytest.mark.parametrize("name", ["Q", "B"])
def test_uv_is_the_oracles(name, max_aniso):
    uv, prim, _, _ = bbo.render(scene(name), flags=bbo.FLAG_OUTPUT_UV)
    for deferred in PASSES:
        g = gpu(name, deferred, max_aniso)
        assert np.array_equal(g.prim, prim)
        assert np.array_equal(bits(g.surf[..., :2])[g.covered], bits(uv[..., :2])[g.covered]), pass_id(deferred)
    if name == "Q":
        assert int(g.covered.sum()) == 5576


# ---------------------------------------------------------------------------------------------------------------------
# 2. differences, exact
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
@pytest.mark.parametrize("name", ["Q", "B"])
def test_differences_are_those_of_the_dumps_own_uv(name, deferred):
    g = gpu(name, deferred, 16)
    clip, _ = RR.scene_primitives(scene(name))
    unclipped = RR.all_in(clip)
    ok = same_on_both_neighbours(g.prim)
    ok &= unclipped[np.where(g.prim == NO, 0, g.prim)]
    y, x = np.nonzero(ok)
    share = len(y) / g.covered.sum()
    print(f"{name}: {len(y)} of {int(g.covered.sum())} covered pixels qualify ({share:.1%})")
    if name == "Q":
        assert share >= 0.90
    assert len(y) >= 10
    uv = g.surf[..., :2]
    want = np.concatenate([uv[y, x + 1] - uv[y, x], uv[y + 1, x] - uv[y, x]], -1)     # dudx dvdx dudy dvdy
    assert np.array_equal(bits(g.surf[y, x, 2:6]), bits(want))


# ---------------------------------------------------------------------------------------------------------------------
# 3. differences on the clipped ground plane
# ---------------------------------------------------------------------------------------------------------------------

def test_differences_on_the_clipped_plane_follow_the_exact_gradient():
    sc = scene("B")
    g = gpu("B", 0, 16)
    clip, _ = RR.scene_primitives(sc)
    plane = [len(clip) - 2, len(clip) - 1]
    assert not RR.all_in(clip[plane]).any(), "the ground plane is meant to be clipped"
    res = RR.rasterise(sc, only=plane, want_uv=False)
    ok = same_on_both_neighbours(g.prim)
    worst, seen = 0.0, 0
    for p in plane:
        y, x = np.nonzero(ok & (g.prim == p))
        if not len(y):
            continue
        pr = res.prims[p]
        X, Y = x.astype(np.float64), y.astype(np.float64)
        here, right, below = pr.vuv(X, Y)[0], pr.vuv(X + 1, Y)[0], pr.vuv(X, Y + 1)[0]
        exact = np.concatenate([right - here, below - here], -1)                      # dudx dvdx dudy dvdy
        length = np.sqrt((exact ** 2).sum(-1))                                        # of the whole 2 x 2 gradient
        err = np.abs(g.surf[y, x, 2:6].astype(np.float64) - exact).max(-1)
        worst = max(worst, float((err / length).max()))
        seen += len(y)
    print(f"clipped plane: {seen} pixels, worst |difference - exact| / |exact gradient| = {worst:.3g}")
    assert seen >= 1000
    assert worst <= 2e-2
    recorded = json.load(open(os.path.join(GOLDEN, "aniso_reference.json")))
    assert recorded["bound"] == 2e-2


# ---------------------------------------------------------------------------------------------------------------------
# 4. tap counts and filtered values
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_aniso", [16, 4])
@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
@pytest.mark.parametrize("name", ["Q", "B", "M"])
def test_taps_and_filtered_values_are_the_rules(name, deferred, max_aniso):
    g = gpu(name, deferred, max_aniso)
    rec = g.surf[g.covered]
    want = A.filter_maps(material_of(name), rec[:, :6], 1, bool(deferred), max_aniso)
    counts = rec[:, 22:28].astype(np.int64)
    assert np.array_equal(counts, want[:, 10:].astype(np.int64)), "tap counts"
    assert np.array_equal(bits(rec[:, 12:28]), bits(want)), "filtered values"
    assert counts.max() <= max_aniso
    seen = set(np.unique(counts[:, 0]).tolist())
    print(f"{name} {pass_id(deferred)} max {max_aniso}: mean taps of the albedo map {counts[:, 0].mean():.2f}, counts seen {sorted(seen)}")
    if name == "Q":
        assert seen >= set(range(2, max_aniso + 1))
    if name == "B":
        assert 1 in seen
    if name == "M":
        assert (counts[:, 0] != counts[:, 2]).any() and (counts[:, 4] != counts[:, 0]).any()     # per map
        if deferred:
            assert counts[:, 5].max() > 1 and rec[:, 18].any()                                      # the height map is live


def test_without_normal_map_and_the_default_material():
    sc = quad_scene({"albedo": maps64()["albedo"]})
    sc.view["enable_normal_map"] = 0
    r = Renderer(W, H)
    r.set_option("max_anisotropy", 16)
    r.render_scene(sc)
    frame, surf = r.read_framebuffer(), r.read_surface()
    r.close()
    rec = surf[surf[..., 22] > 0]
    assert len(rec) == 5576
    want = A.filter_maps({"albedo": maps64()["albedo"]}, rec[:, :6], 0, False, 16)
    assert np.array_equal(bits(rec[:, 12:28]), bits(want))
    assert not rec[:, 19:22].any() and not rec[:, 26].any()
    lit = bbo.light_surface(sc.frame, sc.view, rec[:, 6:18], literal=False)
    assert np.array_equal(bits(frame[surf[..., 22] > 0]), bits(lit))


# ---------------------------------------------------------------------------------------------------------------------
# 5. colour
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_aniso", [16, 1])
@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
@pytest.mark.parametrize("name", ["Q", "B"])
def test_colour_is_the_light_loop_on_the_dumped_surface(name, deferred, max_aniso):
    sc = scene(name)
    g = gpu(name, deferred, max_aniso)
    c = g.covered
    rec = g.surf[c]
    if not deferred:
        lit = bbo.light_surface(sc.frame, sc.view, rec[:, 6:18], literal=False)
    else:
        tex = g.gbuf[c]                                                     # [n, 4 attachments, 4]
        assert np.array_equal(bits(tex[:, 0, :3]), bits(bbo.half_round(rec[:, 6:9])))
        assert np.array_equal(bits(tex[:, 1, :3]), bits(bbo.half_round(rec[:, 9:12])))
        assert np.array_equal(bits(tex[:, 2, :3]), bits(bbo.half_round(rec[:, 12:15])))
        assert np.array_equal(bits(tex[:, 3]), bits(bbo.half_round(rec[:, 15:19])))
        lit = bbo.light_surface(sc.frame, sc.view, np.concatenate([tex[:, 0, :3], tex[:, 1, :3], tex[:, 2, :3], tex[:, 3, :3]], -1),
                                literal=False)
    assert np.array_equal(bits(g.frame[c]), bits(lit))
    if max_aniso == 1:
        ref = bbo.render_deferred(sc, want_gbuffer=False)[0] if deferred else bbo.render(sc)[0]
        assert np.array_equal(bits(g.frame), bits(ref)), "max_anisotropy = 1 is the oracle's frame"
        assert (g.surf[c][:, 22:26] == 1).all()


def test_gbuffer_view_shows_the_filtered_albedo():
    g = gpu("Q", 1, 16, gbuffer_view=2)
    c = g.covered
    assert np.array_equal(bits(g.frame[c][:, :3]), bits(bbo.half_round(g.surf[c][:, 12:15])))
    assert not np.array_equal(bits(g.frame), bits(gpu("Q", 1, 1, gbuffer_view=2).frame))


# ---------------------------------------------------------------------------------------------------------------------
# 6. one-tap pixels are the pixels of max_anisotropy = 1
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
def test_one_tap_pixels_keep_their_bits(deferred):
    """on B: the quad of Q and M is minified and anisotropic everywhere at 64^2 (no one-tap pixel to compare)"""
    name = "B"
    a, b = gpu(name, deferred, 16), gpu(name, deferred, 1)
    one_tap = a.covered & (a.surf[..., 22:28] <= 1).all(-1)
    print(f"{name} {pass_id(deferred)}: {int(one_tap.sum())} one-tap pixels of {int(a.covered.sum())}")
    assert one_tap.sum() >= 2000
    assert np.array_equal(bits(a.frame)[one_tap], bits(b.frame)[one_tap])
    assert np.array_equal(bits(a.frame)[~a.covered], bits(b.frame)[~a.covered])
    assert (bits(a.frame) != bits(b.frame)).any(), "the option changed no pixel"


# ---------------------------------------------------------------------------------------------------------------------
# 7. occlusion invariance
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
def test_an_occluder_changes_nothing_on_the_pixels_it_leaves(deferred):
    q, o = gpu("Q", deferred, 16), gpu("QO", deferred, 16)
    both = (q.prim < 2) & (o.prim < 2)
    assert np.array_equal(q.prim[both], o.prim[both])
    occ = o.prim == 2
    edge = np.zeros(both.shape, bool)
    edge[:, :-1] |= occ[:, 1:]
    edge[:-1, :] |= occ[1:, :]
    edge &= both                                   # the quad's pixels whose right or lower neighbour the occluder wins
    print(f"{int(both.sum())} pixels the quad wins in both frames, {int(edge.sum())} of them at the occluder's outline, "
          f"{int(occ.sum())} pixels of the occluder")
    assert edge.sum() >= 100 and occ.sum() >= 500
    assert np.array_equal(bits(q.surf)[both], bits(o.surf)[both])
    assert np.array_equal(bits(q.frame)[both], bits(o.frame)[both])
    assert (o.surf[edge][:, 22] > 1).any()


# ---------------------------------------------------------------------------------------------------------------------
# 8. invariances
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
def test_tile_shape_and_item_route_do_not_change_a_bit(deferred):
    base = gpu("B", deferred, 16)
    for opts in ({"tile_mode": 0}, {"no_tail_items": 0}, {"no_tail_items": 0, "tile_mode": 0}, {"no_tail_items": 0, "heavy_tiles": 4}):
        g = gpu("B", deferred, 16, **opts)
        assert np.array_equal(bits(g.frame), bits(base.frame)), opts
        assert np.array_equal(bits(g.surf), bits(base.surf)), opts


@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
def test_long_route_replays_and_frames_in_flight(deferred):
    """the long route sizes its launch from the slot's previous frame: replays are where that estimate is in use"""
    sc = scene("B")
    base = gpu("B", deferred, 16)
    for fif in (1, 3):
        for route in ({}, {"no_tail_items": 0}):
            r = Renderer(sc.width, sc.height)
            r.set_option("render_pass", deferred)
            r.set_option("max_anisotropy", 16)
            r.set_option("frames_in_flight", fif)
            for k, v in route.items():
                r.set_option(k, v)
            r.render_scene(sc)
            for _ in range(10):
                r.replay_frame()
            frame = r.read_framebuffer()
            r.close()
            assert np.array_equal(bits(frame), bits(base.frame)), (fif, route)


@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
def test_fused_presentation(deferred):
    sc = scene("B")
    base = gpu("B", deferred, 16)
    r = Renderer(sc.width, sc.height)
    r.set_option("render_pass", deferred)
    r.set_option("max_anisotropy", 16)
    r.set_option("present_fused", 1)
    r.render_scene(sc)
    r.present()
    got = r.read_presented()
    surf = r.read_surface()
    again = r.read_presented()
    r.close()
    want = bbo.present(base.frame, int(sc.frame["enable_tone_mapping"]), float(sc.frame["exposure"]))
    assert np.array_equal(got, want) and np.array_equal(again, want)
    assert np.array_equal(bits(surf), bits(base.surf))


@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
def test_partition_of_three(deferred):
    sc = scene("B")
    base = gpu("B", deferred, 16)
    shards = []
    for rank in range(3):
        r = Renderer(sc.width, sc.height)
        r.set_option("render_pass", deferred)
        r.set_option("max_anisotropy", 16)
        band_rows = r.tile_height()
        r.set_partition(rank, 3, band_rows)
        r.render_scene(sc)
        shards.append(r.read_shard())
        with pytest.raises(BibimError) as e:
            r.read_surface()
        assert e.value.code == -1
        r.close()
    frame = P.unpack_gathered(np.stack(shards), sc.height, band_rows)
    assert np.array_equal(bits(frame), bits(base.frame))


# ---------------------------------------------------------------------------------------------------------------------
# 9. interface
# ---------------------------------------------------------------------------------------------------------------------

def test_option_range_and_read_back_errors():
    sc = scene("Q")
    r = Renderer(W, H)
    for bad in (0, 17, -1):
        with pytest.raises(BibimError) as e:
            r.set_option("max_anisotropy", bad)
        assert e.value.code == -1
    with pytest.raises(BibimError) as e:
        r.read_surface()                       # before a first frame
    assert e.value.code == -6
    for ok in (1, 2, 16):
        r.set_option("max_anisotropy", ok)
    r.render_scene(sc)
    assert r.read_surface().shape == (H, W, 32)
    r.resize(64, 48)
    with pytest.raises(BibimError) as e:
        r.read_surface()                       # after bbr_resize
    assert e.value.code == -6
    assert r._L.bbr_read_surface(r._ctx, None) == -1
    r.close()
