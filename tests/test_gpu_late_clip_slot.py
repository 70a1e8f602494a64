"""GPU: the "late" clip slot of the fragment kernels.

k_raster writes a clipped sub-triangle's clip-arena slot into the fragment word only for the first kClipRefs = 32 clipped
sub-triangles of a tile; a fragment of any further one carries 0 there, and k_shade (its uniform and its gather form) and
k_shade_aniso find the slot one round trip later through the record: clip_base + (ref & 7).  Only a tile with more than 32
clipped sub-triangles gets there, so this scene puts 96 on one.

Scene: one 32 x 32 frame = one tile, 48 triangles that all cross the near plane (two sub-triangles each).  The last one is
huge and nearest over most of the tile, so whole 64-fragment chunks belong to it (the uniform form: scalar loads); a
handful of small ones win a few dozen pixels each in front of it (the gather form).  A dropped late branch shades with the
planes of the unclipped record: wrong numbers, no wild address (DESIGN.md section 2 has the mutant table)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import aniso_reference as A
from bibim_renderer_amd import Renderer, textures
from oracle import bbo, scenes

W = H = 32
N_TRI = 48
NO = bbo.NO_PRIM


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(None)
def materials():
    rng = np.random.default_rng(11)
    m = textures.make_material(16)
    mixed = {"albedo": m["albedo"], "metallic": m["metallic"][::2, ::2].copy(), "roughness": rng.integers(40, 256, (8, 8, 4), dtype=np.uint8),
             "normal": rng.integers(100, 156, (10, 12, 4), dtype=np.uint8), "height": rng.integers(0, 256, (6, 12, 4), dtype=np.uint8)}
    return {"packed": m, "mixed": mixed}


@functools.lru_cache(None)
def scene(material="packed"):
    rng = np.random.default_rng(7)
    v = np.zeros(3 * N_TRI, bbo.VERTEX_DTYPE)
    for t in range(N_TRI):
        if t < N_TRI - 1:
            s = rng.uniform(0.15, 0.5)
            cx, cy = rng.uniform(-0.5, 0.5, 2)
            z = rng.uniform(1.5, 3.5)
        else:
            s, cx, cy, z = 3.0, 0.0, 0.0, 1.0
        v["pos"][3 * t:3 * t + 3] = [(cx - s, cy + s, z), (cx + s, cy + s, z), (cx, cy - 6 * s, -0.5)]   # the apex: behind the camera
    v["uv"] = rng.uniform(-2, 2, (3 * N_TRI, 2))
    v["normal"], v["tangent"] = (0, 0, -1), (1, 0, 0)
    inst = np.zeros(1, bbo.INSTANCE_DTYPE)
    inst[0] = scenes.instance(np.eye(4, dtype=np.float32))
    fu = scenes.frame_uniforms([scenes.light(0, pos=(0.3, 0.5, 0.0), color=(1.0, 0.9, 0.8), intensity=6.0)], 1, 1.2)
    vu = scenes.view_uniforms((0, 0, 0), 0, 0, W, H, 1)
    return bbo.Scene(fu, vu, [bbo.DrawData(v, None, inst, bbo.MaterialData(materials()[material]))], W, H, "late clip slot")


@functools.lru_cache(None)
def oracle(material="packed"):
    sc = scene(material)
    o = SimpleNamespace()
    o.frame, o.prim, o.depth, o.stats = bbo.render(sc)
    o.dframe, o.gbuf, _, _, _ = bbo.render_deferred(sc)
    o.uv = bbo.render(sc, flags=bbo.FLAG_OUTPUT_UV)[0]
    return o


def test_the_scene_reaches_both_forms_of_the_late_route():
    """on the oracle alone, no GPU: more clipped sub-triangles on the one tile than fragment words can name, one primitive
    with whole chunks to itself, several with a few pixels each"""
    o = oracle()
    assert o.stats["n_clipped_prims"] == N_TRI
    assert o.stats["n_raster_tris"] > 32
    owned = np.bincount(o.prim[o.prim != NO], minlength=N_TRI)
    print(f"n_raster_tris {o.stats['n_raster_tris']}, pixels per winning primitive {dict((int(p), int(n)) for p, n in enumerate(owned) if n)}")
    big = int(owned.argmax())
    assert owned[big] >= 512
    assert int((np.delete(owned, big) >= 8).sum()) >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("material", ["packed", "mixed"])
@pytest.mark.parametrize("tile_mode", [0, 1])
def test_forward_frame_winner_depth_and_count(tile_mode, material, item_route):
    sc, o = scene(material), oracle(material)
    r = Renderer(W, H)
    r.set_option("tile_mode", tile_mode)
    r.render_scene(sc)
    frame = r.read_framebuffer()
    prim, depth = r.read_visibility()
    st = r.stats()
    r.close()
    assert np.array_equal(prim, o.prim) and np.array_equal(depth.view(np.uint32), o.depth.view(np.uint32))
    assert st["n_shaded"] == o.stats["n_shaded"] and st["n_clipped_prims"] == N_TRI
    assert np.array_equal(bits(frame), bits(o.frame))


@pytest.mark.gpu
@pytest.mark.parametrize("material", ["packed", "mixed"])
@pytest.mark.parametrize("tile_mode", [0, 1])
def test_deferred_frame_and_gbuffer(tile_mode, material, item_route):
    sc, o = scene(material), oracle(material)
    r = Renderer(W, H)
    r.set_option("render_pass", 1)
    r.set_option("tile_mode", tile_mode)
    r.render_scene(sc)
    frame, g = r.read_framebuffer(), r.read_gbuffer()
    r.close()
    assert np.array_equal(bits(frame), bits(o.dframe))
    assert np.array_equal(bits(g), bits(o.gbuf))


@pytest.mark.gpu
@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("tile_mode", [0, 1])
def test_fused_presentation(tile_mode, deferred):
    sc, o = scene(), oracle()
    r = Renderer(W, H)
    r.set_option("render_pass", deferred)
    r.set_option("tile_mode", tile_mode)
    r.set_option("present_fused", 1)
    r.render_scene(sc)
    got = r.read_presented()
    r.close()
    want = bbo.present(o.dframe if deferred else o.frame, int(sc.frame["enable_tone_mapping"]), float(sc.frame["exposure"]))
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("material", ["packed", "mixed"])
@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("tile_mode", [0, 1])
def test_anisotropic_kernel(tile_mode, deferred, material):
    """k_shade_aniso, in the pieces of test_gpu_aniso.py: the dumped uv is the oracle's, taps and filtered values are
    tests/aniso_reference.py's on the dump, the colour is the oracle's light loop on the dumped surface"""
    sc, o = scene(material), oracle(material)
    r = Renderer(W, H)
    r.set_option("render_pass", deferred)
    r.set_option("tile_mode", tile_mode)
    r.set_option("max_anisotropy", 16)
    r.render_scene(sc)
    frame, surf = r.read_framebuffer(), r.read_surface()
    prim, _ = r.read_visibility()
    gbuf = r.read_gbuffer() if deferred else None
    r.close()
    c = o.prim != NO
    assert np.array_equal(prim, o.prim)
    assert np.array_equal(bits(surf[..., :2])[c], bits(o.uv[..., :2])[c]), "vUV"
    rec = surf[c]
    want = A.filter_maps(materials()[material], rec[:, :6], 1, bool(deferred), 16)
    assert np.array_equal(bits(rec[:, 12:28]), bits(want)), "tap counts and filtered values"
    assert rec[:, 22].max() > 1, "no anisotropic pixel"
    if deferred:
        tex = gbuf[c]
        assert np.array_equal(bits(tex[:, 0, :3]), bits(bbo.half_round(rec[:, 6:9])))
        assert np.array_equal(bits(tex[:, 1, :3]), bits(bbo.half_round(rec[:, 9:12])))
        assert np.array_equal(bits(tex[:, 2, :3]), bits(bbo.half_round(rec[:, 12:15])))
        assert np.array_equal(bits(tex[:, 3]), bits(bbo.half_round(rec[:, 15:19])))
        surface = np.concatenate([tex[:, 0, :3], tex[:, 1, :3], tex[:, 2, :3], tex[:, 3, :3]], -1)
    else:
        surface = rec[:, 6:18]
    assert np.array_equal(bits(frame[c]), bits(bbo.light_surface(sc.frame, sc.view, surface, literal=False)))
