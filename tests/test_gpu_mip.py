"""GPU: mip chains and the trilinear filter (option "mip_levels", k_mip_reduce, k_mip_pack, k_shade_mip) against
tests/mip_reference.py, bit for bit.  Frames are 128 x 128.

  chain     bbr_read_material_level / bbr_read_packed_level equal the model's chain and packed levels byte for byte, for a
            chain built when the option is set on a live material and for one built by an upload under the option
  sampler   per layout x scene x pass x max_anisotropy: the dump's uv is the oracle's, its differences are those of its own
            uv, slots 12..31 are the model's on the dump's own footprint, the census of the scene holds on the dump, and the
            frame is the oracle's light loop on the dumped surface
  the rest  tile shape, item route, fused presentation, replay, frames in flight and a partition change no bit; the late
            clip slot works; "mip_levels" back at 1 gives the frame of a context that never set it"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import aniso_reference as A
import mip_reference as M
import surface_chart as SC
import texture_chart as TC
from bibim_renderer_amd import BibimError, Renderer
from bibim_renderer_amd import partition as P
from oracle import bbo

pytestmark = pytest.mark.gpu

F = np.float32
NO = bbo.NO_PRIM
W, H = M.W, M.H


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def maps1024():
    rng = np.random.Generator(np.random.PCG64(78))
    return {k: TC._map(rng, k, 1024, 1024) for k in A.MAP_NAMES}


@functools.lru_cache(None)
def layout(name):
    """the materials of a layout: a tuple of map dicts"""
    if name == "packed 64x64":
        return (M.maps64(),)
    if name == "packed 1024x1024":
        return (maps1024(),)
    return TC.materials(name)


# ---------------------------------------------------------------------------------------------------------------------
# 1. chain
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_LAYOUTS = ([f"packed {w}x{h}" for w, h in ((2, 2), (4, 4), (5, 3), (3, 5), (6, 10), (7, 1), (1, 7), (17, 5), (48, 80), (64, 2), (130, 2))]
                 + ["packed 1024x1024", "five sizes", "albedo 1x1 rest 6x10", "absent"]
                 # packed with absent shaded maps and four levels: k_mip_pack broadcasts the default texels
                 + ["normal only 6x10", "albedo 6x10 roughness 1x1"])


def read_packed_into(r, handle, level, fill):
    """bbr_read_packed_level into a host buffer filled with `fill`, one byte longer than the level (a canary)"""
    import ctypes as C
    n = C.c_uint64()
    assert r._L.bbr_read_packed_level(r._ctx, handle, level, None, 0, C.byref(n)) == 0
    out = np.full(n.value + 1, fill, np.uint8)
    assert r._L.bbr_read_packed_level(r._ctx, handle, level, out.ctypes.data, n.value, C.byref(n)) == 0
    assert out[-1] == fill
    return out[:-1]


def check_chain(r, handle, maps, cap, fill=None):
    chains = M.material_chains(maps, cap)
    for i, name in enumerate(A.MAP_NAMES):
        for k, want in enumerate(chains[name]):
            got = r.read_material_level(handle, i, k)
            assert got.shape == want.shape and np.array_equal(got, want), (name, k)
        with pytest.raises(BibimError) as e:
            r.read_material_level(handle, i, len(chains[name]))
        assert e.value.code == -1
    packed = M.packed_levels(maps, cap)
    if packed is None:
        assert len(r.read_packed_level(handle, 0)) == 0
        return 0
    for k, want in enumerate(packed):
        got = r.read_packed_level(handle, k) if fill is None else read_packed_into(r, handle, k, fill)
        assert len(got) == len(want) and np.array_equal(got, want), ("packed", k)
    with pytest.raises(BibimError) as e:
        r.read_packed_level(handle, len(packed))
    assert e.value.code == -1
    return len(packed)


@pytest.mark.parametrize("name", CHAIN_LAYOUTS)
def test_chain_is_the_models(name):
    maps = layout(name)[0]
    r = Renderer(64, 64)
    live = r.upload_material(maps)
    assert check_chain(r, live, maps, 1) in (0, 1)                  # no chain yet: level 0 alone
    r.set_option("mip_levels", 15)                                 # the chain of a live material
    n = check_chain(r, live, maps, 15)
    if name.startswith("packed "):
        w, h = map(int, name[7:].split("x"))
        assert n == M.level_count(w, h, 15)
    later = r.upload_material(maps)                                # an upload under the option
    check_chain(r, later, maps, 15)
    r.free_material(later)
    again = r.upload_material(maps)                                # (the allocator may hand the same memory back)
    check_chain(r, again, maps, 15, fill=0xAB)                     # every byte of a packed level is written, padding included
    r.set_option("mip_levels", 1)
    check_chain(r, live, maps, 1)
    r.close()


def test_a_cap_of_three():
    maps = layout("packed 48x80")[0]
    r = Renderer(64, 64)
    r.set_option("mip_levels", 3)
    m = r.upload_material(maps)
    assert check_chain(r, m, maps, 3, fill=0xAB) == 3
    assert r.read_material_level(m, 0, 2).shape == (20, 12, 4)
    r.set_option("mip_levels", 15)
    assert check_chain(r, m, maps, 15) == 7
    r.close()


def test_option_range_and_handles():
    r = Renderer(64, 64)
    for bad in (0, 16, -1):
        with pytest.raises(BibimError) as e:
            r.set_option("mip_levels", bad)
        assert e.value.code == -1
    for ok in (1, 2, 15, 1):
        r.set_option("mip_levels", ok)
    with pytest.raises(BibimError) as e:
        r.read_material_level(0, 0, 0)
    assert e.value.code == -5
    m = r.upload_material({})
    with pytest.raises(BibimError) as e:
        r.read_material_level(m, 6, 0)
    assert e.value.code == -1
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. sampler
# ---------------------------------------------------------------------------------------------------------------------
SAMPLER_LAYOUTS = ("packed 6x10", "packed 64x64", "packed 1024x1024", "five sizes", "both")
# the texture behind slots 28 / 29 on which a scene's census is claimed (tests/test_mip_reference.py shows it on the oracle)
CENSUS_SIZE = {"packed 64x64": (64, 64), "packed 1024x1024": (1024, 1024)}


@functools.lru_cache(None)
def oracle(name, n_materials):
    sc = M.scene(name, layout("both") if n_materials == 2 else (M.maps64(),))
    uv, prim, _, _ = bbo.render(sc, flags=bbo.FLAG_OUTPUT_UV)
    return uv, prim


def render(r, sc, handles, deferred, max_aniso):
    r.set_option("render_pass", deferred)
    r.set_option("max_anisotropy", max_aniso)
    r.render_scene(sc, handles)
    g = SimpleNamespace(frame=r.read_framebuffer(), surf=r.read_surface())
    g.prim, _ = r.read_visibility()
    g.gbuf = r.read_gbuffer() if deferred else None
    g.covered = g.prim != NO
    assert not g.surf[~g.covered].any()
    return g


def check_against_the_model(sc, mats, g, deferred, max_aniso, mip_levels):
    """slots 12..31 on the dump's own footprint, and the frame from the dumped surface"""
    c = g.covered
    rec = g.surf[c]
    want = M.filter_rows(sc, mats, g.prim[c], rec, deferred, max_aniso, mip_levels)
    assert np.array_equal(rec[:, 22:28], want[:, 10:16]), "tap counts"
    assert np.array_equal(bits(rec[:, 28:32]), bits(want[:, 16:20])), "level choice"
    assert np.array_equal(bits(rec[:, 12:28]), bits(want[:, :16])), "filtered values"
    if deferred:
        tex = g.gbuf[c]
        assert np.array_equal(bits(tex[:, 0, :3]), bits(bbo.half_round(rec[:, 6:9])))
        assert np.array_equal(bits(tex[:, 1, :3]), bits(bbo.half_round(rec[:, 9:12])))
        assert np.array_equal(bits(tex[:, 2, :3]), bits(bbo.half_round(rec[:, 12:15])))
        assert np.array_equal(bits(tex[:, 3]), bits(bbo.half_round(rec[:, 15:19])))
        surface = np.concatenate([tex[:, 0, :3], tex[:, 1, :3], tex[:, 2, :3], tex[:, 3, :3]], -1)
    else:
        surface = rec[:, 6:18]
        assert not rec[:, 30:32].any()
    lit = bbo.light_surface(sc.frame, sc.view, surface, literal=False)
    assert SC.equal_but_for_nan_payload(g.frame[c], lit), "the frame is not the light loop on the dumped surface"
    return rec, want


@pytest.mark.parametrize("name", M.SCENES)
@pytest.mark.parametrize("lay", SAMPLER_LAYOUTS)
def test_sampler_is_the_models(lay, name):
    mats = layout(lay)
    sc = M.scene(name, mats)
    uv, prim = oracle(name, len(mats))
    r = Renderer(W, H)
    r.set_option("mip_levels", 15)
    handles = {"mesh": {}, "mat": {}}                              # (one upload for the six frames)
    for deferred in (0, 1):
        for max_aniso in (1, 4, 16):
            g = render(r, sc, handles, deferred, max_aniso)
            c = g.covered
            assert np.array_equal(g.prim, prim)
            assert SC.equal_but_for_nan_payload(g.surf[..., :2][c], uv[..., :2][c]), "vUV"
            diff, ok = M.model_differences(g.surf[..., :2], g.prim)
            assert ok.sum() >= 0.75 * c.sum()
            assert SC.equal_but_for_nan_payload(g.surf[..., 2:6][ok], diff[ok]), "differences"
            rec, want = check_against_the_model(sc, mats, g, deferred, max_aniso, 15)
            if lay in CENSUS_SIZE:
                w, h = CENSUS_SIZE[lay]
                count = M.level_count(w, h, 15)
                d, delta, Pv = M.level_rule(rec[:, :6], w, h, rec[:, 22].astype(np.int64), count)
                assert np.array_equal(d, rec[:, 28].astype(np.int64)) and np.array_equal(bits(delta), bits(rec[:, 29]))
                _, finite = M.long_axis(rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5], w, h)
                out = M.census(name, rec[:, 28], rec[:, 29], Pv, finite, count)
                print(f"{lay} {name} pass {deferred} max_anisotropy {max_aniso}: mean d {rec[:, 28].mean():.2f}, {out}")
    r.close()


@pytest.mark.parametrize("chart", TC.POINT_CHARTS)
def test_point_charts(chart):
    """flat: differences 0 or NaN, every pixel stays on level 0 and keeps the bits of the max_anisotropy path.  steep: the
    differences are huge or not finite -- a finite huge footprint is clamped to the LAST level, so only the pixels the rule
    leaves on level 0 keep those bits; all of them follow the model"""
    lay = "packed 6x10"
    sc = TC.scene(lay, chart)
    mats = TC.materials(lay)
    for deferred in (0, 1):
        frames = {}
        for mip in (1, 15):
            r = Renderer(W, H)
            r.set_option("mip_levels", mip)
            frames[mip] = render(r, sc, None, deferred, 16)
            r.close()
        g = frames[15]
        c = g.covered
        assert np.array_equal(g.prim, frames[1].prim) and not frames[1].surf[..., 28:].any()
        check_against_the_model(sc, mats, g, deferred, 16, 15)
        level0 = c & (g.surf[..., 28:32] == 0).all(-1)
        print(f"{chart} pass {deferred}: {int(level0.sum())} of {int(c.sum())} pixels on level 0")
        if chart == "flat":
            assert level0[c].all()
        else:
            assert level0.sum() >= 1000 and (c & ~level0).sum() >= 1000
        assert np.array_equal(bits(g.frame)[level0], bits(frames[1].frame)[level0])
        assert np.array_equal(bits(g.surf[..., :28])[level0], bits(frames[1].surf[..., :28])[level0])
        assert np.array_equal(bits(g.frame)[~c], bits(frames[1].frame)[~c])


# ---------------------------------------------------------------------------------------------------------------------
# 3. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------
FIXED = ("both", "steps")      # a packed and an unpacked material, every level, whole and blended


@functools.lru_cache(None)
def fixed(deferred, **opts):
    sc = M.scene(FIXED[1], layout(FIXED[0]))
    r = Renderer(W, H)
    r.set_option("mip_levels", 15)
    for k, v in opts.items():
        r.set_option(k, v)
    g = render(r, sc, None, deferred, 16)
    r.close()
    return g


@pytest.mark.parametrize("deferred", [0, 1])
def test_tile_shape_and_item_route_do_not_change_a_bit(deferred):
    base = fixed(deferred)
    assert (base.surf[..., 29] != 0).sum() >= 1500 and (base.surf[..., 28] >= 2).sum() >= 1500
    for opts in ({"tile_mode": 0}, {"no_tail_items": 0}, {"no_tail_items": 0, "heavy_tiles": 4}):
        g = fixed(deferred, **opts)
        assert np.array_equal(bits(g.frame), bits(base.frame)), opts
        assert np.array_equal(bits(g.surf), bits(base.surf)), opts


@pytest.mark.parametrize("deferred", [0, 1])
def test_replay_frames_in_flight_fused_presentation_and_partition(deferred):
    sc = M.scene(FIXED[1], layout(FIXED[0]))
    base = fixed(deferred)

    def renderer(**opts):
        r = Renderer(W, H)
        for k, v in dict(render_pass=deferred, max_anisotropy=16, mip_levels=15, **opts).items():
            r.set_option(k, v)
        return r

    for route in ({}, {"no_tail_items": 0}):
        r = renderer(frames_in_flight=3, **route)
        r.render_scene(sc)
        for _ in range(7):
            r.replay_frame()
        frame = r.read_framebuffer()
        r.close()
        assert np.array_equal(bits(frame), bits(base.frame)), route
    r = renderer(present_fused=1)
    r.render_scene(sc)
    r.present()
    got, surf = r.read_presented(), r.read_surface()
    r.close()
    assert np.array_equal(got, bbo.present(base.frame, int(sc.frame["enable_tone_mapping"]), float(sc.frame["exposure"])))
    assert np.array_equal(bits(surf), bits(base.surf))
    shards = []
    for rank in range(3):
        r = renderer()
        band_rows = r.tile_height()
        r.set_partition(rank, 3, band_rows)
        r.render_scene(sc)
        shards.append(r.read_shard())
        r.close()
    assert np.array_equal(bits(P.unpack_gathered(np.stack(shards), H, band_rows)), bits(base.frame))


@pytest.mark.parametrize("material", ["packed", "mixed"])
@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("tile_mode", [0, 1])
def test_late_clip_slot(tile_mode, deferred, material):
    import test_gpu_late_clip_slot as LC
    sc, o = LC.scene(material), LC.oracle(material)
    r = Renderer(LC.W, LC.H)
    r.set_option("tile_mode", tile_mode)
    r.set_option("mip_levels", 15)
    g = render(r, sc, None, deferred, 16)
    r.close()
    c = o.prim != NO
    assert np.array_equal(g.prim, o.prim)
    assert np.array_equal(bits(g.surf[..., :2])[c], bits(o.uv[..., :2])[c]), "vUV"
    rec, _ = check_against_the_model(sc, (LC.materials()[material],), g, deferred, 16, 15)
    assert (rec[:, 28] > 0).any() or (rec[:, 29] != 0).any(), "no pixel left level 0"


@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("max_aniso", [1, 16])
def test_back_to_one_level_is_the_frame_without_the_option(max_aniso, deferred):
    sc = M.scene(FIXED[1], layout(FIXED[0]))
    r = Renderer(W, H)
    never = render(r, sc, None, deferred, max_aniso)
    r.close()
    r = Renderer(W, H)
    handles = r.render_scene(sc)
    r.set_option("mip_levels", 15)
    with_chain = render(r, sc, handles, deferred, max_aniso)
    r.set_option("mip_levels", 1)
    back = render(r, sc, handles, deferred, max_aniso)
    r.close()
    assert (bits(with_chain.frame) != bits(never.frame)).any(), "the option changed no pixel"
    assert np.array_equal(bits(back.frame), bits(never.frame)) and np.array_equal(bits(back.surf), bits(never.surf))
    assert not back.surf[..., 28:].any()
    if max_aniso == 1:
        ref = bbo.render_deferred(sc, want_gbuffer=False)[0] if deferred else bbo.render(sc)[0]
        assert np.array_equal(bits(never.frame), bits(ref))
