"""GPU: option "sample_shading" 0 (k_sample_merge, k_resolve_merged), bit for bit against tests/sample_merge_reference.py
on the oracle's fine frame and primitive frame.

  sample map    read_sample_map() is rep_map of the oracle's winners
  samples       read_samples() is the oracle's fine frame at every representative and its replication everywhere
  output        read_framebuffer() is the model's merged frame; n_shaded counts the representatives
  the rest      full tiles, the sampler options, the late clip-slot route, presentation (fused and not), the GUI pass,
                partitions and the exchange forms, NaN, the option's state and what it refuses

Where NaN occurs its placement is compared, not its payload.  Every test starts by setting the option, so every one of them
fails on a library without it ("unknown option: sample_shading")."""
import copy

import numpy as np
import pytest

import resolve_reference as RR
import sample_merge_reference as M
import ui_reference as U
from bibim_renderer_amd import BibimError, Renderer
from bibim_renderer_amd import partition as P
from bibim_renderer_amd.renderer import UiDrawData
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

F = np.float32
INVALID, NOT_IN_FRAME = -1, -6
W, H = 37, 23                       # output of the main cases: fine 74 x 46 and 148 x 92 -- partial edge tiles
NS = (2, 4)


def same(a, b):
    """bit for bit; NaN by placement"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def multisampled(w, h, n, **options):
    r = Renderer(w, h)
    r.set_option("sample_shading", 0)
    r.set_option("supersample", n)
    for k, v in options.items():
        r.set_option(k, v)
    return r


def expect(code, call, *args):
    with pytest.raises(BibimError) as e:
        call(*args)
    assert e.value.code == code, e.value
    return e.value


def check_frame(r, fine, prim, n, fused=False):
    """the four statements of the main cases on the frame `r` has just rendered, against the oracle's (fine, prim)"""
    rep = M.rep_map(prim, n)
    own = M.representatives(rep, n)
    got_map = r.read_sample_map()
    assert got_map.shape == rep.shape and np.array_equal(got_map, rep)
    samples = r.read_samples()
    assert same(samples[own], fine[own])
    assert same(samples, M.replicate(fine, rep, n))
    if not fused:
        assert same(r.read_framebuffer(), M.merged(fine, prim, n))
    assert r.stats()["n_shaded"] == int((own & (prim != M.NO_PRIM)).sum())
    return rep


# ---------------------------------------------------------------------------------------------------------------------
# 1. main cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("name", M.SCENES)
@pytest.mark.parametrize("n", NS)
def test_map_samples_output_and_count(name, n, deferred, item_route):
    r = multisampled(W, H, n, render_pass=deferred)
    r.render_scene(M.scene(name, n * W, n * H, n))
    fine, prim = M.oracle(name, n * W, n * H, n, bool(deferred))
    rep = check_frame(r, fine, prim, n)
    out = r.read_framebuffer()
    r.close()
    assert out.shape == (H, W, 4)
    if name in ("ball", "balls") and not deferred:
        assert not same(out, RR.resolve(fine, n))                  # not the per-sample resolve
    if name == "triangle" and not deferred:
        assert ((out[..., 3] > 0) & (out[..., 3] < 1)).any()       # forward alpha stays the covered fraction
    if name == "chart":
        assert len(np.unique(M._blocks(rep, n).reshape(-1, n * n), axis=0)) >= 15


@pytest.mark.parametrize("n", NS)
def test_heavy_tiles_first(n):
    """k_raster's heavy rows in front of the launch: the merge still finds every tile's list at the tile's own place"""
    r = multisampled(W, H, n, heavy_tiles=4, frames_in_flight=1)
    handles = r.render_scene(M.scene("balls", n * W, n * H, n))
    r.render_scene(M.scene("balls", n * W, n * H, n), handles)       # (the second frame of the slot has the heavy rows sized)
    check_frame(r, *M.oracle("balls", n * W, n * H, n), n)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the thinning does not change who wins
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_same_primitive_frame_as_per_sample_mode(n):
    sc = M.scene("balls", n * W, n * H, n)
    r = multisampled(W, H, n)
    r.render_scene(sc)
    rep, g, out = r.read_sample_map(), r.read_samples(), r.read_framebuffer()
    r.close()
    per = Renderer(W, H)
    per.set_option("sample_shading", 1)
    per.set_option("supersample", n)
    per.render_scene(sc)
    fine, per_out = per.read_samples(), per.read_framebuffer()
    identity = per.read_sample_map()
    per.close()
    assert np.array_equal(identity, M.rep_map(np.full((n * H, n * W), M.NO_PRIM, np.uint32), n))    # each sample its own index
    covered = fine[..., 3] == 1                                    # forward: alpha 1 where geometry wins, 0 where nothing does
    assert np.array_equal(g[..., 3] == 1, covered) and same(g[..., 3], fine[..., 3])
    assert same(out[..., 3], per_out[..., 3])
    assert np.array_equal(rep[~covered], identity[~covered])       # an uncovered sample stands for itself
    own = M.representatives(rep, n)
    assert same(g[own], fine[own])                                 # and a representative is shaded as the fine pixel it is


# ---------------------------------------------------------------------------------------------------------------------
# 3. full tiles
# ---------------------------------------------------------------------------------------------------------------------
def one_triangle_scene(w, h):
    """one textured triangle over the whole w x h frame, on the partition chart's camera"""
    v = np.zeros(3, bbo.VERTEX_DTYPE)
    v["pos"] = [(-8.0, -8.0, 0.5), (2.0 * w + 16.0, -8.0, 0.5), (-8.0, 2.0 * h + 16.0, 0.5)]
    v["uv"] = [(0.0, 0.0), (3.0, 0.25), (0.5, 2.0)]
    v["normal"], v["tangent"] = (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)
    one = np.zeros(1, bbo.INSTANCE_DTYPE)
    one[0]["model"] = one[0]["inv_model"] = np.eye(4, dtype=np.float32)
    fu = scenes.frame_uniforms([scenes.light(0, pos=(0.3 * w, 0.4 * h, -60.0), color=(1.0, 0.9, 0.8), intensity=4000.0)])
    return bbo.Scene(fu, M.exact_view(w, h), [bbo.DrawData(v, None, one, M.material())], w, h, "one triangle")


@pytest.mark.parametrize("tile_mode", [1, 0])
def test_full_tiles(tile_mode):
    w, h, n = 96, 64, 2
    sc = one_triangle_scene(n * w, n * h)
    fine, prim = bbo.render(sc)[:2]
    assert (prim == 0).all() and len(np.unique(fine[..., 0])) > 1000
    r = multisampled(w, h, n, broad_threshold=1, tile_mode=tile_mode)   # an every-tile entry: kFullTile tiles
    r.render_scene(sc)
    assert not r.read_sample_map().any()
    assert r.stats()["n_shaded"] == w * h
    out, g = r.read_framebuffer(), r.read_samples()
    r.close()
    assert same(out, fine[::2, ::2]) and same(out, M.merged(fine, prim, n))
    assert same(g, M.replicate(fine, np.zeros(prim.shape, np.uint8), n))


# ---------------------------------------------------------------------------------------------------------------------
# 4. sampler options
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,value", [("max_anisotropy", 4), ("mip_levels", 15)])
def test_sampler_options(option, value):
    n = 2
    sc = M.scene("ball", n * W, n * H, n)
    per = Renderer(W, H)
    per.set_option("sample_shading", 1)
    per.set_option("supersample", n)
    per.set_option(option, value)
    per.render_scene(sc)
    fine = per.read_samples()
    per.close()
    plain, prim = M.oracle("ball", n * W, n * H, n)
    assert not same(fine, plain)                                   # the option reached the fine frame's shading
    r = multisampled(W, H, n, **{option: value})
    r.render_scene(sc)
    check_frame(r, fine, prim, n)                                  # the per-fine-pixel footprint: a per-sample context's values
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the late clip-slot route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1])
def test_late_clip_slot_route(deferred):
    import test_gpu_late_clip_slot as L
    sc, o = L.scene(), L.oracle()
    assert (sc.width, sc.height) == (32, 32) and o.stats["n_raster_tris"] > 32
    n = 2
    r = multisampled(16, 16, n, render_pass=deferred)              # one fine tile
    r.render_scene(sc)
    check_frame(r, o.dframe if deferred else o.frame, o.prim, n)   # sub-triangles of one primitive merge: P is the primitive
    r.close()
    assert (M.rep_map(o.prim, n) != M.rep_map(np.arange(32 * 32, dtype=np.uint32).reshape(32, 32), n)).sum() > 256


# ---------------------------------------------------------------------------------------------------------------------
# 6. presentation and the GUI pass act on the merged frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tone", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_presentation(n, tone):
    name = "balls"
    sc = copy.copy(M.scene(name, n * W, n * H, n))                 # (the shared scene stays as it is)
    sc.frame = sc.frame.copy()
    sc.frame["enable_tone_mapping"], sc.frame["exposure"] = tone, 1.3          # presentation only: the fine frame is linear HDR
    fine, prim = M.oracle(name, n * W, n * H, n)
    model = M.merged(fine, prim, n)
    r = multisampled(W, H, n)
    handles = r.render_scene(sc)
    assert same(r.read_framebuffer(), model)
    want = {}
    for hdr16 in (True, False):
        r.present(hdr16=hdr16)
        want[hdr16] = bbo.present(model, tone, 1.3, hdr16)
        assert np.array_equal(r.read_presented(), want[hdr16]), hdr16
    r.set_option("present_fused", 1)                               # k_resolve_merged's PRESENT form
    r.render_scene(sc, handles)
    r.present()
    assert np.array_equal(r.read_presented(), want[True])
    expect(INVALID, r.read_framebuffer)                            # no W x H fp32 frame
    check_frame(r, fine, prim, n, fused=True)
    r.close()


def test_gui_over_a_multisampled_frame():
    n = 2
    r = multisampled(W, H, n)
    texture = np.array([[[255, 200, 90, 180]]], np.uint8)
    assert r.upload_ui_texture(texture) == 1
    r.render_scene(M.scene("ball", n * W, n * H, n))
    model = M.merged(*M.oracle("ball", n * W, n * H, n), n)
    r.present()
    base = r.read_presented()
    assert np.array_equal(base, bbo.present(model, 0, 1.0))
    draw = U.assemble([((0, 0, W, H), 1, [U.quad(3.25, 2.5, 30.0, 20.75, U.rgba(40, 220, 130, 150))])], (W, H))
    r.draw_ui(UiDrawData(draw.vertices, draw.indices, draw.cmds, draw.display_pos, draw.display_size, draw.framebuffer_scale))
    want = U.render(base, draw, {1: texture})
    assert (want != base).any(axis=2).sum() > 300
    assert np.array_equal(r.read_presented(), want)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. partition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_partition(n):
    import torch
    w, h, band, world = 37, 100, 32, 3
    whole = M.merged(*M.oracle("balls", n * w, n * h, n), n)
    sc = M.scene("balls", n * w, n * h, n)
    ranks = []
    for rank in range(world):
        r = multisampled(w, h, n)
        r.set_partition(rank, world, band)
        assert r.shard_rows() == P.shard_rows(h, world, band)
        r.render_scene(sc)
        assert same(r.read_shard(), P.pack_shard(whole, rank, world, band)), rank       # padding rows zero
        expect(INVALID, r.read_samples)                                                # partitioned
        expect(INVALID, r.read_sample_map)
        ranks.append(r)
    wants = {P.SHARD_RGBA32F: whole, P.SHARD_RGBA8: bbo.present(whole, 0, 1.0), P.SHARD_RGBA16F: bbo.half_round(whole)}
    for form, want in wants.items():
        block = ranks[0].exchange_block_bytes(form)
        gathered = torch.zeros(world * block, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for rank, r in enumerate(ranks):
            if form == P.SHARD_RGBA8:
                r.present()
            r.stage_shard(form, gathered.data_ptr() + rank * block)
            r.synchronize()
        ranks[0].unpack_whole(form, gathered.data_ptr())
        got = ranks[0].read_whole_frame(form)
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), form
    scratch = torch.zeros(ranks[0].exchange_block_bytes(P.SHARD_PACKED), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for r in ranks:
        expect(INVALID, r.stage_shard, P.SHARD_PACKED, scratch.data_ptr())               # still refused with n >= 2
        r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. NaN
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_nan_reaches_what_it_stands_for(n):
    from test_gpu_supersample import nan_scene
    sc = nan_scene(n * W, n * H)
    fine, _, prim, _, _ = bbo.render_deferred(sc, want_gbuffer=False)
    assert np.isnan(fine).any() and np.isfinite(fine[..., :3]).all(axis=2).any()
    r = multisampled(W, H, n, render_pass=1)
    r.render_scene(sc)
    check_frame(r, fine, prim, n)
    out = r.read_framebuffer()
    r.close()
    assert np.isnan(out[..., :3]).any() and np.isfinite(out[..., :3]).all(axis=2).any()


# ---------------------------------------------------------------------------------------------------------------------
# 9. state
# ---------------------------------------------------------------------------------------------------------------------
def test_replay_and_four_frames_in_flight(item_route):
    n = 2
    r = multisampled(W, H, n, frames_in_flight=4, bin_cap=8)      # (bins far too small: the first frame is re-rendered, merge included)
    r.render_scene(M.scene("ball", n * W, n * H, n))
    for _ in range(6):
        r.replay_frame()
    fine, prim = M.oracle("ball", n * W, n * H, n)
    check_frame(r, fine, prim, n)
    r.set_option("timing", 1)
    for _ in range(5):
        r.replay_frame()
    launches, ms = r.resolve_timing()
    frame_ms, shade_ms = r.last_frame_time_ms()
    assert launches == 5 and ms > 0 and frame_ms > shade_ms > 0
    check_frame(r, fine, prim, n)
    r.close()


@pytest.mark.parametrize("n", NS)
def test_switching_the_option(n):
    sc = M.scene("balls", n * W, n * H, n)
    fine, prim = M.oracle("balls", n * W, n * H, n)
    r = Renderer(W, H)
    r.set_option("sample_shading", 1)
    r.set_option("supersample", n)
    handles = r.render_scene(sc)
    per_sample = r.read_framebuffer()
    assert same(per_sample, RR.resolve(fine, n)) and same(r.read_samples(), fine)
    r.set_option("sample_shading", 1)                              # no change: the frame stays current
    assert same(r.read_framebuffer(), per_sample)
    r.set_option("sample_shading", 0)
    expect(NOT_IN_FRAME, r.read_framebuffer)                       # no current frame after the option
    expect(NOT_IN_FRAME, r.read_sample_map)
    r.render_scene(sc, handles)
    check_frame(r, fine, prim, n)
    r.set_option("sample_shading", 1)
    expect(NOT_IN_FRAME, r.read_samples)
    r.render_scene(sc, handles)
    assert same(r.read_framebuffer(), per_sample) and same(r.read_samples(), fine)       # per-sample bits again
    r.set_option("supersample", 1)                                 # stored at any n; without effect at n = 1
    r.set_option("sample_shading", 0)
    one = M.scene("balls", W, H, 1)
    r.render_scene(one, handles)
    assert same(r.read_framebuffer(), bbo.render(one)[0]) and not r.read_sample_map().any()
    r.close()


def test_resize_keeps_the_option():
    n = 2
    r = multisampled(64, 64, n)
    handles = r.render_scene(M.scene("ball", n * 64, n * 64, n))
    r.synchronize()
    r.resize(W, H)
    expect(NOT_IN_FRAME, r.read_sample_map)
    r.render_scene(M.scene("ball", n * W, n * H, n), handles)
    check_frame(r, *M.oracle("ball", n * W, n * H, n), n)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    r = Renderer(W, H)
    r.set_option("sample_shading", 0)
    expect(NOT_IN_FRAME, r.read_sample_map)
    for bad in (2, -1, 3):
        expect(INVALID, r.set_option, "sample_shading", bad)
    expect(INVALID, r.set_option, "supersample", 3)                # the pair (3, 0), this order
    assert r.supersample == 1
    sc = M.scene("ball", 2 * W, 2 * H, 2)
    r.set_option("supersample", 2)
    handles = r.render_scene(sc)
    before = r.read_framebuffer()
    expect(INVALID, r.set_option, "supersample", 3)
    assert same(r.read_framebuffer(), before)                      # the context is unchanged: the frame is still current
    r.set_option("sample_shading", 1)
    r.set_option("supersample", 3)
    expect(INVALID, r.set_option, "sample_shading", 0)             # the pair (3, 0), the other order
    r.render_scene(M.scene("ball", 3 * W, 3 * H, 3), handles)
    assert same(r.read_framebuffer(), RR.resolve(r.read_samples(), 3))        # still per-sample n = 3
    r.close()
    r = multisampled(W, H, 2, overlays=1, render_pass=1)           # what n >= 2 refuses stays refused
    r.render_scene(sc)
    r.present()
    for call in (r.draw_overlays, r.read_visibility, r.read_gbuffer, r.read_surface, r.read_records):
        e = expect(INVALID, call)
        assert "supersample" in str(e), e
    r.close()
