"""GPU: option "supersample" (k_resolve and the render extent behind it), bit for bit.

  fine frame    read_samples() of a W x H context with n is the oracle's frame at nW x nH, and the frame of a second context
                created as nW x nH
  resolve       read_framebuffer() is tests/resolve_reference.py on read_samples() of the same context
  hazards       NaN in the samples, 1 x 1 and 1 x H outputs, rows longer than a workgroup, a caller's buffer with a canary
  the rest      presentation (fused and not), the GUI pass, partitions and the exchange forms act on the resolved values;
                the option's state, range and refusals

Where NaN occurs its placement is compared, not its payload.  Every test starts by setting the option, so every one of them
fails on a library without it ("unknown option: supersample")."""
import functools

import numpy as np
import pytest

import resolve_reference as RR
import ui_reference as U
from bibim_renderer_amd import BibimError, Renderer, configs
from bibim_renderer_amd import partition as P
from bibim_renderer_amd.renderer import UiDrawData
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

F = np.float32
INVALID, NOT_IN_FRAME = -1, -6
W, H = 37, 23                       # output of the main cases: fine 74 x 46, 111 x 69, 148 x 92 -- partial edge tiles, no multiple of 4
NS = (2, 3, 4)
SCENES = ("triangle", "ball")


def same(a, b):
    """bit for bit; NaN by placement"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


@functools.lru_cache(None)
def material():
    from bibim_renderer_amd import textures
    return bbo.MaterialData(textures.make_material(64))


@functools.lru_cache(None)
def scene(name, w, h):
    """the scene whose uniforms belong to a w x h frame (a W x H context with n renders the one of nW x nH)"""
    if name == "triangle":
        return scenes.triangle_scene(w, h)
    return scenes.shaderball_scene(configs.C2.scaled(w, h, 64), material())


@functools.lru_cache(None)
def oracle(name, w, h, deferred=False):
    sc = scene(name, w, h)
    out = (bbo.render_deferred(sc) if deferred else bbo.render(sc))[0]
    out.setflags(write=False)
    return out


def supersampled(w, h, n, **options):
    r = Renderer(w, h)
    r.set_option("supersample", n)
    for k, v in options.items():
        r.set_option(k, v)
    return r


def expect(code, call, *args):
    with pytest.raises(BibimError) as e:
        call(*args)
    assert e.value.code == code, e.value


# ---------------------------------------------------------------------------------------------------------------------
# the fine frame is the oracle's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("n", NS)
def test_fine_frame_is_the_oracles(name, n):
    sc = scene(name, n * W, n * H)
    r = supersampled(W, H, n)
    r.render_scene(sc)
    fine = r.read_samples()
    assert fine.shape == (n * H, n * W, 4)
    assert same(fine, oracle(name, n * W, n * H))
    st = r.stats()
    r.close()
    big = Renderer(n * W, n * H)                    # the definition: a context created at the fine extent, supersample 1
    big.render_scene(sc)
    assert same(fine, big.read_framebuffer())
    assert same(big.read_samples(), fine)           # n = 1: read_samples is read_framebuffer
    bst = big.stats()
    st.pop("bin_overflow"), bst.pop("bin_overflow")  # (capacity growths: a history, not a count of the frame)
    assert st == bst                                # the statistics count fine samples and fine tiles
    big.close()


# ---------------------------------------------------------------------------------------------------------------------
# resolve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("n", NS)
def test_resolve_is_the_models(name, n, deferred, item_route):
    r = supersampled(W, H, n, render_pass=deferred)
    r.render_scene(scene(name, n * W, n * H))
    fine, out = r.read_samples(), r.read_framebuffer()
    r.close()
    assert same(fine, oracle(name, n * W, n * H, bool(deferred)))
    assert out.shape == (H, W, 4) and same(out, RR.resolve(fine, n))
    if not deferred and name == "triangle":
        assert ((out[..., 3] > 0) & (out[..., 3] < 1)).any()       # forward alpha: the covered fraction, on the silhouette
    if deferred:
        assert (out[..., 3] == 1).all()


@pytest.mark.parametrize("option,value", [("max_anisotropy", 4), ("mip_levels", 15)])
def test_resolve_under_the_sampler_options(option, value):
    n = 3
    r = supersampled(W, H, n, **{option: value})
    r.render_scene(scene("ball", n * W, n * H))
    fine, out = r.read_samples(), r.read_framebuffer()
    r.close()
    assert not same(fine, oracle("ball", n * W, n * H))           # the option reached the fine frame's shading
    assert same(out, RR.resolve(fine, n))


# ---------------------------------------------------------------------------------------------------------------------
# hazard inputs for the kernel alone
# ---------------------------------------------------------------------------------------------------------------------
def nan_scene(w, h):
    """the default material (roughness 0) under a point light at the origin: the deferred pass lights the cleared texels at
    distance 0 -- a NaN background around a finite triangle"""
    sc = scenes.triangle_scene(w, h)
    sc.frame = scenes.frame_uniforms([scenes.light(0, pos=(0, 0, 0), color=(1, 1, 1), intensity=10.0)])
    return sc


@pytest.mark.parametrize("n", NS)
def test_nan_goes_through_the_additions(n):
    r = supersampled(W, H, n, render_pass=1)
    r.render_scene(nan_scene(n * W, n * H))
    fine, out = r.read_samples(), r.read_framebuffer()
    r.close()
    if np.isfinite(fine).all():
        pytest.skip("the fine frame of this scene holds neither NaN nor inf")
    want = RR.resolve(fine, n)
    assert np.isnan(fine).any() and np.isfinite(fine[..., :3]).all(axis=2).any()
    assert np.isnan(want[..., :3]).any() and same(out, want)


@pytest.mark.parametrize("w,h,name", [(1, 1, "triangle"), (1, 29, "triangle"), (1, 29, "ball")])
def test_one_pixel_wide_outputs(w, h, name):
    n = 3
    r = supersampled(w, h, n)
    r.render_scene(scene(name, n * w, n * h))
    fine, out = r.read_samples(), r.read_framebuffer()
    r.close()
    assert same(fine, oracle(name, n * w, n * h))
    assert out.shape == (h, w, 4) and same(out, RR.resolve(fine, n))


def test_rows_longer_than_a_workgroups_span():
    """8191 x 2 with n = 4: 32 workgroups per output row, the last one partial; fine rows of 32764 pixels, 524 224 bytes"""
    w, h, n = 8191, 2, 4
    sc = scenes.triangle_scene(n * w, n * h, material())
    sc.view = scenes.view_uniforms((0, 0, 0), 0.0, 0.0, 1, 1, 0)  # aspect 1: the textured triangle stretched over a third of the row
    r = supersampled(w, h, n)
    r.render_scene(sc)
    fine, out = r.read_samples(), r.read_framebuffer()
    r.close()
    covered = (fine[..., 3] == 1).any(axis=0)
    assert covered.sum() > n * w // 8 and len(np.unique(fine[..., 0])) > 100
    assert ((out[..., 3] > 0) & (out[..., 3] < 1)).sum() > w // 8  # partly covered output pixels along the whole span
    assert same(out, RR.resolve(fine, n))


def test_callers_buffer_with_a_canary():
    import torch
    w, h, n = 5, 3, 2
    buf = torch.full((h * w * 4 + 64,), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r = supersampled(w, h, n)
    r.set_output_device_ptr(buf.data_ptr(), h * w * 16)
    sc = scene("ball", n * w, n * h)
    handles = r.render_scene(sc)
    fine = r.read_samples()
    got = buf.cpu().numpy()
    assert same(got[:h * w * 4].reshape(h, w, 4), RR.resolve(fine, n))
    assert (got[h * w * 4:] == -77.0).all()                        # nothing behind the output's last pixel
    assert same(r.read_framebuffer(), RR.resolve(fine, n))
    r.set_option("supersample", 3)                                 # the output size did not change: the buffer stays
    r.render_scene(scene("ball", 3 * w, 3 * h), handles)
    fine = r.read_samples()
    got = buf.cpu().numpy()
    assert same(got[:h * w * 4].reshape(h, w, 4), RR.resolve(fine, 3)) and (got[h * w * 4:] == -77.0).all()
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# presentation and the GUI pass act on the resolved values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tone", [0, 1])
@pytest.mark.parametrize("n", [2, 3])
def test_presentation_of_the_resolved_frame(n, tone):
    sc = scenes.shaderball_scene(configs.C2.scaled(n * W, n * H, 64), material())
    sc.frame["enable_tone_mapping"], sc.frame["exposure"] = tone, 1.3
    r = supersampled(W, H, n)
    handles = r.render_scene(sc)
    resolved = r.read_framebuffer()
    assert same(resolved, RR.resolve(r.read_samples(), n))
    want = {}
    for hdr16 in (True, False):
        r.present(hdr16=hdr16)
        want[hdr16] = bbo.present(resolved, tone, 1.3, hdr16)
        assert np.array_equal(r.read_presented(), want[hdr16]), hdr16
    r.set_option("present_fused", 1)                               # k_resolve's PRESENT form: the bytes of the unfused route
    r.render_scene(sc, handles)
    r.present()
    assert np.array_equal(r.read_presented(), want[True])
    expect(INVALID, r.read_framebuffer)                            # no W x H fp32 frame
    expect(INVALID, r.present, None, False)                        # fused presentation always has the binary16 stage
    assert same(RR.resolve(r.read_samples(), n), resolved)         # the fine frame exists
    r.close()


def test_gui_over_a_supersampled_frame():
    n = 2
    r = supersampled(W, H, n)
    texture = np.array([[[255, 200, 90, 180]]], np.uint8)
    assert r.upload_ui_texture(texture) == 1
    r.render_scene(scene("ball", n * W, n * H))
    resolved = r.read_framebuffer()
    r.present()
    base = r.read_presented()
    assert np.array_equal(base, bbo.present(resolved, 0, 1.0))
    draw = U.assemble([((0, 0, W, H), 1, [U.quad(3.25, 2.5, 30.0, 20.75, U.rgba(40, 220, 130, 150))])], (W, H))
    r.draw_ui(UiDrawData(draw.vertices, draw.indices, draw.cmds, draw.display_pos, draw.display_size, draw.framebuffer_scale))
    got = r.read_presented()
    want = U.render(base, draw, {1: texture})
    assert (want != base).any(axis=2).sum() > 300
    assert np.array_equal(got, want)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# partition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
def test_partition_in_output_rows(n):
    import torch
    w, h, band, world = 37, 100, 32, 3
    sc = scenes.shaderball_scene(configs.C3.scaled(n * w, n * h, 64), material())
    single = supersampled(w, h, n)
    single.render_scene(sc)
    whole = single.read_framebuffer()
    assert same(whole, RR.resolve(single.read_samples(), n))
    single.close()
    ranks = []
    for rank in range(world):
        r = supersampled(w, h, n)
        r.set_partition(rank, world, band)
        assert r.shard_rows() == P.shard_rows(h, world, band)
        r.render_scene(sc)
        shard = r.read_shard()
        assert same(shard, P.pack_shard(whole, rank, world, band)), rank     # padding rows zero
        expect(INVALID, r.read_samples)                                      # partitioned
        ranks.append(r)
    wants = {P.SHARD_RGBA32F: whole, P.SHARD_RGBA8: bbo.present(whole, 0, 1.0), P.SHARD_RGBA16F: bbo.half_round(whole)}
    for form, want in wants.items():
        block = ranks[0].exchange_block_bytes(form)
        assert block == P.exchange_block_bytes(form, h, w, world, band)
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
        expect(INVALID, r.stage_shard, P.SHARD_PACKED, scratch.data_ptr())   # one alpha bit per pixel: not lossless here
        expect(INVALID, r.pack_shard, scratch.data_ptr())
        r.close()
    assert not scratch.cpu().numpy().any()                                   # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# state
# ---------------------------------------------------------------------------------------------------------------------
def test_back_to_one_sample():
    r = supersampled(W, H, 2)
    sc = scene("ball", W, H)
    handles = r.render_scene(scene("ball", 2 * W, 2 * H))
    assert r.read_framebuffer().shape == (H, W, 4)
    r.set_option("supersample", 1)
    expect(NOT_IN_FRAME, r.read_framebuffer)                       # no current frame after the option
    expect(NOT_IN_FRAME, r.read_samples)
    r.render_scene(sc, handles)
    got = r.read_framebuffer()
    r.close()
    plain = Renderer(W, H)
    plain.render_scene(sc)
    assert same(got, plain.read_framebuffer()) and same(got, oracle("ball", W, H))
    plain.close()


def test_resize_keeps_the_option():
    n = 2
    r = supersampled(64, 64, n)
    handles = r.render_scene(scene("ball", n * 64, n * 64))
    r.synchronize()
    r.resize(W, H)
    expect(NOT_IN_FRAME, r.read_samples)
    r.render_scene(scene("ball", n * W, n * H), handles)
    fine = r.read_samples()
    assert same(fine, oracle("ball", n * W, n * H)) and same(r.read_framebuffer(), RR.resolve(fine, n))
    expect(INVALID, r.resize, 16385, 2)                            # 2 x 16385 > 32768
    assert same(r.read_framebuffer(), RR.resolve(fine, n))         # the context is unchanged
    r.close()


def test_replay_and_four_frames_in_flight(item_route):
    n = 3
    r = supersampled(W, H, n, frames_in_flight=4, bin_cap=8)      # (bins far too small: the first frame is re-rendered, resolve included)
    r.render_scene(scene("ball", n * W, n * H))
    for _ in range(6):
        r.replay_frame()
    fine, out = r.read_samples(), r.read_framebuffer()
    assert same(fine, oracle("ball", n * W, n * H)) and same(out, RR.resolve(fine, n))
    r.set_option("timing", 1)
    for _ in range(5):
        r.replay_frame()
    launches, ms = r.resolve_timing()
    frame_ms, shade_ms = r.last_frame_time_ms()
    assert launches == 5 and ms > 0 and frame_ms > shade_ms > 0
    assert same(r.read_framebuffer(), out)
    r.close()


def test_range_of_the_option():
    sc = scene("triangle", W, H)
    r = Renderer(W, H)
    handles = r.render_scene(sc)
    before = r.read_framebuffer()
    r.set_option("supersample", 1)                                 # no change: the frame stays current
    assert same(r.read_framebuffer(), before)
    for bad in (0, 5, -1):
        expect(INVALID, r.set_option, "supersample", bad)
    r.render_scene(sc, handles)
    assert same(r.read_framebuffer(), before) and same(before, oracle("triangle", W, H))
    r.close()
    wide = Renderer(16385, 2)
    expect(INVALID, wide.set_option, "supersample", 2)             # 2 x 16385 > 32768
    wide.render_scene(scene("triangle", 16385, 2))
    assert wide.read_framebuffer().shape == (2, 16385, 4)
    wide.close()


def test_what_is_refused_with_two_samples():
    r = supersampled(W, H, 2, overlays=1)
    r.render_scene(scene("ball", 2 * W, 2 * H))
    r.present()
    r.synchronize()
    expect(INVALID, r.draw_overlays)
    r.set_option("tbn", 1)
    r.render_scene(scene("ball", 2 * W, 2 * H))
    r.present()
    expect(INVALID, r.draw_overlays)
    r.set_option("render_pass", 1)                                 # (read_gbuffer is refused on a forward context anyway)
    r.render_scene(scene("ball", 2 * W, 2 * H))
    for call in (r.draw_overlays, r.read_visibility, r.read_gbuffer, r.read_surface, r.read_records):
        with pytest.raises(BibimError) as e:
            call()
        assert e.value.code == INVALID and "supersample" in str(e.value), e.value      # refused for THIS reason
    assert same(r.read_framebuffer(), RR.resolve(r.read_samples(), 2))
    r.close()
