"""GPU: shadow mapping (option "shadow_map", bbr_render_shadow_map, k_shade_shadow) against the CPU model
of tests/shadow_reference.py on the scenes of tests/shadow_scenes.py.  Everything is bit for bit, NaN in the same places, no
tolerance ("equal": surface_chart.equal_but_for_nan_payload).

  1  map      read_shadow_map() is the oracle's depth of the light's frame: every kind, S and tile mode, called inside the frame
              and after it
  2  mask     read_shadow_mask() is the model on the P of read_surface() (deferred: through bbo.half_round) and the oracle's map,
              for every S and bias, at both frame sizes; the census of tests/test_shadow_reference.py holds on the device's mask
  3  frame    the frame is the model's light loop on the dumped surface (deferred: the G-buffer) with the device's mask; also
              with max_anisotropy 16 and with present_fused (bytes)
  4  nothing shadowed is nothing changed: bias 2, and a light that looks away -- the frame of the same context with option 0
              (k_shade_shadow against k_shade)
  5  state    no map yet, a second call, a change of S, a resize, every refusal, nothing left alive
  6  around   four frames in flight with replay_frame, a partition of three, supersample 2 in both sample modes, a pass that
              overflows its first capacities"""
import ctypes as C
import functools

import numpy as np
import pytest

import sample_merge_reference as MR
import shadow_reference as SR
import shadow_scenes as SS
import surface_chart as SC
from bibim_renderer_amd import BibimError, Renderer
from bibim_renderer_amd import partition as P
from bibim_renderer_amd.renderer import live_resources
from oracle import bbo

pytestmark = pytest.mark.gpu

F = np.float32
INVALID, NOT_IN_FRAME = -1, -6
equal = SC.equal_but_for_nan_payload
bits = SC.bits
pass_id = lambda d: "deferred" if d else "forward"


def expect(code, call, *args):
    with pytest.raises(BibimError) as e:
        call(*args)
    assert e.value.code == code, e.value


def record(r, sc, handles, before_end=None):
    """render_scene, with a call between the draws and end_frame"""
    if handles is None:
        handles = {"mesh": {}, "mat": {}}
    r.set_frame_uniforms(sc.frame)
    r.set_view_uniforms(sc.view)
    r.begin_frame()
    for d in sc.draws:
        if id(d.vertices) not in handles["mesh"]:
            handles["mesh"][id(d.vertices)] = r.upload_mesh(d.vertices, d.indices)
        if id(d.material) not in handles["mat"]:
            handles["mat"][id(d.material)] = r.upload_material(d.material.maps)
        r.draw(handles["mesh"][id(d.vertices)], handles["mat"][id(d.material)], d.instances)
    if before_end:
        before_end()
    r.end_frame()
    return handles


def context(kind, size, side, **options):
    r = Renderer(*size)
    for k, v in options.items():
        r.set_option(k, v)
    r.set_option("shadow_map", side)
    return r


def shadowed(kind, size, side, bias=SS.BIAS, caster=SS.CASTER, **options):
    """a context that has rendered `kind` once, then its map, then the frame again under the map"""
    r = context(kind, size, side, **options)
    sc = SS.scene(kind, size)
    h = r.render_scene(sc)
    r.render_shadow_map(caster, SS.light_view(kind), bias)
    r.replay_frame()
    return r, sc, h


def model_inputs(r, deferred):
    """(light-loop inputs [n, 12], the P the test sees [h, w, 3]) from the device's dumps"""
    surf = r.read_surface()
    if not deferred:
        return SC.surface_values(surf), np.ascontiguousarray(surf[..., 6:9])
    gbuf = r.read_gbuffer()
    Pr = bbo.half_round(np.ascontiguousarray(surf[..., 6:9]))
    assert equal(gbuf[..., 0, :3], Pr), "the G-buffer's position is not the rounded dump"
    return SC.gbuffer_values(gbuf), Pr


@functools.lru_cache(None)
def base_frame(kind, deferred, size=SS.FRAME_SMALL, side=64):
    """the shadowed frame of the default context (the reference of 6), checked against the model on the way"""
    r, sc, _ = shadowed(kind, size, side, render_pass=deferred)
    frame = r.read_framebuffer()
    inputs, _ = model_inputs(r, deferred)
    mask = r.read_shadow_mask()
    r.close()
    assert equal(frame.reshape(-1, 4), SR.lit_frame(sc.frame, sc.view, inputs, mask, SS.CASTER))
    assert (mask == SR.SHADOWED).any() and (mask == SR.LIT).any()
    frame.setflags(write=False)
    return frame


# ---------------------------------------------------------------------------------------------------------------------
# 1. map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_mode", [0, 1])
@pytest.mark.parametrize("side", SS.SIDES)
@pytest.mark.parametrize("kind", SS.KINDS)
def test_map_is_the_oracles_depth(kind, side, tile_mode):
    want = SS.oracle_map(kind, side)
    r = context(kind, SS.FRAME_SMALL, side, tile_mode=tile_mode)
    sc, L = SS.scene(kind), SS.light_view(kind)
    inside = []
    h = record(r, sc, None, lambda: (r.render_shadow_map(SS.CASTER, L, SS.BIAS), inside.append(r.read_shadow_map())))
    assert np.array_equal(bits(inside[0]), bits(want)), f"inside the frame: {int((bits(inside[0]) != bits(want)).sum())} texels differ"
    r.set_option("shadow_map", 0)           # drop it ...
    r.set_option("shadow_map", side)
    expect(NOT_IN_FRAME, r.read_shadow_map)
    r.render_shadow_map(SS.CASTER, L, SS.BIAS)   # ... and again, after the frame
    got = r.read_shadow_map()
    r.close()
    assert got.shape == (side, side)
    assert np.array_equal(bits(got), bits(want)), f"after the frame: {int((bits(got) != bits(want)).sum())} texels differ"


# ---------------------------------------------------------------------------------------------------------------------
# 2. mask
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [SS.FRAME_DUMP, SS.FRAME_SMALL], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("kind", SS.KINDS)
def test_mask_is_the_model(kind, deferred, size):
    # (both frames: at 128 x 128 the receiver's P are binary16 numbers already, so only 97 x 61 sees the deferred rounding there)
    sc, L = SS.scene(kind, size), SS.light_view(kind)
    M = SR.proj_view(L)
    r = Renderer(*size)
    r.set_option("render_pass", deferred)
    h = r.render_scene(sc)
    surf = r.read_surface()
    Ps = Pt = np.ascontiguousarray(surf[..., 6:9])
    if deferred:
        Pt = bbo.half_round(Ps)
    covered = SS.positions64(kind, size)[1]
    for side in SS.SIDES:
        depth = SS.oracle_map(kind, side)
        r.set_option("shadow_map", side)
        masks = {}
        for bias in SS.BIASES:
            r.render_shadow_map(SS.CASTER, L, bias)
            got = masks[bias] = r.read_shadow_mask()
            want = SR.classify(M, side, bias, Pt, depth, covered)
            assert np.array_equal(got, want), f"S = {side}, bias {bias}: {int((got != want).sum())} pixels differ, classes {np.bincount(got.ravel(), minlength=4)}"
        assert equal(r.read_surface(), surf), "the surface dump changed under the map"
        if side >= 33:
            P64 = Pt.astype(np.float64)
            c_bias = SS.census(kind, side, SS.BIAS, P64, covered, depth, masks[SS.BIAS])
            c_zero = SS.census(kind, side, 0.0, P64, covered, depth, masks[0.0], Ps)
            print(f"{kind} {pass_id(deferred)} {size} S = {side}: {c_bias}; bias 0: {c_zero}")
            SS.check_census(kind, side, c_bias, c_zero)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "max_anisotropy 16", "present_fused", "bias 0"])
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("kind", SS.KINDS)
def test_frame_is_the_models_light_loop(kind, deferred, variant):
    size = SS.FRAME_DUMP
    options = {"render_pass": deferred}
    if variant == "max_anisotropy 16":
        options["max_anisotropy"] = 16
    if variant == "present_fused":
        options["present_fused"] = 1
    r, sc, _ = shadowed(kind, size, 64, bias=0.0 if variant == "bias 0" else SS.BIAS, **options)
    frame = r.read_presented() if variant == "present_fused" else r.read_framebuffer()
    inputs, _ = model_inputs(r, deferred)
    mask = r.read_shadow_mask()
    again = r.read_presented() if variant == "present_fused" else r.read_framebuffer()
    r.close()
    assert (mask == SR.SHADOWED).sum() >= 64 and (mask == SR.LIT).sum() >= 64
    want = SR.lit_frame(sc.frame, sc.view, inputs, mask, SS.CASTER).reshape(size[1], size[0], 4)
    plain = bbo.light_surface(sc.frame, sc.view, inputs, literal=False).reshape(size[1], size[0], 4)
    assert not equal(want, plain), "the caster contributes nothing to the shadowed pixels"
    if variant == "present_fused":
        want = bbo.present(want, int(sc.frame["enable_tone_mapping"]), float(sc.frame["exposure"]))
        assert np.array_equal(frame, want), f"{int((frame != want).any(-1).sum())} presented pixels differ"
        assert np.array_equal(again, frame)
    else:
        assert equal(frame, want), f"{int((bits(frame) != bits(want)).any(-1).sum())} pixels differ"
        assert equal(again, frame), "the dumps re-render the frame: the same bits"


# ---------------------------------------------------------------------------------------------------------------------
# 4. nothing shadowed is nothing changed
# ---------------------------------------------------------------------------------------------------------------------
def away_view(kind):
    """the light's view turned round: every pixel of the frame is OUTSIDE"""
    vu = SS.light_view(kind).copy()
    if kind == "ortho":
        p = vu["proj"].copy()
        p[3][0] = 8.0                       # the box moved eight half extents sideways
        vu["proj"] = p
    else:
        eye, target = np.asarray(SS.SPOT_EYE, F), np.asarray(SS.SPOT_TARGET, F)
        vu["view"] = bbo.mat_look_at(eye, eye - (target - eye))
    return vu


@pytest.mark.parametrize("case", ["bias 2", "looks away"])
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("kind", ["ortho", "spot"])
def test_nothing_shadowed_is_nothing_changed(kind, deferred, case):
    size = SS.FRAME_DUMP
    sc = SS.scene(kind, size)
    r = Renderer(*size)
    r.set_option("render_pass", deferred)
    r.render_scene(sc)
    plain = r.read_framebuffer()                      # k_shade
    r.set_option("shadow_map", 33)
    if case == "bias 2":
        r.render_shadow_map(SS.CASTER, SS.light_view(kind), 2.0)
    else:
        r.render_shadow_map(SS.CASTER, away_view(kind), SS.BIAS)
    r.replay_frame()
    got = r.read_framebuffer()                        # k_shade_shadow
    mask = r.read_shadow_mask()
    r.close()
    assert not (mask == SR.SHADOWED).any() and (mask != 0).all()
    if case == "looks away":
        assert (mask == SR.OUTSIDE).all()
    else:
        assert (mask == SR.LIT).sum() >= 64
    assert equal(got, plain), f"{int((bits(got) != bits(plain)).any(-1).sum())} pixels differ"


# ---------------------------------------------------------------------------------------------------------------------
# 5. state
# ---------------------------------------------------------------------------------------------------------------------
def test_state_of_the_option_and_the_map():
    kind, size = "spot", SS.FRAME_SMALL
    sc, L = SS.scene(kind, size), SS.light_view(kind)
    r = Renderer(*size)
    h = r.render_scene(sc)
    plain = r.read_framebuffer()
    # the option at S but no map yet: the frame of option 0
    r.set_option("shadow_map", 64)
    r.replay_frame()
    assert equal(r.read_framebuffer(), plain)
    expect(NOT_IN_FRAME, r.read_shadow_map)
    expect(INVALID, r.read_shadow_mask)
    # a map: the next frame is shadowed
    r.render_shadow_map(SS.CASTER, L, SS.BIAS)
    assert equal(r.read_framebuffer(), plain), "the frame rendered before the call stays as it is"
    r.replay_frame()
    assert equal(r.read_framebuffer(), base_frame(kind, 0))
    # a second call with another index, then another bias, takes effect on the next frame
    r.render_shadow_map(0, L, SS.BIAS)
    r.replay_frame()
    other = r.read_framebuffer()
    inputs, mask = SC.surface_values(r.read_surface()), r.read_shadow_mask()
    assert equal(other.reshape(-1, 4), SR.lit_frame(sc.frame, sc.view, inputs, mask, 0)) and not equal(other, base_frame(kind, 0))
    r.render_shadow_map(7, L, SS.BIAS)                 # past NumLights = 4: shadows nothing
    r.replay_frame()
    assert equal(r.read_framebuffer(), plain) and (r.read_shadow_mask() == SR.SHADOWED).any()
    r.render_shadow_map(SS.CASTER, L, 2.0)
    r.replay_frame()
    assert equal(r.read_framebuffer(), plain)
    # bbr_resize keeps the map, the index and the bias
    r.render_shadow_map(SS.CASTER, L, SS.BIAS)
    r.resize(*SS.FRAME_DUMP)
    assert np.array_equal(bits(r.read_shadow_map()), bits(SS.oracle_map(kind, 64)))
    r.render_scene(SS.scene(kind, SS.FRAME_DUMP), h)
    assert equal(r.read_framebuffer(), base_frame(kind, 0, SS.FRAME_DUMP))
    r.resize(*size)
    # changing S drops the map
    r.set_option("shadow_map", 33)
    expect(NOT_IN_FRAME, r.read_shadow_map)
    r.render_scene(sc, h)
    assert equal(r.read_framebuffer(), plain)
    r.close()


def test_refusals():
    kind, size = "ortho", SS.FRAME_SMALL
    sc, L = SS.scene(kind, size), SS.light_view(kind)
    r = Renderer(*size)
    expect(INVALID, r.render_shadow_map, SS.CASTER, L, SS.BIAS)        # the option is 0
    expect(INVALID, r.read_shadow_map)
    for bad in (-1, 8193, 1 << 40):
        expect(INVALID, r.set_option, "shadow_map", bad)
    r.set_option("shadow_map", 33)
    expect(INVALID, r.set_option, "shadow_map", 8193)                  # ... and leaves the option as it was
    expect(NOT_IN_FRAME, r.render_shadow_map, SS.CASTER, L, SS.BIAS)   # no recorded draws
    r.begin_frame()
    r.render_shadow_map(SS.CASTER, L, SS.BIAS)                         # inside a frame without draws: an empty map
    assert not r.read_shadow_map().any()
    r.end_frame()
    h = r.render_scene(sc)
    for index in (-1, 100):
        expect(INVALID, r.render_shadow_map, index, L, SS.BIAS)
    expect(INVALID, r.render_shadow_map, SS.CASTER, L, float("nan"))
    assert r._L.bbr_render_shadow_map(r._ctx, SS.CASTER, None, C.c_float(0.0)) == INVALID
    assert r._L.bbr_read_shadow_map(r._ctx, None) == INVALID and r._L.bbr_read_shadow_mask(r._ctx, None) == INVALID
    r.render_shadow_map(SS.CASTER, L, float("inf"))                    # any other bias is a bias
    r.render_shadow_map(SS.CASTER, L, SS.BIAS)
    assert np.array_equal(bits(r.read_shadow_map()), bits(SS.oracle_map(kind, 33)))
    # mip_levels >= 2 together with shadow_map > 0, in whichever order
    expect(INVALID, r.set_option, "mip_levels", 2)
    r.set_option("mip_levels", 1)
    r.set_option("shadow_map", 0)
    r.set_option("mip_levels", 4)
    expect(INVALID, r.set_option, "shadow_map", 33)
    r.set_option("mip_levels", 1)
    # the mask has the output extent: refused with supersample >= 2, like the surface dump, and on a partition
    r.set_option("shadow_map", 33)
    r.render_scene(sc, h)
    r.render_shadow_map(SS.CASTER, L, SS.BIAS)
    r.set_option("supersample", 2)
    r.render_scene(sc, h)
    expect(INVALID, r.read_shadow_mask)
    expect(INVALID, r.read_surface)
    r.set_option("supersample", 1)
    expect(NOT_IN_FRAME, r.read_shadow_mask)                           # (the option dropped the frame)
    r.set_partition(0, 2, r.tile_height())
    r.render_scene(sc, h)
    expect(INVALID, r.read_shadow_mask)
    r.close()


def test_nothing_is_left_alive():
    before = live_resources()
    r, _, _ = shadowed("clipped", SS.FRAME_SMALL, 200, render_pass=1)
    r.read_shadow_mask()
    during = live_resources()
    assert during["device_allocs"] > before["device_allocs"]
    r.set_option("shadow_map", 0)                      # the option drops what it owns ...
    dropped = live_resources()
    assert dropped["device_bytes"] <= during["device_bytes"] - 200 * 200 * 8
    r.close()                                          # ... and the context the rest
    assert live_resources() == before
    r = context("spot", SS.FRAME_SMALL, 64)
    r.render_scene(SS.scene("spot"))
    r.render_shadow_map(SS.CASTER, SS.light_view("spot"), 0.0)
    r.close()                                          # with the map alive
    assert live_resources() == before


# ---------------------------------------------------------------------------------------------------------------------
# 6. around it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_four_frames_in_flight_and_replay(deferred):
    kind = "spot"
    r, sc, h = shadowed(kind, SS.FRAME_SMALL, 64, render_pass=deferred, frames_in_flight=4)
    for _ in range(6):
        r.replay_frame()
    assert equal(r.read_framebuffer(), base_frame(kind, deferred))
    for _ in range(3):
        r.render_scene(sc, h)
    r.render_shadow_map(SS.CASTER, SS.light_view(kind), SS.BIAS)        # drains the four, renders, and the frames go on
    for _ in range(5):
        r.replay_frame()
    got = r.read_framebuffer()
    r.close()
    assert equal(got, base_frame(kind, deferred))


@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_partition_of_three(deferred):
    kind, (w, h) = "clipped", SS.FRAME_SMALL
    shards = []
    for rank in range(3):
        r = context(kind, (w, h), 64, render_pass=deferred)
        band_rows = r.tile_height()
        r.set_partition(rank, 3, band_rows)
        r.render_scene(SS.scene(kind))
        r.render_shadow_map(SS.CASTER, SS.light_view(kind), SS.BIAS)
        assert np.array_equal(bits(r.read_shadow_map()), bits(SS.oracle_map(kind, 64))), "every rank renders the whole map"
        r.replay_frame()
        shards.append(r.read_shard())
        r.close()
    assert equal(P.unpack_gathered(np.stack(shards), h, band_rows), base_frame(kind, deferred)), "each shard is the whole frame's rows"


@pytest.mark.parametrize("sample_shading", [1, 0])
def test_supersample_two(sample_shading):
    kind, (w, h) = "spot", (48, 30)
    fine_ctx, _, _ = shadowed(kind, (2 * w, 2 * h), 64)
    fine = fine_ctx.read_framebuffer()
    assert (fine_ctx.read_shadow_mask() == SR.SHADOWED).sum() >= 64
    fine_ctx.close()
    r, _, _ = shadowed(kind, (w, h), 64, sample_shading=sample_shading, supersample=2)
    samples = r.read_samples()
    want = fine if sample_shading else MR.replicate(fine, r.read_sample_map(), 2)
    r.close()
    assert equal(samples, want), f"{int((bits(samples) != bits(want)).any(-1).sum())} samples differ"


def test_pass_overflows_its_first_capacities():
    kind, side = "clipped", 200
    r = context(kind, SS.FRAME_SMALL, side, bin_cap=4, broad_cap=1, clip_cap=1)
    grown = []
    # inside the frame: the pass is the first to meet the capacities
    record(r, SS.scene(kind), None, lambda: (grown.append(r.capacity_growths()),
                                             r.render_shadow_map(SS.CASTER, SS.light_view(kind), SS.BIAS),
                                             grown.append(r.capacity_growths())))
    assert grown[0] == 0 and grown[1] >= 1, grown
    assert np.array_equal(bits(r.read_shadow_map()), bits(SS.oracle_map(kind, side)))
    got = r.read_framebuffer()
    r.close()
    assert equal(got, base_frame(kind, 0, side=side))
