"""GPU: percentage-closer shadow filtering (option "shadow_filter", k_shade_shadow_pcf, bbr_read_shadow_taps; DESIGN.md section
3, "Filtering") against the CPU model of tests/shadow_filter_reference.py on the scenes of tests/shadow_scenes.py and
tests/shadow_faces_scenes.py.  Everything is bit for bit, NaN in the same places, no tolerance ("equal":
surface_chart.equal_but_for_nan_payload).

  1  taps     read_shadow_taps() and read_shadow_mask() are the model on the P of read_surface() (deferred: through
              bbo.half_round) and the oracle's maps: one face for every kind, pass, frame size, S in {1, 2, 33, 64, 200}, R and
              bias; faces for both kinds, S in {33, 64}, both R (there also read_shadow_face_index()); the surface dump is
              unchanged under the filter
  2  frame    the frame is the model's light loop on the dumped surface (deferred: the G-buffer) with the device's k; also with
              max_anisotropy 16, with present_fused (bytes) and at bias 0; at least 64 PARTIAL pixels, and the frame differs
              from the hard rule's on them
  3  degenerate equalities, no model involved: S = 1 is the R = 0 frame, bias 2 the frame without a map, bias -1 the R = 0
              frame at bias -1, and R set back to 0 gives the hard frame's bits again
  4  state    the values refused, the option stored while shadow_map is 0, the map untouched by it, mip_levels 2 still refused,
              read_shadow_taps' refusals, nothing left alive
  5  around   four frames in flight with replay_frame, a partition of three, supersample 2 in both sample modes"""
import functools

import numpy as np
import pytest

import sample_merge_reference as MR
import shadow_faces_scenes as FS
import shadow_filter_reference as PR
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
RADII = (1, 2)
SIDES = (1, 2, 33, 64, 200)
equal = SC.equal_but_for_nan_payload
bits = SC.bits
pass_id = lambda d: "deferred" if d else "forward"
size_id = lambda s: "%dx%d" % s


def expect(code, call, *args):
    with pytest.raises(BibimError) as e:
        call(*args)
    assert e.value.code == code, e.value


def is_faces(kind):
    return kind in FS.KINDS


def scene_of(kind, size):
    return FS.scene(kind, size) if is_faces(kind) else SS.scene(kind, size)


def views_of(kind):
    return FS.faces(kind) if is_faces(kind) else SS.light_view(kind)


def matrices_of(kind):
    return list(FS.matrices(kind)) if is_faces(kind) else [SR.proj_view(SS.light_view(kind))]


def maps_of(kind, side):
    return FS.oracle_maps(kind, side) if is_faces(kind) else SS.oracle_map(kind, side)[None]


def covered_of(kind, size):
    return (FS.positions64 if is_faces(kind) else SS.positions64)(kind, size)[1]


def render_map(r, kind, bias):
    if is_faces(kind):
        r.render_shadow_faces(SS.CASTER, views_of(kind), bias)
    else:
        r.render_shadow_map(SS.CASTER, views_of(kind), bias)


def filtered(kind, size, side, radius, bias=SS.BIAS, **options):
    """a context that has rendered `kind` once, then its map(s), then the frame again under them and the filter"""
    r = Renderer(*size)
    for k, v in options.items():
        r.set_option(k, v)
    r.set_option("shadow_map", side)
    r.set_option("shadow_filter", radius)
    sc = scene_of(kind, size)
    h = r.render_scene(sc)
    render_map(r, kind, bias)
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


def read(r, presented=False):
    return r.read_presented() if presented else r.read_framebuffer()


@functools.lru_cache(None)
def base_frame(kind, deferred, size=SS.FRAME_SMALL, side=64, radius=1):
    """the filtered frame of the default context (the reference of 5), checked against the model on the way"""
    r, sc, _ = filtered(kind, size, side, radius, render_pass=deferred)
    frame = r.read_framebuffer()
    inputs, _ = model_inputs(r, deferred)
    k, mask = r.read_shadow_taps(), r.read_shadow_mask()
    r.close()
    assert equal(frame.reshape(-1, 4), PR.lit_frame(sc.frame, sc.view, inputs, k, SS.CASTER, radius))
    assert (mask == PR.PARTIAL).sum() >= 32 and (mask == SR.SHADOWED).any() and (mask == SR.LIT).any()
    frame.setflags(write=False)
    return frame


# ---------------------------------------------------------------------------------------------------------------------
# 1. taps and mask
# ---------------------------------------------------------------------------------------------------------------------
def assert_taps(r, kind, side, radius, bias, Pt, covered, what):
    want_cls, want_k, want_face = PR.taps(matrices_of(kind), side, bias, Pt, maps_of(kind, side), radius, covered)
    k, mask = r.read_shadow_taps(), r.read_shadow_mask()
    what = f"{what} S = {side}, R = {radius}, bias {bias}"
    assert np.array_equal(k, want_k), f"{what}: {int((k != want_k).sum())} counts differ, by k {np.bincount(k.ravel(), minlength=256)[:26]}"
    assert np.array_equal(mask, want_cls), f"{what}: {int((mask != want_cls).sum())} classes differ, {np.bincount(mask.ravel(), minlength=5)}"
    if is_faces(kind):
        face = r.read_shadow_face_index()
        assert np.array_equal(face, want_face), f"{what}: {int((face != want_face).sum())} face indices differ"
    return mask


@pytest.mark.parametrize("size", [SS.FRAME_DUMP, SS.FRAME_SMALL], ids=size_id)
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("kind", SS.KINDS)
def test_taps_and_mask_are_the_model(kind, deferred, size):
    sc = scene_of(kind, size)
    r = Renderer(*size)
    r.set_option("render_pass", deferred)
    h = r.render_scene(sc)
    surf = r.read_surface()
    Pt = np.ascontiguousarray(surf[..., 6:9])
    if deferred:
        Pt = bbo.half_round(Pt)
    covered = covered_of(kind, size)
    partial = 0
    for side in SIDES:
        r.set_option("shadow_map", side)
        for radius in RADII:
            r.set_option("shadow_filter", radius)
            r.render_scene(sc, h)
            for bias in SS.BIASES:
                render_map(r, kind, bias)
                mask = assert_taps(r, kind, side, radius, bias, Pt, covered, f"{kind} {pass_id(deferred)} {size}")
                partial += int((mask == PR.PARTIAL).sum())
                if side == 1 or bias in (-1.0, 2.0):
                    assert not (mask == PR.PARTIAL).any()
            assert equal(r.read_surface(), surf), "the surface dump changed under the filter"
    r.close()
    assert partial >= 64


@pytest.mark.parametrize("size", [FS.FRAME_DUMP, FS.FRAME_SMALL], ids=size_id)
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("kind", FS.KINDS)
def test_taps_and_mask_are_the_model_with_faces(kind, deferred, size):
    sc = scene_of(kind, size)
    r = Renderer(*size)
    r.set_option("render_pass", deferred)
    h = r.render_scene(sc)
    surf = r.read_surface()
    Pt = np.ascontiguousarray(surf[..., 6:9])
    if deferred:
        Pt = bbo.half_round(Pt)
    covered = covered_of(kind, size)
    for side in (33, 64):
        r.set_option("shadow_map", side)
        for radius in RADII:
            r.set_option("shadow_filter", radius)
            r.render_scene(sc, h)
            for bias in (FS.BIAS, 0.0):
                render_map(r, kind, bias)
                mask = assert_taps(r, kind, side, radius, bias, Pt, covered, f"{kind} {pass_id(deferred)} {size}")
                assert (mask == PR.PARTIAL).sum() >= 64
        assert equal(r.read_surface(), surf), "the surface dump changed under the filter"
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("variant", ["plain", "max_anisotropy 16", "present_fused", "bias 0"])
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("kind", ["clipped", "ortho", "cube"])
def test_frame_is_the_models_light_loop(kind, deferred, variant, radius):
    size, fused = SS.FRAME_DUMP, variant == "present_fused"
    options = {"render_pass": deferred}
    if variant == "max_anisotropy 16":
        options["max_anisotropy"] = 16
    if fused:
        options["present_fused"] = 1
    r, sc, h = filtered(kind, size, 64, radius, bias=0.0 if variant == "bias 0" else SS.BIAS, **options)
    frame = read(r, fused)
    inputs, _ = model_inputs(r, deferred)
    k, mask = r.read_shadow_taps(), r.read_shadow_mask()
    again = read(r, fused)
    r.set_option("shadow_filter", 0)                 # the hard rule's frame of the same context
    r.render_scene(sc, h)
    hard = read(r, fused)
    r.close()
    partial = mask == PR.PARTIAL
    assert partial.sum() >= 64, np.bincount(mask.ravel(), minlength=5)
    assert ((k > 0) & (k < PR.taps_of(radius)) == partial).all()
    want = PR.lit_frame(sc.frame, sc.view, inputs, k, SS.CASTER, radius).reshape(size[1], size[0], 4)
    if fused:
        want = bbo.present(want, int(sc.frame["enable_tone_mapping"]), float(sc.frame["exposure"]))
        differs = (frame != hard).any(-1)
        assert np.array_equal(frame, want), f"{int((frame != want).any(-1).sum())} presented pixels differ"
        assert np.array_equal(again, frame)
    else:
        differs = (bits(frame) != bits(hard)).any(-1)
        assert equal(frame, want), f"{int((bits(frame) != bits(want)).any(-1).sum())} pixels differ"
        assert equal(again, frame), "the dumps re-render the frame: the same bits"
    print(f"{kind} {pass_id(deferred)} {variant} R = {radius}: {int(partial.sum())} PARTIAL pixels, {int((differs & partial).sum())} of them differ "
          f"from the hard rule's frame, {int((differs & ~partial).sum())} others")
    assert (differs & partial).any(), "the filter changes no PARTIAL pixel"
    assert not (differs & ~partial).any(), "a pixel whose taps agree is the hard rule's"


# ---------------------------------------------------------------------------------------------------------------------
# 3. degenerate equalities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("kind", ["ortho", "clipped", "cube"])
def test_degenerate_equalities(kind, deferred, radius):
    size = SS.FRAME_DUMP
    sc = scene_of(kind, size)
    r = Renderer(*size)
    r.set_option("render_pass", deferred)
    h = r.render_scene(sc)
    plain = r.read_framebuffer()                       # no map

    def frame_at(side, bias, R):
        r.set_option("shadow_map", side)
        r.set_option("shadow_filter", R)
        r.render_scene(sc, h)
        render_map(r, kind, bias)
        r.replay_frame()
        return r.read_framebuffer()

    hard_one = frame_at(1, SS.BIAS, 0)
    assert equal(frame_at(1, SS.BIAS, radius), hard_one), "S = 1: every tap is texel (0, 0)"
    assert (r.read_shadow_mask() != PR.PARTIAL).all() and np.isin(r.read_shadow_taps(), (0, PR.taps_of(radius), 255)).all()
    assert equal(frame_at(33, 2.0, radius), plain), "bias 2: every tap is lit"
    assert not (r.read_shadow_mask() == SR.SHADOWED).any()
    hard_dark = frame_at(33, -1.0, 0)
    assert equal(frame_at(33, -1.0, radius), hard_dark), "bias -1: no tap is lit"
    assert not np.isin(r.read_shadow_mask(), (SR.LIT, PR.PARTIAL)).any()
    hard = frame_at(64, SS.BIAS, 0)
    soft = frame_at(64, SS.BIAS, radius)
    assert not equal(soft, hard)
    r.set_option("shadow_filter", 0)                   # back: the map stays, the frame is the hard one's again
    r.render_scene(sc, h)
    assert equal(r.read_framebuffer(), hard)
    k0, m0 = r.read_shadow_taps(), r.read_shadow_mask()
    r.close()
    assert np.array_equal(k0, np.where(m0 == SR.LIT, 1, np.where(m0 == SR.SHADOWED, 0, 255))), "R = 0 is K = 1"
    assert (m0 == SR.LIT).any() and (m0 == SR.SHADOWED).any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. state
# ---------------------------------------------------------------------------------------------------------------------
def test_state_and_refusals():
    kind, size = "clipped", SS.FRAME_SMALL
    sc = scene_of(kind, size)
    before = live_resources()
    r = Renderer(*size)
    for bad in (-1, 3, 1 << 40):
        expect(INVALID, r.set_option, "shadow_filter", bad)
    r.set_option("shadow_filter", 1)                   # stored while shadow_map is 0 ...
    expect(INVALID, r.set_option, "shadow_filter", 3)  # ... and a refused value leaves it as it was
    h = r.render_scene(sc)
    plain = r.read_framebuffer()
    expect(INVALID, r.read_shadow_taps)                # no map
    assert r._L.bbr_read_shadow_taps(r._ctx, None) == INVALID
    r.set_option("shadow_map", 64)
    expect(INVALID, r.read_shadow_taps)                # the option, but no map yet
    r.replay_frame()
    assert equal(r.read_framebuffer(), plain), "no map yet: the frame of option 0"
    render_map(r, kind, SS.BIAS)
    r.replay_frame()
    assert equal(r.read_framebuffer(), base_frame(kind, 0)), "the stored value is in effect once a map exists"
    depth = r.read_shadow_map()
    r.set_option("shadow_filter", 2)                   # keeps the map, leaves no current frame
    assert np.array_equal(bits(r.read_shadow_map()), bits(depth)) and np.array_equal(bits(depth), bits(SS.oracle_map(kind, 64)))
    expect(NOT_IN_FRAME, r.read_shadow_taps)
    expect(NOT_IN_FRAME, r.replay_frame)
    r.render_scene(sc, h)
    assert equal(r.read_framebuffer(), base_frame(kind, 0, radius=2))
    expect(INVALID, r.set_option, "mip_levels", 2)     # still refused
    r.set_option("supersample", 2)
    r.render_scene(sc, h)
    expect(INVALID, r.read_shadow_taps)
    r.set_option("supersample", 1)
    expect(NOT_IN_FRAME, r.read_shadow_taps)
    r.set_partition(0, 2, r.tile_height())
    r.render_scene(sc, h)
    expect(INVALID, r.read_shadow_taps)
    r.close()
    assert live_resources() == before


# ---------------------------------------------------------------------------------------------------------------------
# 5. around it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_four_frames_in_flight_and_replay(deferred):
    kind = "clipped"
    r, sc, h = filtered(kind, SS.FRAME_SMALL, 64, 1, render_pass=deferred, frames_in_flight=4)
    for _ in range(6):
        r.replay_frame()
    assert equal(r.read_framebuffer(), base_frame(kind, deferred))
    for _ in range(3):
        r.render_scene(sc, h)
    render_map(r, kind, SS.BIAS)                       # drains the four, renders, and the frames go on
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
        r = Renderer(w, h)
        r.set_option("render_pass", deferred)
        r.set_option("shadow_map", 64)
        r.set_option("shadow_filter", 1)
        band_rows = r.tile_height()
        r.set_partition(rank, 3, band_rows)
        r.render_scene(scene_of(kind, (w, h)))
        render_map(r, kind, SS.BIAS)
        r.replay_frame()
        shards.append(r.read_shard())
        r.close()
    assert equal(P.unpack_gathered(np.stack(shards), h, band_rows), base_frame(kind, deferred)), "each shard is the whole frame's rows"


@pytest.mark.parametrize("sample_shading", [1, 0])
def test_supersample_two(sample_shading):
    kind, (w, h) = "clipped", (48, 30)
    fine_ctx, _, _ = filtered(kind, (2 * w, 2 * h), 64, 1)
    fine = fine_ctx.read_framebuffer()
    assert (fine_ctx.read_shadow_mask() == PR.PARTIAL).sum() >= 64
    fine_ctx.close()
    r, _, _ = filtered(kind, (w, h), 64, 1, sample_shading=sample_shading, supersample=2)
    samples = r.read_samples()
    want = fine if sample_shading else MR.replicate(fine, r.read_sample_map(), 2)
    r.close()
    assert equal(samples, want), f"{int((bits(samples) != bits(want)).any(-1).sum())} samples differ"
