"""GPU: up to eight shadow casters per context (bbr_render_shadow_caster, k_shade_shadow_casters; DESIGN.md section 3, "Casters")
against the CPU model of tests/shadow_casters_reference.py on the scenes of tests/shadow_casters_scenes.py.  Everything is bit
for bit, NaN in the same places, no tolerance ("equal": surface_chart.equal_but_for_nan_payload).  Every test calls a new symbol.

  1  maps      every slot's every map is the oracle's depth: S in {33, 64}, both tile modes; one slot rendered inside the frame
               and the others after it
  2  verdicts  per slot, mask, face index and taps are the model on the dumped P: R in {0, 1, 2}, both passes, both frame sizes,
               with the census on the device's masks
  3  frame     the frame is the model's light loop on the dumped surface (deferred: the G-buffer) with the device's k-tuples:
               plain, max_anisotropy 16, present_fused (bytes), every bias 0
  4  hence     bit for bit: one caster alone in slot 5 against the same caster through bbr_render_shadow_faces (F = 1 and 6, R =
               0, 1, 2); "mixed" with its casters permuted over the slots; "mixed" with one caster at bias 2, and with one on
               light 50, against the frame without that caster
  5  eight     the frame and all eight masks are the model
  6  state     bbr_get_shadow_casters after each call; every refusal leaves the state unchanged; drop, and drop again; a change
               of S drops all slots; a resize keeps them; live_resources()
  7  around    four frames in flight with replay; a partition of three; supersample 2 in both sample modes; a pass in slot 1 that
               overflows its first capacities"""
import ctypes as C
import functools

import numpy as np
import pytest

import sample_merge_reference as MR
import shadow_casters_reference as CR
import shadow_casters_scenes as CS
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

INVALID, NOT_IN_FRAME = -1, -6
RADII = (0, 1, 2)
equal = SC.equal_but_for_nan_payload
bits = SC.bits
pass_id = lambda d: "deferred" if d else "forward"
size_id = lambda s: "%dx%d" % s


def expect(code, call, *args):
    with pytest.raises(BibimError) as e:
        call(*args)
    assert e.value.code == code, e.value


def record(r, sc, before_end=None):
    """render_scene, with a call between the draws and end_frame"""
    r.set_frame_uniforms(sc.frame)
    r.set_view_uniforms(sc.view)
    r.begin_frame()
    mesh, mat = {}, {}
    for d in sc.draws:
        if id(d.vertices) not in mesh:
            mesh[id(d.vertices)] = r.upload_mesh(d.vertices, d.indices)
        if id(d.material) not in mat:
            mat[id(d.material)] = r.upload_material(d.material.maps)
        r.draw(mesh[id(d.vertices)], mat[id(d.material)], d.instances)
    if before_end:
        before_end()
    r.end_frame()


def context(size, side, radius=0, **options):
    r = Renderer(*size)
    for k, v in options.items():
        r.set_option(k, v)
    r.set_option("shadow_map", side)
    r.set_option("shadow_filter", radius)
    return r


def cast(r, casters):
    for c in casters:
        r.render_shadow_caster(c["slot"], c["light"], c["views"], c["bias"])


def state(r):
    light, faces = r.shadow_casters()
    return light.tolist(), faces.tolist()


def state_of(casters):
    light, faces = [-1] * 8, [0] * 8
    for c in casters:
        light[c["slot"]], faces[c["slot"]] = c["light"], len(c["views"])
    return light, faces


def cast_scene(kind, size, side, radius=0, casters=None, **options):
    """a context that has rendered `kind` once, then its casters' maps, then the frame again under them"""
    casters = CS.casters(kind) if casters is None else casters
    r = context(size, side, radius, **options)
    sc = CS.scene(kind, size)
    h = r.render_scene(sc)
    cast(r, casters)
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


def device_verdicts(r, casters):
    """slot -> (mask, taps, face index) as the device reports them"""
    return {c["slot"]: (r.read_shadow_caster_mask(c["slot"]), r.read_shadow_caster_taps(c["slot"]), r.read_shadow_caster_face_index(c["slot"]))
            for c in casters}


def assert_verdicts(r, kind, casters, side, radius, Pt, size, what):
    covered = CS.positions64(kind, size)[1]
    want = CR.verdicts(casters, side, radius, Pt, lambda c: CS.oracle_maps(kind, c["slot"], side), covered)
    got = device_verdicts(r, casters)
    for s in want:
        for name, g, w in zip(("classes", "counts", "face indices"), got[s], want[s]):
            assert np.array_equal(g, w), f"{what} slot {s}: {int((g != w).sum())} {name} differ, {np.bincount(g.ravel(), minlength=5)[:27]}"
    return got


def model_frame(sc, inputs, got, casters, radius):
    return CR.lit_frame(sc.frame, sc.view, inputs, {s: got[s][1].ravel() for s in got}, {c["slot"]: c["light"] for c in casters}, radius)


@functools.lru_cache(None)
def base_frame(kind, deferred, size=CS.FRAME_SMALL, side=64, radius=1):
    """the frame of the default context under the casters of `kind` (the reference of 7), checked against the model on the way"""
    r, sc, _ = cast_scene(kind, size, side, radius, render_pass=deferred)
    frame = r.read_framebuffer()
    inputs, Pt = model_inputs(r, deferred)
    got = assert_verdicts(r, kind, CS.casters(kind), side, radius, Pt, size, f"{kind} {pass_id(deferred)}")
    r.close()
    assert equal(frame.reshape(-1, 4), model_frame(sc, inputs, got, CS.casters(kind), radius))
    frame.setflags(write=False)
    return frame


# ---------------------------------------------------------------------------------------------------------------------
# 1. maps
# ---------------------------------------------------------------------------------------------------------------------
def assert_maps(r, kind, casters, side, what):
    for c in casters:
        want = CS.oracle_maps(kind, c["slot"], side)
        for f in range(len(c["views"])):
            got = r.read_shadow_caster_face(c["slot"], f)
            assert got.shape == (side, side)
            assert np.array_equal(bits(got), bits(want[f])), f"{what}, slot {c['slot']} face {f}: {int((bits(got) != bits(want[f])).sum())} texels differ"
        expect(INVALID, r.read_shadow_caster_face, c["slot"], len(c["views"]))


@pytest.mark.parametrize("tile_mode", [0, 1])
@pytest.mark.parametrize("side", [33, 64])
def test_maps_are_the_oracles_depths(side, tile_mode):
    kind = "mixed"
    casters = CS.casters(kind)
    r = context(CS.FRAME_SMALL, side, tile_mode=tile_mode)
    inside = casters[1]          # slot 1 inside the frame, after the draws; the others after end_frame
    record(r, CS.scene(kind), lambda: r.render_shadow_caster(inside["slot"], inside["light"], inside["views"], inside["bias"]))
    assert state(r) == state_of([inside])
    cast(r, [casters[0], casters[2]])
    assert state(r) == state_of(casters)
    assert_maps(r, kind, casters, side, f"S = {side}, tile_mode {tile_mode}")
    assert np.array_equal(bits(r.read_shadow_face(0)), bits(r.read_shadow_caster_face(0, 0))), "the existing read-backs are slot 0"
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. verdicts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [CS.FRAME_DUMP, CS.FRAME_SMALL], ids=size_id)
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_verdicts_are_the_model(deferred, size):
    kind, side = "mixed", 64
    casters = CS.casters(kind)
    r, sc, h = cast_scene(kind, size, side, 0, render_pass=deferred)
    surf = r.read_surface()
    Pt = np.ascontiguousarray(surf[..., 6:9])
    if deferred:
        Pt = bbo.half_round(Pt)
    for radius in RADII:
        r.set_option("shadow_filter", radius)
        r.render_scene(sc, h)
        what = f"{kind} {pass_id(deferred)} {size} S = {side} R = {radius}"
        got = assert_verdicts(r, kind, casters, side, radius, Pt, size, what)
        if radius == 0:
            masks = {s: got[s][0] for s in got}
        if radius == 1:
            partial_both = int((sum((got[s][0] == PR.PARTIAL).astype(int) for s in got) >= 2).sum())
            assert partial_both >= CS.MIN_PARTIAL_BOTH, partial_both
        assert equal(r.read_surface(), surf), "the surface dump changed under the casters"
    r.close()
    # the census on the device's masks: a pixel counts where the closed-form position is clear of every threshold AND the device
    # reports that class (the PARTIAL condition: on the device's R = 1 masks, above)
    c = CS.census(kind, side, size, masks=masks)
    print(f"{kind} {pass_id(deferred)} {size}: {c}")
    CS.check_census(kind, c, side)


# ---------------------------------------------------------------------------------------------------------------------
# 3. frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("variant", ["plain", "max_anisotropy 16", "present_fused", "every bias 0"])
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_frame_is_the_models_light_loop(deferred, variant, radius):
    kind, size, side, fused = "mixed", CS.FRAME_DUMP, 64, variant == "present_fused"
    options = {"render_pass": deferred}
    if variant == "max_anisotropy 16":
        options["max_anisotropy"] = 16
    if fused:
        options["present_fused"] = 1
    casters = CS.casters(kind)
    if variant == "every bias 0":
        casters = tuple(dict(c, bias=0.0) for c in casters)
    r, sc, h = cast_scene(kind, size, side, radius, casters, **options)
    frame = read(r, fused)
    inputs, Pt = model_inputs(r, deferred)
    got = assert_verdicts(r, kind, casters, side, radius, Pt, size, f"{variant} R = {radius}")
    again = read(r, fused)
    r.close()
    want = model_frame(sc, inputs, got, casters, radius).reshape(size[1], size[0], 4)
    dark = sum((got[s][0] == SR.SHADOWED).astype(int) for s in got)
    assert (dark >= 2).sum() >= CS.MIN_BOTH, "too few pixels are shadowed in two slots at once"
    if fused:
        want = bbo.present(want, int(sc.frame["enable_tone_mapping"]), float(sc.frame["exposure"]))
        assert np.array_equal(frame, want), f"{int((frame != want).any(-1).sum())} presented pixels differ"
        assert np.array_equal(again, frame)
    else:
        assert equal(frame, want), f"{int((bits(frame) != bits(want)).any(-1).sum())} pixels differ"
        assert equal(again, frame), "the dumps re-render the frame: the same bits"


# ---------------------------------------------------------------------------------------------------------------------
# 4. hence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n_faces", [1, 6])
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_one_caster_in_slot_five_is_the_caster_of_slot_zero(deferred, n_faces, radius):
    size, side = FS.FRAME_SMALL, 64
    sc, views = FS.scene("cube", size), FS.faces("cube")[:n_faces]
    r = context(size, side, radius, render_pass=deferred)
    h = r.render_scene(sc)
    r.render_shadow_faces(FS.CASTER, views, FS.BIAS)
    r.replay_frame()
    want = r.read_framebuffer()
    want_v = (r.read_shadow_mask(), r.read_shadow_taps(), r.read_shadow_face_index())
    assert (want_v[0] == SR.SHADOWED).any() and (want_v[0] == SR.LIT).any()
    assert all(np.array_equal(a, b) for a, b in zip(want_v, device_verdicts(r, [dict(slot=0)])[0])), "the caster read-backs of slot 0"
    r.drop_shadow_caster(0)
    r.render_shadow_caster(5, FS.CASTER, views, FS.BIAS)
    assert state(r) == state_of([dict(slot=5, light=FS.CASTER, views=views)])
    r.replay_frame()
    got = r.read_framebuffer()
    got_v = device_verdicts(r, [dict(slot=5)])[5]
    expect(INVALID, r.read_shadow_mask)                  # slot 0 is not in use
    r.close()
    assert equal(got, want), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ"
    for name, g, w in zip(("classes", "counts", "face indices"), got_v, want_v):
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("radius", [0, 1])
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_permuting_the_casters_over_the_slots_changes_no_bit(deferred, radius):
    kind = "mixed"
    want = base_frame(kind, deferred, radius=radius)
    for slots in ((7, 2, 0), (3, 4, 6)):
        moved = [dict(c, slot=s) for c, s in zip(CS.casters(kind), slots)]
        r, _, _ = cast_scene(kind, CS.FRAME_SMALL, 64, radius, moved, render_pass=deferred)
        got = r.read_framebuffer()
        assert state(r) == state_of(moved)
        r.close()
        assert equal(got, want), f"slots {slots}: {int((bits(got) != bits(want)).any(-1).sum())} pixels differ"


@pytest.mark.parametrize("radius", [0, 1])
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_a_caster_that_shadows_nothing_leaves_the_others_alone(deferred, radius):
    kind, size, side = "mixed", CS.FRAME_SMALL, 64
    casters = CS.casters(kind)
    for out in (1, 2):           # (without slot 1: slot 5 keeps the casters kernel; without slot 5 likewise)
        rest = [c for i, c in enumerate(casters) if i != out]
        r, sc, h = cast_scene(kind, size, side, radius, rest, render_pass=deferred)
        without = r.read_framebuffer()
        assert not equal(without, base_frame(kind, deferred, radius=radius)), "the caster left out shadows something"
        c = casters[out]
        r.render_shadow_caster(c["slot"], c["light"], c["views"], 2.0)
        r.replay_frame()
        lifted = r.read_framebuffer()
        mask = r.read_shadow_caster_mask(c["slot"])
        assert not np.isin(mask, (SR.SHADOWED, PR.PARTIAL)).any() and (mask == SR.LIT).any()
        r.render_shadow_caster(c["slot"], 50, c["views"], c["bias"])
        r.replay_frame()
        beyond = r.read_framebuffer()
        assert (r.read_shadow_caster_mask(c["slot"]) == SR.SHADOWED).any(), "the mask of a caster beyond the lights is still evaluated"
        r.close()
        assert equal(lifted, without), "bias 2"
        assert equal(beyond, without), "light index 50"


# ---------------------------------------------------------------------------------------------------------------------
# 5. eight
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1])
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_eight_casters(deferred, radius):
    kind, size, side = "eight", CS.FRAME_DUMP, 64
    casters = CS.casters(kind)
    r, sc, _ = cast_scene(kind, size, side, radius, render_pass=deferred)
    assert state(r) == state_of(casters)
    frame = r.read_framebuffer()
    inputs, Pt = model_inputs(r, deferred)
    got = assert_verdicts(r, kind, casters, side, radius, Pt, size, f"eight {pass_id(deferred)} R = {radius}")
    r.close()
    assert min(int((got[s][0] == SR.SHADOWED).sum()) for s in got) >= CS.MIN_EIGHT
    want = model_frame(sc, inputs, got, casters, radius)
    assert equal(frame.reshape(-1, 4), want), f"{int((bits(frame.reshape(-1, 4)) != bits(want)).any(-1).sum())} pixels differ"


# ---------------------------------------------------------------------------------------------------------------------
# 6. state
# ---------------------------------------------------------------------------------------------------------------------
def test_state_and_refusals():
    kind, size, side = "mixed", CS.FRAME_SMALL, 64
    casters = CS.casters(kind)
    sc = CS.scene(kind, size)
    one = casters[1]
    before = live_resources()
    r = Renderer(*size)
    assert state(r) == state_of([])
    expect(INVALID, r.render_shadow_caster, 1, one["light"], one["views"], one["bias"])      # the option is 0
    r.set_option("shadow_map", side)
    expect(NOT_IN_FRAME, r.render_shadow_caster, 1, one["light"], one["views"], one["bias"])  # no recorded draws
    h = r.render_scene(sc)
    plain = r.read_framebuffer()
    empty = live_resources()
    r.drop_shadow_caster(3)                                # a slot not in use: BBR_OK
    expect(INVALID, r.drop_shadow_caster, 8)
    expect(INVALID, r.drop_shadow_caster, -1)
    for s in range(8):
        expect(INVALID, r.read_shadow_caster_mask, s)
        expect(INVALID, r.read_shadow_caster_face, s, 0)
    expect(NOT_IN_FRAME, r.read_shadow_face, 0)            # (the call from before there were slots keeps its answer)
    cast(r, casters)
    assert state(r) == state_of(casters)
    grown = live_resources()
    assert grown["device_bytes"] - empty["device_bytes"] >= (6 + 1 + 2) * side * side * 4
    r.replay_frame()
    frame = r.read_framebuffer()
    assert equal(frame, base_frame(kind, 0, radius=0))

    def unchanged(what):
        assert state(r) == state_of(casters), what
        assert_maps(r, kind, casters, side, what)
        r.replay_frame()
        assert equal(r.read_framebuffer(), frame), what

    # every refusal leaves every slot as it was, the slot named included
    for bad in (-1, 8):
        expect(INVALID, r.render_shadow_caster, bad, 1, one["views"], one["bias"])
        expect(INVALID, r.read_shadow_caster_mask, bad)
        expect(INVALID, r.read_shadow_caster_face, bad, 0)
    expect(INVALID, r.render_shadow_caster, 1, 2, one["views"], one["bias"])            # light 2 is slot 0's
    expect(INVALID, r.render_shadow_caster, 4, 3, one["views"], one["bias"])            # light 3 is slot 5's, also for a free slot
    expect(INVALID, r.render_shadow_map, 0, one["views"][0], one["bias"])               # ... and through the calls of slot 0
    expect(INVALID, r.render_shadow_faces, 3, FS.faces("cube"), FS.BIAS)
    seven = np.concatenate([FS.faces("cube"), one["views"]])
    expect(INVALID, r.render_shadow_caster, 1, one["light"], seven, one["bias"])
    expect(INVALID, r.render_shadow_caster, 1, one["light"], one["views"][:0], one["bias"])
    expect(INVALID, r.render_shadow_caster, 1, 100, one["views"], one["bias"])
    expect(INVALID, r.render_shadow_caster, 1, -1, one["views"], one["bias"])
    expect(INVALID, r.render_shadow_caster, 1, one["light"], one["views"], float("nan"))
    assert r._L.bbr_render_shadow_caster(r._ctx, 1, one["light"], 1, None, C.c_float(0.0)) == INVALID
    assert r._L.bbr_get_shadow_casters(r._ctx, None, None) == INVALID
    assert r._L.bbr_read_shadow_caster_mask(r._ctx, 1, None) == INVALID
    expect(INVALID, r.set_option, "mip_levels", 2)
    unchanged("after the refusals")
    # the same light again in its own slot is no duplicate
    r.render_shadow_caster(1, one["light"], one["views"], one["bias"])
    unchanged("slot 1 rendered again")
    # a resize keeps the slots
    r.resize(*CS.FRAME_DUMP)
    assert state(r) == state_of(casters)
    assert_maps(r, kind, casters, side, "after a resize")
    r.resize(*size)
    r.render_scene(sc, h)
    assert equal(r.read_framebuffer(), frame)
    # drop, then drop again: the frame of the other two; then all: the unshadowed kernels
    r.drop_shadow_caster(1)
    r.drop_shadow_caster(1)
    assert state(r) == state_of([casters[0], casters[2]])
    expect(INVALID, r.read_shadow_caster_mask, 1)
    r.replay_frame()
    assert not equal(r.read_framebuffer(), frame)
    r.drop_shadow_caster(5)
    r.replay_frame()
    only0 = r.read_framebuffer()                           # slot 0 alone: the kernels of before
    r.drop_shadow_caster(0)
    assert state(r) == state_of([])
    r.replay_frame()
    assert equal(r.read_framebuffer(), plain), "no slot in use: the frame before a map exists"
    expect(INVALID, r.read_shadow_mask)
    r.render_shadow_faces(2, FS.faces("cube"), CS.BIAS)
    r.replay_frame()
    assert equal(r.read_framebuffer(), only0), "slot 0 alone is bbr_render_shadow_faces"
    # a change of S drops every slot
    cast(r, casters[1:])
    r.set_option("shadow_map", 33)
    assert state(r) == state_of([])
    for s in (0, 1, 5):
        expect(INVALID, r.read_shadow_caster_face, s, 0)
    r.render_scene(sc, h)
    assert equal(r.read_framebuffer(), plain)
    settled = live_resources()
    cast(r, casters)
    assert live_resources()["device_bytes"] - settled["device_bytes"] >= (6 + 1 + 2) * 33 * 33 * 4
    for c in casters:
        r.drop_shadow_caster(c["slot"])
    r.set_option("shadow_map", 0)
    assert live_resources() == settled, "the drops and shadow_map 0 give back what the casters took"
    r.close()
    assert live_resources() == before
    r, _, _ = cast_scene(kind, size, side)
    r.close()                                              # with the maps and the table alive
    assert live_resources() == before


# ---------------------------------------------------------------------------------------------------------------------
# 7. around it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_four_frames_in_flight_and_replay(deferred):
    kind = "mixed"
    r, sc, h = cast_scene(kind, CS.FRAME_SMALL, 64, 1, render_pass=deferred, frames_in_flight=4)
    for _ in range(6):
        r.replay_frame()
    assert equal(r.read_framebuffer(), base_frame(kind, deferred))
    for _ in range(3):
        r.render_scene(sc, h)
    cast(r, CS.casters(kind)[1:])                          # each drains the four, renders, and the frames go on
    for _ in range(5):
        r.replay_frame()
    got = r.read_framebuffer()
    r.close()
    assert equal(got, base_frame(kind, deferred))


@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_partition_of_three(deferred):
    kind, (w, h) = "mixed", CS.FRAME_SMALL
    shards = []
    for rank in range(3):
        r = context((w, h), 64, 1, render_pass=deferred)
        band_rows = r.tile_height()
        r.set_partition(rank, 3, band_rows)
        r.render_scene(CS.scene(kind, (w, h)))
        cast(r, CS.casters(kind))
        assert_maps(r, kind, CS.casters(kind), 64, "every rank renders all the maps")
        r.replay_frame()
        shards.append(r.read_shard())
        r.close()
    assert equal(P.unpack_gathered(np.stack(shards), h, band_rows), base_frame(kind, deferred)), "each shard is the whole frame's rows"


@pytest.mark.parametrize("sample_shading", [1, 0])
def test_supersample_two(sample_shading):
    kind, (w, h) = "mixed", (48, 30)
    fine_ctx, _, _ = cast_scene(kind, (2 * w, 2 * h), 64, 1)
    fine = fine_ctx.read_framebuffer()
    assert all((fine_ctx.read_shadow_caster_mask(c["slot"]) == SR.SHADOWED).sum() >= 64 for c in CS.casters(kind))
    fine_ctx.close()
    r, _, _ = cast_scene(kind, (w, h), 64, 1, sample_shading=sample_shading, supersample=2)
    expect(INVALID, r.read_shadow_caster_mask, 1)          # the output extent: refused like its namesake
    samples = r.read_samples()
    want = fine if sample_shading else MR.replicate(fine, r.read_sample_map(), 2)
    r.close()
    assert equal(samples, want), f"{int((bits(samples) != bits(want)).any(-1).sum())} samples differ"


def test_pass_in_slot_one_overflows_its_first_capacities():
    kind, side = "mixed", 200
    casters = CS.casters(kind)
    r = context(CS.FRAME_SMALL, side, 0, bin_cap=4, broad_cap=1, clip_cap=1)
    grown = []
    one = casters[1]
    # inside the frame: the pass is the first to meet the capacities
    record(r, CS.scene(kind), lambda: (grown.append(r.capacity_growths()),
                                       r.render_shadow_caster(one["slot"], one["light"], one["views"], one["bias"]),
                                       grown.append(r.capacity_growths())))
    assert grown[0] == 0 and grown[1] >= 1, grown
    cast(r, [casters[0], casters[2]])
    assert_maps(r, kind, casters, side, "after the growth")
    r.replay_frame()
    got = r.read_framebuffer()
    r.close()
    assert equal(got, base_frame(kind, 0, side=side, radius=0))
