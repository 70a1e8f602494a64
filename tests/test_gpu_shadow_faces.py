"""GPU: shadow maps of up to six faces (bbr_render_shadow_faces, k_shade_shadow_faces; DESIGN.md section 3, "Faces") against
the CPU model of tests/shadow_faces_reference.py on the scenes of tests/shadow_faces_scenes.py.  Everything is bit for bit, NaN
in the same places, no tolerance ("equal": surface_chart.equal_but_for_nan_payload).

  1  maps     read_shadow_face(f) is the oracle's depth of face f's frame: S and tile mode, inside the frame and after it
  2  mask     read_shadow_mask() and read_shadow_face_index() are the model on the P of read_surface() (deferred: through
              bbo.half_round) and the oracle's maps, for every S and bias, at both frame sizes; the census of
              tests/test_shadow_faces_reference.py holds on the device's output
  3  frame    the frame is the model's light loop on the dumped surface with the device's mask; also with max_anisotropy 16
              and with present_fused (bytes)
  4  one face through the new call is bbr_render_shadow_map: map, mask, frame (k_shade_shadow's path)
  5  prefixes F = 3: what the full cube gives to faces 3 .. 5 is OUTSIDE, face 255; F = 2, 4, 5 against the model
  6  cascade  two nested orthographic faces against the model
  7  state    six faces then two, a change of S, a resize, every refusal, nothing left alive
  8  around   four frames in flight with replay_frame, a partition of three, supersample 2 in both sample modes, a pass that
              overflows its first capacities"""
import ctypes as C
import functools

import numpy as np
import pytest

import sample_merge_reference as MR
import shadow_faces_reference as FR
import shadow_faces_scenes as FS
import shadow_reference as SR
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


def context(size, side, **options):
    r = Renderer(*size)
    for k, v in options.items():
        r.set_option(k, v)
    r.set_option("shadow_map", side)
    return r


def shadowed(kind, size, side, bias=FS.BIAS, n_faces=None, **options):
    """a context that has rendered `kind` once, then its first n_faces maps, then the frame again under them"""
    r = context(size, side, **options)
    sc = FS.scene(kind, size)
    h = r.render_scene(sc)
    r.render_shadow_faces(FS.CASTER, FS.faces(kind)[:n_faces], bias)
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


def assert_maps(r, kind, side, n_faces, what):
    want = FS.oracle_maps(kind, side)
    for f in range(n_faces):
        got = r.read_shadow_face(f)
        assert got.shape == (side, side)
        assert np.array_equal(bits(got), bits(want[f])), f"{what}, face {f}: {int((bits(got) != bits(want[f])).sum())} texels differ"
    assert np.array_equal(bits(r.read_shadow_map()), bits(want[0])), "read_shadow_map reads face 0"


def assert_model(r, kind, side, bias, deferred, size, n_faces=None, census=False):
    """mask, face index and frame of the context's last frame against the model; returns (mask, face)"""
    sc = FS.scene(kind, size)
    frame = r.read_framebuffer()
    inputs, Pt = model_inputs(r, deferred)
    mask, face = r.read_shadow_mask(), r.read_shadow_face_index()
    covered = FS.positions64(kind, size)[1]
    want_mask, want_face = FR.classify(FS.matrices(kind)[:n_faces], side, bias, Pt, FS.oracle_maps(kind, side)[:n_faces], covered)
    what = f"{kind} {pass_id(deferred)} {size} S = {side}, bias {bias}, F = {n_faces}"
    assert np.array_equal(mask, want_mask), f"{what}: {int((mask != want_mask).sum())} classes differ, {np.bincount(mask.ravel(), minlength=4)}"
    assert np.array_equal(face, want_face), f"{what}: {int((face != want_face).sum())} face indices differ"
    assert equal(frame.reshape(-1, 4), SR.lit_frame(sc.frame, sc.view, inputs, mask, FS.CASTER)), f"{what}: the frame"
    if census:
        c = FS.census(mask, face, covered, 6)
        print(f"{what}: {c}")
        FS.check_census(c, size, what)
    return mask, face


@functools.lru_cache(None)
def base_frame(kind, deferred, size=FS.FRAME_SMALL, side=64):
    """the shadowed frame of the default context (the reference of 8), checked against the model on the way"""
    r, _, _ = shadowed(kind, size, side, render_pass=deferred)
    frame = r.read_framebuffer()
    mask, face = assert_model(r, kind, side, FS.BIAS, deferred, size)
    r.close()
    assert (mask == SR.SHADOWED).any() and len(np.unique(face[face != 255])) == len(FS.faces(kind))
    frame.setflags(write=False)
    return frame


# ---------------------------------------------------------------------------------------------------------------------
# 1. maps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side, tile_mode", [(33, 0), (33, 1), (64, 0), (64, 1), (1, 1), (200, 0)])
def test_maps_are_the_oracles_depths(side, tile_mode):
    kind = "cube"
    r = context(FS.FRAME_SMALL, side, tile_mode=tile_mode)
    sc, Ls = FS.scene(kind), FS.faces(kind)
    record(r, sc, lambda: (r.render_shadow_faces(FS.CASTER, Ls, FS.BIAS), assert_maps(r, kind, side, 6, "inside the frame")))
    r.set_option("shadow_map", 0)           # drop them ...
    r.set_option("shadow_map", side)
    expect(NOT_IN_FRAME, r.read_shadow_face, 0)
    r.render_shadow_faces(FS.CASTER, Ls, FS.BIAS)   # ... and again, after the frame
    assert_maps(r, kind, side, 6, "after the frame")
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. mask and face index
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [FS.FRAME_DUMP, FS.FRAME_SMALL], ids=size_id)
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_mask_and_face_index_are_the_model(deferred, size):
    kind = "cube"
    sc, Ls, Ms = FS.scene(kind, size), FS.faces(kind), FS.matrices(kind)
    r = Renderer(*size)
    r.set_option("render_pass", deferred)
    r.render_scene(sc)
    surf = r.read_surface()
    Pt = np.ascontiguousarray(surf[..., 6:9])
    if deferred:
        Pt = bbo.half_round(Pt)
    covered = FS.positions64(kind, size)[1]
    for side in FS.SIDES:
        maps = FS.oracle_maps(kind, side)
        r.set_option("shadow_map", side)
        for bias in FS.BIASES:
            r.render_shadow_faces(FS.CASTER, Ls, bias)
            mask, face = r.read_shadow_mask(), r.read_shadow_face_index()
            want_mask, want_face = FR.classify(Ms, side, bias, Pt, maps, covered)
            what = f"S = {side}, bias {bias}"
            assert np.array_equal(mask, want_mask), f"{what}: {int((mask != want_mask).sum())} classes differ, {np.bincount(mask.ravel(), minlength=4)}"
            assert np.array_equal(face, want_face), f"{what}: {int((face != want_face).sum())} face indices differ"
            if bias == FS.BIAS:
                c = FS.census(mask, face, covered, 6)
                print(f"cube {pass_id(deferred)} {size} S = {side}: {c}")
                FS.check_census(c, size, what)
            if bias == -1.0:
                assert not (mask == SR.LIT).any()
            if bias == 2.0:
                assert not (mask == SR.SHADOWED).any()
        assert equal(r.read_surface(), surf), "the surface dump changed under the maps"
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "max_anisotropy 16", "present_fused"])
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_frame_is_the_models_light_loop(deferred, variant):
    kind, size = "cube", FS.FRAME_DUMP
    options = {"render_pass": deferred}
    if variant == "max_anisotropy 16":
        options["max_anisotropy"] = 16
    if variant == "present_fused":
        options["present_fused"] = 1
    r, sc, _ = shadowed(kind, size, 64, **options)
    frame = r.read_presented() if variant == "present_fused" else r.read_framebuffer()
    inputs, _ = model_inputs(r, deferred)
    mask, face = r.read_shadow_mask(), r.read_shadow_face_index()
    again = r.read_presented() if variant == "present_fused" else r.read_framebuffer()
    r.close()
    FS.check_census(FS.census(mask, face, FS.positions64(kind, size)[1], 6), size, variant)
    want = SR.lit_frame(sc.frame, sc.view, inputs, mask, FS.CASTER).reshape(size[1], size[0], 4)
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
# 4. one face
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("kind, f", [("cube", 0), ("cube", 3), ("cascade", 1)])
def test_one_face_is_render_shadow_map(kind, f, deferred):
    size, side = FS.FRAME_SMALL, 64
    L = FS.faces(kind)[f:f + 1]
    got = {}
    for call in ("render_shadow_map", "render_shadow_faces"):
        r = context(size, side, render_pass=deferred)
        r.render_scene(FS.scene(kind, size))
        if call == "render_shadow_map":
            r.render_shadow_map(FS.CASTER, np.array(L[0]), FS.BIAS)
        else:
            r.render_shadow_faces(FS.CASTER, L, FS.BIAS)
        r.replay_frame()
        got[call] = (r.read_shadow_map(), r.read_shadow_face(0), r.read_shadow_mask(), r.read_shadow_face_index(), r.read_framebuffer())
        expect(INVALID, r.read_shadow_face, 1)
        r.close()
    a, b = got["render_shadow_map"], got["render_shadow_faces"]
    assert np.array_equal(bits(a[0]), bits(FS.oracle_maps(kind, side)[f]))
    assert (a[2] == SR.SHADOWED).sum() >= 32 and (a[2] == SR.LIT).sum() >= 32
    for k in (0, 1):
        assert np.array_equal(bits(a[k]), bits(b[k])), "the map"
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), "mask and face index"
    assert np.array_equal(a[3], np.where((a[2] == SR.LIT) | (a[2] == SR.SHADOWED), 0, 255))
    assert equal(a[4], b[4]), "the frame"


# ---------------------------------------------------------------------------------------------------------------------
# 5. prefixes
# ---------------------------------------------------------------------------------------------------------------------
def test_prefix_of_three_leaves_the_rest_outside():
    kind, size, side = "cube", FS.FRAME_DUMP, 64
    full = shadowed(kind, size, side)[0]
    full_face = full.read_shadow_face_index()
    full.close()
    r, _, _ = shadowed(kind, size, side, n_faces=3)
    mask, face = assert_model(r, kind, side, FS.BIAS, 0, size, n_faces=3)
    expect(INVALID, r.read_shadow_face, 3)
    r.close()
    later = (full_face >= 3) & (full_face <= 5)
    assert later.sum() >= 300
    assert (mask[later] == SR.OUTSIDE).all() and (face[later] == 255).all()
    assert np.array_equal(face[~later], full_face[~later])


@pytest.mark.parametrize("n_faces", [2, 4, 5])
def test_other_prefixes_against_the_model(n_faces):
    kind, size, side = "cube", FS.FRAME_SMALL, 33
    r, _, _ = shadowed(kind, size, side, n_faces=n_faces, render_pass=n_faces % 2)
    assert_maps(r, kind, side, n_faces, f"F = {n_faces}")
    _, face = assert_model(r, kind, side, FS.BIAS, n_faces % 2, size, n_faces=n_faces)
    r.close()
    assert sorted(np.unique(face)) == list(range(n_faces)) + [255]


# ---------------------------------------------------------------------------------------------------------------------
# 6. cascade
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
@pytest.mark.parametrize("side", [33, 200])
def test_cascade_is_the_model(side, deferred):
    kind, size = "cascade", FS.FRAME_SMALL
    r, _, _ = shadowed(kind, size, side, render_pass=deferred)
    assert_maps(r, kind, side, 2, "cascade")
    mask, face = assert_model(r, kind, side, FS.BIAS, deferred, size)
    r.close()
    for f in (0, 1):
        assert ((mask == SR.LIT) & (face == f)).sum() >= 32 and ((mask == SR.SHADOWED) & (face == f)).sum() >= 32, f
    assert ((mask == SR.OUTSIDE) & (face == 255)).sum() >= 32


# ---------------------------------------------------------------------------------------------------------------------
# 7. state
# ---------------------------------------------------------------------------------------------------------------------
def test_six_faces_then_two_then_other_sizes():
    kind, size = "cube", FS.FRAME_SMALL
    before = live_resources()
    r, sc, h = shadowed(kind, size, 64)
    assert equal(r.read_framebuffer(), base_frame(kind, 0))
    assert_model(r, kind, 64, FS.BIAS, 0, size)
    six = live_resources()
    assert six["device_bytes"] - before["device_bytes"] >= 6 * 64 * 64 * 4
    # two faces: the frame follows, face 2 is gone, no buffer is added
    r.render_shadow_faces(FS.CASTER, FS.faces(kind)[:2], FS.BIAS)
    assert equal(r.read_framebuffer(), base_frame(kind, 0)), "the frame rendered before the call stays as it is"
    r.replay_frame()
    assert_model(r, kind, 64, FS.BIAS, 0, size, n_faces=2)
    expect(INVALID, r.read_shadow_face, 2)
    assert live_resources() == six, "the read-backs' buffers are gone and the maps' buffer is the one of six faces"
    # ... and one: k_shade_shadow again
    r.render_shadow_map(FS.CASTER, np.array(FS.faces(kind)[0]), FS.BIAS)
    r.replay_frame()
    assert_model(r, kind, 64, FS.BIAS, 0, size, n_faces=1)
    # bbr_resize keeps the maps, the index and the bias
    r.render_shadow_faces(FS.CASTER, FS.faces(kind), FS.BIAS)
    r.resize(*FS.FRAME_DUMP)
    assert_maps(r, kind, 64, 6, "after a resize")
    r.render_scene(FS.scene(kind, FS.FRAME_DUMP), h)
    assert_model(r, kind, 64, FS.BIAS, 0, FS.FRAME_DUMP, census=True)
    r.resize(*size)
    # changing S drops the maps: the frame of option 0 until they are rendered again
    r.set_option("shadow_map", 33)
    expect(NOT_IN_FRAME, r.read_shadow_face, 0)
    r.render_scene(sc, h)
    plain = r.read_framebuffer()
    expect(INVALID, r.read_shadow_face_index)
    r.render_shadow_faces(FS.CASTER, FS.faces(kind), FS.BIAS)
    r.replay_frame()
    assert_model(r, kind, 33, FS.BIAS, 0, size)
    assert not equal(r.read_framebuffer(), plain)
    # the tile mode drops the pass's tile buffers, not the maps
    r.set_option("tile_mode", 1)
    assert_maps(r, kind, 33, 6, "after tile_mode")
    r.render_scene(sc, h)
    r.render_shadow_faces(FS.CASTER, FS.faces(kind), FS.BIAS)
    assert_maps(r, kind, 33, 6, "rendered in the other tile mode")
    r.set_option("shadow_map", 0)                      # the option drops what it owns ...
    assert live_resources()["device_bytes"] <= six["device_bytes"] - 6 * 64 * 64 * 4
    r.close()                                          # ... and the context the rest
    assert live_resources() == before
    r, _, _ = shadowed(kind, size, 64)
    r.close()                                          # with the maps alive
    assert live_resources() == before


def test_refusals():
    kind, size = "cube", FS.FRAME_SMALL
    sc, Ls = FS.scene(kind, size), FS.faces(kind)
    r = Renderer(*size)
    expect(INVALID, r.render_shadow_faces, FS.CASTER, Ls, FS.BIAS)        # the option is 0
    expect(INVALID, r.read_shadow_face, 0)
    r.set_option("shadow_map", 33)
    expect(NOT_IN_FRAME, r.render_shadow_faces, FS.CASTER, Ls, FS.BIAS)   # no recorded draws
    h = r.render_scene(sc)
    seven = np.concatenate([Ls, Ls[:1]])
    expect(INVALID, r.render_shadow_faces, FS.CASTER, seven, FS.BIAS)     # n_faces 7 ...
    expect(INVALID, r.render_shadow_faces, FS.CASTER, Ls[:0], FS.BIAS)    # ... and 0
    assert r._L.bbr_render_shadow_faces(r._ctx, FS.CASTER, -1, Ls.ctypes.data_as(C.c_void_p), C.c_float(0.0)) == INVALID
    assert r._L.bbr_render_shadow_faces(r._ctx, FS.CASTER, 6, None, C.c_float(0.0)) == INVALID
    for index in (-1, 100):
        expect(INVALID, r.render_shadow_faces, index, Ls, FS.BIAS)
    expect(INVALID, r.render_shadow_faces, FS.CASTER, Ls, float("nan"))
    expect(NOT_IN_FRAME, r.read_shadow_face, 0)                           # nothing of the above rendered a map
    r.render_shadow_faces(FS.CASTER, Ls[:4], FS.BIAS)
    for bad in (-1, 4, 6, 255):
        expect(INVALID, r.read_shadow_face, bad)
    assert r._L.bbr_read_shadow_face(r._ctx, 0, None) == INVALID and r._L.bbr_read_shadow_face_index(r._ctx, None) == INVALID
    assert_maps(r, kind, 33, 4, "after the refusals")
    # mip_levels >= 2 together with shadow_map > 0
    expect(INVALID, r.set_option, "mip_levels", 2)
    # mask and face index have the output extent: refused with supersample >= 2, and on a partition
    r.set_option("supersample", 2)
    r.render_scene(sc, h)
    expect(INVALID, r.read_shadow_mask)
    expect(INVALID, r.read_shadow_face_index)
    r.set_option("supersample", 1)
    expect(NOT_IN_FRAME, r.read_shadow_face_index)                        # (the option dropped the frame)
    r.set_partition(0, 2, r.tile_height())
    r.render_scene(sc, h)
    expect(INVALID, r.read_shadow_mask)
    expect(INVALID, r.read_shadow_face_index)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. around it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_four_frames_in_flight_and_replay(deferred):
    kind = "cube"
    r, sc, h = shadowed(kind, FS.FRAME_SMALL, 64, render_pass=deferred, frames_in_flight=4)
    for _ in range(6):
        r.replay_frame()
    assert equal(r.read_framebuffer(), base_frame(kind, deferred))
    for _ in range(3):
        r.render_scene(sc, h)
    r.render_shadow_faces(FS.CASTER, FS.faces(kind), FS.BIAS)        # drains the four, renders, and the frames go on
    for _ in range(5):
        r.replay_frame()
    got = r.read_framebuffer()
    r.close()
    assert equal(got, base_frame(kind, deferred))


@pytest.mark.parametrize("deferred", [0, 1], ids=pass_id)
def test_partition_of_three(deferred):
    kind, (w, h) = "cube", FS.FRAME_SMALL
    shards = []
    for rank in range(3):
        r = context((w, h), 64, render_pass=deferred)
        band_rows = r.tile_height()
        r.set_partition(rank, 3, band_rows)
        r.render_scene(FS.scene(kind))
        r.render_shadow_faces(FS.CASTER, FS.faces(kind), FS.BIAS)
        assert_maps(r, kind, 64, 6, "every rank renders all the maps")
        r.replay_frame()
        shards.append(r.read_shard())
        r.close()
    assert equal(P.unpack_gathered(np.stack(shards), h, band_rows), base_frame(kind, deferred)), "each shard is the whole frame's rows"


@pytest.mark.parametrize("sample_shading", [1, 0])
def test_supersample_two(sample_shading):
    kind, (w, h) = "cube", (48, 30)
    fine_ctx, _, _ = shadowed(kind, (2 * w, 2 * h), 64)
    fine = fine_ctx.read_framebuffer()
    face = fine_ctx.read_shadow_face_index()
    assert (fine_ctx.read_shadow_mask() == SR.SHADOWED).sum() >= 64 and len(np.unique(face)) >= 6
    fine_ctx.close()
    r, _, _ = shadowed(kind, (w, h), 64, sample_shading=sample_shading, supersample=2)
    samples = r.read_samples()
    want = fine if sample_shading else MR.replicate(fine, r.read_sample_map(), 2)
    r.close()
    assert equal(samples, want), f"{int((bits(samples) != bits(want)).any(-1).sum())} samples differ"


def test_pass_overflows_its_first_capacities():
    kind, side = "cube", 200
    r = context(FS.FRAME_SMALL, side, bin_cap=4, broad_cap=1, clip_cap=1)
    grown = []
    # inside the frame: the pass is the first to meet the capacities
    record(r, FS.scene(kind), lambda: (grown.append(r.capacity_growths()),
                                       r.render_shadow_faces(FS.CASTER, FS.faces(kind), FS.BIAS),
                                       grown.append(r.capacity_growths())))
    assert grown[0] == 0 and grown[1] >= 1, grown
    assert_maps(r, kind, side, 6, "after the growth")
    got = r.read_framebuffer()
    r.close()
    assert equal(got, base_frame(kind, 0, side=side))
