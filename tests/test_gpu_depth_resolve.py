"""GPU: option "depth_resolve" (k_resolve_depth and the overlay pass behind it under "supersample" n >= 2).  Every comparison is
bit for bit -- byte for byte for presented images -- against the oracle at n W x n H plus tests/depth_resolve_reference.py.

  samples      read_sample_visibility() is the oracle's winners and depth at the fine extent
  the rule     read_visibility() (the dumping form of the kernel) and read_depth() (the plain one, option "overlays") are the
               model's in all three modes; 1 x 1, 1 x 23 and 8191 x 2 outputs
  overlays     present + draw_overlays on the comb and on `balls` with the gizmo is bbo.overlay (and tbn_reference) on the
               model's depth at the output extent, with "tbn" 0 and 1, fused presentation, the deferred path
  frames       four frames in flight, replay, the overflow re-render
  state        value 0 refuses as before, invalid values, switching, n = 1, partitions, what stays refused

Every test uses the option or one of the two new entry points, so every one of them fails on a library without them."""
import numpy as np
import pytest

import depth_resolve_reference as DR
import depth_resolve_scenes as S
import resolve_reference as RR
from bibim_renderer_amd import BibimError, Renderer
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
INVALID, NOT_IN_FRAME = -1, -6
W, H = 37, 23                       # output of the main cases: fine 74 x 46, 111 x 69, 148 x 92 -- partial edge tiles; the 3 x 3
NS = (2, 3, 4)                      # blocks of n = 3 straddle the tiles
OW, OH = S.COMB_W, S.COMB_H         # output of the overlay cases
GIZMO = 24


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def renderer(w, h, n, **options):
    r = Renderer(w, h)
    r.set_option("supersample", n)
    for k, v in options.items():
        r.set_option(k, v)
    return r


def expect(code, call, *args):
    with pytest.raises(BibimError) as e:
        call(*args)
    assert e.value.code == code, e.value
    return e.value


def shadings(n):
    return (1,) if n == 3 else (1, 0)                 # ("supersample" 3 with "sample_shading" 0 is refused)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the samples the rule chooses from
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("name", S.SCENES)
@pytest.mark.parametrize("n", NS)
def test_sample_visibility_is_the_oracles(name, n, deferred):
    sc = S.scene(name, n * W, n * H, n)
    _, want_prim, want_depth = S.oracle(name, n * W, n * H, n, bool(deferred))
    for shading in shadings(n):
        r = Renderer(W, H)
        r.set_option("sample_shading", shading)
        r.set_option("supersample", n)
        r.set_option("render_pass", deferred)
        handles = None
        for tile_mode in (1, 0):
            r.set_option("tile_mode", tile_mode)
            handles = r.render_scene(sc, handles)
            prim, depth = r.read_sample_visibility()
            assert prim.shape == depth.shape == (n * H, n * W)
            assert np.array_equal(prim, want_prim), (shading, tile_mode, int((prim != want_prim).sum()))
            assert np.array_equal(bits(depth), bits(want_depth)), (shading, tile_mode)
        r.close()


def test_sample_visibility_with_one_sample_is_read_visibility():
    sc = S.scene("ball", W, H, 1)
    r = Renderer(W, H)
    r.render_scene(sc)
    prim, depth = r.read_visibility()
    fine_prim, fine_depth = r.read_sample_visibility()
    r.close()
    _, want_prim, want_depth = S.oracle("ball", W, H, 1)
    assert np.array_equal(prim, want_prim) and np.array_equal(bits(depth), bits(want_depth))
    assert np.array_equal(fine_prim, prim) and np.array_equal(bits(fine_depth), bits(depth))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the rule: the dumping form behind read_visibility, the plain form behind read_depth
# ---------------------------------------------------------------------------------------------------------------------
def check_rule(r, sc, fine_prim, fine_depth, n, handles=None):
    """every mode on one context: the frame is rendered again after the option dropped it"""
    for mode in DR.MODES:
        r.set_option("depth_resolve", mode)
        handles = r.render_scene(sc, handles)
        want_depth, want_prim = DR.resolve(fine_depth, fine_prim, n, mode)
        kept = r.read_depth()
        prim, depth = r.read_visibility()
        assert kept.shape == want_depth.shape and prim.shape == want_prim.shape
        assert np.array_equal(bits(kept), bits(want_depth)), (mode, int((bits(kept) != bits(want_depth)).sum()))
        assert np.array_equal(bits(depth), bits(want_depth)), (mode, int((bits(depth) != bits(want_depth)).sum()))
        assert np.array_equal(prim, want_prim), (mode, int((prim != want_prim).sum()))
        assert np.array_equal(bits(r.read_depth()), bits(want_depth))      # the dump's re-render leaves the kept depth as it was
    return handles


@pytest.mark.parametrize("name", S.SCENES)
@pytest.mark.parametrize("n", NS)
def test_resolved_visibility_and_depth_are_the_models(name, n):
    sc = S.scene(name, n * W, n * H, n)
    _, fine_prim, fine_depth = S.oracle(name, n * W, n * H, n)
    for shading in shadings(n):
        r = renderer(W, H, n, overlays=1, sample_shading=shading)
        check_rule(r, sc, fine_prim, fine_depth, n)
        r.close()


@pytest.mark.parametrize("n", [2, 3])
def test_resolved_visibility_deferred_and_large_tiles(n):
    sc = S.scene("balls", n * W, n * H, n)
    _, fine_prim, fine_depth = S.oracle("balls", n * W, n * H, n, True)
    r = renderer(W, H, n, overlays=1, render_pass=1, tile_mode=0)
    check_rule(r, sc, fine_prim, fine_depth, n)
    r.close()


def test_read_visibility_needs_no_overlays_option():
    n = 2
    sc = S.scene("ball", n * W, n * H, n)
    _, fine_prim, fine_depth = S.oracle("ball", n * W, n * H, n)
    r = renderer(W, H, n, depth_resolve=DR.MAX)
    r.render_scene(sc)
    prim, depth = r.read_visibility()
    want_depth, want_prim = DR.resolve(fine_depth, fine_prim, n, DR.MAX)
    assert np.array_equal(prim, want_prim) and np.array_equal(bits(depth), bits(want_depth))
    err = expect(INVALID, r.read_depth)                               # nothing was kept: the frame has no option "overlays"
    assert "overlays" in str(err)
    r.close()


@pytest.mark.parametrize("w,h,name", [(1, 1, "triangle"), (1, 23, "triangle"), (1, 23, "ball")])
def test_one_pixel_wide_outputs(w, h, name):
    n = 3
    sc = S.scene(name, n * w, n * h, n)
    _, fine_prim, fine_depth = S.oracle(name, n * w, n * h, n)
    r = renderer(w, h, n, overlays=1)
    check_rule(r, sc, fine_prim, fine_depth, n)
    r.close()


def test_rows_longer_than_a_workgroups_span():
    """8191 x 2 with n = 4: 32 workgroups per output row, the last one partial; fine rows of 32764 depths, 131 056 bytes"""
    w, h, n = 8191, 2, 4
    sc = scenes.triangle_scene(n * w, n * h, S.SM.material())
    sc.view = scenes.view_uniforms((0, 0, 0), 0.0, 0.0, 1, 1, 0)     # aspect 1: the triangle stretched over a third of the row
    _, fine_prim, fine_depth, _ = bbo.render(sc)
    covered = (fine_prim != DR.NO_PRIM).any(axis=0)
    assert covered.sum() > n * w // 8
    d = {m: DR.resolve(fine_depth, fine_prim, n, m)[0].view(U) for m in DR.MODES}
    assert (d[DR.MIN] != d[DR.MAX]).sum() > w // 8                    # partly covered output pixels along the whole span
    r = renderer(w, h, n, overlays=1)
    check_rule(r, sc, fine_prim, fine_depth, n)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the overlay pass at the output extent, against the resolved depth
# ---------------------------------------------------------------------------------------------------------------------
def check_overlays(r, name, n, modes, tbns, deferred=False, handles=None):
    sc = S.scene(name, n * OW, n * OH, n)
    extent = GIZMO if name == "balls" else 0
    for mode in modes:
        r.set_option("depth_resolve", mode)
        for tbn in tbns:
            r.set_option("tbn", tbn)
            handles = r.render_scene(sc, handles)
            r.present()
            base, _, want = S.overlaid(name, n * OW, n * OH, n, mode, deferred, bool(tbn), extent)
            assert np.array_equal(r.read_presented(), base), (mode, tbn)
            r.draw_overlays(extent)
            got = r.read_presented()
            bad = (got != want).any(axis=2)
            assert not bad.any(), (mode, tbn, int(bad.sum()), np.argwhere(bad)[:5])
            assert (want != base).any() or (name == "comb" and mode == DR.MAX and not tbn)   # (MAX hides every marker of the comb)
    return handles


@pytest.mark.parametrize("n", NS)
def test_overlays_on_the_comb(n):
    r = renderer(OW, OH, n, overlays=1)
    check_overlays(r, "comb", n, DR.MODES, (0, 1))
    r.close()


@pytest.mark.parametrize("n", NS)
def test_overlays_on_the_balls_with_the_gizmo(n):
    raw, gi, _ = S.gizmo()
    r = renderer(OW, OH, n, overlays=1)
    r.upload_gizmo(raw, gi)
    check_overlays(r, "balls", n, DR.MODES, (0, 1) if n == 2 else (0,))     # (the TBN reference of `balls` resolves a million records)
    r.close()


@pytest.mark.parametrize("name", ["comb", "balls"])
def test_overlays_with_fused_presentation(name):
    n = 2
    raw, gi, _ = S.gizmo()
    r = renderer(OW, OH, n, overlays=1, present_fused=1)
    r.upload_gizmo(raw, gi)
    check_overlays(r, name, n, DR.MODES, (0, 1) if name == "comb" else (0,))
    r.close()


@pytest.mark.parametrize("name", ["comb", "balls"])
def test_overlays_deferred(name):
    n = 3
    raw, gi, _ = S.gizmo()
    r = renderer(OW, OH, n, overlays=1, render_pass=1, tile_mode=0)
    r.upload_gizmo(raw, gi)
    check_overlays(r, name, n, DR.MODES, (0, 1) if name == "comb" else (0,), deferred=True)
    r.close()


def test_overlays_with_multisampling():
    """option "sample_shading" 0: the samples keep their own depth, the presented frame is k_resolve_merged's"""
    n, mode = 4, DR.SAMPLE_ZERO
    sc = S.scene("comb", n * OW, n * OH, n)
    _, _, fine_depth = S.oracle("comb", n * OW, n * OH, n)
    r = renderer(OW, OH, n, overlays=1, sample_shading=0, depth_resolve=mode)
    r.render_scene(sc)
    r.present()
    base = r.read_presented()
    depth, _ = DR.resolve(fine_depth, None, n, mode)
    assert np.array_equal(bits(r.read_depth()), bits(depth))
    want, _ = bbo.overlay(sc.frame, sc.view, depth, base, None, None, 0)
    r.draw_overlays(0)
    assert (want != base).any(axis=2).sum() == 178 and np.array_equal(r.read_presented(), want)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. frames in flight, replay, the overflow re-render
# ---------------------------------------------------------------------------------------------------------------------
def test_four_frames_in_flight_and_replay():
    n, mode = 2, DR.MAX
    names = ("triangle", "ball", "chart", "balls")                   # the last one's depth is the one the overlays test against
    r = renderer(W, H, n, overlays=1, frames_in_flight=4, depth_resolve=mode)
    raw, gi, gv = S.gizmo()
    r.upload_gizmo(raw, gi)
    for name in names:
        r.render_scene(S.scene(name, n * W, n * H, n))               # (no read in between: four frames are queued)
    fine, fine_prim, fine_depth = S.oracle("balls", n * W, n * H, n)
    want_depth, want_prim = DR.resolve(fine_depth, fine_prim, n, mode)
    sc = S.scene("balls", n * W, n * H, n)

    def check():
        r.present()
        base = r.read_presented()
        assert np.array_equal(base, bbo.present(RR.resolve(fine, n), 0, 1.0))
        assert np.array_equal(bits(r.read_depth()), bits(want_depth))
        r.draw_overlays(12)
        want, _ = bbo.overlay(sc.frame, sc.view, want_depth, base, gv, gi, 12)
        assert (want != base).any() and np.array_equal(r.read_presented(), want)
    check()
    for _ in range(5):                                               # every slot renders the frame once more, its depth resolve included
        r.replay_frame()
    check()
    prim, depth = r.read_visibility()
    assert np.array_equal(prim, want_prim) and np.array_equal(bits(depth), bits(want_depth))
    r.close()


@pytest.mark.parametrize("layout", [0, 1])
def test_other_stream_layouts(layout):
    """k_raster on a stream of its own (1) or with the geometry (0), shading on another: the kept depth is complete when the
    slot's frame is"""
    n = 3
    r = renderer(W, H, n, overlays=1, frames_in_flight=3, stream_layout=layout, depth_resolve=DR.MIN)
    sc = S.scene("balls", n * W, n * H, n)
    r.render_scene(sc)
    for _ in range(4):
        r.replay_frame()
    _, fine_prim, fine_depth = S.oracle("balls", n * W, n * H, n)
    assert np.array_equal(bits(r.read_depth()), bits(DR.resolve(fine_depth, None, n, DR.MIN)[0]))
    r.close()


def test_overflow_re_render():
    n = 3
    r = renderer(W, H, n, overlays=1, bin_cap=8, depth_resolve=DR.SAMPLE_ZERO)   # bins far too small: the frame is rendered again
    sc = S.scene("balls", n * W, n * H, n)
    _, fine_prim, fine_depth = S.oracle("balls", n * W, n * H, n)
    before = r.capacity_growths()
    r.render_scene(sc)
    want_depth, want_prim = DR.resolve(fine_depth, fine_prim, n, DR.SAMPLE_ZERO)
    assert np.array_equal(bits(r.read_depth()), bits(want_depth))
    assert r.capacity_growths() > before
    prim, depth = r.read_visibility()
    assert np.array_equal(prim, want_prim) and np.array_equal(bits(depth), bits(want_depth))
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. state and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_value_zero_refuses_as_before():
    n = 2
    r = renderer(W, H, n, overlays=1, depth_resolve=0)
    r.render_scene(S.scene("ball", n * W, n * H, n))
    r.present()
    for call in (r.draw_overlays, r.read_visibility, r.read_depth):
        err = expect(INVALID, call)
        assert "supersample" in str(err), err
    prim, depth = r.read_sample_visibility()                          # the samples need no rule
    _, want_prim, want_depth = S.oracle("ball", n * W, n * H, n)
    assert np.array_equal(prim, want_prim) and np.array_equal(bits(depth), bits(want_depth))
    r.close()


def test_invalid_values():
    r = renderer(W, H, 2)
    r.set_option("depth_resolve", DR.MIN)
    for bad in (2, 3, -1, 5, 16):
        expect(INVALID, r.set_option, "depth_resolve", bad)
    n = 2
    r.render_scene(S.scene("ball", n * W, n * H, n))                  # the refused calls left MIN in force
    _, fine_prim, fine_depth = S.oracle("ball", n * W, n * H, n)
    prim, depth = r.read_visibility()
    want_depth, want_prim = DR.resolve(fine_depth, fine_prim, n, DR.MIN)
    assert np.array_equal(prim, want_prim) and np.array_equal(bits(depth), bits(want_depth))
    r.close()


def test_switching_drops_the_frame_with_samples_and_nothing_with_one():
    n = 2
    r = renderer(W, H, n, overlays=1, depth_resolve=DR.MIN)
    handles = r.render_scene(S.scene("ball", n * W, n * H, n))
    out = r.read_framebuffer()
    r.set_option("depth_resolve", DR.MIN)                             # the same value: the frame stays current
    assert np.array_equal(bits(r.read_framebuffer()), bits(out))
    r.set_option("depth_resolve", DR.MAX)
    for call in (r.read_framebuffer, r.read_depth, r.read_visibility, r.read_sample_visibility):
        expect(NOT_IN_FRAME, call)
    r.render_scene(S.scene("ball", n * W, n * H, n), handles)
    _, _, fine_depth = S.oracle("ball", n * W, n * H, n)
    assert np.array_equal(bits(r.read_depth()), bits(DR.resolve(fine_depth, None, n, DR.MAX)[0]))
    r.close()
    one = Renderer(W, H)                                              # n = 1: the option is stored and changes nothing
    one.set_option("overlays", 1)
    one.render_scene(S.scene("ball", W, H, 1))
    frame, (prim, depth) = one.read_framebuffer(), one.read_visibility()
    for mode in (DR.MAX, DR.SAMPLE_ZERO, 0, DR.MIN):
        one.set_option("depth_resolve", mode)
        again_prim, again_depth = one.read_visibility()
        assert np.array_equal(bits(one.read_framebuffer()), bits(frame))
        assert np.array_equal(again_prim, prim) and np.array_equal(bits(again_depth), bits(depth))
        assert np.array_equal(bits(one.read_depth()), bits(depth))    # n = 1: the bits of read_visibility's depth
    one.set_option("supersample", 2)                                  # ... and is in force once there are samples
    one.render_scene(S.scene("ball", 2 * W, 2 * H, 2))
    assert np.array_equal(bits(one.read_depth()), bits(DR.resolve(fine_depth, None, 2, DR.MIN)[0]))
    one.close()


def test_a_partition_stays_refused():
    n = 2
    r = renderer(W, 64, n, overlays=1, depth_resolve=DR.MAX)
    r.set_partition(0, 2, 32)
    r.render_scene(S.scene("ball", n * W, n * 64, n))
    r.present()
    for call in (r.draw_overlays, r.read_visibility, r.read_sample_visibility, r.read_depth):
        expect(INVALID, call)
    r.close()


def test_what_stays_refused_with_samples():
    n = 2
    r = renderer(W, H, n, overlays=1, depth_resolve=DR.MAX, render_pass=1)
    r.render_scene(S.scene("ball", n * W, n * H, n))
    for call in (r.read_gbuffer, r.read_surface, r.read_records):
        err = expect(INVALID, call)
        assert "supersample" in str(err), err
    r.close()
