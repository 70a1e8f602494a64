"""GPU: the overlay subpass (`bbr_draw_overlays`: the host's matrix folds, k_geometry / k_raster <.., OVERLAY>,
k_shade_overlay; csrc/bibim_hip.hip, csrc/bb_kernels.hip.h) on hazard lights and gizmos -- the overlay chart.

tests/overlay_chart.py builds 160 x 128 cases whose lights and gizmo meshes are chosen class by class (its CLASSES) and a
model of the pass that does not go through the oracle's C; tests/test_overlay_chart.py holds the oracle to that model.
  1  bytes: per case and tile size the presented image is the oracle's base, and after draw_overlays bbo.overlay's, byte for
     byte; two cases again under the deferred pass and two with the fused present.  NumLights outside [0, 100) never reaches the
     pass: bbr_set_frame_uniforms refuses it (the reference asserts it, src/main.cpp:1289-1290) and the context keeps the block
     it had, so the next frame and its overlay are the previous lights' -- 99 lights are the most the pass can be given
  2  model: the GPU's image against the model directly, on every decided pixel (holds whatever the oracle does)
  3  growth: bins (99 lights at one position; bin_cap 8), clip arena (clip_cap 1) and every-tile list (broad_cap 1) outgrown
     inside the pass: capacity_growths() rises and the bytes are the same
  4  call sites: twice in a row, three frames in flight, after a resize, an extent change on one presented frame
Each case is one frame of 20 480 pixels and at most 24 markers (the growth case: 99)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import overlay_chart as OC
from bibim_renderer_amd import BibimError, Renderer
from oracle import bbo

pytestmark = pytest.mark.gpu

W, H = OC.W, OC.H
REFUSED = ("count -4", "count 100", "count 250")        # bbr_set_frame_uniforms takes NumLights in [0, 100) only (test_1_counts_...)
CASES = [(n, m) for n in OC.cases() if n not in REFUSED for m in (0, 1)]
case_id = lambda c: f"{c[0]}, tile_mode {c[1]}"


def renderer(name, width=W, height=H, **options):
    r = Renderer(width, height)
    for k, v in options.items():
        r.set_option(k, v)
    r.set_option("overlays", 1)
    raw, gi, _ = OC.gizmo_upload(name)
    if raw is not None:
        r.upload_gizmo(raw, gi)
    return r


def differing(got, want):
    bad = (got != want).any(axis=2)
    return f"{int(bad.sum())} pixels differ, first (y, x) = {tuple(np.argwhere(bad)[0])}" if bad.any() else ""


@functools.lru_cache(None)
def gpu(name, tile_mode, deferred=0, fused=0, caps=()):
    """one case rendered, presented and overlaid once, shared (read-only) by the checks; `caps`: options set once the frame is
    on the screen, so a growth can only be the overlay pass's"""
    r = renderer(name, tile_mode=tile_mode, render_pass=deferred, present_fused=fused)
    r.render_scene(OC.scene(name))
    r.present()
    g = SimpleNamespace(base=r.read_presented())
    for k, v in caps:
        r.set_option(k, v)
    before = r.capacity_growths()
    r.draw_overlays(OC.cases()[name].extent)
    g.got = r.read_presented()
    g.growths = r.capacity_growths() - before
    r.close()
    return g


def check_bytes(name, g, deferred=False):
    o = OC.oracle_frame(name, deferred)
    assert np.array_equal(g.base, o.base), "base: " + differing(g.base, o.base)
    assert np.array_equal(g.got, o.want), "overlaid: " + differing(g.got, o.want)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_1_bytes(case):
    name, tile_mode = case
    check_bytes(name, gpu(name, tile_mode))


def test_1_counts_outside_the_range_are_refused_and_change_nothing():
    name = "count 0"
    r = renderer(name)
    sc = OC.scene("depth")
    handles = r.render_scene(sc)
    for refused in REFUSED:
        with pytest.raises(BibimError) as e:
            r.set_frame_uniforms(OC.frame_uniforms(OC.cases()[refused]))
        assert e.value.code == -1
        r.begin_frame()                                     # a frame under the uniforms the context still holds: "depth"'s
        for d in sc.draws:
            r.draw(handles["mesh"][id(d.vertices)], handles["mat"][id(d.material)], d.instances)
        r.end_frame()
        r.present()
        r.draw_overlays(0)
        got, o = r.read_presented(), OC.oracle_frame("depth")
        assert np.array_equal(got, o.want), refused + ": " + differing(got, o.want)
    r.close()


@pytest.mark.parametrize("name", ["depth", "gizmo hand"])
def test_1_bytes_deferred(name):
    check_bytes(name, gpu(name, 0, deferred=1), deferred=True)


@pytest.mark.parametrize("name", ["ties", "gizmo 100"])
def test_1_bytes_fused_present(name):
    check_bytes(name, gpu(name, 1, fused=1))


@pytest.mark.parametrize("case", [c for c in CASES if OC.cases()[c[0]].model], ids=case_id)
def test_2_model(case):
    name, tile_mode = case
    g = gpu(name, tile_mode)
    ratio = OC.check_image(name, g.got, g.base, "GPU, ")
    print(f"\n{case_id(case)}: colour error / tolerance {ratio:.4f}")
    assert ratio <= 1.0


GROWTH = {"99 lights": ("many", ()), "bin_cap": ("ties", (("bin_cap", 8),)), "clip_cap": ("near", (("clip_cap", 1),)),
          "broad_cap": ("near", (("broad_cap", 1), ("broad_threshold", 1)))}


@pytest.mark.parametrize("tile_mode", [0, 1])
@pytest.mark.parametrize("which", list(GROWTH))
def test_3_growth_inside_the_pass(which, tile_mode):
    name, caps = GROWTH[which]
    g = gpu(name, tile_mode, caps=caps)
    assert g.growths > 0, "the pass was to outgrow its buffers"
    check_bytes(name, g)


def test_4_twice_in_a_row():
    name = "gizmo hand"
    r = renderer(name)
    r.render_scene(OC.scene(name))
    r.present()
    for _ in range(2):
        r.draw_overlays(OC.cases()[name].extent)
        got = r.read_presented()
        assert np.array_equal(got, OC.oracle_frame(name).want), differing(got, OC.oracle_frame(name).want)
    r.close()


def test_4_three_frames_in_flight():
    """nothing synchronises between the frames; the overlay lands on the last one, with its lights, its view and its depth"""
    names = ["depth", "ties", "gizmo yawed"]
    r = renderer(names[-1], frames_in_flight=3)
    handles = None
    for name in names:
        handles = r.render_scene(OC.scene(name), handles)
        r.present()
    r.draw_overlays(OC.cases()[names[-1]].extent)
    got, o = r.read_presented(), OC.oracle_frame(names[-1])
    assert np.array_equal(got, o.want), differing(got, o.want)
    assert not np.array_equal(o.depth, OC.oracle_frame(names[0]).depth)
    r.close()


def test_4_after_a_resize():
    """96 x 64: the 100-pixel gizmo square is wider and taller than the frame"""
    name = "gizmo 100"
    r = renderer(name)
    r.render_scene(OC.scene(name))
    r.present()
    r.draw_overlays(100)
    r.resize(96, 64)
    r.render_scene(OC.scene(name, 96, 64))
    r.present()
    o = OC.oracle_frame(name, False, 96, 64)
    base = r.read_presented()
    assert np.array_equal(base, o.base), differing(base, o.base)
    r.draw_overlays(100)
    got = r.read_presented()
    assert (o.want != o.base).any() and np.array_equal(got, o.want), differing(got, o.want)
    r.close()


def test_4_extent_change_on_one_presented_frame():
    """the second call draws over the first one's image, against the scene's depth again"""
    name = "gizmo 100"
    o = OC.oracle_frame(name)
    _, gi, gv = OC.gizmo_upload(name)
    second, _ = bbo.overlay(o.scene.frame, o.scene.view, o.depth, o.want, gv, gi, 33)
    assert (second != o.want).any()
    r = renderer(name)
    r.render_scene(OC.scene(name))
    r.present()
    r.draw_overlays(100)
    r.draw_overlays(33)
    got = r.read_presented()
    assert np.array_equal(got, second), differing(got, second)
    r.close()
