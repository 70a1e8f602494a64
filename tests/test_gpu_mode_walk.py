"""GPU: a context's history does not matter.  ONE context (37 x 23, the triangle scene, two frames in flight) is walked through
the modes a frame can have -- plain, fused presentation, per-sample and merged supersampling, overlays, timing -- and after every
step everything that can be read back is compared bit for bit with the oracle and the numpy models (resolve_reference,
sample_merge_reference, the oracle's presentation and overlay pass), never with a second context.

Every step renders two frames and reads after each, so both frame slots have held every mode: what a slot allocates for a
mode, and what it remembers of the frame it holds, must not depend on the modes it held before."""
import functools
import os

import numpy as np
import pytest

import resolve_reference as RR
import sample_merge_reference as M
from conftest import GOLDEN
from bibim_renderer_amd import BibimError, Renderer
from oracle import bbo, scenes

pytestmark = pytest.mark.gpu

F = np.float32
INVALID = -1
W, H = 37, 23                       # the supersample tests' output: partial edge tiles, not a multiple of 4
GIZMO_EXTENT = 32                   # (the oracle's gizmo covers 76 pixels of the corner at this extent)


def same(a, b):
    """bit for bit; NaN by placement"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


@functools.lru_cache(None)
def scene(n):
    return scenes.triangle_scene(n * W, n * H)


@functools.lru_cache(None)
def oracle(n):
    """(fine frame, winners, depth) of the triangle at n W x n H, read-only"""
    fine, prim, depth, _ = bbo.render(scene(n))
    for a in (fine, prim, depth):
        a.setflags(write=False)
    return fine, prim, depth


@functools.lru_cache(None)
def model(n, merged):
    """the W x H frame, the sample map and read_samples() of a frame with n x n samples"""
    fine, prim, _ = oracle(n)
    rep = M.rep_map(prim if merged else np.full(prim.shape, M.NO_PRIM, np.uint32), n)
    samples = M.replicate(fine, rep, n)
    return RR.resolve(samples, n), rep, samples


def presented(n, merged):
    fu = scene(n).frame
    return bbo.present(model(n, merged)[0], int(fu["enable_tone_mapping"]), float(fu["exposure"]))


def refused(call, word=None):
    with pytest.raises(BibimError) as e:
        call()
    assert e.value.code == INVALID, e.value
    if word:
        assert word in str(e.value), e.value


def test_mode_walk():
    g = np.load(os.path.join(GOLDEN, "gizmo.npz"))
    gv = np.zeros(len(g["vertices"]), bbo.GIZMO_VERTEX_DTYPE)
    gv["pos"], gv["color"], gv["normal"] = g["vertices"][:, 0:3], g["vertices"][:, 3:6], g["vertices"][:, 6:9]

    r = Renderer(W, H)
    r.set_option("frames_in_flight", 2)
    r.upload_gizmo(g["vertices"], g["indices"])
    handles = {"mesh": {}, "mat": {}}

    def step(name, n, merged, fused, frames=2, overlay=None):
        """`frames` frames of the mode the context is in now, everything readable checked after each"""
        frame, rep, samples = model(n, merged)
        for i in range(frames):
            where = f"{name}, frame {i}"
            r.render_scene(scene(n), handles)
            assert np.array_equal(r.read_sample_map(), rep), where
            if fused:
                refused(r.read_framebuffer, "present_fused")           # no W x H fp32 frame
                if n == 1:
                    refused(r.read_samples, "present_fused")           # one sample per pixel: the frame itself
            else:
                assert same(r.read_framebuffer(), frame), where
            if n > 1 or not fused:
                assert same(r.read_samples(), samples), where
            r.present()
            base = presented(n, merged)
            assert np.array_equal(r.read_presented(), base), where
            if overlay == "refused":
                refused(r.draw_overlays, "supersample")
                assert np.array_equal(r.read_presented(), base), where
            elif overlay == "drawn":
                sc = scene(1)
                want, _ = bbo.overlay(sc.frame, sc.view, oracle(1)[2], base, gv, g["indices"], GIZMO_EXTENT)
                assert (want != base).any(axis=2).sum() > 50
                r.draw_overlays(GIZMO_EXTENT)
                assert np.array_equal(r.read_presented(), want), where
                assert same(r.read_framebuffer(), frame), where         # the overlays go into the presented image only

    step("1 defaults", 1, False, False)
    r.set_option("present_fused", 1)
    step("2 present_fused 1", 1, False, True)
    r.set_option("supersample", 2)
    step("3 supersample 2, fused", 2, False, True)
    r.set_option("sample_shading", 0)
    step("4 sample_shading 0, fused", 2, True, True)
    assert not np.array_equal(model(2, True)[1], model(2, False)[1])    # (the merged map is not the identity here)
    r.set_option("present_fused", 0)
    step("5 present_fused 0", 2, True, False)
    r.set_option("overlays", 1)
    step("6 overlays 1", 2, True, False, overlay="refused")
    r.set_option("supersample", 1)                                     # ("sample_shading" 0 is stored, without effect at n = 1)
    step("7 supersample 1, overlays drawn", 1, False, False, overlay="drawn")
    r.set_option("supersample", 4)
    step("8 supersample 4, merged", 4, True, False, overlay="refused")
    r.set_option("timing", 1)
    step("9 timing 1", 4, True, False, frames=3, overlay="refused")
    launches, ms = r.resolve_timing()
    frame_ms, shade_ms = r.last_frame_time_ms()
    assert launches == 3 and ms > 0 and frame_ms > shade_ms > 0        # a frame's interval ends behind its resolve
    r.set_option("sample_shading", 1)
    r.set_option("supersample", 1)
    step("10 supersample 1, sample_shading 1", 1, False, False, overlay="drawn")
    frame_ms, shade_ms = r.last_frame_time_ms()
    assert r.resolve_timing()[0] == 0 and frame_ms > shade_ms > 0      # ... and behind its shading without one
    assert r.timing_summary()[0] == 2
    r.close()
