"""CPU: the shadow rule's model (tests/shadow_reference.py) and its scenes (tests/shadow_scenes.py), held against the oracle;
and the new symbols of the C ABI.  No GPU.

  1  the model's single-point form equals its array form; its M equals the oracle's P * V
  2  census on the oracle's maps: every kind x S >= 33 has enough LIT, SHADOWED and OUTSIDE pixels a factor 2 clear of their
     thresholds, the spot kinds enough pixels behind the light, and at bias 0 enough pixels whose map texel is their own
     depth; the shares are those recorded in tests/golden/shadow_map.json (tools/shadow_map_record.py)
  3  every knob of the rule matters: each mutant of the model changes the mask (the caster's index: the frame) on every kind
     x S >= 33
  4  the entry points are declared in include/bibim_hip.h, exported by the library and bound by the package"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import shadow_reference as SR
import shadow_scenes as SS
import surface_chart as SC
from conftest import GOLDEN
from test_capi_symbols import declared
from bibim_renderer_amd import _capi
from oracle import bbo

F = np.float32
SIDES = [s for s in SS.SIDES if s >= 33]
NEW_SYMBOLS = ("bbr_render_shadow_map", "bbr_read_shadow_map", "bbr_read_shadow_mask")


@functools.lru_cache(None)
def case(kind, side, bias=SS.BIAS):
    """(M, P float32 [h, w, 3], covered, map, mask) of the small frame"""
    P64, covered, _ = SS.positions64(kind)
    M = SR.proj_view(SS.light_view(kind))
    P = P64.astype(F)
    depth = SS.oracle_map(kind, side)
    return M, P, covered, depth, SR.classify(M, side, bias, P, depth, covered)


# ---------------------------------------------------------------------------------------------------------------------
# 1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SS.KINDS)
def test_proj_view_is_the_oracles(kind):
    L = SS.light_view(kind)
    want = np.zeros((4, 4), F)
    bbo.lib().bbo_proj_view(bbo._p(L), bbo._p(want))
    assert np.array_equal(SC.bits(SR.proj_view(L)), SC.bits(want))


@pytest.mark.parametrize("bias", SS.BIASES)
@pytest.mark.parametrize("side", SS.SIDES)
@pytest.mark.parametrize("kind", SS.KINDS)
def test_point_form_equals_array_form(kind, side, bias):
    M, P, covered, depth, _ = case(kind, side)
    mask = SR.classify(M, side, bias, P, depth)
    h, w = mask.shape
    ys, xs = np.meshgrid(np.arange(0, h, 3), np.arange(0, w, 3), indexing="ij")      # every third pixel each way
    for y, x in zip(ys.ravel(), xs.ravel()):
        assert SR.classify_point(M, side, bias, P[y, x], depth) == mask[y, x], (y, x)
    if bias == -1.0:
        assert not (mask == SR.LIT).any()
    if bias == 2.0:
        assert not (mask == SR.SHADOWED).any()


def test_hazard_points():
    """NaN and w <= 0 land OUTSIDE; a NaN t is not shadowed"""
    M, _, _, depth, _ = case("spot", 33)
    behind = np.asarray(SS.SPOT_EYE, F) + (np.asarray(SS.SPOT_EYE, F) - np.asarray(SS.SPOT_TARGET, F))
    pts = np.array([[np.nan, 0, 0], [np.inf, 0, 0], behind, SS.SPOT_EYE], F)
    assert (SR.classify(M, 33, 0.0, pts, depth) == SR.OUTSIDE).all()
    on_axis = np.asarray(SS.SPOT_TARGET, F)
    assert SR.classify(M, 33, np.nan, on_axis[None], depth)[0] == SR.LIT
    assert SR.classify_point(M, 33, np.nan, on_axis, depth) == SR.LIT


# ---------------------------------------------------------------------------------------------------------------------
# 2
# ---------------------------------------------------------------------------------------------------------------------
def census_pair(kind, side):
    M, P, covered, depth, mask = case(kind, side)
    P64 = SS.positions64(kind)[0]
    zero = SR.classify(M, side, 0.0, P, depth, covered)
    return SS.census(kind, side, SS.BIAS, P64, covered, depth, mask), SS.census(kind, side, 0.0, P64, covered, depth, zero)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", SS.KINDS)
def test_census_on_the_oracle(kind, side):
    c_bias, c_zero = census_pair(kind, side)
    print(f"{kind} S = {side}: {c_bias}; bias 0: {c_zero}")
    SS.check_census(kind, side, c_bias, c_zero)
    rec = json.load(open(os.path.join(GOLDEN, "shadow_map.json")))["census"][f"{kind} {side}"]
    assert rec == {"bias": {k: round(v, 4) for k, v in c_bias.items()}, "zero": {k: round(v, 4) for k, v in c_zero.items()}}


@pytest.mark.parametrize("kind", SS.KINDS)
def test_scene_shape(kind):
    """what the scenes promise: the frame is covered, the caster is light 2 of 4, the map of the clipped kind differs from the
    spot's (the triangle through the near plane is in it), the sliver is a few texels of the largest map"""
    sc = SS.scene(kind)
    assert int(sc.frame["num_lights"]) == 4 and SS.CASTER == 2
    assert int(sc.frame["lights"][SS.CASTER]["type"]) == (2 if kind == "ortho" else 1)
    assert SS.positions64(kind)[1].all()
    if kind == "clipped":
        for side in SIDES:
            assert not np.array_equal(SS.oracle_map("clipped", side), SS.oracle_map("spot", side))
        st = bbo.render(SS.map_scene("clipped", 64), want_prim=False, want_depth=False)[3]
        assert st["n_clipped_prims"] >= 1, st
    assert (SS.oracle_map(kind, 1) != 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3
# ---------------------------------------------------------------------------------------------------------------------
MASK_MUTANTS = {
    ">= for >": dict(shadowed=np.greater_equal),
    "rint for the truncation": dict(to_int=np.rint),
    "h off by half a texel": dict(h_offset=0.5),
    "the bias subtracted": dict(bias_sign=-1.0),
}


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", SS.KINDS)
@pytest.mark.parametrize("mutant", list(MASK_MUTANTS) + ["M transposed", "the deferred P unrounded"])
def test_model_mutants_change_the_mask(mutant, kind, side):
    M, P, covered, depth, mask = case(kind, side)
    if mutant == "M transposed":
        got = SR.classify(np.ascontiguousarray(M.T), side, SS.BIAS, P, depth, covered)
    elif mutant == "the deferred P unrounded":
        # the deferred pass tests the P of its G-buffer: the rule's mask is the one on the rounded P (at bias 0, where the
        # map holds the fragment's own depth and 2^-11 of P decides; at 2^-8 only pixels on a texel's edge would notice)
        mask = SR.classify(M, side, 0.0, bbo.half_round(P), depth, covered)
        got = SR.classify(M, side, 0.0, P, depth, covered)
    elif mutant == ">= for >":
        # (only where the two sides can be equal: the map holds the fragment's own depth at bias 0)
        mask = SR.classify(M, side, 0.0, P, depth, covered)
        got = SR.classify(M, side, 0.0, P, depth, covered, **MASK_MUTANTS[mutant])
    else:
        got = SR.classify(M, side, SS.BIAS, P, depth, covered, **MASK_MUTANTS[mutant])
    n = int((got != mask).sum())
    print(f"{mutant} | {kind} S = {side}: {n} pixels change class")
    assert n > 0


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", SS.KINDS)
def test_caster_index_off_by_one_changes_the_frame(kind, side):
    """the mask does not know the index: the frame does"""
    M, P, covered, depth, mask = case(kind, side)
    sc = SS.scene(kind)
    dark = np.flatnonzero(mask.ravel() == SR.SHADOWED)[::7]
    surf = np.zeros((len(dark), 12), F)
    surf[:, 0:3] = P.reshape(-1, 3)[dark]
    surf[:, 3:6] = (SC.TILT[0], SC.TILT[1], -1.0)
    surf[:, 6:9], surf[:, 10], surf[:, 11] = 0.5, 0.5, 1.0
    m = np.full(len(dark), SR.SHADOWED, np.uint8)
    want = SR.lit_frame(sc.frame, sc.view, surf, m, SS.CASTER)
    plain = bbo.light_surface(sc.frame, sc.view, surf, literal=False)
    assert not SC.equal_but_for_nan_payload(want, plain), "the caster gives these pixels nothing"
    for other in (SS.CASTER - 1, SS.CASTER + 1):
        assert not SC.equal_but_for_nan_payload(SR.lit_frame(sc.frame, sc.view, surf, m, other), want), other
    # an index past the frame's lights shadows nothing
    assert SC.equal_but_for_nan_payload(SR.lit_frame(sc.frame, sc.view, surf, m, 4), plain)
    # ... and the unknown type is the whole of it: the same scene with that type in the block from the start
    off = SS.scene(kind, caster_type=SR.UNKNOWN_TYPE)
    assert SC.equal_but_for_nan_payload(bbo.light_surface(off.frame, off.view, surf, literal=False), want)


# ---------------------------------------------------------------------------------------------------------------------
# 4
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    names = declared("bibim_hip.h")
    L = C.CDLL(_capi.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in names, f"{n} is not declared in include/bibim_hip.h"
        assert hasattr(L, n), f"{n} declared but not exported"
        assert n in _capi.SIGNATURES, f"{n} is not in the binding table"
    from bibim_renderer_amd import Renderer
    for m in ("render_shadow_map", "read_shadow_map", "read_shadow_mask"):
        assert callable(getattr(Renderer, m, None)), m
    scene_h = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "bibim_scene.h")).read()
    assert "renderShadowMap(bbr_context *ctx, int32_t light, const ViewUniformBlock &lightView, float bias)" in scene_h
