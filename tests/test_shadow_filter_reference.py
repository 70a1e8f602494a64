"""CPU: the model of percentage-closer shadow filtering (tests/shadow_filter_reference.py; option "shadow_filter") on the scenes
of tests/shadow_scenes.py and tests/shadow_faces_scenes.py, and the new symbol of the C ABI.  No GPU.

  1  the model's single-point form equals its array form, one face and six
  2  R = 0 is the hard rule (SR.classify / FR.classify); S = 1 and S = 2 -- a window wider than the map -- agree with the hard
     rule wherever they must: every pixel at S = 1, and at S = 2 wherever all texels of the map compare alike
  3  census on the "clipped" scene at 128 x 128, bias BIAS, S in {33, 64}, R in {1, 2}: every k in 0 .. K occurs and the PARTIAL
     pixels number at least half of 666 / 357 (R = 1) and 1297 / 702 (R = 2).  The other kinds and S = 200 are only printed:
     several k do not occur there
  4  every knob of the taps matters: each mutant changes k on at least 20 covered pixels (half the least count measured, 40)
     in all four combinations; `>=` for `>` at bias 0, where it changes at least 800 (half of 1600)
  5  faces: "taps read face 0's map" and "taps may cross into the next face's memory" on "cube" and "cascade"
  6  every knob of the loop matters on the oracle's surface of the "clipped" scene
  7  the entry point is declared, exported and bound"""
import ctypes as C
import functools

import numpy as np
import pytest

import shadow_faces_reference as FR
import shadow_faces_scenes as FS
import shadow_filter_reference as PR
import shadow_reference as SR
import shadow_scenes as SS
import surface_chart as SC
from test_capi_symbols import declared
from bibim_renderer_amd import _capi
from oracle import bbo

F = np.float32
RADII = (1, 2)
CENSUS_SIDES = (33, 64)
MIN_PARTIAL = {(1, 33): 666, (1, 64): 357, (2, 33): 1297, (2, 64): 702}     # measured; asserted halved
MIN_MUTANT, MIN_GE = 40, 1600                                                 # measured; asserted halved
equal = SC.equal_but_for_nan_payload


@functools.lru_cache(None)
def case(kind, side, size=SS.FRAME_DUMP):
    """(M, P float32 [h, w, 3], covered, map) of one face"""
    P64, covered, _ = SS.positions64(kind, size)
    return SR.proj_view(SS.light_view(kind)), P64.astype(F), covered, SS.oracle_map(kind, side)


@functools.lru_cache(None)
def faces_case(kind, side, size=FS.FRAME_DUMP):
    P64, covered = FS.positions64(kind, size)
    return FS.matrices(kind), P64.astype(F), covered, FS.oracle_maps(kind, side)


@functools.lru_cache(None)
def rule(kind, side, radius, bias=SS.BIAS):
    M, P, covered, depth = case(kind, side)
    return PR.taps([M], side, bias, P, [depth], radius, covered)


# ---------------------------------------------------------------------------------------------------------------------
# 1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", (0,) + RADII)
@pytest.mark.parametrize("side", (1, 2, 33, 64))
@pytest.mark.parametrize("kind", SS.KINDS)
def test_point_form_equals_array_form(kind, side, radius):
    M, P, _, depth = case(kind, side, SS.FRAME_SMALL)
    for bias in (0.0, SS.BIAS):
        cls, k, face = PR.taps([M], side, bias, P, [depth], radius)
        h, w = cls.shape
        for y in range(0, h, 5):
            for x in range(0, w, 5):
                assert PR.taps_point([M], side, bias, P[y, x], [depth], radius) == (cls[y, x], k[y, x], face[y, x]), (y, x, bias)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("kind", FS.KINDS)
def test_point_form_equals_array_form_with_faces(kind, radius):
    Ms, P, _, maps = faces_case(kind, 33, FS.FRAME_SMALL)
    cls, k, face = PR.taps(Ms, 33, FS.BIAS, P, maps, radius)
    h, w = cls.shape
    for y in range(0, h, 4):
        for x in range(0, w, 4):
            assert PR.taps_point(Ms, 33, FS.BIAS, P[y, x], maps, radius) == (cls[y, x], k[y, x], face[y, x]), (y, x)
    assert len(np.unique(face)) >= len(Ms)


def test_hazard_points():
    """NaN and w <= 0 land OUTSIDE and read no tap; a NaN t makes every tap lit"""
    M, _, _, depth = case("spot", 33)
    behind = np.asarray(SS.SPOT_EYE, F) + (np.asarray(SS.SPOT_EYE, F) - np.asarray(SS.SPOT_TARGET, F))
    pts = np.array([[np.nan, 0, 0], [np.inf, 0, 0], behind, SS.SPOT_EYE], F)
    cls, k, face = PR.taps([M], 33, 0.0, pts, [depth], 2)
    assert (cls == PR.OUTSIDE).all() and (k == 255).all() and (face == 255).all()
    on_axis = np.asarray(SS.SPOT_TARGET, F)
    assert [int(v[0]) for v in PR.taps([M], 33, np.nan, on_axis[None], [depth], 2)] == [PR.LIT, 25, 0]
    assert PR.taps_point([M], 33, np.nan, on_axis, [depth], 1) == (PR.LIT, 9, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", SS.BIASES)
@pytest.mark.parametrize("side", SS.SIDES)
@pytest.mark.parametrize("kind", SS.KINDS)
def test_radius_zero_is_the_hard_rule(kind, side, bias):
    M, P, covered, depth = case(kind, side, SS.FRAME_SMALL)
    cls, k, face = PR.taps([M], side, bias, P, [depth], 0, covered)
    want = SR.classify(M, side, bias, P, depth, covered)
    assert np.array_equal(cls, want)
    assert np.array_equal(k, np.where(want == SR.LIT, 1, np.where(want == SR.SHADOWED, 0, 255)))
    assert np.array_equal(face, np.where((want == SR.LIT) | (want == SR.SHADOWED), 0, 255))


@pytest.mark.parametrize("kind", FS.KINDS)
def test_radius_zero_is_the_hard_rule_with_faces(kind):
    Ms, P, covered, maps = faces_case(kind, 33, FS.FRAME_SMALL)
    cls, _, face = PR.taps(Ms, 33, FS.BIAS, P, maps, 0, covered)
    want_cls, want_face = FR.classify(Ms, 33, FS.BIAS, P, maps, covered)
    assert np.array_equal(cls, want_cls) and np.array_equal(face, want_face)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("bias", SS.BIASES)
@pytest.mark.parametrize("kind", SS.KINDS)
def test_a_window_wider_than_the_map(kind, bias, radius):
    """S = 1: every tap is texel (0, 0), k is 0 or K and the class is the hard rule's.  S = 2: the window holds all four texels
    (some of them several times), so k is 0 or K exactly where the four compare alike, and there the class is the hard rule's"""
    K = PR.taps_of(radius)
    for side in (1, 2):
        M, P, covered, depth = case(kind, side, SS.FRAME_SMALL)
        cls, k, _ = PR.taps([M], side, bias, P, [depth], radius, covered)
        want = SR.classify(M, side, bias, P, depth, covered)
        inside, _, _, t = PR.texel(M, side, bias, P)
        with np.errstate(all="ignore"):
            lit = ~(depth.reshape(-1)[:, None, None] > t[None])            # [S * S, h, w]
        alike = lit.all(0) | ~lit.any(0)
        if side == 1:
            assert alike.all()
        assert np.array_equal(cls[alike], want[alike])
        assert np.isin(k[alike & inside], (0, K)).all() and not np.isin(k[~alike & inside], (0, K)).any()
        assert ((cls == PR.PARTIAL) == (~alike & inside & covered)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3
# ---------------------------------------------------------------------------------------------------------------------
def counts(cls, k, radius):
    return np.bincount(k[(cls != PR.NONE) & (cls != PR.OUTSIDE)].ravel(), minlength=PR.taps_of(radius) + 1)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("side", CENSUS_SIDES)
def test_census_on_the_clipped_scene(side, radius):
    cls, k, _ = rule("clipped", side, radius)
    n, partial = counts(cls, k, radius), int((cls == PR.PARTIAL).sum())
    print(f"clipped S = {side} R = {radius}: pixels by k {n.tolist()}, PARTIAL {partial}")
    assert len(n) == PR.taps_of(radius) + 1 and (n > 0).all(), n
    assert partial >= MIN_PARTIAL[radius, side] // 2
    assert partial == int(n[1:-1].sum())
    assert ((cls == PR.LIT) == (k == PR.taps_of(radius))).all() and ((cls == PR.SHADOWED) == (k == 0)).all()


@pytest.mark.parametrize("radius", RADII)
def test_census_elsewhere_is_only_printed(radius):
    for kind in SS.KINDS:
        for side in (33, 64, 200):
            if kind == "clipped" and side in CENSUS_SIDES:
                continue
            cls, k, _ = rule(kind, side, radius)
            print(f"{kind} S = {side} R = {radius}: pixels by k {counts(cls, k, radius).tolist()}, PARTIAL {int((cls == PR.PARTIAL).sum())}")


# ---------------------------------------------------------------------------------------------------------------------
# 4
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("side", CENSUS_SIDES)
@pytest.mark.parametrize("mutant", list(PR.TAP_MUTANTS))
def test_tap_mutants_change_k(mutant, side, radius):
    M, P, covered, depth = case("clipped", side)
    _, k, _ = rule("clipped", side, radius)
    _, got, _ = PR.taps([M], side, SS.BIAS, P, [depth], radius, covered, **PR.TAP_MUTANTS[mutant])
    n = int(((got != k) & covered).sum())
    print(f"{mutant} | clipped S = {side} R = {radius}: k changes on {n} pixels")
    assert n >= MIN_MUTANT // 2


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("side", CENSUS_SIDES)
def test_greater_equal_changes_k_at_bias_zero(side, radius):
    M, P, covered, depth = case("clipped", side)
    ge = dict(lit=lambda a, t: ~(a >= t))
    at_bias = PR.taps([M], side, SS.BIAS, P, [depth], radius, covered, **ge)[1]
    assert np.array_equal(at_bias, rule("clipped", side, radius)[1]), "at the working bias no texel equals t"
    got = PR.taps([M], side, 0.0, P, [depth], radius, covered, **ge)[1]
    n = int(((got != rule("clipped", side, radius, 0.0)[1]) & covered).sum())
    print(f">= for > | clipped S = {side} R = {radius}, bias 0: k changes on {n} pixels")
    assert n >= MIN_GE // 2


# ---------------------------------------------------------------------------------------------------------------------
# 5
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("side", CENSUS_SIDES)
@pytest.mark.parametrize("kind", FS.KINDS)
@pytest.mark.parametrize("mutant", list(PR.FACE_MUTANTS))
def test_face_mutants_change_k(mutant, kind, side, radius):
    """Pixels of the 128 x 128 frame whose k changes, bias BIAS (S = 33 R = 1, 33 R = 2, 64 R = 1, 64 R = 2):
         taps read face 0's map                       cube 7212, 8193, 6518, 7365    cascade 4420, 5030, 4162, 4506
         taps may cross into the next face's memory   cube  161,  407,   71,  169    cascade   62,  121,   36,   88
    Both change at least one pixel on both scenes, so both are kept."""
    Ms, P, covered, maps = faces_case(kind, side)
    _, k, face = PR.taps(Ms, side, FS.BIAS, P, maps, radius, covered)
    _, got, got_face = PR.taps(Ms, side, FS.BIAS, P, maps, radius, covered, **PR.FACE_MUTANTS[mutant])
    n = int(((got != k) & covered).sum())
    print(f"{mutant} | {kind} S = {side} R = {radius}: k changes on {n} pixels")
    assert np.array_equal(face, got_face), "the deciding face does not depend on the taps"
    assert n >= 1


# ---------------------------------------------------------------------------------------------------------------------
# 6
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def clipped_surface():
    """light-loop inputs on the "clipped" scene's positions: the receiver's normal, a mid-grey dielectric"""
    _, P, _, _ = case("clipped", 33)
    surf = np.zeros((P.shape[0] * P.shape[1], 12), F)
    surf[:, 0:3] = P.reshape(-1, 3)
    surf[:, 3:6] = (SC.TILT[0], SC.TILT[1], -1.0)
    surf[:, 6:9], surf[:, 10], surf[:, 11] = 0.5, 0.5, 1.0
    return surf


@pytest.mark.parametrize("radius", RADII)
def test_lit_frame_groups(radius):
    """k = K is the plain loop, k = 0 the hard rule's shadowed pixel, and a PARTIAL pixel lies between the two"""
    sc = SS.scene("clipped", SS.FRAME_DUMP)
    cls, k, _ = rule("clipped", 33, radius)
    surf, kk = clipped_surface(), k.ravel()
    got = PR.lit_frame(sc.frame, sc.view, surf, kk, SS.CASTER, radius)
    plain = bbo.light_surface(sc.frame, sc.view, surf, literal=False)
    dark = SR.lit_frame(sc.frame, sc.view, surf, np.full(len(surf), SR.SHADOWED, np.uint8), SS.CASTER)
    full, none, part = kk == PR.taps_of(radius), kk == 0, cls.ravel() == PR.PARTIAL
    assert full.any() and none.any() and part.any()
    assert equal(got[full], plain[full]) and equal(got[none], dark[none])
    assert equal(got[kk == 255], plain[kk == 255])
    g, lo, hi = got[part][:, :3], dark[part][:, :3], plain[part][:, :3]
    assert (g >= lo).all() and (g <= hi).all() and (g < hi).any() and (g > lo).any()
    # a caster past the frame's lights scales nothing
    assert equal(PR.lit_frame(sc.frame, sc.view, surf, kk, 4, radius), plain)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("mutant", list(PR.LOOP_MUTANTS))
def test_loop_mutants_change_the_frame(mutant, radius):
    """Pixels of the "clipped" scene (S = 33) whose bits change (R = 1, R = 2):
         (color * intensity) * v                  427, 460
         v the correctly rounded quotient k / K   0, 478: EQUIVALENT at R = 1, where (float)k * RK[9] is the correctly rounded k / 9
                                                  for every k in 1 .. 8 (at K = 25 the two differ for k = 5, 9, 10, 15, 18, 20, 23)
         k = K scaled instead of untouched        0, 0: EQUIVALENT at both radii, K * RK[K] rounds to 1 for K = 9 and K = 25 and
                                                  intensity * 1 is intensity
    A mutant is equivalent exactly where it gives every count the rule's v, which is checked here on the numbers alone."""
    K, knobs = PR.taps_of(radius), PR.LOOP_MUTANTS[mutant]
    rule_v = lambda c: PR._product(c, K) if c < K else F(1.0)
    same_v = not knobs.get("colour_after") and all(
        knobs.get("v_of", PR._product)(c, K) == rule_v(c) for c in range(1, K + 1 if knobs.get("scale_full") else K))
    sc = SS.scene("clipped", SS.FRAME_DUMP)
    _, k, _ = rule("clipped", 33, radius)
    surf = clipped_surface()
    want = PR.lit_frame(sc.frame, sc.view, surf, k.ravel(), SS.CASTER, radius)
    got = PR.lit_frame(sc.frame, sc.view, surf, k.ravel(), SS.CASTER, radius, **PR.LOOP_MUTANTS[mutant])
    n = int((SC.bits(got) != SC.bits(want)).any(-1).sum())
    print(f"{mutant} | R = {radius}: {n} pixels change")
    if same_v:
        print(f"{mutant} | R = {radius}: EQUIVALENT on these counts")
        assert n == 0
    else:
        assert n >= 1


# ---------------------------------------------------------------------------------------------------------------------
# 7
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbol_is_declared_exported_and_bound():
    assert "bbr_read_shadow_taps" in declared("bibim_hip.h"), "not declared in include/bibim_hip.h"
    assert hasattr(C.CDLL(_capi.LIB_PATH), "bbr_read_shadow_taps"), "declared but not exported"
    assert "bbr_read_shadow_taps" in _capi.SIGNATURES, "not in the binding table"
    from bibim_renderer_amd import Renderer
    assert callable(getattr(Renderer, "read_shadow_taps", None))
