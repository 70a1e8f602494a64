"""CPU: the model of shadow maps of up to six faces (tests/shadow_faces_reference.py) and its scenes
(tests/shadow_faces_scenes.py), held against the oracle; the host shim's cube views; the new symbols.  No GPU.

  1  with F = 1 the model is shadow_reference.classify; its single-point form equals its array form
  2  census of the cube scene on the oracle's maps at 96 degrees (bias 2^-8, binary32 model on binary64-derived positions):
     every face decides enough LIT and enough SHADOWED covered pixels, no covered pixel is OUTSIDE everywhere, and more
     than one face is not OUTSIDE for enough pixels.  At exactly 90 degrees covered pixels of the 128 x 128 frame ARE
     OUTSIDE everywhere: the documented seam
  3  the cascade: the inner face decides inside its extent, the outer one only beyond it
  4  every knob of the rule matters: each mutant of the model changes the mask or the face index on every S >= 33
  5  bbs_cube_shadow_views is six oracle lookAt / perspective blocks bit for bit; the entry points are declared, exported
     and bound"""
import ctypes as C
import functools

import numpy as np
import pytest

import shadow_faces_reference as FR
import shadow_faces_scenes as FS
import shadow_reference as SR
import shadow_scenes as SS
import surface_chart as SC
from test_capi_symbols import declared
from bibim_renderer_amd import _capi
from oracle import bbo

F = np.float32
NEW_SYMBOLS = ("bbr_render_shadow_faces", "bbr_read_shadow_face", "bbr_read_shadow_face_index")
size_id = lambda s: "%dx%d" % s


@functools.lru_cache(None)
def case(kind, side, size=FS.FRAME_SMALL, fov=FS.FOV, bias=FS.BIAS):
    """(Ms, P float32 [h, w, 3], covered, maps, class, face)"""
    P64, covered = FS.positions64(kind, size)
    Ms, maps, P = FS.matrices(kind, fov), FS.oracle_maps(kind, side, fov), P64.astype(F)
    cls, face = FR.classify(Ms, side, bias, P, maps, covered)
    return Ms, P, covered, maps, cls, face


# ---------------------------------------------------------------------------------------------------------------------
# 1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", FS.BIASES)
@pytest.mark.parametrize("kind", FS.KINDS)
def test_one_face_is_the_single_map_rule(kind, bias):
    Ms, P, covered, maps, _, _ = case(kind, 64)
    for f in range(len(Ms)):
        cls, face = FR.classify(Ms[f:f + 1], 64, bias, P, maps[f:f + 1], covered)
        want = SR.classify(Ms[f], 64, bias, P, maps[f], covered)
        assert np.array_equal(cls, want)
        assert np.array_equal(face, np.where((want == SR.LIT) | (want == SR.SHADOWED), 0, 255))


@pytest.mark.parametrize("bias", FS.BIASES)
@pytest.mark.parametrize("side", (1,) + FS.SIDES)
@pytest.mark.parametrize("kind", FS.KINDS)
def test_point_form_equals_array_form(kind, side, bias):
    Ms, P, _, maps, _, _ = case(kind, side)
    cls, face = FR.classify(Ms, side, bias, P, maps)
    h, w = cls.shape
    ys, xs = np.meshgrid(np.arange(0, h, 3), np.arange(0, w, 3), indexing="ij")      # every third pixel each way
    for y, x in zip(ys.ravel(), xs.ravel()):
        assert FR.classify_point(Ms, side, bias, P[y, x], maps) == (cls[y, x], face[y, x]), (y, x)


def test_hazard_points():
    """NaN and a point every face has behind it are OUTSIDE with face 255"""
    Ms, _, _, maps, _, _ = case("cube", 33)
    P = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], FS.E], F)       # (E itself: w = 0 in every face)
    cls, face = FR.classify(Ms, 33, FS.BIAS, P, maps)
    assert (cls == SR.OUTSIDE).all() and (face == 255).all()
    for p in P:
        assert FR.classify_point(Ms, 33, FS.BIAS, p, maps) == (SR.OUTSIDE, 255)


# ---------------------------------------------------------------------------------------------------------------------
# 2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [FS.FRAME_SMALL, FS.FRAME_DUMP], ids=size_id)
@pytest.mark.parametrize("side", FS.SIDES)
def test_census_of_the_cube_scene(side, size):
    Ms, P, covered, maps, cls, face = case("cube", side, size)
    c = FS.census(cls, face, covered, 6)
    each = FR.per_face(Ms, side, FS.BIAS, P, maps)
    overlap = int((((each != SR.OUTSIDE).sum(0) > 1) & covered).sum())
    print(f"cube {size} S = {side}: {c}, overlap {overlap}, covered {int(covered.sum())}")
    FS.check_census(c, size)
    assert overlap >= FS.MIN_OVERLAP
    # where faces overlap the earlier one decides: the face index is the first face that is not OUTSIDE
    first = np.where((each != SR.OUTSIDE).any(0), (each != SR.OUTSIDE).argmax(0), 255)
    assert np.array_equal(face[covered], first[covered])


def test_at_exactly_90_degrees_the_seams_are_outside_everywhere():
    """a statement about the rule: a pixel ON a seam plane is rejected by both neighbours (xs == S or ys == S)"""
    _, _, covered, _, cls, face = case("cube", 64, FS.FRAME_DUMP, 90.0)
    n = int(((cls == SR.OUTSIDE) & covered).sum())
    print(f"90 degrees, 128 x 128: {n} of {int(covered.sum())} covered pixels are OUTSIDE every face")
    assert n >= 1
    assert (face[(cls == SR.OUTSIDE) & covered] == 255).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", FS.SIDES)
def test_cascade_inner_face_first(side):
    Ms, P, covered, maps, cls, face = case("cascade", side)
    inner_half, outer_half = FS.CASCADE_HALVES
    c = SS.clip64("ortho", np.asarray(P, np.float64))                    # the outer face IS shadow_scenes' light (half extent 3)
    reach = np.maximum(np.abs(c[..., 0]), np.abs(c[..., 1])) * outer_half  # the larger light-space |x|, |y|
    texel = 2.0 * outer_half / side
    well_in, between = reach < inner_half - texel, (reach > inner_half + texel) & (reach < outer_half - texel)
    assert (well_in & covered).sum() >= 64 and (between & covered).sum() >= 64
    assert (face[well_in & covered] == 0).all(), "inside the inner extent the inner face decides"
    assert (face[between & covered] == 1).all(), "the outer face decides only beyond it"
    assert (face[(reach > outer_half + texel) & covered] == 255).all()
    for f in (0, 1):
        assert ((cls == SR.LIT) & (face == f)).sum() >= 32 and ((cls == SR.SHADOWED) & (face == f)).sum() >= 32, (f, side)


# ---------------------------------------------------------------------------------------------------------------------
# 4
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", FS.SIDES)
@pytest.mark.parametrize("name", list(FR.MUTANTS))
def test_every_knob_of_the_rule_matters(name, side):
    Ms, P, covered, maps, cls, face = case("cube", side)
    m_cls, m_face = FR.classify(Ms, side, FS.BIAS, P, maps, covered, **FR.mutant(name, side))
    changed = int(((m_cls != cls) | (m_face != face)).sum())
    print(f"{name}, S = {side}: {changed} pixels change")
    assert changed >= 1


# ---------------------------------------------------------------------------------------------------------------------
# 5
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [FS.E, (3.0, -1.25, 0.5), (12345.678, -98765.4, 4321.0)], ids=["E", "near", "large"])
def test_cube_shadow_views_are_the_oracles_blocks(pos):
    from bibim_renderer_amd.scene import cube_shadow_views
    for fov, near, far in ((FS.FOV, FS.NEAR, FS.FAR), (90.0, 0.5, 100.0)):
        got = cube_shadow_views(pos, fov, near, far)
        want = FS.cube_views(pos, fov, near, far)
        assert got.shape == (6, 36) and got.dtype == np.float32
        for f in range(6):
            assert np.array_equal(SC.bits(got[f][:16]), SC.bits(want[f]["view"]).ravel()), f"face {f}: view"
            assert np.array_equal(SC.bits(got[f][16:32]), SC.bits(want[f]["proj"]).ravel()), f"face {f}: proj"
            assert np.array_equal(SC.bits(got[f][32:35]), SC.bits(SC.f32(pos))), f"face {f}: view_pos"
            assert got[f][35].view(np.int32) == 0


def test_new_symbols_are_declared_exported_and_bound():
    names = declared("bibim_hip.h")
    L = C.CDLL(_capi.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in names, f"{n} is not declared in include/bibim_hip.h"
        assert hasattr(L, n), f"{n} declared but not exported"
        assert n in _capi.SIGNATURES, f"{n} is not in the binding table"
    assert "bbs_cube_shadow_views" in declared("bibim_scene.h") and hasattr(L, "bbs_cube_shadow_views")
    from bibim_renderer_amd import Renderer
    for m in ("render_shadow_faces", "read_shadow_face", "read_shadow_face_index"):
        assert callable(getattr(Renderer, m, None)), m
