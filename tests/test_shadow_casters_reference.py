"""CPU: the model of up to eight shadow casters per context (tests/shadow_casters_reference.py; bbr_render_shadow_caster) on the
scenes of tests/shadow_casters_scenes.py, and the new symbols of the C ABI.  No GPU.

  1  with one slot, the model equals shadow_filter_reference bit for bit: verdicts and frame, on the existing scenes ("clipped",
     "cube", "cascade"), R in {0, 1, 2}, whichever slot the caster sits in
  2  the census holds on both kinds, both frame sizes and every S, and is the one recorded in tests/golden/shadow_casters.json
     (tools/shadow_casters_record.py)
  3  every knob matters: each mutant of the model changes the frame on "mixed" (the bias mutant: on "mixed" with the caster
     of slot 1 at bias 2, since the casters of "mixed" share one bias)
  4  the "hence" equalities hold in the model itself: slot permutation, a caster at bias 2, a caster on light 50
  5  the entry points are declared in include/bibim_hip.h, exported by the library and bound by the package"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import shadow_casters_reference as CR
import shadow_casters_scenes as CS
import shadow_faces_scenes as FS
import shadow_filter_reference as PR
import shadow_reference as SR
import shadow_scenes as SS
import surface_chart as SC
from test_capi_symbols import declared
from bibim_renderer_amd import _capi

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RADII = (0, 1, 2)
SYMBOLS = ("bbr_render_shadow_caster", "bbr_drop_shadow_caster", "bbr_get_shadow_casters", "bbr_read_shadow_caster_face",
           "bbr_read_shadow_caster_mask", "bbr_read_shadow_caster_face_index", "bbr_read_shadow_caster_taps")
equal = SC.equal_but_for_nan_payload


def surface_on(P):
    """light-loop inputs on positions P[h, w, 3]: the receiver's normal, a mid-grey dielectric"""
    surf = np.zeros((P.shape[0] * P.shape[1], 12), F)
    surf[:, 0:3] = P.reshape(-1, 3)
    surf[:, 3:6] = (SC.TILT[0], SC.TILT[1], -1.0)
    surf[:, 6:9], surf[:, 10], surf[:, 11] = 0.5, 0.5, 1.0
    return surf


# ---------------------------------------------------------------------------------------------------------------------
# 1
# ---------------------------------------------------------------------------------------------------------------------
def existing(kind, side, size=SS.FRAME_SMALL):
    """(scene, views, P float32, covered, maps) of a scene of the earlier steps"""
    if kind in FS.KINDS:
        P64, covered = FS.positions64(kind, size)
        return FS.scene(kind, size), FS.faces(kind), P64.astype(F), covered, FS.oracle_maps(kind, side)
    P64, covered, _ = SS.positions64(kind, size)
    return SS.scene(kind, size), np.array([SS.light_view(kind)]), P64.astype(F), covered, SS.oracle_map(kind, side)[None]


@pytest.mark.parametrize("slot", [0, 5])
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("kind", ["clipped", "cube", "cascade"])
def test_one_slot_is_the_filter_model(kind, radius, slot):
    side = 33
    sc, views, P, covered, maps = existing(kind, side)
    caster = dict(slot=slot, light=SS.CASTER, views=views, bias=SS.BIAS)
    got = CR.verdicts([caster], side, radius, P, lambda c: maps, covered)
    assert list(got) == [slot]
    cls, k, face = got[slot]
    Ms = [SR.proj_view(L) for L in views]
    if radius:
        want_cls, want_k, want_face = PR.taps(Ms, side, SS.BIAS, P, maps, radius, covered)
        assert np.array_equal(k, want_k)
    else:
        want_cls, want_face = PR.hard(Ms, side, SS.BIAS, P, maps, covered)
        assert np.array_equal(k, np.where(want_cls == SR.LIT, 1, np.where(want_cls == SR.SHADOWED, 0, 255)))
    assert np.array_equal(cls, want_cls) and np.array_equal(face, want_face)
    assert (cls == SR.SHADOWED).any() and (cls == SR.LIT).any()
    surf = surface_on(P)
    frame = CR.lit_frame(sc.frame, sc.view, surf, {slot: k.ravel()}, {slot: SS.CASTER}, radius)
    if radius:
        want = PR.lit_frame(sc.frame, sc.view, surf, k.ravel(), SS.CASTER, radius)
    else:
        want = SR.lit_frame(sc.frame, sc.view, surf, cls.ravel(), SS.CASTER)
    assert equal(frame, want)


# ---------------------------------------------------------------------------------------------------------------------
# 2
# ---------------------------------------------------------------------------------------------------------------------
def recorded(kind, c):
    """what the record keeps of a census"""
    if kind == "eight":
        return {"shadowed_count": {str(s): n for s, n in c["shadowed_count"].items()}}
    return {"lit": {str(s): round(v, 4) for s, v in c["lit"].items()}, "shadowed": {str(s): round(v, 4) for s, v in c["shadowed"].items()},
            "both_shadowed": c["both_shadowed"], "pair": c["pair"], "both_partial": c["both_partial"]}


@pytest.mark.parametrize("side", CS.SIDES)
@pytest.mark.parametrize("size", [CS.FRAME_SMALL, CS.FRAME_DUMP], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", CS.KINDS)
def test_census_holds_and_is_the_record(kind, size, side):
    c = CS.census(kind, side, size)
    print(f"{kind} {size} S = {side}: {c}")
    CS.check_census(kind, c, side)
    rec = json.load(open(os.path.join(GOLDEN, "shadow_casters.json")))
    assert rec["census"][f"{kind} {size[0]}x{size[1]} {side}"] == recorded(kind, c)
    assert rec["casters"][kind] == [[q["slot"], q["light"], len(q["views"])] for q in CS.casters(kind)]


def test_the_scenes_are_what_the_issue_names():
    mixed = CS.casters("mixed")
    assert [(c["slot"], c["light"], len(c["views"])) for c in mixed] == [(0, 2, 6), (1, 0, 1), (5, 3, 2)]
    eight = CS.casters("eight")
    assert [c["slot"] for c in eight] == list(range(8)) and sorted(c["light"] for c in eight) == list(range(8))
    assert all(len(c["views"]) == 1 for c in eight) and len({c["views"].tobytes() for c in eight}) == 8
    assert int(CS.scene("eight").frame["num_lights"]) == 8 and int(CS.scene("mixed").frame["num_lights"]) == 4


# ---------------------------------------------------------------------------------------------------------------------
# 3, 4
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def mixed(radius, side=33, size=CS.FRAME_SMALL):
    """(scene, P, covered, surf, verdicts, frame) of the rule on "mixed" """
    sc = CS.scene("mixed", size)
    P64, covered = CS.positions64("mixed", size)
    P = P64.astype(F)
    surf = surface_on(P)
    v = CR.verdicts(CS.casters("mixed"), side, radius, P, lambda c: CS.oracle_maps("mixed", c["slot"], side), covered)
    return sc, P, covered, surf, v, frame_of(sc, surf, v, CS.casters("mixed"), radius)


def frame_of(sc, surf, v, casters, radius, **knobs):
    return CR.lit_frame(sc.frame, sc.view, surf, {s: v[s][1].ravel() for s in v}, {c["slot"]: c["light"] for c in casters}, radius, **knobs)


def changed(a, b):
    return int((SC.bits(a) != SC.bits(b)).any(-1).sum())


# (R = 0 has no partial scale: "all partial scales multiplied into each" is a knob of R >= 1 only)
@pytest.mark.parametrize("mutant,radius", [(m, r) for m in CR.LOOP_MUTANTS for r in (0, 1) if r or "partial" not in m])
def test_loop_mutants_change_the_frame(mutant, radius):
    sc, _, _, surf, v, want = mixed(radius)
    got = frame_of(sc, surf, v, CS.casters("mixed"), radius, **CR.LOOP_MUTANTS[mutant])
    n = changed(got, want)
    print(f"{mutant} | R = {radius}: {n} pixels change")
    assert n >= 1


@pytest.mark.parametrize("radius", [0, 1])
@pytest.mark.parametrize("mutant", list(CR.VERDICT_MUTANTS))
def test_verdict_mutants_change_the_frame(mutant, radius):
    side, size = 33, CS.FRAME_SMALL
    casters = list(CS.casters("mixed"))
    if "bias" in mutant:        # (the casters of "mixed" share one bias: the knob shows where one does not)
        casters[1] = dict(casters[1], bias=2.0)
    sc, P, covered, surf, _, _ = mixed(radius)
    maps_of = lambda c: CS.oracle_maps("mixed", c["slot"], side)
    want = frame_of(sc, surf, CR.verdicts(casters, side, radius, P, maps_of, covered), casters, radius)
    got = frame_of(sc, surf, CR.verdicts(casters, side, radius, P, maps_of, covered, **CR.VERDICT_MUTANTS[mutant]), casters, radius)
    n = changed(got, want)
    print(f"{mutant} | R = {radius}: {n} pixels change")
    assert n >= 1


@pytest.mark.parametrize("radius", [0, 1])
def test_hence_equalities_in_the_model(radius):
    side = 33
    sc, P, covered, surf, v, want = mixed(radius)
    maps_of = lambda c: CS.oracle_maps("mixed", c["slot"], side)
    casters = CS.casters("mixed")
    # permuted over the slots 7, 2, 0: a dict of the same casters under other keys
    moved = [dict(c, slot=s) for c, s in zip(casters, (7, 2, 0))]
    by_slot = {m["slot"]: c["slot"] for m, c in zip(moved, casters)}
    v2 = CR.verdicts(moved, side, radius, P, lambda c: maps_of(dict(c, slot=by_slot[c["slot"]])), covered)
    assert equal(frame_of(sc, surf, v2, moved, radius), want)
    # the caster of slot 1 at bias 2, and on light 50: the frame of the other two
    two = [casters[0], casters[2]]
    without = frame_of(sc, surf, {s: v[s] for s in (0, 5)}, two, radius)
    assert changed(without, want) >= 1
    lifted = [casters[0], dict(casters[1], bias=2.0), casters[2]]
    v3 = CR.verdicts(lifted, side, radius, P, maps_of, covered)
    assert not (v3[1][0] == SR.SHADOWED).any() and not (v3[1][0] == PR.PARTIAL).any()
    assert equal(frame_of(sc, surf, v3, lifted, radius), without)
    beyond = [casters[0], dict(casters[1], light=50), casters[2]]
    assert equal(frame_of(sc, surf, v, beyond, radius), without)


# ---------------------------------------------------------------------------------------------------------------------
# 5
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symbol", SYMBOLS)
def test_new_symbols_are_declared_exported_and_bound(symbol):
    assert symbol in declared("bibim_hip.h"), "not declared in include/bibim_hip.h"
    assert hasattr(C.CDLL(_capi.LIB_PATH), symbol), "declared but not exported"
    assert symbol in _capi.SIGNATURES, "not in the binding table"
    from bibim_renderer_amd import Renderer
    for method in ("render_shadow_caster", "drop_shadow_caster", "shadow_casters", "read_shadow_caster_face", "read_shadow_caster_mask",
                   "read_shadow_caster_face_index", "read_shadow_caster_taps"):
        assert callable(getattr(Renderer, method, None)), method
