"""CPU: the shadow chart (tests/shadow_chart.py) held against the shipped models of the shadow rule and the oracle's maps.  No
GPU.

  1  the chart's own classify step (the copy with the extra knobs) IS shadow_reference.classify when no knob is turned, and the
     single-point form agrees on the pixels that sit on a boundary
  2  census: every chart x light x S reaches what it was built for -- xs == 0, xs == S, ys == 0, ys == S, integer xs, c.w == 0,
     c.w < 0 on at least 64 pixels each, at least 1024 pixels whose map texel is within one ulp of their own depth, at least 32
     pixels per cube face and 64 quads of mixed faces, at least 64 LIT and 64 SHADOWED pixels everywhere
  3  model mutants: t as one fma, t by division, r one ulp up, xs unfused, > 0 for >= 0, <= S for < S, the c.w test left out --
     each changes at least 64 classes on the chart built for it.  ">= 0 for > 0 on c.w" is EQUIVALENT under the rule and is
     shown to be: at c.w == +-0 the reciprocal is infinite, xs is infinite or NaN, and the fragment is OUTSIDE either way
  4  the window of the filter at R = 1 clamps at columns and rows 0 and S - 1 on "edges": every tap mutant of
     shadow_filter_reference changes at least 64 counts there
  5  what 2 .. 4 measure is what tests/golden/shadow_chart.json records (tools/shadow_chart_record.py)"""
import functools
import json
import os

import numpy as np
import pytest

import shadow_casters_reference as CR
import shadow_chart as CH
import shadow_filter_reference as PR
import shadow_reference as SR
from conftest import GOLDEN

F = np.float32
ONE_FACE = ("persp", "edges", "thirds", "behind")
CASES = [(light, side) for light in ONE_FACE for side in CH.SIDES[light]]
case_id = lambda c: f"{c[0]} {c[1]}"
# mutant -> the light whose population was built for it
BUILT_FOR = {"t fused": "persp", "t by division": "persp", "r one ulp up": "persp", "xs unfused": "thirds",
             "> 0 for >= 0": "edges", "<= S for < S": "edges", "no test of c.w": "behind"}
EQUIVALENT = (">= 0 for > 0 on c.w",)
bias_key = lambda b: repr(float(b))


@functools.lru_cache(None)
def mutant_counts(light, side):
    """mutant -> bias -> the number of pixels whose class it changes"""
    P, covered = CH.positions(CH.CHART_OF[light])
    M, depth = CH.matrices(light)[0], CH.oracle_maps(light, side)[0]
    out = {name: {} for name in CH.KNOBS}
    for bias in CH.BIASES[light]:
        base = CH.classify(M, side, bias, P, depth, covered)
        for name, knob in CH.KNOBS.items():
            out[name][bias_key(bias)] = int((CH.classify(M, side, bias, P, depth, covered, **knob) != base).sum())
    return out


@functools.lru_cache(None)
def tap_mutant_counts():
    """shadow_filter_reference's tap mutants on "edges" at R = 1: mutant -> the number of pixels whose count k changes"""
    P, covered = CH.positions("steps")
    Ms, maps = CH.matrices("edges"), CH.oracle_maps("edges", 64)
    base = PR.taps(Ms, 64, 0.0, P, maps, 1, covered)[1]
    return {name: int((PR.taps(Ms, 64, 0.0, P, maps, 1, covered, **knob)[1] != base).sum()) for name, knob in PR.TAP_MUTANTS.items()}


@functools.lru_cache(None)
def three_census():
    """slot -> classes of the three casters on the terrain at R = 0: [NONE, LIT, SHADOWED, OUTSIDE] counts"""
    P, covered = CH.positions("terrain")
    v = CR.verdicts(CH.three_casters(), 64, 0, P, lambda c: CH.oracle_maps(c["name"], 64), covered)
    return {str(s): np.bincount(v[s][0].ravel(), minlength=4).tolist() for s in v}


def measured():
    """the whole record: what tools/shadow_chart_record.py writes"""
    return {"seed_z": CH.SEED_Z, "cube_e": list(CH.CUBE_E), "cube3_faces": list(CH.CUBE3_FACES),
            "minima": {"equal": CH.MIN_EQUAL, "ties": CH.MIN_TIES, "per_face": CH.MIN_PER_FACE, "mixed_quads": CH.MIN_MIXED_QUADS,
                       "class": CH.MIN_CLASS, "mutant": CH.MIN_MUTANT},
            "census": {case_id(c): CH.census(*c) for c in CASES},
            "faces": {f"{light} 64": CH.face_census(light, 64) for light in ("cube", "cube3")},
            "three": three_census(),
            "mutants": {case_id(c): mutant_counts(*c) for c in CASES},
            "tap_mutants": tap_mutant_counts()}


@functools.lru_cache(None)
def recorded():
    return json.load(open(os.path.join(GOLDEN, "shadow_chart.json")))


# ---------------------------------------------------------------------------------------------------------------------
# 1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_copy_with_no_knob_turned_is_the_shipped_model(case):
    light, side = case
    P, covered = CH.positions(CH.CHART_OF[light])
    M, depth = CH.matrices(light)[0], CH.oracle_maps(light, side)[0]
    for bias in CH.BIASES[light]:
        want = SR.classify(M, side, bias, P, depth, covered)
        assert np.array_equal(CH.classify(M, side, bias, P, depth, covered), want), bias
    # the single-point form on the pixels of a boundary (and every 37th of the rest)
    c, r, xs, ys, _ = CH.terms(M, side, 0.0, P)
    on = (xs == 0) | (xs == side) | (ys == 0) | (ys == side) | (c[..., 3] == 0)
    on.reshape(-1)[::37] = True
    want = SR.classify(M, side, 0.0, P, depth)
    for y, x in zip(*np.nonzero(on)):
        assert SR.classify_point(M, side, 0.0, P[y, x], depth) == want[y, x], (y, x)


def test_steps_positions_are_binary16_numbers():
    P, covered = CH.positions("steps")      # (asserts P == (x, y, z_q) on the oracle's G-buffer)
    assert covered.all() and len(np.unique(P[..., 2])) >= 700      # (1024 draws from 1921 values)
    z = CH.quad_z().astype(np.float64)
    assert (z * 512 == np.rint(z * 512)).all() and np.abs(z).max() <= 1.875
    assert int((CH.quad_z() == F(CH.BEHIND_Z)).sum()) >= 40


# ---------------------------------------------------------------------------------------------------------------------
# 2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_census_of_a_one_face_light(case):
    light, side = case
    c = CH.census(light, side)
    print(f"{light} S = {side}: {c}")
    CH.check_census(light, c)
    assert recorded()["census"][case_id(case)] == c


@pytest.mark.parametrize("light", ["cube", "cube3"])
def test_census_of_the_faces(light):
    c = CH.face_census(light, 64)
    print(f"{light}: {c}")
    CH.check_face_census(light, c)
    if light == "cube3":
        assert c["no face"] >= CH.MIN_CLASS, "part of the frame is outside every face"
    assert recorded()["faces"][f"{light} 64"] == c


def test_census_of_the_three_casters():
    c = three_census()
    print(c)
    for s, counts in c.items():
        assert counts[SR.LIT] >= CH.MIN_CLASS and counts[SR.SHADOWED] >= CH.MIN_CLASS, (s, counts)
    assert sorted(c) == ["1", "4", "7"] and [len(x["views"]) for x in CH.three_casters()] == [1, 3, 6]
    assert recorded()["three"] == c


# ---------------------------------------------------------------------------------------------------------------------
# 3
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", list(BUILT_FOR))
def test_model_mutant_changes_the_classes(mutant):
    light = BUILT_FOR[mutant]
    for side in CH.SIDES[light]:
        counts = mutant_counts(light, side)[mutant]
        print(f"{mutant} | {light} S = {side}: {counts}")
        assert max(counts.values()) >= CH.MIN_MUTANT, (mutant, light, side, counts)
    if light == "persp":
        assert all(mutant_counts(light, side)[mutant][bias_key(CH.BIAS)] == 0 for side in CH.SIDES[light]), \
            "the working bias hides the last bit: that is why the chart has biases below one ulp"


@pytest.mark.parametrize("mutant", EQUIVALENT)
def test_equivalent_mutant_is_equivalent(mutant):
    """c.w == +-0: r = 1 / c.w is +-inf, c.x * r is +-inf or (c.x == 0) NaN, fmaf(that, h, h) likewise, and no infinity and no
    NaN passes xs >= 0 && xs < S.  So ">= 0" classifies every fragment as "> 0" does, on any population."""
    for case in CASES:
        assert set(mutant_counts(*case)[mutant].values()) == {0}, case
    h = F(100.0)
    with np.errstate(all="ignore"):
        for w in (F(0.0), F(-0.0)):
            r = F(1.0) / w
            for cx in (F(0.0), F(-0.0), F(1e-45), F(-1e-45), F(1.0), F(-3.0), F(3e38), F(np.inf), F(np.nan)):
                xs = CH.fmaf(np.array([cx * r], F), h, h)[0]
                assert not (xs >= 0 and xs < 200), (w, cx, xs)


def test_every_mutant_is_recorded():
    assert set(CH.KNOBS) == set(BUILT_FOR) | set(EQUIVALENT)
    for case in CASES:
        assert recorded()["mutants"][case_id(case)] == mutant_counts(*case), case


# ---------------------------------------------------------------------------------------------------------------------
# 4
# ---------------------------------------------------------------------------------------------------------------------
def test_filter_window_clamps_on_the_edges_chart():
    P, covered = CH.positions("steps")
    c, r, xs, ys, _ = CH.terms(CH.matrices("edges")[0], 64, 0.0, P)
    inside = (xs >= 0) & (xs < 64) & (ys >= 0) & (ys < 64)
    for at in (0, 63):
        assert int((inside & (xs == at)).sum()) >= CH.MIN_EQUAL and int((inside & (ys == at)).sum()) >= CH.MIN_EQUAL
    counts = tap_mutant_counts()
    print(counts)
    assert min(counts.values()) >= CH.MIN_MUTANT, counts
    assert recorded()["tap_mutants"] == counts


# ---------------------------------------------------------------------------------------------------------------------
# 5
# ---------------------------------------------------------------------------------------------------------------------
def test_record_is_whole():
    rec = recorded()
    assert rec["seed_z"] == CH.SEED_Z and rec["cube_e"] == list(CH.CUBE_E) and rec["cube3_faces"] == list(CH.CUBE3_FACES)
    assert rec["minima"] == measured()["minima"]
    assert set(rec["census"]) == set(rec["mutants"]) == {case_id(c) for c in CASES}
