"""GPU: the four shadow kernels (k_shade_shadow, k_shade_shadow_faces, k_shade_shadow_pcf, k_shade_shadow_casters) on the shadow
chart (tests/shadow_chart.py; DESIGN.md section 3, "Shadow chart") against the shipped CPU models.  Everything is bit for bit,
NaN in the same places, no tolerance ("equal": surface_chart.equal_but_for_nan_payload).

Every case is checked the same way (`check`): each map against the oracle's depth; class, count k and face index of every slot
against the model on the dumped P (deferred: the G-buffer's P, asserted equal to the rounded dump); the frame against the model's
light loop on the dumped surface under the device's counts; the frame again after the dumps.

  1  steps    "persp" at every bias below one ulp of the depths and both S, "edges", "thirds" and "behind" at bias 0 and 2^-8,
              both passes: through k_shade_shadow, at R = 1 through k_shade_shadow_pcf (the window clamps exactly where xs is 0
              and S - 1), and "persp" once more with the caster in slot 5 alone (k_shade_shadow_casters).  The dumped P is the
              chart's (x, y, z_q), a binary16 number, and the census of tests/test_shadow_chart.py holds on it
  2  terrain  the cube at R = 0 (k_shade_shadow_faces), 1 and 2; three casters in slots 1, 4, 7 with F = 1, 3, 6 at R = 0 and 1;
              both passes; every face decides pixels and quads of 4 x 4 pixels have lanes deciding at different faces
  3  routes   one case per kernel on the long route (no_tail_items 0), the long route with heavy_tiles 4 and the long route with
              tile_mode 0: the frame and every read-back against the model AND against the short route's bits; a plain frame
              after the DUMP read-backs; ten replay_frame() with frames_in_flight 1 and 3 on the long route"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import shadow_casters_reference as CR
import shadow_chart as CH
import shadow_filter_reference as PR
import shadow_reference as SR
import surface_chart as SC
from bibim_renderer_amd import Renderer
from oracle import bbo

pytestmark = pytest.mark.gpu

equal = SC.equal_but_for_nan_payload
bits = SC.bits
pass_id = lambda d: "deferred" if d else "forward"
PASSES = [0, 1]
NAMES = ("classes", "counts", "face indices")


def one(light, bias, slot=0):
    """the caster list of one light of the chart"""
    return (dict(slot=slot, light=CH.CASTER, views=CH.views(light), bias=bias, name=light),)


def case(casters, side, radius=0):
    return SimpleNamespace(casters=tuple(casters), side=side, radius=radius, chart=CH.CHART_OF[casters[0]["name"]])


def context(cs, deferred, **options):
    """the options are set explicitly, after construction"""
    r = Renderer(*CH.SIZE)
    r.set_option("render_pass", deferred)
    for k, v in options.items():
        r.set_option(k, v)
    r.set_option("shadow_map", cs.side)
    r.set_option("shadow_filter", cs.radius)
    return r


def cast(r, cs):
    """slot 0 alone goes through the calls of before there were slots: bbr_render_shadow_map (one face) / _faces"""
    for c in cs.casters:
        if len(cs.casters) == 1 and c["slot"] == 0:
            if len(c["views"]) == 1:
                r.render_shadow_map(c["light"], c["views"][0], c["bias"])
            else:
                r.render_shadow_faces(c["light"], c["views"], c["bias"])
        else:
            r.render_shadow_caster(c["slot"], c["light"], c["views"], c["bias"])


def model_inputs(r, cs, deferred):
    """(light-loop inputs [n, 12], the P the test sees [h, w, 3]) from the device's dumps; on "steps" P is the chart's own"""
    surf = r.read_surface()
    Ps = np.ascontiguousarray(surf[..., 6:9])
    P, covered = CH.positions(cs.chart)
    if cs.chart == "steps":
        assert np.array_equal(bits(Ps), bits(P)), "steps: the dumped P is not (x, y, z_q)"
        assert np.array_equal(bits(bbo.half_round(Ps)), bits(Ps)), "steps: P is not made of binary16 numbers"
    if not deferred:
        return SC.surface_values(surf), Ps
    gbuf = r.read_gbuffer()
    Pr = bbo.half_round(Ps)
    assert equal(gbuf[..., 0, :3], Pr), "the G-buffer's position is not the rounded dump"
    assert np.array_equal(bits(Pr), bits(P)), "the deferred pass's P is not the oracle's"
    return SC.gbuffer_values(gbuf), Pr


def device_verdicts(r, cs):
    """slot -> (mask, taps, face index) as the device reports them; slot 0 alone through the read-backs of before the slots"""
    out = {}
    for c in cs.casters:
        s = c["slot"]
        if len(cs.casters) == 1 and s == 0:
            out[s] = (r.read_shadow_mask(), r.read_shadow_taps(), r.read_shadow_face_index())
        else:
            out[s] = (r.read_shadow_caster_mask(s), r.read_shadow_caster_taps(s), r.read_shadow_caster_face_index(s))
    return out


def check(r, cs, deferred, what, inputs=None):
    """the current frame of `r` and all its read-backs against the model; returns them.  `inputs`: model_inputs of the same
    context from an earlier call (the surface does not depend on the casters)"""
    sc = CH.scene(cs.chart)
    covered = CH.positions(cs.chart)[1]
    frame = r.read_framebuffer()
    for c in cs.casters:
        want = CH.oracle_maps(c["name"], cs.side)
        for f in range(len(c["views"])):
            got = r.read_shadow_caster_face(c["slot"], f)
            assert np.array_equal(bits(got), bits(want[f])), f"{what}, slot {c['slot']} face {f}: {int((bits(got) != bits(want[f])).sum())} texels differ"
    surf, Pt = model_inputs(r, cs, deferred) if inputs is None else inputs
    got = device_verdicts(r, cs)
    again = r.read_framebuffer()
    want = CR.verdicts(cs.casters, cs.side, cs.radius, Pt, lambda c: CH.oracle_maps(c["name"], cs.side), covered)
    for s in want:
        differ = [int((g != w).sum()) for g, w in zip(got[s], want[s])]
        print(f"{what} slot {s}: {differ} {NAMES} differ, classes {np.bincount(got[s][0].ravel(), minlength=5).tolist()}")
        for name, g, w in zip(NAMES, got[s], want[s]):
            assert np.array_equal(g, w), f"{what} slot {s}: {int((g != w).sum())} {name} differ"
    model = CR.lit_frame(sc.frame, sc.view, surf, {s: got[s][1].ravel() for s in got}, {c["slot"]: c["light"] for c in cs.casters}, cs.radius)
    model = model.reshape(CH.H, CH.W, 4)
    assert equal(frame, model), f"{what}: {int((bits(frame) != bits(model)).any(-1).sum())} pixels differ from the model's light loop"
    assert equal(again, frame), f"{what}: the dumps re-render the frame: the same bits"
    if len(cs.casters) == 1 and cs.radius == 0:     # one caster, a hard compare: the first model's own light loop as well
        first = SR.lit_frame(sc.frame, sc.view, surf, got[cs.casters[0]["slot"]][0], cs.casters[0]["light"]).reshape(CH.H, CH.W, 4)
        assert equal(frame, first), what
    if len(cs.casters) == 1 and cs.radius >= 1:
        c = cs.casters[0]
        second = PR.lit_frame(sc.frame, sc.view, surf, got[c["slot"]][1], c["light"], cs.radius).reshape(CH.H, CH.W, 4)
        assert equal(frame, second), what
    return SimpleNamespace(frame=frame, got=got, inputs=(surf, Pt))


def first_frame(r, cs):
    """render the chart once, then the casters' maps, then the frame again under them"""
    r.render_scene(CH.scene(cs.chart))
    cast(r, cs)
    r.replay_frame()


# ---------------------------------------------------------------------------------------------------------------------
# 1. steps
# ---------------------------------------------------------------------------------------------------------------------
STEPS = [(light, side) for light in ("persp", "edges", "thirds", "behind") for side in CH.SIDES[light]]
steps_id = lambda c: f"{c[0]} {c[1]}"


def sweep(light, side, deferred, radius, slot):
    """one context, every bias of the light: the class of a pixel hangs on the last bit of t"""
    cs = case(one(light, 0.0, slot), side, radius)
    r = context(cs, deferred)
    r.render_scene(CH.scene(cs.chart))
    inputs, masks = None, {}
    for bias in CH.BIASES[light]:
        cs = case(one(light, bias, slot), side, radius)
        cast(r, cs)
        r.replay_frame()
        out = check(r, cs, deferred, f"{light} S = {side} R = {radius} slot {slot} bias {bias!r} {pass_id(deferred)}", inputs)
        inputs, masks[bias] = out.inputs, out.got[slot][0]
    r.close()
    # what the chart was built to reach, on the device's P and with the device's classes
    P, covered = inputs[1], CH.positions("steps")[1]
    c = CH.census(light, side, P, covered)
    print(f"{light} S = {side}: {c}")
    CH.check_census(light, c)
    if radius == 0:
        zero = masks[0.0]
        assert (zero == SR.LIT).sum() == c["lit"] and (zero == SR.SHADOWED).sum() == c["shadowed"] and (zero == SR.OUTSIDE).sum() == c["outside"]
    if light == "persp" and radius == 0:
        assert not np.array_equal(masks[-2.0 ** -28], masks[0.0]), "a bias of one ulp of the depths changes no class"


@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
@pytest.mark.parametrize("steps", STEPS, ids=steps_id)
def test_steps_through_k_shade_shadow(steps, deferred):
    sweep(*steps, deferred, 0, 0)


@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
@pytest.mark.parametrize("steps", STEPS, ids=steps_id)
def test_steps_through_k_shade_shadow_pcf(steps, deferred):
    sweep(*steps, deferred, 1, 0)


@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
@pytest.mark.parametrize("side", CH.SIDES["persp"])
def test_steps_persp_in_slot_five_through_k_shade_shadow_casters(side, deferred):
    sweep("persp", side, deferred, 0, 5)


# ---------------------------------------------------------------------------------------------------------------------
# 2. terrain
# ---------------------------------------------------------------------------------------------------------------------
def three(side=64, radius=0):
    return case(CH.three_casters(), side, radius)


@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
@pytest.mark.parametrize("radius", [0, 1, 2])
def test_terrain_under_the_cube(radius, deferred):
    cs = case(one("cube", CH.BIAS), 64, radius)
    r = context(cs, deferred)
    first_frame(r, cs)
    out = check(r, cs, deferred, f"cube R = {radius} {pass_id(deferred)}")
    r.close()
    mask, taps, face = out.got[0]
    covered = CH.positions("terrain")[1]
    per_face = [int(((face == f) & covered).sum()) for f in range(6)]
    mixed = CH.mixed_quads(face, covered)
    print(f"cube R = {radius} {pass_id(deferred)}: per face {per_face}, mixed quads {mixed}, classes {np.bincount(mask.ravel(), minlength=5).tolist()}")
    assert min(per_face) >= CH.MIN_PER_FACE and mixed >= CH.MIN_MIXED_QUADS
    assert (mask == SR.LIT).sum() >= CH.MIN_CLASS and (mask == SR.SHADOWED).sum() >= CH.MIN_CLASS
    if radius:
        assert (mask == PR.PARTIAL).sum() >= CH.MIN_CLASS


@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
@pytest.mark.parametrize("radius", [0, 1])
def test_terrain_under_three_casters(radius, deferred):
    cs = three(64, radius)
    r = context(cs, deferred)
    first_frame(r, cs)
    out = check(r, cs, deferred, f"three R = {radius} {pass_id(deferred)}")
    r.close()
    for s, (mask, taps, face) in out.got.items():
        assert (mask == SR.LIT).sum() >= CH.MIN_CLASS and (mask == SR.SHADOWED).sum() >= CH.MIN_CLASS, s
    assert (out.got[4][0] == SR.OUTSIDE).sum() >= CH.MIN_CLASS, "three faces leave part of the frame outside"


# ---------------------------------------------------------------------------------------------------------------------
# 3. routes
# ---------------------------------------------------------------------------------------------------------------------
KERNELS = {"k_shade_shadow": lambda: case(one("persp", -2.0 ** -28), 200, 0),
           "k_shade_shadow_faces": lambda: case(one("cube", CH.BIAS), 64, 0),
           "k_shade_shadow_pcf": lambda: case(one("edges", 0.0), 64, 1),
           "k_shade_shadow_casters": lambda: three(64, 1)}
ROUTES = {"long": {"no_tail_items": 0}, "long, heavy_tiles 4": {"no_tail_items": 0, "heavy_tiles": 4},
          "long, tile_mode 0": {"no_tail_items": 0, "tile_mode": 0}}


@functools.lru_cache(None)
def short_route(kernel, deferred):
    """the frame and the read-backs of the default (short) route, checked against the model on the way"""
    cs = KERNELS[kernel]()
    r = context(cs, deferred)
    first_frame(r, cs)
    out = check(r, cs, deferred, f"{kernel} {pass_id(deferred)}, short route")
    r.close()
    return out


def assert_same_bits(out, base, what):
    assert equal(out.frame, base.frame), f"{what}: {int((bits(out.frame) != bits(base.frame)).any(-1).sum())} pixels differ from the short route's"
    assert equal(out.inputs[0], base.inputs[0]), f"{what}: the surface differs from the short route's"
    for s in base.got:
        for name, g, w in zip(NAMES, out.got[s], base.got[s]):
            assert np.array_equal(g, w), f"{what} slot {s}: {name} differ from the short route's"


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_route_does_not_change_a_bit(kernel, deferred, route):
    base = short_route(kernel, deferred)
    cs = KERNELS[kernel]()
    what = f"{kernel} {pass_id(deferred)}, {route}"
    r = context(cs, deferred, **ROUTES[route])
    first_frame(r, cs)
    out = check(r, cs, deferred, what)
    assert_same_bits(out, base, what)
    # the DUMP forms re-rendered through this route: a plain frame after them carries nothing of theirs
    r.replay_frame()
    plain = r.read_framebuffer()
    r.close()
    assert equal(plain, base.frame), f"{what}: a plain frame after the read-backs differs"


@pytest.mark.parametrize("deferred", PASSES, ids=pass_id)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_long_route_replays_and_frames_in_flight(kernel, deferred):
    """the long route sizes its launch from the slot's previous frame: replays are where that estimate is in use"""
    base = short_route(kernel, deferred)
    cs = KERNELS[kernel]()
    for fif in (1, 3):
        what = f"{kernel} {pass_id(deferred)}, long route, {fif} in flight"
        r = context(cs, deferred, frames_in_flight=fif, no_tail_items=0)
        r.render_scene(CH.scene(cs.chart))
        cast(r, cs)
        for _ in range(10):
            r.replay_frame()
        frame = r.read_framebuffer()
        assert equal(frame, base.frame), f"{what}: {int((bits(frame) != bits(base.frame)).any(-1).sum())} pixels differ after ten replays"
        got = device_verdicts(r, cs)
        for s in base.got:
            for name, g, w in zip(NAMES, got[s], base.got[s]):
                assert np.array_equal(g, w), f"{what} slot {s}: {name} differ"
        for _ in range(2):
            r.replay_frame()
        again = r.read_framebuffer()
        r.close()
        assert equal(again, base.frame), f"{what}: a plain frame after the read-backs differs"
