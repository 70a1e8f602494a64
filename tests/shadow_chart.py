"""Shadow chart: 128 x 128 frames whose pixels are a CHOSEN population of positions for the shadow test (shadow_texel and
the pieces the four shadow kernels share in csrc/bb_kernels.hip.h; DESIGN.md section 3, "Shadow chart").  TEST INFRASTRUCTURE ONLY; no test lives
here.

The scenes of tests/shadow_scenes.py and its descendants put every receiver on ONE plane perpendicular to the caster's axis: the
arithmetic of t, r and xs is exercised at a handful of values there, and no pixel sits on a boundary of a comparison.  The
charts below use the surface chart's camera (surface_chart.ortho_view, s = 1): a pixel's world x, y are its centre, exactly.

  charts  "steps"    surface_chart._fine_mesh's 32 x 32 quads of 4 x 4 pixels, every quad FLAT at its own z_q, a random multiple
                     of 2^-9 in [-1.875, 1.875] (the first BEHIND_QUADS quads: 0.5): 1024 depths under a light that looks along
                     +z, and P = (x, y, z_q) is made of binary16 numbers -- bb_half_round(P) == P, the deferred pass sees the
                     forward pass's P
          "terrain"  the fine mesh as it is: a random z per corner, 8 triangles per wave
  lights  "persp"    steps; look_at((0, 0, -6), 0) with mat_perspective(100, 1, 1, 16), S in {200, 333}, biases below one ulp of
                     the depths (0.06 .. 0.19) and 2^-8: the map holds the quad's own depth, so the LAST BIT of t decides
          "edges"    steps; an orthographic light along +z, its axis half a pixel off the frame's centre, every entry dyadic,
                     S = 64: xs = i - 32 and ys = j - 32 EXACTLY for pixel (i, j) -- every pixel centre is a texel corner, and
                     columns 32 and 96 (rows likewise) are xs == 0 and xs == S
          "thirds"   steps; "edges" with half extent 3 and S = 96: h = 48 is no power of two and proj[0][0] is the binary32
                     nearest 1/3, so c.x * r * h is inexact while xs is (nearly) an integer on every pixel -- where fmaf(c.x * r,
                     h, h) and the two-rounding form (c.x * r) * h + h fall on different sides of a texel edge
          "behind"   steps; a perspective light with its eye inside the box, at z = 0.5: c.w == 0 on the quads at 0.5, < 0 on
                     the nearer ones
          "cube"     terrain; the six faces of a point light inside the box (shadow_faces_scenes.cube_views): lanes of one wave
                     decide at different faces
          "cube3"    terrain; faces -X, +Y and -Z of "cube" alone: part of the frame is outside every face
          "over"     terrain; "persp"'s view block
          three casters (`three_casters`) in slots 1, 4 and 7 with F = 1 ("over"), 3 ("cube3") and 6 ("cube") on lights 0, 3, 2
A light's name gives its view blocks (`views`), the map sides it is used at (SIDES) and its biases (BIASES)."""
from __future__ import annotations

import functools

import numpy as np

import shadow_faces_reference as FR
import shadow_faces_scenes as FS
import shadow_reference as SR
import surface_chart as SC
from aniso_reference import fmaf
from oracle import bbo

F = np.float32
W = H = SC.W
SIZE = (W, H)
CASTER = 2                       # the caster's light index wherever there is one caster (never 0)
SEED_Z = 77
BEHIND_QUADS = 40                # steps: this many quads lie in the plane of the "behind" light's eye
BEHIND_Z = 0.5
CHART_OF = {"persp": "steps", "edges": "steps", "thirds": "steps", "behind": "steps", "cube": "terrain", "cube3": "terrain", "over": "terrain"}
SIDES = {"persp": (200, 333), "edges": (64,), "thirds": (96,), "behind": (200,), "cube": (64,), "cube3": (64,), "over": (64,)}
SUB_ULP = (2.0 ** -29, 3 * 2.0 ** -30, 2.0 ** -28)
BIAS = 2.0 ** -8
BIASES = {"persp": (0.0,) + tuple(s * b for b in SUB_ULP for s in (1.0, -1.0)) + (BIAS,),
          "edges": (0.0, BIAS), "thirds": (0.0, BIAS), "behind": (0.0, BIAS), "cube": (BIAS,)}
CUBE_E = (0.375, -0.625, 0.25)   # the point light of "cube": inside the box, off every quad edge
CUBE_FOV, CUBE_NEAR, CUBE_FAR = 96.0, 0.0625, 16.0
CUBE3_FACES = (1, 2, 5)
BEHIND_FOV, BEHIND_NEAR = 150.0, 0.03125
# three casters on the terrain: slot, light, the light whose views they take, bias
THREE = ((1, 0, "over", BIAS), (4, 3, "cube3", BIAS), (7, 2, "cube", BIAS))
# the census minima (conditions, not measurements)
MIN_EQUAL, MIN_TIES, MIN_PER_FACE, MIN_MIXED_QUADS, MIN_CLASS, MIN_MUTANT = 64, 1024, 32, 64, 64, 64


# ---------------------------------------------------------------------------------------------------------------------
# charts
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def quad_z():
    """z_q of the 1024 quads of "steps", float32: multiples of 2^-9"""
    rng = np.random.Generator(np.random.PCG64(SEED_Z))
    z = (rng.integers(-960, 961, 1024) * 2.0 ** -9).astype(F)
    z[:BEHIND_QUADS] = F(BEHIND_Z)
    z.setflags(write=False)
    return z


@functools.lru_cache(None)
def _draws(chart):
    draws, nm = SC.chart("fine")
    if chart == "steps":
        d = draws[0]
        v = d.vertices.copy()
        v["pos"][:, 2] = np.repeat(quad_z(), 4)
        draws = [bbo.DrawData(v, d.indices, d.instances, d.material)]
    return tuple(draws), nm


@functools.lru_cache(None)
def scene(chart):
    """the camera's frame of a chart under the surface chart's regular lights (set a: types 0, 1, 2, 0)"""
    draws, nm = _draws(chart)
    ls, view_pos = SC.set_a()
    fu, vu = SC.uniforms(ls, view_pos, 1.0, nm)
    return bbo.Scene(fu, vu, list(draws), W, H, f"shadow chart {chart}")


@functools.lru_cache(None)
def positions(chart):
    """(P float32 [H, W, 3], covered bool [H, W]): the position attachment of the oracle's G-buffer -- the P the deferred pass
    tests.  On "steps" that is (x, y, z_q) exactly, the forward pass's P too (asserted here)."""
    _, gbuf, prim, _, _ = bbo.render_deferred(scene(chart))
    covered = prim != bbo.NO_PRIM
    P = np.ascontiguousarray(gbuf[..., 0, :3], F)
    if chart == "steps":
        x, y = SC.pixel_xy()
        want = np.stack([x, y, quad_z()[np.where(covered, prim, 0) // 2]], -1).astype(F)
        assert covered.all() and np.array_equal(SC.bits(P), SC.bits(want)), "steps: P is not (x, y, z_q)"
        assert np.array_equal(SC.bits(bbo.half_round(P)), SC.bits(P))
    P.setflags(write=False)
    return P, covered


# ---------------------------------------------------------------------------------------------------------------------
# lights
# ---------------------------------------------------------------------------------------------------------------------
def _block(view, proj, eye):
    vu = np.zeros((), bbo.VIEW_DTYPE)
    vu["view"], vu["proj"], vu["view_pos"] = view, proj, eye
    return vu


@functools.lru_cache(None)
def views(light):
    """the light's view blocks, [F] of bbo.VIEW_DTYPE"""
    if light in ("persp", "over"):
        eye = F((0.0, 0.0, -6.0))
        one = _block(bbo.mat_look_at(eye, F((0.0, 0.0, 0.0))), bbo.mat_perspective(100.0, 1.0, 1.0, 16.0), eye)
    elif light in ("edges", "thirds"):
        eye = F((1.0 / 32.0, -1.0 / 32.0, -6.0))
        a = F(0.5) if light == "edges" else F(1.0) / F(3.0)
        p = np.zeros((4, 4), F)             # m[col][row]; half extent 1 / a, depth = 1 - view distance / 16
        p[0][0], p[1][1], p[2][2], p[3][2], p[3][3] = a, -a, -1.0 / 16.0, 1.0, 1.0
        one = _block(bbo.mat_look_at(eye, F((1.0 / 32.0, -1.0 / 32.0, 0.0))), p, eye)
    elif light == "behind":
        eye = F((0.0, 0.0, BEHIND_Z))
        one = _block(bbo.mat_look_at(eye, F((0.0, 0.0, 4.0))), bbo.mat_perspective(BEHIND_FOV, 1.0, BEHIND_NEAR, 16.0), eye)
    elif light in ("cube", "cube3"):
        out = FS.cube_views(CUBE_E, CUBE_FOV, CUBE_NEAR, CUBE_FAR)
        out = out[list(CUBE3_FACES)].copy() if light == "cube3" else out
        out.setflags(write=False)
        return out
    else:
        raise KeyError(light)
    out = np.array([one])
    out.setflags(write=False)
    return out


@functools.lru_cache(None)
def matrices(light):
    return tuple(SR.proj_view(L) for L in views(light))


@functools.lru_cache(None)
def oracle_maps(light, side):
    """[F, S, S] float32: bbo.render's depth of each of the light's frames of its chart's draws"""
    sc = scene(CHART_OF[light])
    maps = np.stack([bbo.render(bbo.Scene(sc.frame, np.array(L), sc.draws, side, side, f"{light} face {f}"), want_prim=False)[2]
                     for f, L in enumerate(views(light))])
    maps.setflags(write=False)
    return maps


def oracle_map(chart, light, side):
    """[S, S] float32: the map of a one-face light"""
    assert CHART_OF[light] == chart and len(views(light)) == 1
    return oracle_maps(light, side)[0]


def three_casters():
    """the casters of "three", dicts as tests/shadow_casters_scenes.py makes them (plus `name`, the light whose maps they hold)"""
    return tuple(dict(slot=s, light=l, views=views(name), bias=b, name=name) for s, l, name, b in THREE)


# ---------------------------------------------------------------------------------------------------------------------
# the classify step with the knobs of tests/test_shadow_chart.py: a LOCAL copy, the shipped models stay as they are
# ---------------------------------------------------------------------------------------------------------------------
KNOBS = {
    "t fused": dict(t="fused"),
    "t by division": dict(t="division"),
    "r one ulp up": dict(r_ulp=True),
    "xs unfused": dict(xs_unfused=True),
    "> 0 for >= 0": dict(low=np.greater),
    "<= S for < S": dict(high=np.less_equal),
    ">= 0 for > 0 on c.w": dict(front=np.greater_equal),
    "no test of c.w": dict(front=lambda w, zero: np.ones(w.shape, bool)),
}


def terms(M, side, bias, P, *, t="rule", r_ulp=False, xs_unfused=False):
    """(c, r, xs, ys, t) of the rule in binary32 for P[..., 3]"""
    S = int(side)
    c = SR.clip(np.asarray(M, F), P)
    with np.errstate(all="ignore"):
        r = (F(1.0) / c[..., 3]).astype(F)
        if r_ulp:
            r = np.nextafter(r, F(np.inf)).astype(F)
        h = F(F(0.5) * F(S))
        if xs_unfused:
            xs, ys = ((c[..., 0] * r).astype(F) * h + h).astype(F), ((c[..., 1] * r).astype(F) * h + h).astype(F)
        else:
            xs, ys = fmaf(c[..., 0] * r, h, h), fmaf(c[..., 1] * r, h, h)
        if t == "fused":
            tt = fmaf(c[..., 2], r, np.full(r.shape, F(bias)))
        elif t == "division":
            tt = (c[..., 2] / c[..., 3]).astype(F) + F(bias)
        else:
            tt = (c[..., 2] * r).astype(F) + F(bias)
    return c, r, xs, ys, tt


def classify(M, side, bias, P, depth_map, covered=None, *, low=np.greater_equal, high=np.less, front=np.greater, **arith):
    """shadow_reference.classify again, with the knobs the shipped model does not have (the defaults ARE the rule; a mutant's
    texel index is clamped into the map)"""
    S = int(side)
    c, r, xs, ys, t = terms(M, S, bias, P, **arith)
    with np.errstate(all="ignore"):
        inside = front(c[..., 3], F(0.0)) & low(xs, F(0.0)) & high(xs, F(S)) & low(ys, F(0.0)) & high(ys, F(S))
        i = np.clip(np.where(inside, np.trunc(np.where(inside, xs, F(0.0))), 0).astype(np.int64), 0, S - 1)
        j = np.clip(np.where(inside, np.trunc(np.where(inside, ys, F(0.0))), 0).astype(np.int64), 0, S - 1)
        dark = np.asarray(depth_map, F)[j, i] > t
    out = np.where(inside, np.where(dark, SR.SHADOWED, SR.LIT), SR.OUTSIDE).astype(np.uint8)
    return out if covered is None else np.where(covered, out, SR.NONE).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------------
def census(light, side, P=None, covered=None, bias=0.0):
    """What a chart reaches under a one-face light, counted on the covered pixels: EXACTLY where equality is meant (the rule's
    own binary32 xs, ys and c.w), in binary64 where a threshold is involved.
      xs == 0, xs == S, ys == 0, ys == S   among the pixels in front of the light
      w == 0, w < 0, w > 0
      integer   pixels inside the map whose xs AND ys are integers: (int)xs truncates nothing
      unfused   pixels in front of the light where trunc(xs) or trunc(ys) of the two-rounding form differs from the rule's
      ties      pixels inside the map whose texel is within one ulp of their own c.z * r
      lit, shadowed, outside               the model's classes at `bias`"""
    if P is None:
        P, covered = positions(CHART_OF[light])
    S = int(side)
    M, depth = matrices(light)[0], oracle_maps(light, S)[0]
    c, r, xs, ys, t0 = terms(M, S, 0.0, P)
    w = c[..., 3]
    front = covered & (w > 0)
    with np.errstate(all="ignore"):
        inside = front & (xs >= 0) & (xs < S) & (ys >= 0) & (ys < S)
        i = np.clip(np.where(inside, xs, 0).astype(np.int64), 0, S - 1)
        j = np.clip(np.where(inside, ys, 0).astype(np.int64), 0, S - 1)
        gap = np.abs(depth[j, i].astype(np.float64) - t0.astype(np.float64))
        ties = inside & (gap <= np.spacing(np.abs(t0)).astype(np.float64))
    _, _, xu, yu, _ = terms(M, S, 0.0, P, xs_unfused=True)
    unfused = front & ((np.trunc(xu) != np.trunc(xs)) | (np.trunc(yu) != np.trunc(ys)))
    cls = SR.classify(M, S, bias, P, depth, covered)
    n = lambda a: int(a.sum())
    return {"xs == 0": n(front & (xs == 0)), "xs == S": n(front & (xs == S)), "ys == 0": n(front & (ys == 0)),
            "ys == S": n(front & (ys == S)), "w == 0": n(covered & (w == 0)), "w < 0": n(covered & (w < 0)), "w > 0": n(front),
            "integer": n(inside & (xs == np.trunc(xs)) & (ys == np.trunc(ys))), "unfused": n(unfused),
            "ties": n(ties),
            "lit": n(cls == SR.LIT), "shadowed": n(cls == SR.SHADOWED), "outside": n(cls == SR.OUTSIDE)}


def mixed_quads(face, covered):
    """the number of 4 x 4 pixel quads of the fine mesh whose covered pixels have at least two different deciding faces (255,
    outside every face, is no face)"""
    f = np.where(covered & (face != FR.NO_FACE), face.astype(np.int64), -1).reshape(H // 4, 4, W // 4, 4).transpose(0, 2, 1, 3)
    f = f.reshape(-1, 16)
    hi = f.max(1)
    lo = np.where(f < 0, 99, f).min(1)
    return int(((hi >= 0) & (lo < hi)).sum())


def face_census(light, side, P=None, covered=None, bias=BIAS):
    """terrain under a light of several faces: the pixels each face decides, the pixels outside every face, the quads of mixed
    faces, and the model's classes"""
    if P is None:
        P, covered = positions(CHART_OF[light])
    cls, face = FR.classify(matrices(light), side, bias, P, oracle_maps(light, side), covered)
    n_faces = len(views(light))
    return {"per face": [int(((face == f) & covered).sum()) for f in range(n_faces)], "no face": int(((face == FR.NO_FACE) & covered).sum()),
            "mixed quads": mixed_quads(face, covered), "lit": int((cls == SR.LIT).sum()), "shadowed": int((cls == SR.SHADOWED).sum())}


def check_census(light, c):
    """the minima of a one-face light's census"""
    if light == "persp":
        assert c["ties"] >= MIN_TIES, (light, c)
    if light == "edges":
        for k in ("xs == 0", "xs == S", "ys == 0", "ys == S", "integer"):
            assert c[k] >= MIN_EQUAL, (light, k, c)
    if light == "thirds":
        assert c["integer"] >= MIN_EQUAL and c["unfused"] >= MIN_EQUAL, (light, c)
    if light == "behind":
        for k in ("w == 0", "w < 0", "w > 0"):
            assert c[k] >= MIN_EQUAL, (light, k, c)
    assert c["lit"] >= MIN_CLASS and c["shadowed"] >= MIN_CLASS, (light, c)


def check_face_census(light, c):
    assert min(c["per face"]) >= MIN_PER_FACE, (light, c)
    assert c["mixed quads"] >= MIN_MIXED_QUADS, (light, c)
    assert c["lit"] >= MIN_CLASS and c["shadowed"] >= MIN_CLASS, (light, c)
