"""Scenes for up to eight shadow casters per context (bbr_render_shadow_caster; DESIGN.md section 3, "Casters"), on top of
tests/shadow_faces_scenes.py's "cube" draws: its camera (the surface chart's), receiver, wall and occluders, and the four-light
list.  TEST INFRASTRUCTURE ONLY; no test lives here.

The draws are "cube"'s two and a third: one block (BLOCKS) 0.75 in front of the receiver, placed where the spot view and both
cascade faces see it and sized until the oracle alone met the census below -- without it the spot and the cascade shadow 2 % of
the covered pixels each.

  "mixed"  three casters in slots 0, 1 and 5 (a gap, and a slot past 3):
             slot 0  light 2 through the six 96-degree cube faces at shadow_faces_scenes.E
             slot 1  light 0 through shadow_scenes' spot view, one face
             slot 5  light 3 through the two nested orthographic faces of "cascade"
  "eight"  eight lights (the four, and four more point lights), each a one-face caster with a view of its own: the spot view
           with its eye moved off the receiver's normal and turned about that normal in eight steps of 45 degrees, looking at
           the spot's target.  Slots 0 .. 7; slot s holds light (3 s) mod 8, so that no slot index is its light index

A caster is a dict: slot, light, views ([F] of bbo.VIEW_DTYPE), bias.  The views need not be where the lights are: a caster is
a light INDEX and a list of views, and the rule knows nothing else."""
from __future__ import annotations

import functools

import numpy as np

import shadow_faces_scenes as FS
import shadow_reference as SR
import shadow_scenes as SS
import surface_chart as SC
from oracle import bbo

KINDS = ("mixed", "eight")
MAX_CASTERS = 8
FRAME_SMALL, FRAME_DUMP = SS.FRAME_SMALL, SS.FRAME_DUMP
SIDES = (33, 64, 200)
BIAS = SS.BIAS
# x0, x1, y0, y1, dz of the blocks this module adds in front of the receiver, where the spot and the cascade both see them
BLOCKS = ((1.0, 2.4, -2.2, 0.2, 0.75),)
EIGHT_OFFSET = 1.0                       # "eight": the eye's distance from the receiver's normal through the target
# the census (conditions, not measurements)
MIN_SHARE, MIN_BOTH, MIN_PAIR, MIN_PARTIAL_BOTH, MIN_EIGHT = 0.05, 64, 64, 64, 32
PARTIAL_SIDE_MAX = 64

f32 = SC.f32


def _eight_views():
    n = SS.NORMAL / np.sqrt((SS.NORMAL * SS.NORMAL).sum())
    u = np.cross(n, (0.0, 1.0, 0.0))
    u /= np.sqrt((u * u).sum())
    v = np.cross(n, u)
    out = np.zeros(8, bbo.VIEW_DTYPE)
    for k in range(8):
        a = 2.0 * np.pi * k / 8.0
        eye = np.asarray(SS.SPOT_TARGET) + 1.5 * n + EIGHT_OFFSET * (np.cos(a) * u + np.sin(a) * v)
        out[k]["view"] = bbo.mat_look_at(f32(eye), f32(SS.SPOT_TARGET))
        out[k]["proj"] = bbo.mat_perspective(SS.SPOT_FOV, 1.0, SS.NEAR, SS.FAR)
        out[k]["view_pos"] = f32(eye)
    return out


@functools.lru_cache(None)
def casters(kind):
    """the casters of `kind`, a tuple of dicts in slot order"""
    if kind == "mixed":
        return (dict(slot=0, light=2, views=FS.faces("cube"), bias=BIAS),
                dict(slot=1, light=0, views=np.array([SS.light_view("spot")]), bias=BIAS),
                dict(slot=5, light=3, views=FS.faces("cascade"), bias=BIAS))
    views = _eight_views()
    return tuple(dict(slot=s, light=(3 * s) % 8, views=views[s:s + 1], bias=BIAS) for s in range(8))


def lights(kind):
    a, view_pos = FS.lights("cube")
    if kind == "eight":
        a = a + [SC.L(0, pos=(4.0, -6.0, -5.5), color=(0.4, 0.9, 0.5), intensity=120.0),
                 SC.L(0, pos=(-3.0, 8.0, -6.0), color=(0.8, 0.8, 0.3), intensity=140.0),
                 SC.L(0, pos=(7.0, -2.0, -7.0), color=(0.5, 0.4, 1.0), intensity=150.0),
                 SC.L(0, pos=(-6.0, 1.0, -5.0), color=(1.0, 0.5, 0.7), intensity=100.0)]
    return a, view_pos


@functools.lru_cache(None)
def _draws():
    """"cube"'s two draws and a third: the blocks of BLOCKS, parallel to the receiver like the occluders there"""
    recv, occ = FS._draws("cube")
    quads = np.concatenate([SS._quad(x0, x1, y0, y1, dz) for x0, x1, y0, y1, dz in BLOCKS])
    idx = np.concatenate([SC.QUAD_INDEX + 4 * k for k in range(len(BLOCKS))]).astype(np.uint32)
    return (recv, occ, bbo.DrawData(quads, idx, recv.instances, recv.material))


def scene(kind, size=FRAME_SMALL):
    ls, view_pos = lights(kind)
    fu, vu = SC.uniforms(ls, view_pos, 1.0, 1)
    return bbo.Scene(fu, vu, list(_draws()), size[0], size[1], f"shadow casters {kind}")


@functools.lru_cache(None)
def oracle_maps(kind, slot, side):
    """[F, S, S] float32: bbo.render's depth of each of the slot's faces"""
    sc = scene(kind)
    views = next(c for c in casters(kind) if c["slot"] == slot)["views"]
    maps = np.stack([bbo.render(bbo.Scene(sc.frame, np.array(L), sc.draws, side, side, f"slot {slot} face {f}"), want_prim=False)[2]
                     for f, L in enumerate(views)])
    maps.setflags(write=False)
    return maps


@functools.lru_cache(None)
def matrices(kind, slot):
    return tuple(SR.proj_view(L) for L in next(c for c in casters(kind) if c["slot"] == slot)["views"])


def positions64(kind, size=FRAME_SMALL):
    """([h, w, 3] binary64 world positions of the camera's pixels, [h, w] bool covered): shadow_faces_scenes.positions64 for these draws (both kinds
    have the same draws and the same camera)"""
    return _positions64(tuple(size))


@functools.lru_cache(None)
def _positions64(size):
    sc = scene("mixed", size)
    prim = bbo.render(sc, want_depth=False)[1]
    tris = np.concatenate([d.vertices["pos"][d.indices.reshape(-1, 3)].astype(np.float64) for d in sc.draws])
    covered = prim != bbo.NO_PRIM
    p = tris[np.where(covered, prim, 0)]
    x, y = SS.pixel_xy64(size)
    nrm = np.cross(p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :])
    z = p[..., 0, 2] - (nrm[..., 0] * (x - p[..., 0, 0]) + nrm[..., 1] * (y - p[..., 0, 1])) / nrm[..., 2]
    P = np.stack([x, y, z], -1)
    P.setflags(write=False)
    return P, covered


# ---------------------------------------------------------------------------------------------------------------------
# census, in binary64 on the oracle's maps, a factor 2 clear of each threshold
# ---------------------------------------------------------------------------------------------------------------------
def clear_classes(views, side, bias, P, maps, radius=0):
    """(lit, shadowed, partial) bool [h, w] of one caster on positions P[h, w, 3] in binary64: True only where the class is a
    factor 2 clear of every threshold that decides it.
      face     a face decides where the fragment is at least one texel inside it (and 2^-8 texel away from a texel edge) and at
               least one texel outside every earlier face (or behind it)
      tap      clearly dark: the texel lies more than 2 |bias| above the fragment's depth; clearly lit: less than |bias| / 2
      classes  shadowed: every tap of the window clearly dark; lit: every tap clearly lit; partial: all taps clear, both kinds"""
    S, R = int(side), int(radius)
    P = np.asarray(P, np.float64)
    shape = P.shape[:-1]
    lit, shadowed, partial = (np.zeros(shape, bool) for _ in range(3))
    open_ = np.ones(shape, bool)                 # every earlier face is clearly outside
    hom = np.concatenate([P, np.ones(shape + (1,))], -1)
    for f, L in enumerate(views):
        M = L["proj"].astype(np.float64).T @ L["view"].astype(np.float64).T      # (the blocks store m[col][row])
        c = hom @ M.T
        with np.errstate(all="ignore"):
            w = c[..., 3]
            xs, ys, z = (c[..., 0] / w * 0.5 + 0.5) * S, (c[..., 1] / w * 0.5 + 0.5) * S, c[..., 2] / w
            out = (w <= 0) | (xs <= -1) | (xs >= S + 1) | (ys <= -1) | (ys >= S + 1)
            edge = lambda a: np.abs(a - np.rint(a)) >= 2.0 ** -8
            inside = (w > 0) & (xs >= 1) & (xs <= S - 1) & (ys >= 1) & (ys <= S - 1) & edge(xs) & edge(ys)
            i = np.where(inside, xs, 0).astype(np.int64)
            j = np.where(inside, ys, 0).astype(np.int64)
            dark, bright, clear = np.ones(shape, bool), np.ones(shape, bool), np.ones(shape, bool)
            for dj in range(-R, R + 1):
                for di in range(-R, R + 1):
                    gap = maps[f][np.clip(j + dj, 0, S - 1), np.clip(i + di, 0, S - 1)].astype(np.float64) - z
                    d, b = gap > 2 * abs(bias), gap < abs(bias) / 2
                    dark, bright, clear = dark & d, bright & b, clear & (d | b)
        here = open_ & inside
        shadowed |= here & dark
        lit |= here & bright
        partial |= here & clear & ~dark & ~bright
        open_ &= out
    return lit, shadowed, partial


def census(kind, side, size=FRAME_SMALL, masks=None, P=None):
    """the counts the conditions are about.  `masks` (slot -> the classes somebody computed): a clear pixel must carry its class
    too.  `P`: the positions to judge instead of the closed-form ones (the device's dump)."""
    P64, covered = positions64(kind, size)
    P = P64 if P is None else np.asarray(P, np.float64)
    cs = casters(kind)
    lit, dark, part = {}, {}, {}
    for c in cs:
        s = c["slot"]
        lit[s], dark[s], _ = clear_classes(c["views"], side, c["bias"], P, oracle_maps(kind, s, side))
        _, _, part[s] = clear_classes(c["views"], side, c["bias"], P, oracle_maps(kind, s, side), 1)
        lit[s], dark[s], part[s] = lit[s] & covered, dark[s] & covered, part[s] & covered
        if masks is not None:
            lit[s], dark[s] = lit[s] & (masks[s] == SR.LIT), dark[s] & (masks[s] == SR.SHADOWED)
    n = max(int(covered.sum()), 1)
    slots = [c["slot"] for c in cs]
    return {"lit": {s: float(lit[s].sum()) / n for s in slots},
            "shadowed": {s: float(dark[s].sum()) / n for s in slots},
            "shadowed_count": {s: int(dark[s].sum()) for s in slots},
            "both_shadowed": int((sum(dark[s].astype(int) for s in slots) >= 2).sum()),
            "pair": {f"{s}>{t}": int((dark[s] & lit[t]).sum()) for s in slots for t in slots if s != t},
            "both_partial": int((sum(part[s].astype(int) for s in slots) >= 2).sum())}


def check_census(kind, c, side, what=""):
    """the conditions.  The one on PARTIAL pixels is judged at S <= PARTIAL_SIDE_MAX: a window of S = 200 is narrower than a pixel
    of the small frame, and what is PARTIAL there in two slots at once is a handful of pixels whatever the scene"""
    if kind == "eight":
        assert min(c["shadowed_count"].values()) >= MIN_EIGHT, (what, c)
        return
    assert min(c["lit"].values()) >= MIN_SHARE and min(c["shadowed"].values()) >= MIN_SHARE, (what, c)
    assert c["both_shadowed"] >= MIN_BOTH, (what, c)
    assert min(c["pair"].values()) >= MIN_PAIR, (what, c)
    assert side > PARTIAL_SIDE_MAX or c["both_partial"] >= MIN_PARTIAL_BOTH, (what, c)
