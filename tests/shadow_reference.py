"""CPU statement of the shadow rule (option "shadow_map"), in numpy binary32.  TEST INFRASTRUCTURE ONLY.

Written from the rule, not from the kernel; fmaf is aniso_reference.fmaf (one rounding), every other operation is a binary32
operation of numpy (one rounding each, no contraction).

  map      texel (i, j) = the depth bbo.render returns for pixel (i, j) of Scene(frame, L, draws, S, S): the recorded draws
           under gl_Position = (L.proj L.view) posWorld with the frame's own fixed-function state.  Nothing is modelled here:
           the oracle IS the map (shadow_scenes.oracle_map).
  M        proj_view(L): column j of M is proj applied to column j of view, M[j][i] = fmaf(p[3][i], v[j][3], fmaf(p[2][i],
           v[j][2], fmaf(p[1][i], v[j][1], p[0][i] * v[j][0])))   (m[col][row], as the blocks store them)
  test     on the position P the light loop receives (the deferred pass: P after the binary16 rounding of its G-buffer):
             c = M (P, 1), each row i as fmaf(M[3][i], 1, fmaf(M[2][i], P.z, fmaf(M[1][i], P.y, M[0][i] * P.x)))
             !(c.w > 0)                                      -> OUTSIDE
             r = 1 / c.w correctly rounded;  h = 0.5f * S
             xs = fmaf(c.x * r, h, h);  ys = fmaf(c.y * r, h, h)
             !(xs >= 0 && xs < S && ys >= 0 && ys < S)       -> OUTSIDE   (NaN lands here)
             i = (int)xs;  j = (int)ys;  t = c.z * r + bias
             map[j][i] > t                                   -> SHADOWED  (a NaN t is not shadowed)
             otherwise                                       -> LIT
  classes  0 not covered, 1 LIT, 2 SHADOWED, 3 OUTSIDE
  loop     the caster's iteration of a SHADOWED fragment contributes nothing -- exactly what the light loop does for a light
           of unknown type: the lit frame is bbo.light_surface per pixel, with the caster's `type` set to an unknown value
           where the pixel is SHADOWED.

`classify` takes the rule's knobs as keyword arguments so that tests/test_shadow_reference.py can turn each into a mutant."""
from __future__ import annotations

import numpy as np

from aniso_reference import fmaf
from oracle import bbo

F = np.float32
NONE, LIT, SHADOWED, OUTSIDE = 0, 1, 2, 3
UNKNOWN_TYPE = 5


def proj_view(view_block):
    """M[col][row] of the light's view block, in the vertex stage's fma chain"""
    v, p = np.asarray(view_block["view"], F), np.asarray(view_block["proj"], F)
    m = np.zeros((4, 4), F)
    for c in range(4):      # (row i of column c, all four rows at once)
        m[c] = fmaf(p[3], v[c][3], fmaf(p[2], v[c][2], fmaf(p[1], v[c][1], p[0] * v[c][0])))
    return m


def clip(M, P):
    """c = M (P, 1) for P[..., 3]: [..., 4]"""
    P = np.asarray(P, F)
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(all="ignore"):
        return np.stack([fmaf(M[3][i], F(1.0), fmaf(M[2][i], z, fmaf(M[1][i], y, M[0][i] * x))) for i in range(4)], -1)


def classify(M, side, bias, P, depth_map, covered=None, *, shadowed=np.greater, to_int=np.trunc, h_offset=0.0, bias_sign=1.0):
    """array form: the class of every P[..., 3] (uint8); `covered` False gives NONE.  The keyword arguments are the rule's knobs
    (the defaults ARE the rule)."""
    M = np.asarray(M, F)
    depth_map = np.asarray(depth_map, F)
    S = int(side)
    c = clip(M, P)
    with np.errstate(all="ignore"):
        front = c[..., 3] > F(0.0)
        r = (F(1.0) / c[..., 3]).astype(F)
        h = F(F(0.5) * F(S) + F(h_offset))
        xs, ys = fmaf(c[..., 0] * r, h, h), fmaf(c[..., 1] * r, h, h)
        inside = front & (xs >= F(0.0)) & (xs < F(S)) & (ys >= F(0.0)) & (ys < F(S))
        i = np.where(inside, to_int(np.where(inside, xs, F(0.0))), 0).astype(np.int64)
        j = np.where(inside, to_int(np.where(inside, ys, F(0.0))), 0).astype(np.int64)
        i, j = np.clip(i, 0, S - 1), np.clip(j, 0, S - 1)       # (a mutant's rint may leave the map; the rule cannot)
        t = (c[..., 2] * r).astype(F) + F(F(bias) * F(bias_sign))
        dark = shadowed(depth_map[j, i], t)
    out = np.where(inside, np.where(dark, SHADOWED, LIT), OUTSIDE).astype(np.uint8)
    if covered is not None:
        out = np.where(covered, out, NONE).astype(np.uint8)
    return out


def classify_point(M, side, bias, P, depth_map):
    """single-point form, statement by statement"""
    M = np.asarray(M, F)
    x, y, z = (F(v) for v in P)
    fma = lambda a, b, c: F(fmaf(a, b, c).reshape(-1)[0])     # (the scalar of a one-element array)
    c = [fma(M[3][i], F(1.0), fma(M[2][i], z, fma(M[1][i], y, F(M[0][i] * x)))) for i in range(4)]
    if not c[3] > F(0.0):
        return OUTSIDE
    with np.errstate(all="ignore"):
        r = F(F(1.0) / c[3])
        S = F(side)
        h = F(F(0.5) * S)
        xs, ys = fma(F(c[0] * r), h, h), fma(F(c[1] * r), h, h)
        if not (xs >= F(0.0) and xs < S and ys >= F(0.0) and ys < S):
            return OUTSIDE
        i, j = int(xs), int(ys)
        t = F(F(c[2] * r) + F(bias))
    return SHADOWED if depth_map[j][i] > t else LIT


def lit_frame(frame, view, surf, mask, caster):
    """the light loop on surf[n, 12] with the caster switched off where mask says SHADOWED: [n, 4] float32.  `caster` beyond
    the frame's lights shadows nothing."""
    surf = np.ascontiguousarray(surf, F).reshape(-1, 12)
    mask = np.asarray(mask).reshape(-1)
    out = bbo.light_surface(frame, view, surf, literal=False)
    dark = np.flatnonzero(mask == SHADOWED)
    if len(dark) and 0 <= caster < int(frame["num_lights"]):
        off = frame.copy()
        off["lights"][caster]["type"] = UNKNOWN_TYPE
        out[dark] = bbo.light_surface(off, view, surf[dark], literal=False)
    return out
