"""CPU statement of the rule for percentage-closer shadow filtering (option "shadow_filter" = R in 0 .. 2; DESIGN.md section 3,
"Filtering"), on top of tests/shadow_reference.py and tests/shadow_faces_reference.py.  TEST INFRASTRUCTURE ONLY.  Written from
the rule, not from the kernel; every operation is a binary32 operation of numpy (one rounding each, no contraction), fmaf is
aniso_reference.fmaf.

  face, i, j, t   the hard rule's (shadow_reference, shadow_faces_reference): the deciding face f is the first face the fragment
           is not OUTSIDE of; i, j and t = c.z * r + bias on the P the light loop receives.  OUTSIDE and "not covered" are
           decided before any tap is read
  taps     K = (2R + 1)^2.  for dj = -R .. R, di = -R .. R: tap (di, dj) reads map_f[clamp(j + dj, 0, S - 1)][clamp(i + di, 0,
           S - 1)] and is lit iff !(texel > t) (a NaN t: every tap is lit).  k = the number of lit taps.  Taps never leave the
           deciding face's map
  classes  0 not covered, 1 LIT (k = K), 2 SHADOWED (k = 0), 3 OUTSIDE, 4 PARTIAL (0 < k < K)
  loop     k = K: untouched.  k = 0: the caster's iteration contributes nothing.  0 < k < K: the light loop with the caster's
           `intensity` replaced by the binary32 product intensity * v, v = (float)k * RK, RK[K] the binary32 nearest 1 / K.
           bb_oracle.c's contract form cooks color * intensity once per light, so a pixel with count k IS bbo.light_surface on
           a frame whose caster has that intensity: at most K - 1 frames.  A caster beyond the frame's lights changes nothing.

`taps` and `lit_frame` take the rule's knobs as keyword arguments so that tests/test_shadow_filter_reference.py can turn each
into a mutant (the defaults ARE the rule); the maps are read through one flat buffer, as the device holds them."""
from __future__ import annotations

import numpy as np

import shadow_faces_reference as FR
import shadow_reference as SR
from aniso_reference import fmaf
from oracle import bbo

F = np.float32
NONE, LIT, SHADOWED, OUTSIDE, PARTIAL = SR.NONE, SR.LIT, SR.SHADOWED, SR.OUTSIDE, 4
NO_FACE = NO_TAPS = 255
RK = {1: F(1.0), 9: F(1.0) / F(9.0), 25: F(1.0) / F(25.0)}      # (a correctly rounded quotient: the binary32 nearest 1 / K)
assert RK[9].view(np.uint32) == 0x3DE38E39 and RK[25].view(np.uint32) == 0x3D23D70A


def taps_of(radius):
    return (2 * int(radius) + 1) ** 2


def texel(M, side, bias, P):
    """(inside, i, j, t) of every P[..., 3]: the hard rule's statements up to the compare"""
    M = np.asarray(M, F)
    S = int(side)
    c = SR.clip(M, P)
    with np.errstate(all="ignore"):
        front = c[..., 3] > F(0.0)
        r = (F(1.0) / c[..., 3]).astype(F)
        h = F(F(0.5) * F(S))
        xs, ys = fmaf(c[..., 0] * r, h, h), fmaf(c[..., 1] * r, h, h)
        inside = front & (xs >= F(0.0)) & (xs < F(S)) & (ys >= F(0.0)) & (ys < F(S))
        i = np.where(inside, np.trunc(np.where(inside, xs, F(0.0))), 0).astype(np.int64)
        j = np.where(inside, np.trunc(np.where(inside, ys, F(0.0))), 0).astype(np.int64)
        t = (c[..., 2] * r).astype(F) + F(bias)
    return inside, i, j, t


def _not_greater(a, t):
    return ~(a > t)


def taps(Ms, side, bias, P, maps, radius, covered=None, *, wrap=False, out_of_map=None, shift=(0, 0), lit=_not_greater,
         map_of=lambda f: f, clamp_high=True):
    """array form: (class, k, face) of every P[..., 3], all uint8; `covered` False gives (NONE, 255, 255).  Ms and maps hold
    F >= 1 faces.  The knobs: `wrap` addresses modulo S instead of clamping; `out_of_map` "lit" / "dark" counts a tap outside
    [0, S)^2 so instead of reading the clamped texel; `shift` moves the window; `lit` is the compare; `map_of(f)` is the map the
    taps of face f read; clamp_high False leaves the upper clamp out, so that an address runs on into the next row and the next
    face's memory (zeros behind the last face)."""
    S, R, n_faces = int(side), int(radius), len(Ms)
    K = taps_of(R)
    pad = np.zeros((R + 2) * (S + 1), F)
    flat = np.concatenate([np.ascontiguousarray(maps, F).reshape(-1), pad])
    assert flat.size == n_faces * S * S + pad.size
    shape = np.shape(P)[:-1]
    cls, k, face = np.full(shape, OUTSIDE, np.uint8), np.full(shape, NO_TAPS, np.uint8), np.full(shape, NO_FACE, np.uint8)
    searching = np.ones(shape, bool)
    for f in range(n_faces):
        inside, i, j, t = texel(Ms[f], S, bias, P)
        take = inside & searching
        base = map_of(f) * S * S
        n = np.zeros(shape, np.int64)
        for dj in range(-R, R + 1):
            for di in range(-R, R + 1):
                ii, jj = i + di + shift[0], j + dj + shift[1]
                beyond = (ii < 0) | (ii >= S) | (jj < 0) | (jj >= S)
                if wrap:
                    ii, jj = ii % S, jj % S
                else:
                    ii, jj = np.maximum(ii, 0), np.maximum(jj, 0)
                    if clamp_high:
                        ii, jj = np.minimum(ii, S - 1), np.minimum(jj, S - 1)
                with np.errstate(all="ignore"):
                    on = lit(flat[base + jj * S + ii], t)
                if out_of_map is not None:
                    on = np.where(beyond, out_of_map == "lit", on)
                n += on
        c = np.where(n == K, LIT, np.where(n == 0, SHADOWED, PARTIAL))
        cls, k, face = (np.where(take, v, old).astype(np.uint8) for v, old in ((c, cls), (n, k), (f, face)))
        searching = searching & ~take
    if covered is not None:
        cls = np.where(covered, cls, NONE).astype(np.uint8)
        k, face = np.where(covered, k, NO_TAPS).astype(np.uint8), np.where(covered, face, NO_FACE).astype(np.uint8)
    return cls, k, face


def taps_point(Ms, side, bias, P, maps, radius):
    """single-point form, statement by statement: (class, k, face)"""
    S, R = int(side), int(radius)
    x, y, z = (F(v) for v in P)
    fma = lambda a, b, c: F(fmaf(a, b, c).reshape(-1)[0])     # (the scalar of a one-element array)
    for f in range(len(Ms)):
        M = np.asarray(Ms[f], F)
        c = [fma(M[3][q], F(1.0), fma(M[2][q], z, fma(M[1][q], y, F(M[0][q] * x)))) for q in range(4)]
        if not c[3] > F(0.0):
            continue
        with np.errstate(all="ignore"):
            r = F(F(1.0) / c[3])
            h = F(F(0.5) * F(S))
            xs, ys = fma(F(c[0] * r), h, h), fma(F(c[1] * r), h, h)
            if not (xs >= F(0.0) and xs < F(S) and ys >= F(0.0) and ys < F(S)):
                continue
            i, j = int(xs), int(ys)
            t = F(F(c[2] * r) + F(bias))
        k = 0
        for dj in range(-R, R + 1):
            for di in range(-R, R + 1):
                if not maps[f][min(max(j + dj, 0), S - 1)][min(max(i + di, 0), S - 1)] > t:
                    k += 1
        K = taps_of(R)
        return (LIT if k == K else SHADOWED if k == 0 else PARTIAL), k, f
    return OUTSIDE, NO_TAPS, NO_FACE


def _product(k, K):
    return F(F(k) * RK[K])


def lit_frame(frame, view, surf, k, caster, radius, *, v_of=_product, colour_after=False, scale_full=False):
    """the light loop on surf[n, 12] under the counts k[n] (255: the caster untouched): [n, 4] float32, pixels grouped by k, each
    group bbo.light_surface on a frame of its own.  The knobs: `v_of(k, K)` is v; colour_after scales the cooked colour,
    (color * intensity) * v, instead of the intensity; scale_full runs k = K through the scaling too."""
    surf = np.ascontiguousarray(surf, F).reshape(-1, 12)
    k = np.asarray(k).reshape(-1)
    K = taps_of(radius)
    out = bbo.light_surface(frame, view, surf, literal=False)
    if not 0 <= caster < int(frame["num_lights"]):
        return out
    for count in range(0, K + 1 if scale_full else K):
        at = np.flatnonzero(k == count)
        if not len(at):
            continue
        other = frame.copy()
        light = other["lights"][caster]
        if count == 0:
            light["type"] = SR.UNKNOWN_TYPE
        elif colour_after:
            with np.errstate(all="ignore"):
                light["color"] = (light["color"] * light["intensity"]).astype(F) * v_of(count, K)
            light["intensity"] = F(1.0)
        else:
            with np.errstate(all="ignore"):
                light["intensity"] = F(light["intensity"] * v_of(count, K))
        out[at] = bbo.light_surface(other, view, surf[at], literal=False)
    return out


def hard(Ms, side, bias, P, maps, covered=None):
    """the hard rule's (class, face) through the two existing reference modules"""
    return FR.classify(Ms, side, bias, P, maps, covered)


# what tests/test_shadow_filter_reference.py turns the knobs to
TAP_MUTANTS = {
    "wrap instead of clamp": dict(wrap=True),
    "an out-of-map tap counted lit": dict(out_of_map="lit"),
    "an out-of-map tap counted dark": dict(out_of_map="dark"),
    "the window shifted by (+1, +1)": dict(shift=(1, 1)),
}
FACE_MUTANTS = {
    "taps read face 0's map": dict(map_of=lambda f: 0),
    "taps may cross into the next face's memory": dict(clamp_high=False),
}
LOOP_MUTANTS = {
    "v the correctly rounded quotient k / K": dict(v_of=lambda k, K: F(F(k) / F(K))),
    "(color * intensity) * v": dict(colour_after=True),
    "k = K scaled instead of untouched": dict(scale_full=True),
}
