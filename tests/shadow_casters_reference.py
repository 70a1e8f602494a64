"""CPU statement of the rule for up to eight shadow casters per context (bbr_render_shadow_caster; DESIGN.md section 3,
"Casters"), on top of tests/shadow_filter_reference.py.  TEST INFRASTRUCTURE ONLY.  Written from the rule, not from the kernel.

  slots    a context has 8 caster slots.  A slot in use holds a light index, F = 1 .. 6 view blocks, their F maps of S x S and a
           bias; S and R are the context's
  test     for every slot in use, independently of the others: (class_s, face_s, k_s) = shadow_filter_reference.taps (R >= 1) or
           .hard (R = 0: K = 1, k = 1 where LIT, 0 where SHADOWED) with that slot's matrices, maps and bias, on the P the light
           loop receives.  Slots do not see each other
  loop     iteration li looks for the slot in use whose light index is li (at most one).  None, or class OUTSIDE, or k = K:
           untouched.  k = 0: the iteration contributes nothing -- the light's `type` set unknown.  0 < k < K: the light's
           `intensity` replaced by the binary32 product intensity * ((float)k * RK[K]).  A slot whose light index is >=
           NumLights changes nothing.  bb_oracle.c cooks color * intensity once per light, so a pixel IS bbo.light_surface on
           a frame whose casters' lights are changed so: the pixels are grouped by their tuple (k_0 .. k_7), one frame each

A caster is a dict(slot, light, views, bias) as tests/shadow_casters_scenes.py makes them.  `verdicts` and `lit_frame` take the
rule's knobs as keyword arguments so that tests/test_shadow_casters_reference.py can turn each into a mutant (the defaults ARE
the rule)."""
from __future__ import annotations

import numpy as np

import shadow_filter_reference as PR
import shadow_reference as SR
from oracle import bbo

F = np.float32
NONE, LIT, SHADOWED, OUTSIDE, PARTIAL = PR.NONE, PR.LIT, PR.SHADOWED, PR.OUTSIDE, PR.PARTIAL
NO_FACE = NO_TAPS = 255
MAX_CASTERS = 8


def slot_verdict(Ms, side, bias, P, maps, radius, covered=None):
    """(class, k, face) of one slot, all uint8 of P's shape: 255 for k and face where the class is NONE or OUTSIDE"""
    if int(radius) == 0:
        cls, face = PR.hard(Ms, side, bias, P, maps, covered)
        k = np.where(cls == LIT, 1, np.where(cls == SHADOWED, 0, NO_TAPS)).astype(np.uint8)
        return cls, k, face
    return PR.taps(Ms, side, bias, P, maps, radius, covered)


def verdicts(casters, side, radius, P, maps_of, covered=None, *, bias_of=lambda c, first: c["bias"], maps_from=lambda c, first: c):
    """slot -> (class, k, face).  `maps_of(caster)` gives the caster's [F, S, S] maps.  The knobs: `bias_of(caster, first)` is the
    bias a caster is tested with, `maps_from(caster, first)` the caster whose maps it reads (its first F of them); `first` is
    the caster of the lowest slot"""
    first = min(casters, key=lambda c: c["slot"])
    out = {}
    for c in casters:
        Ms = [SR.proj_view(L) for L in c["views"]]
        maps = np.asarray(maps_of(maps_from(c, first)))
        if len(maps) < len(Ms):     # (a mutant's: fewer maps than faces; the last one again)
            maps = np.concatenate([maps, np.repeat(maps[-1:], len(Ms) - len(maps), 0)])
        out[c["slot"]] = slot_verdict(Ms, side, bias_of(c, first), P, maps[:len(Ms)], radius, covered)
    return out


def lit_frame(frame, view, surf, ks, light_of, radius, *, verdict_of=lambda s, first: s, first_dark_only=False, scales_multiplied=False):
    """the light loop on surf[n, 12] under the counts ks[slot][n] (255: that caster's light untouched) of the casters on lights
    light_of[slot]: [n, 4] float32.  The knobs: `verdict_of(slot, first)` is the slot whose k a caster's light is treated by;
    first_dark_only lets only the first caster (in slot order) with k = 0 drop its iteration; scales_multiplied gives every
    partly lit caster's light the product of all partial v."""
    surf = np.ascontiguousarray(surf, F).reshape(-1, 12)
    K = PR.taps_of(radius)
    slots = sorted(ks)
    n_lights = int(frame["num_lights"])
    out = bbo.light_surface(frame, view, surf, literal=False)
    if not slots:
        return out
    first = slots[0]
    table = np.stack([np.asarray(ks[verdict_of(s, first)]).reshape(-1) for s in slots], -1)       # [n, slots]
    tuples, where = np.unique(table, axis=0, return_inverse=True)
    where = where.reshape(-1)
    for t, counts in enumerate(tuples):
        acts = [(s, int(k)) for s, k in zip(slots, counts) if 0 <= light_of[s] < n_lights and int(k) != NO_TAPS and int(k) != K]
        if not acts:
            continue
        other = frame.copy()
        dark_seen = False
        with np.errstate(all="ignore"):
            all_v = F(1.0)
            for s, k in acts:
                if k:
                    all_v = F(all_v * F(F(k) * PR.RK[K]))
            for s, k in acts:
                light = other["lights"][light_of[s]]
                if k == 0:
                    if not (first_dark_only and dark_seen):
                        light["type"] = SR.UNKNOWN_TYPE
                    dark_seen = True
                else:
                    light["intensity"] = F(light["intensity"] * (all_v if scales_multiplied else F(F(k) * PR.RK[K])))
        at = np.flatnonzero(where == t)
        out[at] = bbo.light_surface(other, view, surf[at], literal=False)
    return out


# what tests/test_shadow_casters_reference.py turns the knobs to
VERDICT_MUTANTS = {
    "slot 0's bias used for all": dict(bias_of=lambda c, first: first["bias"]),
    "slot 0's maps used for all": dict(maps_from=lambda c, first: first),
}
LOOP_MUTANTS = {
    "slot 0's verdict applied to every caster's light": dict(verdict_of=lambda s, first: first),
    "only the first shadowed caster skipped": dict(first_dark_only=True),
    "all partial scales multiplied into each": dict(scales_multiplied=True),
}
