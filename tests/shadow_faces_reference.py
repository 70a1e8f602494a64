"""CPU statement of the rule for shadow maps of up to six faces (bbr_render_shadow_faces; DESIGN.md section 3, "Faces"), on
top of tests/shadow_reference.py.  TEST INFRASTRUCTURE ONLY.  Written from the rule, not from the kernel:

  faces    F in 1 .. 6 view blocks L_0 .. L_{F-1} for ONE light index and ONE bias
  maps     map_f = shadow_reference's map for L_f (the oracle's depth of Scene(frame, L_f, draws, S, S)); in memory the maps
           follow each other, S * S texels apart
  test     for f = 0 .. F - 1 in this order: cls_f = shadow_reference.classify with M_f = proj_view(L_f) and map_f;
           the first cls_f != OUTSIDE is the class, f the face; none: OUTSIDE, face 255
  loop     unchanged: shadow_reference.lit_frame with the class

`classify` takes the rule's knobs as keyword arguments so that tests/test_shadow_faces_reference.py can turn each into a
mutant; the maps are read through one flat buffer, as the device holds them, so that a wrong stride is a wrong texel."""
from __future__ import annotations

import numpy as np

import shadow_reference as SR

F32 = np.float32
NO_FACE = 255
NONE, LIT, SHADOWED, OUTSIDE = SR.NONE, SR.LIT, SR.SHADOWED, SR.OUTSIDE


def per_face(Ms, side, bias, P, maps):
    """[F, ...] uint8: cls_f of every P for every face, each alone"""
    return np.stack([SR.classify(M, side, bias, P, m) for M, m in zip(Ms, maps)])


def classify(Ms, side, bias, P, maps, covered=None, *, last_wins=False, stop_at_outside=False, stride=None,
             map_of=lambda f, n: f, matrix_of=lambda f: f):
    """array form: (class, face) of every P[..., 3], both uint8; `covered` False gives (NONE, 255).  The keyword arguments are
    the rule's knobs (the defaults ARE the rule)."""
    S, n = int(side), len(Ms)
    flat = np.ascontiguousarray(maps, F32).reshape(-1)
    assert flat.size == n * S * S
    stride = S * S if stride is None else int(stride)
    shape = np.shape(P)[:-1]
    cls, face = np.full(shape, OUTSIDE, np.uint8), np.full(shape, NO_FACE, np.uint8)
    searching = np.ones(shape, bool)
    for f in range(n):
        at = map_of(f, n) * stride
        cf = SR.classify(Ms[matrix_of(f)], S, bias, P, flat[at:at + S * S].reshape(S, S))
        take = (cf != OUTSIDE) & (True if last_wins else searching)
        cls, face = np.where(take, cf, cls).astype(np.uint8), np.where(take, f, face).astype(np.uint8)
        searching = searching & ~take
        if stop_at_outside:
            searching = searching & (cf != OUTSIDE)
    if covered is not None:
        cls, face = np.where(covered, cls, NONE).astype(np.uint8), np.where(covered, face, NO_FACE).astype(np.uint8)
    return cls, face


def classify_point(Ms, side, bias, P, maps):
    """single-point form, statement by statement: (class, face)"""
    for f in range(len(Ms)):
        c = SR.classify_point(Ms[f], side, bias, P, maps[f])
        if c != OUTSIDE:
            return c, f
    return OUTSIDE, NO_FACE


MUTANTS = {
    "the last face wins": dict(last_wins=True),
    "the search stops at the first OUTSIDE": dict(stop_at_outside=True),
    "the face stride is S": "stride",      # (needs S: classify(..., stride=S))
    "face f reads map (f + 1) mod F": dict(map_of=lambda f, n: (f + 1) % n),
    "M_f is face 0's": dict(matrix_of=lambda f: 0),
}


def mutant(name, side):
    k = MUTANTS[name]
    return dict(stride=int(side)) if k == "stride" else k
