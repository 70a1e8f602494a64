"""An ideal rasteriser for the fixed-function triangle stage, written from the Vulkan model DESIGN.md sections 2 / 3 name
and NOT from oracle/bb_oracle.c: no clipper, no snapping, no per-triangle binary32 planes, no fan.

From the oracle it takes what other tests already pin: bbo.vertex_stage (binary32 clip position + varyings) and the scene
containers.  From those binary32 clip coordinates on, every quantity is exact (Python integers):

  rows r_i = (x_i, y_i, w_i) of the three ORIGINAL vertices, M = [r_0; r_1; r_2], adj(M) column i = r_(i+1) x r_(i+2).
  For a screen point p = (X, Y, 1) in NDC:  e_i(p) = p . adj(M)[:, i] = det(M) * b_i / w   (b = barycentrics in clip space),
  so  1/w = sum e_i / det,  z/w = sum z_i e_i / det,  a = sum a_i e_i / sum e_i  (perspective-correct, wrt the original
  triangle), all linear in the pixel index, and valid for vertices with w <= 0.  Front = clockwise in y-down framebuffer
  space = det(M) > 0 (Vulkan 1.2 sec. 27.12.1: CLOCKWISE makes the negative-area polygon front-facing, area = -1/2 sum
  x_i y_(i+1) - x_(i+1) y_i).  The visible part is the intersection of the half planes e_i >= 0 (edges), z/w >= 0 (far,
  reverse-Z) and z/w <= 1 (near); x / y clipping changes no pixel in exact arithmetic.  Pixel centres sit at +0.5.

Each half plane is a functional L(px, py) = A px + B py + C with integer A, B, C; the perpendicular distance of a pixel
centre to its line is L / sqrt(A^2 + B^2) pixels and is compared with the position uncertainty delta EXACTLY (squares of
integers).  binary64 numpy pre-selects: it evaluates L with a rigorous error bound (2^-50 (|A| px + |B| py + |C|)) and
only the pixels it cannot classify go through the integers.  Depths and varyings are compared under tolerances that are
>= 2^20 times binary64's rounding; the binary64 evaluation error of a depth is added to its tolerance, and a pixel whose
depth order binary64 cannot separate is left undecided.

POSITION UNCERTAINTY  delta = 1/512 + C_POS * 2^-24 * m  [+ the clipper's share, below]   (pixels)
  1/512 is half a 24.8 step (rintf).  Between a clip coordinate and the snapped integer DESIGN's contract has three
  binary32 roundings, each of relative size u = 2^-24:  r = 1/w,  p = x * r,  xs = fmaf(p, half_extent, centre)
  (xs * 256 is exact).  The first two act on p * half_extent = xs - centre, the third on xs, so the error is at most
  u (2 |xs - centre| + |xs|) <= 3 u m  with  m = the largest of |xs|, |ys|, |xs - cx|, |ys - cy| over the primitive's
  vertices (after clipping to the guard band, +-32 w, i.e. +-32.5 x extent) -- the viewport centre has to be in m because
  the first two roundings are relative to the distance from it.  C_POS = 3.
  Clip-generated vertices: t = din / (din - dout) has four roundings (two plane distances, the difference -- din and dout
  have opposite signs, so it does not cancel -- and the division): |dt| <= 4 u t.  c_k = fmaf(t, out_k - in_k, in_k) has two
  more, |d c_k| <= u (2 |c_k| + |in_k|), plus what in and out carried.  These are CLIP-space errors; on the screen they
  are (hw (d c_x + |x/w| d c_w) + hh (d c_y + |y/w| d c_w)) / w, which next to the near plane (w small against in_w) no
  constant times u m bounds.  So for clipped primitives the clipper's share is evaluated per generated vertex (binary64:
  a tolerance, not a decision) and kept in two parts: the error of t moves the vertex ALONG the edge it was cut from --
  it moves the cut (the near / far line) but neither that edge's own line nor the depth and varying planes, which contain
  the whole edge; the rest may point anywhere.  An edge of the clipped polygon through vertices A, B displaced by dA, dB
  is displaced by at most dA (1 - s) + dB s at parameter s, taken over the part of the edge inside the viewport (edges
  that pass no pixel do not count).  Each of the five half planes (three edges, near, far) so gets its own delta.
  This DELIBERATELY replaces the form "c counts the clipper's roundings too" (c = 9 by that count): a constant times u m
  cannot bound a vertex generated next to the near plane, so a larger c was not tried; the per-vertex bound was derived
  first and is what the tests have always run with.  It comes out above 8 u m for some primitives (largest delta recorded:
  0.026 pixel).  The binary64 clipper below feeds these tolerances only: a clipped primitive is examined over the whole
  frame and the exact half planes alone say where it is.

DEPTH TOLERANCE  delta (|dz/dx| + |dz/dy|) + K_DEPTH u (|z_0| + |dzdx Dx| + |dzdy Dy| + max |z_i|)
  z_i = c_z * r: two roundings, 2 u max|z_i| anywhere inside the triangle (a plane through perturbed vertices moves by
  a convex combination of the perturbations).  Slopes: rounded once from binary64, u each.  (float)(Xc - X0): one rounding
  once the difference exceeds 2^24 sub-pixel units.  z = fmaf(dzdx, dx, fmaf(dzdy, dy, z0)): the inner rounding is relative
  to |z0| + |dzdy Dy|, the outer to all three.  Weights: max|z_i| 2, |z0| 2, |dzdx Dx| 3, |dzdy Dy| 4.  K_DEPTH = 4.
  For a clipped primitive the fan's vertex 0 is the clipper's business, so |z0| and max|z_i| are taken as 1 (depth lies in
  [0, 1]) and Dx, Dy as the distance to the farthest vertex of the clipped polygon; delta is the part of the position
  uncertainty that is not along an edge, and (d c_z + |z/w| d c_w) / w of the generated vertices is added.

VARYING TOLERANCE  delta (|da/dx| + |da/dy|) + K_VARY u (amp F D_a + max|a_i|)
  F = 1 + sum_{i=1,2} |dl_i/dx Dx| + |dl_i/dy Dy| is the size of the terms of the screen-space barycentric planes relative
  to vertex 0 (slivers: >> 1), four roundings each as for depth; amp = max_i (1/w_i) * w(pixel) is how much the
  perspective division magnifies an error of l_i; D_a = max |a_i - a_0|.  After the planes: l0 (2), l_i * rw_i (2: rw and
  the product), the sum (2), rcp (1), b_i (1), the clipped fan's beta (3, plus the 6 of the clipper's own barycentrics),
  interpolate (3) = 20, every one relative to a quantity <= amp F D_a + max|a_i|.  K_VARY = 4 + 20 = 24.
  For a clipped primitive F is the maximum over all vertex triples of the clipped polygon (a superset of any fan)."""
from __future__ import annotations

import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from oracle import bbo

U = 2.0 ** -24
C_POS = 3
K_DEPTH = 4
K_VARY = 24
GUARD = 32          # the contract's x / y clip planes: +-32 w
EPS64 = 2.0 ** -50  # bound of the relative error of a three-term binary64 evaluation with rounded coefficients
NONE = -1


def scene_primitives(scene):
    """binary32 clip positions [n, 3, 4] and vUV [n, 3, 2] of every primitive in API order (draw, instance, triangle),
    from bbo.vertex_stage"""
    L = bbo.lib()
    view = np.ascontiguousarray(scene.view)
    vp = view.ctypes.data
    clips, uvs = [], []
    for d in scene.draws:
        nv, ni = len(d.vertices), len(d.instances)
        idx = d.indices if d.indices is not None else np.arange(nv, dtype=np.uint32)
        tri = np.asarray(idx[: len(idx) // 3 * 3], np.int64).reshape(-1, 3)
        used = np.unique(tri)
        clip = np.zeros((ni, nv, 4), np.float32)
        vary = np.zeros((ni, nv, 14), np.float32)
        vb, ib, cb, yb = d.vertices.ctypes.data, d.instances.ctypes.data, clip.ctypes.data, vary.ctypes.data
        fn = L.bbo_vertex_stage
        for i in range(ni):
            for v in used.tolist():
                o = i * nv + v
                fn(vp, ib + 128 * i, vb + 44 * v, cb + 16 * o, yb + 56 * o)
        clips.append(clip[:, tri].reshape(-1, 3, 4))
        uvs.append(vary[:, tri, :2].reshape(-1, 3, 2))
    if not clips:
        return np.zeros((0, 3, 4), np.float32), np.zeros((0, 3, 2), np.float32)
    return np.concatenate(clips), np.concatenate(uvs)


def _common_ints(values):
    """exact: the floats as integers over one common power-of-two denominator"""
    fr = [float(v).as_integer_ratio() for v in values]
    den = max(f[1] for f in fr)   # powers of two: the largest is the common one
    return [f[0] * (den // f[1]) for f in fr], den


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


class _Func:
    """L(px, py) = A px + B py + C at pixel centres, exact integers + the binary64 image of the coefficients"""
    __slots__ = ("A", "B", "C", "G2", "a", "b", "c", "g")

    def __init__(self, hom, W, H):
        a, b, c = hom
        self.A, self.B = 2 * a * H, 2 * b * W
        self.C = a * (1 - W) * H + b * (1 - H) * W + c * W * H
        self.G2 = self.A * self.A + self.B * self.B

    def to_float(self, shift):
        s = 1 << shift
        self.a, self.b, self.c = self.A / s, self.B / s, self.C / s
        self.g = math.hypot(self.a, self.b)

    def at(self, px, py):
        return self.A * px + self.B * py + self.C

    def f64(self, X, Y):
        """value and error bound on pixel grids X, Y (>= 0)"""
        v = self.a * X + self.b * Y + self.c
        e = EPS64 * (abs(self.a) * X + abs(self.b) * Y + abs(self.c))
        return v, e


_PLANES = ((0, 0, -1, 1), (0, 0, 1, 0), (1, 0, 0, GUARD), (-1, 0, 0, GUARD), (0, 1, 0, GUARD), (0, -1, 0, GUARD))  # near far guard x4
NEAR_TAG, FAR_TAG = 3, 4   # tags 0..2: the original edge from vertex k to k + 1; 5..8: the guard band


class _PolyVertex:
    """c: clip coordinates; e_any: bound of the clipper's error in any direction; e_along: bound of the part that moves the
    vertex ALONG the original edge / cut edge it was generated on (tag `slid`); tag: which line the polygon edge that starts
    here lies on"""
    __slots__ = ("c", "e_any", "e_along", "slid", "tag", "generated")

    def __init__(self, c, e_any, e_along, slid, tag, generated):
        self.c, self.e_any, self.e_along, self.slid, self.tag, self.generated = c, e_any, e_along, slid, tag, generated


def _clip_polygon64(c3, clip_err=None):
    """binary64 Sutherland-Hodgman against near, far and the guard band: the clipped polygon's vertices, which line each of
    its edges lies on, and the bound of the binary32 clipper's error on each vertex (docstring of the module).  Tolerance
    bookkeeping only; decides no pixel (clipped primitives are examined over the whole frame).  `clip_err` [3, 4]: what the
    original vertices already carry (clip coordinates that are not binary32 inputs), in any direction."""
    seed = np.zeros((3, 4)) if clip_err is None else np.asarray(clip_err, np.float64)
    poly = [_PolyVertex(np.array(c, np.float64), seed[k].copy(), np.zeros(4), None, k, False) for k, c in enumerate(c3)]
    for n_plane, coef in enumerate(_PLANES):
        coef = np.array(coef, np.float64)
        out = []
        n = len(poly)
        for i in range(n):
            a, b = poly[i], poly[(i + 1) % n]
            da, db = float(coef @ a.c), float(coef @ b.c)
            if da >= 0:
                out.append(a)
            if (da >= 0) != (db >= 0):
                pin, din, pout, dout = (a, da, b, db) if da >= 0 else (b, db, a, da)
                t = din / (din - dout)
                c = pin.c + t * (pout.c - pin.c)
                carried_in, carried_out = pin.e_any + pin.e_along, pout.e_any + pout.e_along
                e_any = carried_in + carried_out + U * (2 * np.abs(c) + np.abs(pin.c))
                dt = 4 * U * t + float(np.abs(coef) @ (carried_in + carried_out)) / abs(din - dout)
                e_along = dt * np.abs(pout.c - pin.c)
                # leaving: the next polygon edge runs along the clip plane; entering: it continues the edge a -> b
                out.append(_PolyVertex(c, e_any, e_along, a.tag, 3 + n_plane if da >= 0 else a.tag, True))
        poly = out
        if len(poly) < 3:
            return []
    return poly


def _segment_in_rect(a, b, lo, hi):
    """Liang-Barsky: the parameter range [s0, s1] of a + s (b - a), 0 <= s <= 1, inside the rectangle, or None"""
    s0, s1 = 0.0, 1.0
    for k in range(2):
        d = b[k] - a[k]
        if d == 0:
            if a[k] < lo[k] or a[k] > hi[k]:
                return None
            continue
        t0, t1 = (lo[k] - a[k]) / d, (hi[k] - a[k]) / d
        if t0 > t1:
            t0, t1 = t1, t0
        s0, s1 = max(s0, t0), min(s1, t1)
        if s0 > s1:
            return None
    return s0, s1


class Prim:
    """exact setup of one primitive; None-like (self.skip) when it can touch no pixel.  `clip_err` [3, 4]: bound of the error the
    clip coordinates carry when they are not the binary32 inputs themselves (a vertex stage evaluated in binary64), projected to
    pixels the way the clipper's share is; `origin`: where this W x H viewport sits in a larger target (the third rounding of the
    viewport transform is relative to the coordinate in that target)."""

    def __init__(self, index, clip, uv, W, H, clip_err=None, origin=(0.0, 0.0)):
        self.index, self.skip = index, True
        ints, den = _common_ints(clip.reshape(-1))
        x, y, z, w = ([ints[4 * i + k] for i in range(3)] for k in range(4))
        # exact trivial reject: all three vertices outside one plane of the clip volume or of the viewport
        if clip_err is not None:   # ... by more than the error they carry (binary64: 2^-29 of the margin it leaves is ample)
            c, e = clip.astype(np.float64), np.asarray(clip_err, np.float64) * (1.0 + 2.0 ** -20)
            outside = [(c[:, 3] - c[:, 2], e[:, 3] + e[:, 2]), (c[:, 2], e[:, 2]), (c[:, 3] + c[:, 0], e[:, 3] + e[:, 0]),
                       (c[:, 3] - c[:, 0], e[:, 3] + e[:, 0]), (c[:, 3] + c[:, 1], e[:, 3] + e[:, 1]), (c[:, 3] - c[:, 1], e[:, 3] + e[:, 1])]
            if any(bool((v + ev < 0).all()) for v, ev in outside):
                return
        elif (all(w[i] - z[i] < 0 for i in range(3)) or all(z[i] < 0 for i in range(3)) or all(w[i] + x[i] < 0 for i in range(3))
                or all(w[i] - x[i] < 0 for i in range(3)) or all(w[i] + y[i] < 0 for i in range(3)) or all(w[i] - y[i] < 0 for i in range(3))):
            return
        self.all_in = all(0 <= z[i] <= w[i] and w[i] > 0 and abs(x[i]) <= GUARD * w[i] and abs(y[i]) <= GUARD * w[i] for i in range(3))
        r = [(x[i], y[i], w[i]) for i in range(3)]
        col = [_cross(r[(i + 1) % 3], r[(i + 2) % 3]) for i in range(3)]
        det = sum(r[0][k] * col[0][k] for k in range(3))
        if det == 0:   # zero area: no fragment (and no plane to take a depth from)
            return
        self.front = det > 0
        sgn = (det > 0) - (det < 0)
        comb = lambda q: tuple(sum(q[i] * col[i][k] for i in range(3)) for k in range(3))
        self.edge = [_Func(col[i], W, H) for i in range(3)]
        self.Z = _Func(comb(z), W, H)
        self.Wn = _Func(comb([1, 1, 1]), W, H)
        self.detp = det * W * H
        one = _Func(comb(w), W, H)
        assert one.A == 0 and one.B == 0 and one.C == self.detp
        finite_uv = bool(np.isfinite(uv).all())
        uvi, self.uv_den = _common_ints(uv.reshape(-1)) if finite_uv else ([0] * 6, 1)
        self.UV = [_Func(comb([uvi[2 * i + k] for i in range(3)]), W, H) for k in range(2)]
        self.uv_ok = finite_uv
        self.uv_vertex = uv.astype(np.float64)
        near = _Func((0, 0, 0), W, H)
        near.A, near.B, near.C = -sgn * self.Z.A, -sgn * self.Z.B, sgn * (self.detp - self.Z.C)
        far = _Func((0, 0, 0), W, H)
        far.A, far.B, far.C = sgn * self.Z.A, sgn * self.Z.B, sgn * self.Z.C
        near.G2 = far.G2 = self.Z.G2
        self.planes = self.edge + ([near, far] if sgn else [])
        funcs = self.planes + [self.Z, self.Wn] + self.UV
        bits = max(max(abs(f.A), abs(f.B), abs(f.C)).bit_length() for f in funcs + [one])
        shift = max(0, bits - 300)
        for f in funcs:
            f.to_float(shift)
        self.detf = self.detp / (1 << shift)
        self.lam = [float(Fraction(w[i] << shift, self.detp)) if det else 0.0 for i in range(3)]  # d lambda_i = lam_i * d e_i
        self.rw_scale = 1.0 / den
        # ---- tolerances' ingredients (binary64) ----
        c64 = clip.astype(np.float64)
        hw, hh = 0.5 * W, 0.5 * H
        extra_z = 0.0
        plane_extra = [0.0] * 5      # per half plane (3 edges, near, far): the clipper's share of delta
        any_extra = 0.0              # the part that is not along an edge: what moves the depth / varying planes
        if self.all_in:
            pts = np.stack([c64[:, 0] / c64[:, 3] * hw + hw, c64[:, 1] / c64[:, 3] * hh + hh], -1)
            self.z0 = abs(c64[0, 2] / c64[0, 3])
            self.zmax = float(np.max(np.abs(c64[:, 2] / c64[:, 3])))
            self.rw_max = float(np.max(1.0 / c64[:, 3]))
            if clip_err is not None:
                e, r = np.asarray(clip_err, np.float64), 1.0 / c64[:, 3]
                any_extra = float(np.max((hw * (e[:, 0] + np.abs(c64[:, 0] * r) * e[:, 3]) + hh * (e[:, 1] + np.abs(c64[:, 1] * r) * e[:, 3])) * r))
                plane_extra = [any_extra] * 5
                extra_z = float(np.max((e[:, 2] + np.abs(c64[:, 2] * r) * e[:, 3]) * r))
        else:
            poly = _clip_polygon64(c64, clip_err)
            ok = len(poly) >= 3 and all(v.c[3] > 0 for v in poly)
            if ok:
                P = np.array([v.c for v in poly])
                pts = np.stack([P[:, 0] / P[:, 3] * hw + hw, P[:, 1] / P[:, 3] * hh + hh], -1)

                def on_screen(v, e):  # clip-space error bound -> pixels
                    return float((hw * (e[0] + abs(v.c[0] / v.c[3]) * e[3]) + hh * (e[1] + abs(v.c[1] / v.c[3]) * e[3])) / v.c[3])

                lo, hi = np.array([-2.0, -2.0]), np.array([W + 2.0, H + 2.0])
                for k, v in enumerate(poly):
                    nxt = poly[(k + 1) % len(poly)]
                    span = _segment_in_rect(pts[k], pts[(k + 1) % len(poly)], lo, hi)
                    if span is None:
                        continue   # this edge of the polygon passes no pixel
                    ends = [on_screen(q, q.e_any) + (on_screen(q, q.e_along) if q.slid != v.tag else 0.0) for q in (v, nxt)]
                    worst = max(ends[0] * (1 - s_) + ends[1] * s_ for s_ in span)
                    plain = max(on_screen(v, v.e_any) * (1 - s_) + on_screen(nxt, nxt.e_any) * s_ for s_ in span)
                    any_extra = max(any_extra, plain)
                    j = {0: 2, 1: 0, 2: 1, NEAR_TAG: 3, FAR_TAG: 4}.get(v.tag)   # edge k -> k+1 is the line e_(k+2) = 0
                    if j is not None:
                        plane_extra[j] = max(plane_extra[j], worst)
                extra_z = max(float((v.e_any[2] + abs(v.c[2] / v.c[3]) * v.e_any[3]) / v.c[3]) for v in poly)
                self.rw_max = float(np.max(1.0 / P[:, 3]))
            else:
                # binary64 finds no polygon (the triangle passes a corner of the clip volume, or touches w = 0): the half
                # planes below still decide every pixel; the vertices are taken to sit anywhere inside the guard band
                pts = np.array([[-1.0, -1.0], [W + 1.0, -1.0], [W + 1.0, H + 1.0], [-1.0, H + 1.0]]) * (GUARD + 0.5)
                self.rw_max = math.inf
                if clip_err is not None:
                    any_extra = math.inf   # no polygon to project the carried error on: position unknown
            self.z0 = self.zmax = 1.0
        self.pts = pts
        m = float(np.max(np.abs(np.concatenate([(pts + np.asarray(origin, np.float64)).reshape(-1), (pts - [hw, hh]).reshape(-1)]))))
        m = min(m, (GUARD + 0.5) * max(W, H))
        self.m = m
        base = 1.0 / 512 + C_POS * U * m
        d = base + max([any_extra] + plane_extra)
        self.known = math.isfinite(d)      # False: position unknown, everything in reach is "may"
        self.delta_f = base + any_extra    # what moves the depth and varying planes
        self.plane_delta = [Fraction(base + e) if self.known else None for e in plane_extra]
        self.plane_delta_f = [base + e for e in plane_extra]
        self.max_delta = d
        self.extra_z = extra_z
        lo = np.floor(pts.min(0) - (d if math.isfinite(d) else 0) - 2)
        hi = np.ceil(pts.max(0) + (d if math.isfinite(d) else 0) + 2)
        if not self.all_in:   # the binary64 polygon only feeds tolerances: where a clipped primitive is, the half planes decide
            lo, hi = np.array([0.0, 0.0]), np.array([W, H], np.float64)
        self.x0, self.y0 = int(max(0, lo[0])), int(max(0, lo[1]))
        self.x1, self.y1 = int(min(W, hi[0])), int(min(H, hi[1]))
        if self.x1 <= self.x0 or self.y1 <= self.y0:
            return
        if self.all_in:
            self.F_slope = None
        else:
            n = len(pts)
            worst = 0.0
            for i in range(n):
                for j in range(i + 1, n):
                    for k in range(j + 1, n):
                        d1, d2 = pts[j] - pts[i], pts[k] - pts[i]
                        S = max(abs(d1[0] * d2[1] - d2[0] * d1[1]), 2.0 ** -16)
                        worst = max(worst, float(np.abs(d1).sum() + np.abs(d2).sum()) / S)
            self.F_slope = worst
        self.skip = False

    # ---- coverage ----
    def _exact_class(self, px, py):
        """+1 surely inside, 0 may, -1 surely outside; exact"""
        if not self.known:
            return 0
        sure = self.front
        for f, delta in zip(self.planes, self.plane_delta):
            p, q = delta.numerator, delta.denominator
            L = f.at(px, py)
            far_from_line = L * L * q * q > p * p * f.G2 if f.G2 else L != 0
            if L < 0 and far_from_line:
                return -1
            if not (L > 0 and far_from_line):
                sure = False
        return 1 if sure else 0

    def coverage(self):
        """(flat local indices sure, flat local indices may-only, X grid, Y grid) inside the bounding box"""
        xs = np.arange(self.x0, self.x1, dtype=np.float64)
        ys = np.arange(self.y0, self.y1, dtype=np.float64)
        X, Y = np.meshgrid(xs, ys)
        out = np.zeros(X.shape, bool)
        sure = np.full(X.shape, self.front and self.known)
        unknown = np.zeros(X.shape, bool)
        if self.known:
            for f, delta in zip(self.planes, self.plane_delta_f):
                v, e = f.f64(X, Y)
                thr = delta * f.g
                e = e + thr * (4 * EPS64)
                is_out = v + thr < -e
                is_in = v - thr > e
                is_mid = (np.abs(v) < thr - e)
                out |= is_out
                sure &= is_in
                unknown |= ~(is_out | is_in | is_mid)
        may = ~out & ~sure
        for iy, ix in zip(*np.nonzero(unknown & ~out)):
            c = self._exact_class(int(xs[ix]), int(ys[iy]))
            sure[iy, ix], may[iy, ix] = c == 1, c == 0
        return sure, may & ~sure, X, Y

    # ---- values at pixels (binary64; tolerances include the evaluation's own error) ----
    def depth(self, X, Y):
        v, e = self.Z.f64(X, Y)
        d = v / self.detf
        gx, gy = abs(self.Z.a / self.detf), abs(self.Z.b / self.detf)
        Dx, Dy = self._reach(X, Y)
        tol = self.delta_f * (gx + gy) + K_DEPTH * U * (self.z0 + gx * Dx + gy * Dy + self.zmax) + self.extra_z
        if not self.known:
            tol = np.full(np.shape(d), np.inf)
        return np.clip(d, 0.0, 1.0), tol + 4 * e / abs(self.detf)

    def _reach(self, X, Y):
        cx, cy = X + 0.5, Y + 0.5
        if self.all_in:
            return np.abs(cx - self.pts[0, 0]), np.abs(cy - self.pts[0, 1])
        return (np.max(np.abs(cx[..., None] - self.pts[:, 0]), -1), np.max(np.abs(cy[..., None] - self.pts[:, 1]), -1))

    def vuv(self, X, Y):
        """exact perspective-correct vUV [.., 2] and its tolerance [.., 2]"""
        wn, we = self.Wn.f64(X, Y)
        Dx, Dy = self._reach(X, Y)
        if self.all_in:
            F = 1.0 + sum(abs(self.edge[i].a * self.lam[i]) * Dx + abs(self.edge[i].b * self.lam[i]) * Dy for i in (1, 2))
        else:
            F = 1.0 + self.F_slope * np.maximum(Dx, Dy)
        amp = self.rw_max * self.rw_scale * self.detf / wn
        val, tol = [], []
        for k in range(2):
            un, ue = self.UV[k].f64(X, Y)
            a = un / wn / self.uv_den
            gx = (self.UV[k].a * wn - un * self.Wn.a) / (wn * wn) / self.uv_den
            gy = (self.UV[k].b * wn - un * self.Wn.b) / (wn * wn) / self.uv_den
            av = self.uv_vertex[:, k]
            D, M = float(np.max(np.abs(av - av[0]))), float(np.max(np.abs(av)))
            t = self.delta_f * (np.abs(gx) + np.abs(gy)) + K_VARY * U * (amp * F * D + M)
            t = t + 4 * (ue / np.abs(wn) / self.uv_den + np.abs(a) * we / np.abs(wn))
            val.append(a); tol.append(t)
        return np.stack(val, -1), np.stack(tol, -1)

    def attr(self, X, Y, av):
        """vuv's value and tolerance for ANY per-vertex attribute av [3] (finite): a = sum a_i e_i / sum e_i in binary64"""
        av = np.asarray(av, np.float64)
        wn, we = self.Wn.f64(X, Y)
        Dx, Dy = self._reach(X, Y)
        if self.all_in:
            F = 1.0 + sum(abs(self.edge[i].a * self.lam[i]) * Dx + abs(self.edge[i].b * self.lam[i]) * Dy for i in (1, 2))
        else:
            F = 1.0 + self.F_slope * np.maximum(Dx, Dy)
        amp = self.rw_max * self.rw_scale * self.detf / wn
        ua, ub = (sum(av[i] * getattr(self.edge[i], k) for i in range(3)) for k in "ab")
        ev = [self.edge[i].f64(X, Y) for i in range(3)]
        un, ue = sum(av[i] * ev[i][0] for i in range(3)), sum(abs(av[i]) * ev[i][1] for i in range(3))
        a = un / wn
        gx, gy = (ua * wn - un * self.Wn.a) / (wn * wn), (ub * wn - un * self.Wn.b) / (wn * wn)
        D, M = float(np.max(np.abs(av - av[0]))), float(np.max(np.abs(av)))
        t = self.delta_f * (np.abs(gx) + np.abs(gy)) + K_VARY * U * (amp * F * D + M)
        return a, t + 4 * (ue / np.abs(wn) + np.abs(a) * we / np.abs(wn))


def rasterise(scene, only=None, want_uv=True):
    """The ideal frame of `scene` (finite primitives only; `only` = iterable of primitive indices to draw alone).  Returns a
    namespace: per pixel `winner` (primitive index or NONE), `decided`, the winner's exact `depth` / `depth_tol` and `uv` /
    `uv_tol`; per primitive `sure_count` (pixels surely covered) and the Prim objects."""
    clip, uv = scene_primitives(scene)
    return rasterise_clip(clip, uv, scene.width, scene.height, only, want_uv)


def rasterise_clip(clip, uv, W, H, only=None, want_uv=True, clip_err=None, origin=(0.0, 0.0), groups=None):
    """rasterise() on bare clip coordinates [n, 3, 4] and attributes uv [n, 3, 2] of a W x H viewport.  With `clip_err`
    [n, 3, 4] (see Prim) the clip coordinates may be binary64.  Also returns `hi`: per pixel the largest depth + tolerance of
    every primitive that surely or possibly covers it (-inf: none can); with `groups` (per primitive a tuple of labels),
    `group_sure`: {label: [H, W] bool, the pixels a primitive of that label surely covers}."""
    n = len(clip)
    finite = np.isfinite(clip).all(axis=(1, 2))
    keep = finite.copy()
    if only is not None:
        sel = np.zeros(n, bool); sel[list(only)] = True
        keep &= sel
    # binary64 pre-selection over all primitives: clearly off-screen, or clearly back-facing and not thin
    c = clip.astype(np.float64)
    with np.errstate(all="ignore"):
        wpos = (c[:, :, 3] > 0).all(1)
        sx = c[:, :, 0] / c[:, :, 3] * (0.5 * W) + 0.5 * W
        sy = c[:, :, 1] / c[:, :, 3] * (0.5 * H) + 0.5 * H
        inside_z = ((c[:, :, 2] >= 0) & (c[:, :, 2] <= c[:, :, 3])).all(1)
        off = wpos & inside_z & ((sx.max(1) < -3) | (sx.min(1) > W + 3) | (sy.max(1) < -3) | (sy.min(1) > H + 3))
        d1x, d1y, d2x, d2y = sx[:, 1] - sx[:, 0], sy[:, 1] - sy[:, 0], sx[:, 2] - sx[:, 0], sy[:, 2] - sy[:, 0]
        S = d1x * d2y - d2x * d1y
        longest = np.sqrt(np.maximum(np.maximum(d1x ** 2 + d1y ** 2, d2x ** 2 + d2y ** 2), (d2x - d1x) ** 2 + (d2y - d1y) ** 2))
        m = np.maximum(np.abs(sx).max(1), np.abs(sy).max(1)) + max(W, H)
        back_fat = wpos & inside_z & (S < 0) & (-S > 8 * (1.0 / 512 + 16 * U * m) * longest)
        # no pixel centre within a margin (1/16 pixel + 64 u m, far above delta and binary64's error) of the bounding box
        pad = 1.0 / 16 + 64 * U * m
        no_centre = wpos & inside_z & ((np.floor(sx.min(1) - pad - 0.5) == np.floor(sx.max(1) + pad - 0.5))
                                       | (np.floor(sy.min(1) - pad - 0.5) == np.floor(sy.max(1) + pad - 0.5)))
    if clip_err is not None:   # the margins above (3 pixels, 1/16 pixel) pre-select only where the carried error is far below them
        e = np.asarray(clip_err, np.float64)
        with np.errstate(all="ignore"):
            pe = ((0.5 * W * (e[..., 0] + np.abs(c[..., 0] / c[..., 3]) * e[..., 3]) + 0.5 * H * (e[..., 1] + np.abs(c[..., 1] / c[..., 3]) * e[..., 3]))
                  / c[..., 3]).max(1)
        small = pe < 1.0 / 64
        off, back_fat, no_centre = off & small, back_fat & small, no_centre & small
    keep &= ~off & ~back_fat & ~no_centre

    res = SimpleNamespace()
    res.width, res.height, res.n_prims = W, H, n
    res.finite = finite
    npx = W * H
    hi1 = np.full(npx, -np.inf); id1 = np.full(npx, NONE, np.int64); hi2 = np.full(npx, -np.inf)
    lo_best = np.full(npx, -np.inf); id_best = np.full(npx, NONE, np.int64)
    d_best = np.zeros(npx); tol_best = np.zeros(npx)
    res.prims, res.sure_count, res.group_sure = {}, {}, {}
    res.max_delta = 0.0
    for p in np.nonzero(keep)[0].tolist():
        pr = Prim(p, clip[p], uv[p], W, H, None if clip_err is None else clip_err[p], origin)
        if pr.skip:
            continue
        sure, may, X, Y = pr.coverage()
        both = sure | may
        if not both.any():
            continue
        if pr.known:
            res.max_delta = max(res.max_delta, pr.max_delta)
        iy, ix = np.nonzero(both)
        flat = (iy + pr.y0) * W + (ix + pr.x0)
        d, tol = pr.depth(X[iy, ix], Y[iy, ix])
        s = sure[iy, ix]
        hi = d + tol
        # top two of d + tol over everything that surely or possibly is there: a pixel is decided when the best surely covering
        # primitive is ahead of ALL of them -- a "may cover" primitive that cannot win does not undo a decision, one that could does
        gt1 = hi > hi1[flat]
        hi2[flat] = np.where(gt1, hi1[flat], np.maximum(hi2[flat], hi))
        id1[flat] = np.where(gt1, p, id1[flat])
        hi1[flat] = np.where(gt1, hi, hi1[flat])
        fs = flat[s]
        lo = (d - tol)[s]
        better = lo > lo_best[fs]
        fb = fs[better]
        lo_best[fb], id_best[fb], d_best[fb], tol_best[fb] = lo[better], p, d[s][better], tol[s][better]
        res.prims[p] = pr
        res.sure_count[p] = int(s.sum())
        if groups is not None and s.any():
            for g in groups[p]:
                res.group_sure.setdefault(g, np.zeros(npx, bool))[fs] = True
    rival = np.where(id1 == id_best, hi2, hi1)
    nothing = (id1 == NONE)
    with np.errstate(invalid="ignore"):   # (-inf) - (-inf) where nothing is
        won = (id_best != NONE) & (lo_best - rival > 2.0 ** -40)
    res.decided = (nothing | won).reshape(H, W)
    res.winner = np.where(won, id_best, NONE).reshape(H, W)
    res.depth = np.where(won, d_best, 0.0).reshape(H, W)
    res.depth_tol = np.where(won, tol_best, 0.0).reshape(H, W)
    res.hi = hi1.reshape(H, W)
    res.group_sure = {g: m.reshape(H, W) for g, m in res.group_sure.items()}
    res.clip = clip
    res.not_all_in = int((finite & ~all_in(clip)).sum())
    if want_uv:
        res.uv = np.zeros((H, W, 2)); res.uv_tol = np.full((H, W, 2), np.inf)
        wy, wx = np.nonzero(res.winner != NONE)
        ids = res.winner[wy, wx]
        for p in np.unique(ids).tolist():
            pr = res.prims[p]
            if not pr.uv_ok:
                continue
            k = ids == p
            v, t = pr.vuv(wx[k].astype(np.float64), wy[k].astype(np.float64))
            res.uv[wy[k], wx[k]], res.uv_tol[wy[k], wx[k]] = v, t
    return res


def all_in(clip):
    """exact, [n] bool: every vertex of clip[n, 3, 4] inside the six planes of the contract's clip volume (near, far, guard band).
    binary32 values and their power-of-two multiples compare exactly in binary64."""
    c = np.asarray(clip, np.float32).astype(np.float64)
    x, y, z, w = (c[..., k] for k in range(4))
    with np.errstate(invalid="ignore"):
        ok = (0 <= z) & (z <= w) & (w > 0) & (np.abs(x) <= GUARD * w) & (np.abs(y) <= GUARD * w)
    return ok.all(-1)


# ---------------------------------------------------------------------------------------------------------------------
# the checks both test files share
# ---------------------------------------------------------------------------------------------------------------------

MAX_UNDECIDED = 0.01


def check_visibility(res, prim, depth, report=None):
    """on every decided pixel: `prim` is the reference's winner (or NO_PRIM) and `depth` within the tolerance.  At most
    1 % of the frame may be undecided.  Returns the worst error / tolerance ratio."""
    share = 1.0 - res.decided.mean()
    assert share <= MAX_UNDECIDED, f"{share:.4%} of the frame undecided"
    want = np.where(res.winner == NONE, np.int64(bbo.NO_PRIM), res.winner)
    # primitives the reference dropped as non-finite are covered by parity, not here: a pixel they win is not compared
    got = prim.astype(np.int64)
    dropped = np.isin(got, np.nonzero(~res.finite)[0]) if not res.finite.all() else np.zeros(got.shape, bool)
    cmp = res.decided & ~dropped
    bad = cmp & (got != want)
    assert not bad.any(), (f"{int(bad.sum())} decided pixels pick another primitive, first (y, x) = "
                           f"{tuple(np.argwhere(bad)[0])}: got {got[bad][0]}, reference {want[bad][0]}")
    won = cmp & (res.winner != NONE)
    err = np.abs(depth.astype(np.float64)[won] - res.depth[won])
    ratio = float(np.max(err / res.depth_tol[won])) if won.any() else 0.0
    assert ratio <= 1.0, f"depth error {ratio:.3f} x tolerance"
    assert (depth[cmp & (res.winner == NONE)] == 0).all()
    if report is not None:
        report.update(undecided=float(share), depth_ratio=ratio, max_delta=res.max_delta)
    return ratio


def check_uv(res, uv_image, report=None):
    won = res.decided & (res.winner != NONE) & np.isfinite(res.uv_tol).all(-1)
    err = np.abs(uv_image[..., :2].astype(np.float64)[won] - res.uv[won])
    ratio = float(np.max(err / res.uv_tol[won])) if won.any() else 0.0
    assert ratio <= 1.0, f"vUV error {ratio:.3f} x tolerance"
    if report is not None:
        report.update(uv_ratio=ratio)
    return ratio


def check_stats(res, stats):
    """a primitive with a surely covered pixel was not culled; a primitive inside all six planes is not counted as clipped"""
    visible = sum(1 for n in res.sure_count.values() if n > 0)
    assert stats["n_raster_tris"] >= visible, (stats, visible)
    if res.finite.all():
        assert stats["n_clipped_prims"] <= res.not_all_in, (stats, res.not_all_in)
