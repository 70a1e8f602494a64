"""Overlay chart: 160 x 128 frames whose lights and gizmo meshes are a CHOSEN population for the overlay subpass
(`bbr_draw_overlays`: k_geometry / k_raster <.., OVERLAY>, k_shade_overlay, the host's matrix folds; oracle `bbo_overlay`).
TEST INFRASTRUCTURE ONLY.

  frame     160 x 128, so that both tile shapes have interior borders.  Camera: scenes.view_uniforms' default (fov 60, near
            0.1) at the origin; "main" looks down +z, the other views turn it (pitch +-90, a yawed one).  A marker (radius
            0.1) at distance d is about 11.1 / d pixels in radius.
  scene     two screen-parallel quads ("walls") at view depth 2 and 1 over the cleared background, so the scene depth under
            every marker of the main view is known by construction.
  cases     one light list, one gizmo mesh, one extent, one view each; CLASSES says what every class is there for and
            census() proves, per class, that the pixels it exists for are there.

THE MODEL is written from the Vulkan rules and light.vert / light.frag / gizmo.vert / gizmo.frag, not from the oracle's C:
  vertex programs in binary64 on the binary32 uniforms; coverage, depth order and interpolation by the exact rasteriser
  (raster_reference.rasterise_clip); depth test GREATER_OR_EQUAL against the scene depth of bbo.render (which
  test_gpu_raster_reference.py pins to the GPU bit for bit); the gizmo is a frame of its own, extent x extent, placed at
  (width - extent, 0) and cropped, over a cleared depth: where it has a fragment it owns the pixel, elsewhere the marker layer
  stays.  Two overlay primitives with IDENTICAL clip coordinates (two lights at one position, two coincident gizmo triangles)
  have equal depth everywhere: the later one owns their pixels -- only the last of such a set is rasterised.

Tolerances, u = 2^-24, first order with a factor 1 + 2^-10.  A k-term fmaf chain r = fl(sum a_i b_i) has |r - sum a_i b_i| <=
k u sum |a_i b_i| (vertex_chart.py).  |.| entry by entry, row vectors (clip = pos @ V @ P), A = |V| |P| >= |P*V|:
  marker   the host folds PV = fl(V P) (4 terms: e_PV = 4 u A), then column 3, c3 = fl((pos, 1) PV) (4 terms:
           e_c3 = 4 u (|pos|, 1) A + (|pos|, 1) e_PV = 8 u (|pos|, 1) A); the kernel's vertex is clip = fl(p PV[:3] + c3)
           (4 terms): e_clip = 4 u (|p| A[:3] + |c3|) + |p| e_PV[:3] + e_c3 = 8 u |p| A[:3] + 12 u (|pos|, 1) A.
  gizmo    V' = V with its translation row replaced by -dot(look * -27, axis): one rounding for the scale, three for the dot
           product, e_V'[3, k] = 4 u 27 |look| . |axis_k|.  P' = P with [0][0] = d, [1][1] = -d, d = 1 / tanf(0.261799f):
           tanf within one ulp (2 u relative) and the division, e_d = 3 u d.  PV' = fl(V' P'): e_PV' = 4 u |V'| |P'| +
           e_V' |P'| + |V'| e_P'.  clip = fl((p, 1) PV'): e_clip = 4 u (|p|, 1) |V'| |P'| + (|p|, 1) e_PV'.
           vNormal = mat3(V') n, 3 terms: e_n = 3 u |n| |V'[:3, :3]|.
  position e_clip goes to pixels as raster_reference projects the clipper's share, (hw (e_x + |x/w| e_w) + hh (e_y + |y/w|
           e_w)) / w per vertex, and is added to its 1/512 + C_POS u m for every half plane and for the depth and varying planes;
           for a clipped primitive it seeds the clipper's bookkeeping.  The depth takes (e_z + |z/w| e_w) / w.  For the gizmo m
           counts the coordinate in the whole target (origin = (width - extent, 0)).
  depth    a pixel is "changed" when its winner's depth - raster_reference's depth tolerance > scene depth, "unchanged" when
           nothing can cover it or every candidate's depth + tolerance < scene depth, else undecided.
  colour   marker: the three vertices carry the light's colour c, so D_a = 0 and raster_reference's varying tolerance is
           K_VARY u |c|.  gizmo: colour c +- t_c and normal N +- t_N from Prim.attr (t_N also takes e_n); with rho = ||t_N|| /
           ||N||, g = -N_z / ||N|| moves by at most 2 rho (every component of a normalised vector does, vertex_chart.py) + 4 u
           for its evaluation; rho >= 1/2 leaves the pixel undecided.  The value v = c max(g, 0) then has
           t_v = |c| t_g + max(g, 0) t_c + t_c t_g + 2 u |v|, and is exactly 0 once g + t_g < 0.  All three normals zero: N is
           NaN, max(NaN, 0) = 0, v = 0.
  bytes    byte b of a channel stands for the linear interval [T_b, T_b+1), T = (-inf, bbo.srgb_thresholds(), +inf): sRGB
           UNORM8, round to nearest.  A decided changed pixel passes when every channel's exact value is within its tolerance
           of its byte's interval; the error / tolerance ratio is that distance over the tolerance.  NaN gives byte 0
           (max(NaN, .) clamps to 0), negative 0, >= 1 and +inf 255; alpha is 255."""
from __future__ import annotations

import functools
import math
import os
from types import SimpleNamespace

import numpy as np

import raster_reference as rr
from oracle import bbo, scenes

W, H = 160, 128
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
F = np.float32
f64 = lambda a: np.asarray(a, np.float64)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VIEWS = {"main": (0.0, 0.0), "pitch +90": (0.0, 90.0), "pitch -90": (0.0, -90.0), "yawed": (35.0, -20.0)}
WALLS = ((8, 8, 72, 56, 2.0), (8, 72, 72, 120, 1.0))      # x0, y0, x1, y1 [pixels, main view], view depth
UNCHANGED, MARKER, GIZMO, UNDECIDED = 0, 1, 2, 3
MAX_UNDECIDED = rr.MAX_UNDECIDED

CLASSES = {
    "front": "wholly in front of a wall: every covered pixel changes",
    "hidden": "wholly behind a wall: covered, nothing changes",
    "cut": "centre on a wall's plane, off axis: part changes, part stays",
    "background": "over the cleared depth 0",
    "tie": "two lights at one position: the later one owns every pixel both cover",
    "overlap": "two markers overlapping on the screen at different distances: the nearer one wins where both cover",
    "near": "front-facing triangles cross the near plane (d = 0.18): clipped and visible",
    "inside": "the camera inside the marker: nothing drawn",
    "behind": "behind the camera: nothing drawn",
    "edge": "across a frame edge / a corner / the tile crossing at (64, 64)",
    "tiny": "d = 20 and 40 on a pixel centre: a pixel or two",
    "nonfinite": "position NaN / +inf / 1e30: nothing drawn, the others unaffected",
    "colour": "components outside [0, 1], non-finite, denormal, on sRGB thresholds and their neighbours",
    "count": "NumLights outside 0..100",
    "gizmo": "the gizmo has pixels, and none outside its rectangle",
    "under": "a marker nearer than every gizmo fragment loses where the gizmo has one and stays where it has none",
    "scissor": "a triangle beyond the viewport square: cut at width - extent",
    "g overlap": "two gizmo triangles at different depths: the nearer wins where both cover",
    "g tie": "two coincident gizmo triangles: the later wins",
    "g zero normals": "three zero normals: written black",
    "g one zero normal": "one zero normal",
    "g away": "a normal pointing away: written black",
    "g colour 3": "a colour of 3.0: 255",
}


# ---------------------------------------------------------------------------------------------------------------------
# camera, scene
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def view_uniforms(name, width=W, height=H):
    yaw, pitch = VIEWS[name]
    return scenes.view_uniforms((0.0, 0.0, 0.0), yaw, pitch, width, height, 1, 60.0, 0.1, 1000.0)


def _solve(C, sx, sy, w, width, height):
    """the point p with (p, 1) @ C projecting to pixel position (sx, sy) at clip w; C binary64"""
    nx, ny = sx / (0.5 * width) - 1.0, sy / (0.5 * height) - 1.0
    cols = [C[:, 0] - nx * C[:, 3], C[:, 1] - ny * C[:, 3], C[:, 3]]
    A = np.stack([c[:3] for c in cols])
    b = np.array([-cols[0][3], -cols[1][3], w - cols[2][3]])
    return np.linalg.solve(A, b)


def place(view, sx, sy, d):
    """binary32 world position seen at pixel (sx, sy) at view depth d"""
    vu = view_uniforms(view)
    return _solve(f64(vu["view"]) @ f64(vu["proj"]), sx, sy, d, W, H).astype(F)


def _front(C, p):
    c = np.stack([np.append(f64(q), 1.0) @ C for q in p])
    return np.linalg.det(c[:, [0, 1, 3]]) > 0


@functools.lru_cache(None)
def wall_draw():
    v = np.zeros(4 * len(WALLS), bbo.VERTEX_DTYPE)
    idx = []
    vu = view_uniforms("main")
    C = f64(vu["view"]) @ f64(vu["proj"])
    for k, (x0, y0, x1, y1, d) in enumerate(WALLS):
        p = np.stack([place("main", x, y, d) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))])
        v["pos"][4 * k:4 * k + 4] = p
        order = (0, 1, 2, 2, 3, 0) if _front(C, p[[0, 1, 2]]) else (0, 2, 1, 2, 0, 3)
        idx += [4 * k + i for i in order]
    v["uv"] = [(0, 0), (1, 0), (1, 1), (0, 1)] * len(WALLS)
    v["normal"], v["tangent"] = (0, 0, -1), (1, 0, 0)
    inst = np.zeros(1, bbo.INSTANCE_DTYPE)
    inst[0]["model"] = inst[0]["inv_model"] = np.eye(4, dtype=F)
    return bbo.DrawData(v, np.array(idx, np.uint32), inst, bbo.MaterialData())


# ---------------------------------------------------------------------------------------------------------------------
# gizmo meshes
# ---------------------------------------------------------------------------------------------------------------------
def gizmo_fold(vu):
    """gizmo.vert:13-24 in binary64 on the binary32 uniforms, and the bounds of the binary32 fold (module docstring)"""
    V, P = f64(vu["view"]).copy(), f64(vu["proj"]).copy()
    axes = [V[:3, k].copy() for k in range(3)]          # right, up, look: (uViewMat[0][k], [1][k], [2][k])
    view_pos = axes[2] * -27.0
    e_V, e_P = np.zeros((4, 4)), np.zeros((4, 4))
    for k in range(3):
        V[3, k] = -float(view_pos @ axes[k])
        e_V[3, k] = 4 * U * 27.0 * float(np.abs(axes[2]) @ np.abs(axes[k]))
    d = 1.0 / math.tan(float(F(0.261799)))
    P[0, 0], P[1, 1] = d, -d
    e_P[0, 0] = e_P[1, 1] = 3 * U * d
    aV, aP = np.abs(V), np.abs(P)
    e_PV = 4 * U * (aV @ aP) + e_V @ aP + aV @ e_P
    return SimpleNamespace(V=V, P=P, PV=V @ P, A=aV @ aP, e_PV=e_PV)


def _gizmo_vertices(raw):
    gv = np.zeros(len(raw), bbo.GIZMO_VERTEX_DTYPE)
    gv["pos"], gv["color"], gv["normal"] = raw[:, 0:3], raw[:, 3:6], raw[:, 6:9]
    return gv


@functools.lru_cache(None)
def reference_gizmo():
    g = np.load(os.path.join(GOLDEN, "gizmo.npz"))
    return np.ascontiguousarray(g["vertices"], F), np.ascontiguousarray(g["indices"], np.uint32)


HAND_EXTENT = 100
# name, corners [viewport pixels of the 100 x 100 square], view depth, colour, normals (view space, main view), class
HAND = (
    ("big", ((-20, 50), (120, -20), (120, 120)), 40.0, (0.5, 0.5, 0.5), ((0, 0, -1),) * 3, "scissor"),
    ("near first", ((12, 10), (40, 12), (14, 40)), 25.0, (0.9, 0.1, 0.1), ((0, 0, -1),) * 3, "g overlap"),
    ("far second", ((16, 14), (44, 16), (18, 44)), 30.0, (0.1, 0.9, 0.1), ((0, 0, -1),) * 3, "g overlap"),
    ("far first", ((66, 14), (94, 16), (68, 44)), 30.0, (0.1, 0.9, 0.1), ((0, 0, -1),) * 3, "g overlap"),
    ("near second", ((62, 10), (90, 12), (64, 40)), 25.0, (0.9, 0.1, 0.1), ((0, 0, -1),) * 3, "g overlap"),
    ("coincident first", ((10, 62), (40, 64), (12, 92)), 25.0, (0.2, 0.3, 0.8), ((0, 0, -1),) * 3, "g tie"),
    ("coincident second", ((10, 62), (40, 64), (12, 92)), 25.0, (0.8, 0.7, 0.2), ((0, 0, -1),) * 3, "g tie"),
    ("zero normals", ((46, 6), (58, 8), (47, 30)), 25.0, (0.7, 0.7, 0.7), ((0, 0, 0),) * 3, "g zero normals"),
    ("one zero normal", ((46, 36), (58, 38), (47, 60)), 25.0, (0.6, 0.7, 0.8), ((0.3, 0.2, -1), (0.1, -0.2, -1), (0, 0, 0)), "g one zero normal"),
    ("away", ((46, 66), (58, 68), (47, 94)), 25.0, (0.7, 0.7, 0.7), ((0.1, 0.2, 1),) * 3, "g away"),
    ("colour 3", ((64, 62), (94, 64), (66, 94)), 25.0, (3.0, 3.0, 3.0), ((0.2, 0.1, -1),) * 3, "g colour 3"),
)


@functools.lru_cache(None)
def hand_gizmo():
    """a dozen triangles solved through the main view's gizmo fold: raw vertices [3 n, 9] in triangle order"""
    fold = gizmo_fold(view_uniforms("main"))
    raw = np.zeros((3 * len(HAND), 9), F)
    for t, (_, corners, w, colour, normals, _) in enumerate(HAND):
        p = np.stack([_solve(fold.PV, u, v, w * (1.0 + 0.01 * k), HAND_EXTENT, HAND_EXTENT) for k, (u, v) in enumerate(corners)])
        order = [0, 1, 2] if _front(fold.PV, p) else [0, 2, 1]
        for slot, k in enumerate(order):
            raw[3 * t + slot] = (*p[k], *colour, *normals[k])     # main view: mat3(V') is the identity
    return raw


def gizmo_mesh(kind):
    """(raw vertices [n, 9], indices or None) as uploaded"""
    if kind == "reference":
        return reference_gizmo()
    raw = hand_gizmo()
    if kind == "hand":
        return raw, None
    assert kind == "hand indexed"
    perm = np.random.Generator(np.random.PCG64(53)).permutation(len(raw))     # a shuffled vertex buffer behind an index buffer
    inv = np.empty_like(perm); inv[perm] = np.arange(len(raw))
    return np.ascontiguousarray(raw[perm]), inv.astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _light(view, sx, sy, d, colour, type=0):
    return scenes.light(type, pos=place(view, sx, sy, d), dir=(0.0, -1.0, 0.0), color=colour, intensity=1.0, inner=0.9, outer=0.8)


def _at(pos, colour, type=0):
    return scenes.light(type, pos=pos, dir=(0.0, -1.0, 0.0), color=colour, intensity=1.0)


def _next(x, k):
    return np.nextafter(F(x), F(np.inf if k > 0 else -np.inf))


@functools.lru_cache(None)
def cases():
    """{name: namespace(view, lights, num_lights, gizmo, extent, classes, model)}; classes: {class: [light indices]} (gizmo classes: [])"""
    out = {}

    def add(name, view, lights, classes, gizmo=None, extent=0, num_lights=None, model=True):
        out[name] = SimpleNamespace(name=name, view=view, lights=lights, classes=classes, gizmo=gizmo, extent=extent,
                                    num_lights=len(lights) if num_lights is None else num_lights, model=model)

    R, G, B, Y = (0.9, 0.2, 0.1), (0.1, 0.8, 0.3), (0.2, 0.3, 0.9), (0.9, 0.8, 0.1)
    m = "main"
    add("depth", m, [_light(m, 24, 32, 1.5, R, 0), _light(m, 56, 32, 2.5, G, 1), _light(m, 30, 100, 1.0, B, 2), _light(m, 120, 90, 1.2, Y, 0),
                     _light(m, 100.5, 20.5, 20.0, R, 1), _light(m, 110.5, 20.5, 40.0, G, 2)],
        {"front": [0], "hidden": [1], "cut": [2], "background": [3], "tiny": [4, 5]})
    add("ties", m, [_light(m, 100, 30, 2.0, R), _light(m, 100, 30, 2.0, G), _light(m, 140, 30, 2.0, G), _light(m, 140, 30, 2.0, R),
                    _light(m, 100, 90, 2.0, B), _light(m, 106, 92, 1.5, Y), _light(m, 135, 90, 1.5, Y), _light(m, 141, 92, 2.0, B),
                    _light(m, 40, 32, 1.5, R), _light(m, 40, 32, 1.5, B, 2)],       # (a tie in front of a wall too)
        {"tie": [0, 1, 2, 3, 8, 9], "overlap": [4, 5, 6, 7]})
    add("near", m, [_at((0.09, 0.02, 0.1546), R), _at((0.01, 0.02, 0.043), G), _at((0.0, 0.0, -1.0), B), _light(m, 30, 30, 1.5, Y),
                    _light(m, 120, 100, 3.0, G)],
        {"near": [0], "inside": [1], "behind": [2], "front": [3], "background": [4]})
    add("edge", m, [_light(m, 1, 64, 1.5, R), _light(m, 159, 40, 1.5, G), _light(m, 90, 1, 1.5, B), _light(m, 100, 127, 1.5, Y),
                    _light(m, 2, 126, 1.5, G), _light(m, 64, 64, 1.5, R, 1)],
        {"edge": [0, 1, 2, 3, 4, 5]})
    add("nonfinite", m, [_light(m, 100, 40, 2.0, R), _at((np.nan, 0.0, 2.0), G), _at((0.0, np.inf, 2.0), B), _at((0.0, 0.0, 1e30), Y),
                         _at((1e30, 0.0, 2.0), Y), _light(m, 120, 80, 2.0, G)],
        {"nonfinite": [1, 2, 3, 4], "background": [0, 5]})
    thr = bbo.srgb_thresholds()
    vals = [2.0, -1.0, -0.0, np.nan, np.inf, 1e-41, 0.0031308, _next(0.0031308, -1), _next(0.0031308, 1)]
    for k in (0, 63, 127, 254):
        vals += [thr[k], _next(thr[k], -1), _next(thr[k], 1)]
    vals = np.array(vals, F).reshape(-1, 3)
    add("colour", m, [_light(m, 84 + 11 * (i % 7), 74 + 11 * (i // 7), 3.0, tuple(c)) for i, c in enumerate(vals)],
        {"colour": list(range(len(vals)))})
    three = [_light(m, 100, 40, 2.0, R), _light(m, 130, 70, 2.0, G, 2), _light(m, 40, 30, 1.5, B, 1)]
    for n in (0, -4, 100, 250):
        add(f"count {n}", m, three, {"count": [0, 1, 2]}, num_lights=n)
    add("many", m, [_light(m, 100, 60, 1.5, (0.01 * i, 1.0 - 0.01 * i, 0.5)) for i in range(99)], {}, model=False)
    # a marker over the middle of the gizmo's rectangle (the axes start there), one elsewhere
    mid = lambda e: (min(W - 0.5 * e + 3.0, W - 0.5), min(0.5 * e + 2.0, H - 3.0))
    for extent in (1, 33, 100, 150, 200):
        add(f"gizmo {extent}", m, [_light(m, *mid(extent), 0.8, R), _light(m, 30, 64, 0.8, G, 2)], {"gizmo": [], "under": [0]},
            gizmo="reference", extent=extent)
    for v in ("pitch +90", "pitch -90", "yawed"):
        add(f"gizmo {v}", v, [_light(v, *mid(100), 0.8, R), _light(v, 30, 64, 1.5, G, 1)], {"gizmo": [], "under": [0]},
            gizmo="reference", extent=100)
    hand = {c: [] for *_, c in HAND}
    hand["under"] = [0, 1]
    for kind in ("hand", "hand indexed"):
        add(f"gizmo {kind}", m, [_light(m, 68, 8, 2.8, B), _light(m, 150, 100, 2.0, Y), _light(m, 60, 50, 2.0, R)], dict(hand),
            gizmo=kind, extent=HAND_EXTENT)
    return out


def modelled():
    return [n for n, c in cases().items() if c.model]


def frame_uniforms(c):
    fu = scenes.frame_uniforms(c.lights)
    fu["num_lights"] = c.num_lights
    return fu


def scene(name, width=W, height=H):
    c = cases()[name]
    return bbo.Scene(frame_uniforms(c), view_uniforms(c.view, width, height), [wall_draw()], width, height, f"overlay chart {name}")


def gizmo_upload(name):
    """(raw, indices or None, oracle vertex records or None) of a case"""
    c = cases()[name]
    if c.gizmo is None:
        return None, None, None
    raw, gi = gizmo_mesh(c.gizmo)
    return raw, gi, _gizmo_vertices(raw)


@functools.lru_cache(None)
def oracle_frame(name, deferred=False, width=W, height=H):
    """the oracle's base image, scene depth and overlaid image of a case, computed once -- read-only"""
    c, sc = cases()[name], scene(name, width, height)
    if deferred:
        hdr, _, _, depth, _ = bbo.render_deferred(sc)
    else:
        hdr, _, depth, _ = bbo.render(sc)
    base = bbo.present(hdr, 0, 1.0)
    _, gi, gv = gizmo_upload(name)
    want, st = bbo.overlay(sc.frame, sc.view, depth, base, gv, gi, c.extent)
    for a in (base, depth, want):
        a.setflags(write=False)
    return SimpleNamespace(scene=sc, base=base, depth=depth, want=want, stats=st)


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def _last_of_identical(clip):
    """(representatives, groups): of primitives with identical clip coordinates only the last is drawn; groups[p] = every
    primitive it stands for"""
    last, members = {}, {}
    for p in range(len(clip)):
        k = clip[p].tobytes()
        last[k] = p
        members.setdefault(k, []).append(p)
    return sorted(last.values()), {last[k]: tuple(v) for k, v in members.items()}


def marker_layer(fu, vu, depth):
    """light.vert in binary64, the exact rasteriser, the depth test: namespace of [H, W] kind, light, covered, and res"""
    n = min(max(int(fu["num_lights"]), 0), 100)
    pos, idx = bbo.uv_sphere(0.1, 16, 16)                 # generateUVSphereMesh(0.1, 16, 16); pinned by tests/golden/uv_sphere.npz
    tri = idx.reshape(-1, 3).astype(np.int64)
    V, P = f64(vu["view"]), f64(vu["proj"])
    PV, A = V @ P, np.abs(V) @ np.abs(P)
    p = f64(pos)
    clips, errs = [], []
    with np.errstate(all="ignore"):
        for li in range(n):
            lp = f64(fu["lights"][li]["pos"])
            world = np.concatenate([p + lp, np.ones((len(p), 1))], 1)       # modelMat * vec4(aPos, 1)
            c = world @ PV
            e = SLACK * (8 * U * (np.abs(p) @ A[:3]) + 12 * U * (np.append(np.abs(lp), 1.0) @ A))
            clips.append(c[tri]); errs.append(e[tri])
    out = SimpleNamespace(kind=np.zeros((H, W), np.uint8), light=np.full((H, W), -1), covered=np.zeros((H, W), bool), res=None, n_tris=len(tri))
    if not n:
        return out
    clip, err = np.concatenate(clips), np.concatenate(errs)
    reps, groups = _last_of_identical(clip)
    light_groups = {r: tuple(sorted({q // len(tri) for q in g})) for r, g in groups.items()}
    res = rr.rasterise_clip(clip, np.zeros((len(clip), 3, 2)), W, H, only=reps, want_uv=False, clip_err=err, groups=light_groups)
    S = f64(depth)
    won = res.decided & (res.winner != rr.NONE)
    changed = won & (res.depth - res.depth_tol > S)
    out.covered = res.hi > -np.inf
    unchanged = ~out.covered | (res.hi < S)
    out.kind = np.where(changed, MARKER, np.where(unchanged, UNCHANGED, UNDECIDED)).astype(np.uint8)
    out.light = np.where(changed, res.winner // len(tri), -1)
    out.res = res
    return out


def gizmo_layer(vu, raw, gi, extent):
    """gizmo.vert / gizmo.frag in binary64 over an extent x extent frame of its own: namespace of [extent, extent] kind, prim,
    val / tol [.., 3], and res"""
    fold = gizmo_fold(vu)
    raw = f64(raw)
    tri = (np.asarray(gi, np.int64) if gi is not None else np.arange(len(raw) // 3 * 3)).reshape(-1, 3)
    p1 = np.concatenate([raw[:, :3], np.ones((len(raw), 1))], 1)
    clip = (p1 @ fold.PV)[tri]
    err = (SLACK * (4 * U * (np.abs(p1) @ fold.A) + np.abs(p1) @ fold.e_PV))[tri]
    colour = raw[:, 3:6][tri]
    normal = (raw[:, 6:9] @ fold.V[:3, :3])[tri]                   # mat3(viewMat) * aNormal
    e_n = (SLACK * 3 * U * (np.abs(raw[:, 6:9]) @ np.abs(fold.V[:3, :3])))[tri]
    reps, groups = _last_of_identical(clip)
    res = rr.rasterise_clip(clip, np.zeros((len(clip), 3, 2)), extent, extent, only=reps, want_uv=False, clip_err=err,
                            origin=(float(W - extent), 0.0), groups=groups)
    kind = np.where(res.decided, np.where(res.winner != rr.NONE, GIZMO, UNCHANGED), UNDECIDED).astype(np.uint8)
    val, tol = np.zeros((extent, extent, 3)), np.zeros((extent, extent, 3))
    wy, wx = np.nonzero(kind == GIZMO)
    ids = res.winner[wy, wx]
    for t in np.unique(ids).tolist():
        k = ids == t
        y, x = wy[k], wx[k]
        pr, X, Y = res.prims[t], x.astype(np.float64), y.astype(np.float64)
        if not normal[t].any():                                        # N = normalize(0) is NaN: max(NaN, 0) = 0
            continue
        c, tc = zip(*[pr.attr(X, Y, colour[t][:, j]) for j in range(3)])
        nn, tn = zip(*[pr.attr(X, Y, normal[t][:, j]) for j in range(3)])
        c, tc, nn = np.stack(c, -1), np.stack(tc, -1), np.stack(nn, -1)
        tn = np.stack(tn, -1) + e_n[t].max(0)
        length = np.sqrt((nn * nn).sum(-1))
        with np.errstate(all="ignore"):
            rho = np.sqrt((tn * tn).sum(-1)) / length
            g = -nn[:, 2] / length
        vague = ~(rho < 0.5)
        tg = 2 * rho + 4 * U
        diff = np.maximum(g, 0.0)
        v = c * diff[:, None]
        tv = (np.abs(c) * tg[:, None] + diff[:, None] * tc + tc * tg[:, None] + 2 * U * np.abs(v)) * SLACK
        dark = g + tg < 0
        v[dark], tv[dark] = 0.0, 0.0
        val[y, x], tol[y, x] = v, tv
        kind[y[vague], x[vague]] = UNDECIDED
    return SimpleNamespace(kind=kind, prim=res.winner, val=val, tol=tol, res=res, groups=groups)


@functools.lru_cache(None)
def model(name):
    """what the frame of a case must be: [H, W] kind (UNCHANGED / MARKER / GIZMO / UNDECIDED), light (MARKER), prim (GIZMO),
    [H, W, 3] val +- tol of the linear colour; .markers / .gizmo are the two layers"""
    c, o = cases()[name], oracle_frame(name)
    fu, vu = o.scene.frame, o.scene.view
    mk = marker_layer(fu, vu, o.depth)
    out = SimpleNamespace(kind=mk.kind.copy(), light=mk.light.copy(), prim=np.full((H, W), rr.NONE), markers=mk, gizmo=None,
                          val=np.zeros((H, W, 3)), tol=np.zeros((H, W, 3)), rect=np.zeros((H, W), bool), x0=W - c.extent)
    with np.errstate(all="ignore"):
        colours = f64(fu["lights"]["color"])
        out.val[mk.kind == MARKER] = colours[mk.light[mk.kind == MARKER]]
        out.tol = rr.K_VARY * U * np.abs(out.val) * SLACK
    if c.gizmo is not None and c.extent > 0:
        raw, gi, _ = gizmo_upload(name)
        gz = gizmo_layer(vu, raw, gi, c.extent)
        x0 = W - c.extent
        ys, xs = slice(0, min(c.extent, H)), slice(max(x0, 0), W)
        us = slice(max(x0, 0) - x0, c.extent)
        k = gz.kind[ys, us]
        out.rect[ys, xs] = True
        for dst, src in ((out.kind, np.where(k == UNCHANGED, out.kind[ys, xs], k)), (out.prim, gz.prim[ys, us]),
                         (out.val, np.where((k == GIZMO)[..., None], gz.val[ys, us], out.val[ys, xs])),
                         (out.tol, np.where((k == GIZMO)[..., None], gz.tol[ys, us], out.tol[ys, xs]))):
            dst[ys, xs] = src
        out.gizmo = gz
    return out


_T = None


def byte_intervals():
    global _T
    if _T is None:
        _T = np.concatenate([[-np.inf], f64(bbo.srgb_thresholds()), [np.inf]])
    return _T


def check_image(name, image, base, what=""):
    """`image` [H, W, 4] against the model of a case on every decided pixel; `base` is the presented image before the pass.
    Returns the largest error / tolerance ratio of a colour channel."""
    mo = model(name)
    share = float((mo.kind == UNDECIDED).mean())
    assert share <= MAX_UNDECIDED, f"{name}: {share:.4%} of the frame undecided"
    same = (image == base).all(-1)
    bad = (mo.kind == UNCHANGED) & ~same
    assert not bad.any(), f"{what}{name}: {int(bad.sum())} pixels changed that must stay, first (y, x) = {tuple(np.argwhere(bad)[0])}"
    ch = (mo.kind == MARKER) | (mo.kind == GIZMO)
    assert (image[ch][:, 3] == 255).all(), f"{what}{name}: alpha"
    T = byte_intervals()
    b = image[..., :3].astype(np.int64)
    lo, hi = T[b], T[b + 1]
    with np.errstate(all="ignore"):
        v = np.where(np.isnan(mo.val), -1.0, mo.val)                   # NaN: byte 0, as a negative value
        dist = np.where(np.isinf(v), np.where((v >= lo) & ((v < hi) | (hi == np.inf)), 0.0, np.inf),
                        np.maximum(np.maximum(lo - v, v - hi), 0.0))
        dist = np.where((v == hi) & (dist == 0), np.finfo(np.float64).tiny, dist)     # the interval is open above
        ratio = np.where(dist == 0, 0.0, np.where(np.isfinite(dist) & (mo.tol > 0), dist / mo.tol, np.inf))
    ratio = np.where(ch[..., None], ratio, 0.0)
    bad = (ratio > 1.0).any(-1)
    assert not bad.any(), (f"{what}{name}: {int(bad.sum())} changed pixels outside the model, first (y, x) = {tuple(np.argwhere(bad)[0])}: "
                           f"got {image[bad][0]}, value {mo.val[bad][0]} +- {mo.tol[bad][0]}")
    return float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------------
def _sure(layer_res, members):
    m = np.zeros(layer_res.hi.shape, bool)
    for g in members:
        if g in layer_res.group_sure:
            m |= layer_res.group_sure[g]
    return m


def census(name):
    """{class: {"changed", "covered unchanged", "undecided", ...}} of a case, asserting that every class has the pixels it exists
    for (CLASSES)"""
    c, mo, o = cases()[name], model(name), oracle_frame(name)
    mk, out = mo.markers, {}
    none = np.zeros((H, W), bool)
    sure_of = lambda ls: _sure(mk.res, ls) if mk.res is not None else none
    won_by = lambda ls: (mo.kind == MARKER) & np.isin(mo.light, ls)
    for cls, ls in c.classes.items():
        if cls.startswith("g ") or cls in ("gizmo", "scissor"):
            continue
        sure = sure_of(ls)
        n = {"changed": int(won_by(ls).sum()), "covered unchanged": int((sure & (mo.kind == UNCHANGED)).sum()),
             "undecided": int((sure & (mo.kind == UNDECIDED)).sum())}
        out[cls] = n
        if cls == "front":
            assert n["changed"] > 0 and n["covered unchanged"] == 0 and (o.depth[won_by(ls)] > 0).all(), (name, cls, n)
        elif cls == "hidden":
            assert n["changed"] == 0 and n["covered unchanged"] > 0, (name, cls, n)
        elif cls == "cut":
            assert n["changed"] > 0 and n["covered unchanged"] > 0, (name, cls, n)
        elif cls == "background":
            assert n["changed"] > 0 and (o.depth[won_by(ls)] == 0).all(), (name, cls, n)
        elif cls in ("tie", "overlap"):
            n["both cover"] = 0
            for a, b in zip(ls[0::2], ls[1::2]):
                both = sure_of([a]) & sure_of([b]) & (mo.kind != UNDECIDED)
                if cls == "tie":
                    winner = b                                         # the later one
                else:
                    da, db = (float(np.linalg.norm(f64(c.lights[i]["pos"]))) for i in (a, b))
                    winner = a if da < db else b                       # the nearer one
                n["both cover"] += int(both.sum())
                assert both.sum() > 20 and (mo.light[both] == winner).all(), (name, cls, a, b, int(both.sum()))
        elif cls == "near":
            clipped = [p for p, pr in mk.res.prims.items() if p // mk.n_tris in ls and not pr.all_in and mk.res.sure_count[p] > 0]
            n["clipped visible triangles"] = len(clipped)
            assert n["changed"] > 100 and clipped, (name, cls, n)
        elif cls in ("inside", "behind", "nonfinite"):
            n["footprint"] = int(sure.sum())
            assert n["changed"] == 0 and n["footprint"] == 0 and n["undecided"] == 0, (name, cls, n)
        elif cls == "edge":
            ch = won_by(ls)
            n["on the border"] = int(ch[0].sum() + ch[-1].sum() + ch[:, 0].sum() + ch[:, -1].sum())
            assert ch[0].any() and ch[-1].any() and ch[:, 0].any() and ch[:, -1].any() and ch[H - 1, 0], (name, cls)
            assert ch[63:65, 63:65].all(), (name, cls, "tile crossing")
            assert all(won_by([i]).any() for i in ls)
        elif cls in ("tiny", "colour", "count"):
            per = [int(won_by([i]).sum()) for i in ls]
            n["per light"] = per
            if cls == "count":
                drawn = min(max(c.num_lights, 0), 100)
                assert all((k > 0) == (i < drawn) for i, k in zip(ls, per)), (name, cls, per)
            else:
                assert all(k > 0 for k in per) and (cls != "tiny" or max(per) <= 4), (name, cls, per)
        elif cls == "under":
            sure = sure_of(ls) & mo.rect
            n["lost to the gizmo"] = int((sure & (mo.kind == GIZMO)).sum())
            n["kept"] = int((won_by(ls) & mo.rect).sum())
            n["covers the rectangle"] = int(sure.sum())
            assert (n["kept"] > 0 and n["lost to the gizmo"] > 0) or (c.extent == 1 and n["covers the rectangle"] == 1), (name, cls, n)
    if mo.gizmo is not None:
        gz = mo.gizmo
        g = mo.kind == GIZMO
        out["gizmo"] = {"changed": int(g.sum()), "undecided": int(((mo.kind == UNDECIDED) & mo.rect).sum())}
        # (a one-pixel viewport holds the whole gizmo and its centre pixel may see none of it: the class is that the pass copes)
        assert (g.any() or c.extent == 1) and not (g & ~mo.rect).any(), (name, "gizmo")
        names = [h[0] for h in HAND]
        tri = lambda nm: names.index(nm)
        own = lambda t: (gz.kind == GIZMO) & (gz.prim == t)
        gsure = lambda t: _sure(gz.res, [t])
        for cls in c.classes:
            if cls == "scissor":
                pr, x0 = gz.res.prims[tri("big")], mo.x0
                rows = [y for y in range(H) if mo.kind[y, x0] == GIZMO and mo.prim[y, x0] == tri("big")]
                outside = [y for y in rows if all(f.at(-1, y) > 0 for f in pr.edge)]      # the exact footprint goes on at column x0 - 1
                out[cls] = {"rows cut at x0": len(outside), "x0": x0}
                assert outside and x0 % 32 and all(mo.kind[y, x0 - 1] != GIZMO for y in outside), (name, cls)
                assert (own(tri("big"))[:, -1]).any() and (own(tri("big"))[-1]).any(), "reaches the right and the bottom side"
            elif cls == "g overlap":
                k = 0
                for a, b, w in (("near first", "far second", "near first"), ("far first", "near second", "near second")):
                    both = gsure(tri(a)) & gsure(tri(b)) & (gz.kind != UNDECIDED)
                    k += int(both.sum())
                    assert both.sum() > 50 and (gz.prim[both] == tri(w)).all(), (name, cls, a, b)
                out[cls] = {"both cover": k}
            elif cls == "g tie":
                both = gsure(tri("coincident first")) & gsure(tri("coincident second")) & (gz.kind != UNDECIDED)
                out[cls] = {"both cover": int(both.sum())}
                assert both.sum() > 50 and (gz.prim[both] == tri("coincident second")).all(), (name, cls)
            elif cls in ("g zero normals", "g away"):
                m = own(tri("zero normals" if cls == "g zero normals" else "away"))
                out[cls] = {"black": int(m.sum())}
                assert m.sum() > 20 and not gz.val[m].any() and not gz.tol[m].any(), (name, cls)
            elif cls == "g one zero normal":
                m = own(tri("one zero normal"))
                out[cls] = {"changed": int(m.sum()), "undecided": int((gsure(tri("one zero normal")) & (gz.kind == UNDECIDED)).sum())}
                assert m.sum() > 20 and gz.val[m].min() > 0.3, (name, cls)
            elif cls == "g colour 3":
                m = own(tri("colour 3"))
                out[cls] = {"changed": int(m.sum())}
                assert m.sum() > 50 and (gz.val[m] - gz.tol[m] > 1.0).all(), (name, cls)
    out["frame"] = {"changed": int(((mo.kind == MARKER) | (mo.kind == GIZMO)).sum()), "undecided": int((mo.kind == UNDECIDED).sum())}
    assert out["frame"]["undecided"] <= MAX_UNDECIDED * W * H, (name, out["frame"])
    return out
